"""Every case of tests/helpers/matmul_cases.py on the fp32 batched matmul of matmul.hip (matmul_kernel in its 16 instances,
matmul_splitk_reduce) through ops.matmul, against the fp64 product of the SAME float operands, per element.  Before a case
runs, buctd_matmul_plan must report, for the pointers of the call, the tile and the split state the table names; the host-only
closure test (test_matmul_plan_cover.py) proves that the cases reach every layout pair on every tile with and without split-K.
The operands, the reference and the write set come from the addressing formulas of the header comment of matmul.hip
(matmul_cases.build), not from ops.matmul; every buffer element that is no operand element is NaN.

Metric and bar (not taken from what the kernels give):
  |err| / (|alpha| * (|A| @ |B|) + |bias|) <= min(2e-6, (K + 4) * 2^-24): the worst case of a K-term fp32 fmaf chain with the
  alpha / bias epilogue (or the split sums of the reduce kernel), capped by the project's fp32-class bar.  One dropped term
  is about 1 / K.  Asserted on the whole result and again on the last row tile, the last column tile (BM / BN of the plan
  query) and the rows of the last 16-row fragment; the message names the worst element.
Every element of the C allocation outside the write set of the case - a guard band before and after, the columns between
N and ldc, the other heads and groups - keeps its sentinel bitwise, with and without split-K; a split case run twice gives
identical bits.

Measured on an MI355X (worst |err| / sum|terms| over the cases of a tile, next to torch's fp32 CPU matmul by the same metric
on the case that gave it):
  tile                        0 (128x64 scalar)   1 (128x48)   2 (128x96)   3 (128x128)
  one split                       4.60e-07 *       3.87e-07 *   6.01e-07 *   3.94e-07 *
      torch fp32                  5.42e-07         3.93e-07     6.01e-07     3.75e-07
    random-normal operands        2.27e-07         2.57e-07     2.19e-07     2.15e-07
      torch fp32                  1.47e-07         1.80e-07     2.00e-07     1.92e-07
  split-K                         7.73e-08         2.21e-07 *   7.71e-08     8.96e-08
      torch fp32                  5.71e-08         1.88e-07     6.05e-08     5.42e-08
    random-normal operands        7.73e-08         1.00e-07     7.71e-08     8.96e-08
      torch fp32                  5.71e-08         9.17e-08     6.05e-08     5.42e-08
  (* the hard-operands case of the tile, K = 72, and K = 1040 for the split one.  The tightest bars: K = 3 gives 1.24e-07 on the
  scalar tile and 1.12e-07 on vector loads against 4.17e-07, both equal to torch's fp32 result.)  No case exceeds its bar, and
  no kernel bug was found.
Wall time of the module: 3.6 s (98 tests, fp64 references included; 1.0 s of it is the first launch, every other test takes
less than 0.1 s).
"""
import time

import pytest
import torch

from tests.helpers import matmul_cases as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = -12345.678
GUARD = 4096 + 37            # elements of the guard band on either side of C
WORST = {}


def bar_of(K):
    return min(2e-6, (K + 4) * U)


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print("\nworst |err| / sum|terms| per (tile, K split) (kernel / torch fp32 on the CPU, case):")
    for k in sorted(WORST):
        v = WORST[k]
        print(f"  tile {k[0]} split {int(k[1])}   {v[0]:.2e} / {v[1]:.2e}   at {v[2]}")
    print(f"wall time of the module: {time.time() - t0:.1f} s")


def subsets(c, pl):
    """boolean masks over [batch][M][N]"""
    m = torch.arange(c.M).view(1, c.M, 1)
    n = torch.arange(c.N).view(1, 1, c.N)
    full = lambda x: x.expand(c.batch, c.M, c.N)
    return {"whole result": None,
            "last row tile": full(m // pl["BM"] == (c.M - 1) // pl["BM"]),
            "last column tile": full(n // pl["BN"] == (c.N - 1) // pl["BN"]),
            "last 16-row fragment": full(m // 16 == (c.M - 1) // 16)}


def launch(ops, dev, c, a_d, b_d, bias_d, c_len):
    """ops.matmul into the middle of a sentinel-filled allocation; returns the whole allocation on the CPU"""
    big = torch.full((2 * GUARD + c_len,), SENTINEL, dtype=torch.float32, device=dev)
    ops.matmul(a_d, b_d, big[GUARD:GUARD + c_len], batch=c.batch, M=c.M, N=c.N, K=c.K, a_layout=c.a_layout, b_layout=c.b_layout,
               lda=c.lda, ldb=c.ldb, ldc=c.ldc, stride_a=c.stride_a, stride_b=c.stride_b, stride_c=c.stride_c, Kc=c.Kc, gsa=c.gsa,
               gsbk=c.gsbk, Nc=c.Nc, gsbn=c.gsbn, gsc=c.gsc, alpha=c.alpha, bias=bias_d, bias_axis=c.bias_axis or 0,
               a_off=c.a_off, b_off=c.b_off, c_off=c.c_off)
    return big.cpu()


@pytest.mark.parametrize("c", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_against_fp64(dev, c):
    from buctd_amd import ops
    name = T.case_id(c)
    b = T.build(c)
    a_d, b_d = b.a_buf.to(dev), b.b_buf.to(dev)
    bias_d = None if b.bias is None else b.bias.float().to(dev)
    assert a_d.data_ptr() % 16 == 0 and b_d.data_ptr() % 16 == 0
    pl = T.plan(c, a_d.data_ptr(), b_d.data_ptr())
    assert pl is not None and (pl["tile"], pl["vec"], pl["nsplit"]) == (c.tile, int(c.tile != 0), c.nsplit), \
        f"{name}: not on the kernel under test: {pl}"

    out = launch(ops, dev, c, a_d, b_d, bias_d, b.c_len)
    at_c = (GUARD + b.c_addr).reshape(-1)
    got = out[at_c].view(c.batch, c.M, c.N)

    ref = c.alpha * (b.A @ b.B)
    mag = abs(c.alpha) * (b.A.abs() @ b.B.abs())
    cpu = c.alpha * (b.A.float() @ b.B.float())
    if b.bias is not None:
        bv = b.bias.view(1, 1, c.N) if c.bias_axis == 0 else b.bias.view(1, c.M, 1)
        ref, mag, cpu = ref + bv, mag + bv.abs(), cpu + bv.float()
    r = (got.double() - ref).abs() / mag.clamp_min(1e-300)
    r_cpu = float(((cpu.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    bar = bar_of(c.K)
    worst = float(r.max())
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"{name}: error / sum|terms| {worst:.3e} at (b, m, n) = {at} (bar {bar:.3e}, K = {c.K}; torch fp32 on the CPU {r_cpu:.3e}); "
          f"tile {pl['tile']} {pl['BM']}x{pl['BN']} vec {pl['vec']} nsplit {pl['nsplit']} x {pl['k_per_split']}")
    key = (pl["tile"], pl["nsplit"] > 1)
    if not worst <= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (worst, r_cpu, name)
    assert torch.isfinite(got).all(), f"{name}: non-finite result (an operand read outside A / B, or an element never written)"
    for where, m in subsets(c, pl).items():
        rr = r if m is None else torch.where(m, r, torch.zeros((), dtype=r.dtype))
        w_ = float(rr.max())
        a_ = tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))
        assert w_ <= bar, (f"{name} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at (b, m, n) = {a_}: got {float(got[a_])!r}, "
                           f"fp64 {float(ref[a_])!r} (worst of the result {worst:.3e} at {at}; torch fp32 on the CPU {r_cpu:.3e}; "
                           f"plan {pl})")

    # everything outside the write set keeps the sentinel, bit for bit
    outside = torch.ones(out.numel(), dtype=torch.bool)
    outside[at_c] = False
    bits = out.view(torch.int32)
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
    hit = torch.nonzero(outside & (bits != want)).flatten()
    assert hit.numel() == 0, (f"{name}: {hit.numel()} elements outside the write set were written, the first at element "
                              f"{int(hit[0]) - GUARD} of C (value {float(out[hit[0]])!r}); plan {pl}")
    if pl["nsplit"] > 1:
        again = launch(ops, dev, c, a_d, b_d, bias_d, b.c_len)
        assert torch.equal(again.view(torch.int32), bits), f"{name}: two runs of the split case differ"


# ---- the head and group forms of the table are the descriptors ops.py builds ---------------------------------------------
def recorded(monkeypatch, ops):
    calls = []
    real = ops.matmul

    def rec(A, B, Cout, **kw):
        calls.append(kw)
        return real(A, B, Cout, **kw)

    monkeypatch.setattr(ops, "matmul", rec)
    return calls


def same_call(c, kw):
    d = dict(stride_a=0, stride_b=0, stride_c=0, Kc=None, gsa=0, gsbk=0, Nc=None, gsbn=0, gsc=0, alpha=1.0, bias_axis=0,
             a_off=0, b_off=0, c_off=0)
    d.update({k: v for k, v in kw.items() if k != "bias"})
    d["Kc"], d["Nc"] = d["Kc"] or d["K"], d["Nc"] or d["N"]
    mine = c._asdict()
    mine["bias_axis"] = c.bias_axis or 0
    return all(mine[k] == v for k, v in d.items()) and (c.bias_axis is not None) == (kw.get("bias") is not None)


def test_head_cases_are_the_calls_of_position_attention(dev, monkeypatch):
    from buctd_amd import ops
    calls = recorded(monkeypatch, ops)
    g = torch.Generator().manual_seed(11)
    for (B, Tq, Tk, h, d, tile), packed in [(s, False) for s in T.HEAD_SHAPES] + [(s, True) for s in T.HEAD_SHAPES_PACKED]:
        v = torch.randn(B, Tk, h * d, generator=g).to(dev).requires_grad_(True)
        if packed:
            q, k = torch.randn(B, Tq, 2 * h * d, generator=g).to(dev).requires_grad_(True), None
        else:
            q = torch.randn(B, Tq, h * d, generator=g).to(dev).requires_grad_(True)
            k = torch.randn(B, Tk, h * d, generator=g).to(dev).requires_grad_(True)
        ops.PositionAttention.apply(q, k, v, h, 0.0, False).sum().backward()
    assert len(calls) == 4 * 6 * 2
    for c in T.HEAD_CASES:
        assert any(same_call(c, kw) for kw in calls), f"{T.case_id(c)}: PositionAttention makes no such call"


def test_group_cases_are_the_calls_of_channel_attention(dev, monkeypatch):
    from buctd_amd import ops
    calls = recorded(monkeypatch, ops)
    g = torch.Generator().manual_seed(12)
    for B, Tn, Cn in ((3, 48, 16), (4, 20, 24), (3, 13, 6)):
        qn = torch.randn(B, Tn, Cn, generator=g).to(dev).requires_grad_(True)
        yn = torch.randn(B, Tn, Cn, generator=g).to(dev).requires_grad_(True)
        w = (torch.randn(Tn, Tn, generator=g) * 0.1).to(dev).requires_grad_(True)
        bias = torch.randn(Tn, generator=g).to(dev).requires_grad_(True)
        ops.ChannelAttention.apply(qn, yn, w, bias, 1, 0.0, False).sum().backward()
    for c in T.GROUP_CASES:
        assert any(same_call(c, kw) for kw in calls), f"{T.case_id(c)}: ChannelAttention makes no such call"
