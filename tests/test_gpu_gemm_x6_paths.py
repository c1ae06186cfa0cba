"""Every case of tests/helpers/gemm_x6_cases.py on the bf16x6 GEMM of gemm_x6.hip (x6_image_kernel + x6_gemm_kernel) through
ops.x6_image / ops.x6_gemm, against the fp64 product of the SAME float operands, per element; the operand images on their own,
decoded on the host; power-of-two scaling; and the three fc_o products inside ops.ChannelAttention.  The host-only closure test
(test_gemm_x6_plan_cover.py) proves that the cases reach every workgroup order, every branch of the XCD remap, both load paths
of the image kernel in both roles and every epilogue form.  Operands, reference and write set come from the two addressing
formulas of include/buctd_hip.h (gemm_x6_cases.build), not from ops.py; every source element that is no operand element is NaN.

Metric and bar (the bar of the other bf16x6 modules, not taken from what this kernel gives):
  r = |err| / (|alpha| * (|A| @ |B|) + |bias|) must be <= 2e-6 and <= 3 * r32 + 2e-7, r32 the same ratio of the exact-fp32 kernel
  (ops.matmul) on the same operands over the same elements.  Asserted on the whole result, on the last row tile and on the last
  column tile (128 / 192, from the plan query); the message names the worst (m, n).
C is prefilled with NaN inside the write set and with a sentinel everywhere else - a band before (it covers the space in front
of c_off) and after, the columns between N and ldc, the gaps between column groups: every written element must be finite, every
other one keeps the sentinel bitwise.  Both images end in front of a band at buctd_x6_image_bytes that must come back
untouched.  Two runs give identical bits.

The image format (header comment of gemm_x6.hip): block (vb, kb) = [3 pieces][64 lanes][8 bf16], lane l holds row vb * 16 +
(l & 15), slots kb * 32 + (l >> 4) * 8 ..; blocks [Vpad / 16][Kpad / 32].  float(h) + float(m) + float(l), summed in fp64, must
equal the source element exactly, and every padding slot must be +0 in all three pieces.  Two limits of the exact split are
stated here and not exercised: a magnitude above the largest bf16 (3.39e38) overflows the first piece, and a value so small
that its third piece (about 2^-16 of it) falls below the smallest normal bf16 (2^-126) loses bits; the operands here stay
within 2^+-75.

The weight image of fc_o behind ops._x6_weight_image following an in-place weight change (optimizer step, weights_updated)
bit for bit is proved on the GPU by tests/test_derived_cache.py (test_refresh_is_one_launch_per_family_and_linear_images_
rebuild_lazily, test_rebuild_counter_on_the_linear_image_and_the_bn_fold); it is not repeated here.

Measured on an MI355X (worst |err| / sum|terms| over the cases of a group, next to the fp32 kernel's on the case that gave it):
  group                                   bf16x6     fp32 kernel
  grid  (12 workgroup orders, K = 8)      1.22e-07   2.07e-07     6 x 9 = 54 workgroups
  tail  (23 edges of M, N and K)          1.52e-07   1.24e-07     33 x 20 x 257, transposed operands
  addr  (32 address functions)            1.95e-07   2.27e-07     A contiguous, off 2
  fc_o  (6 layouts of ChannelAttention)   2.05e-07   2.72e-07     data gradient, B 3 T 160 C 48
  epi   (11 epilogue forms)               1.65e-07   2.29e-07     ldc = N + 5, c_off = 3, bias per row, alpha
  hard  (3 cases)                         6.74e-07   7.61e-07     128 x 192 x 256
  The tightest bars: M = N = K = 1 gives 2.59e-08 on both kernels against 2.78e-07; K = 1 on 33 x 20 gives 1.03e-07 against
  3.72e-07 (fp32 kernel 5.73e-08: one product has no dropped piece products to hide).
  ChannelAttention at T = 512, B = 2, C = 96 (bf16x6 route / fp32 route, both against fp64): out 3.24e-07 / 3.34e-07, d fc_w
  4.36e-07 / 4.92e-07, d fc_b 9.08e-08 / 9.08e-08, d qn 1.94e-06 / 1.73e-06, d yn 1.72e-06 / 1.50e-06.  d qn and d yn are
  measured against the terms of their LAST contraction only; the soft-max backward in front of it cancels, which is why the
  exact-fp32 route alone comes to 1.7e-06 there and the margin to 2e-06 is narrow on both routes.
  No case exceeds its bar, every image decodes exactly, scaling keeps every bit, no band was touched: no defect in the arithmetic,
  the remap or the epilogue.  The one defect is the alignment predicate of the image kernel (it tested the element offset, not
  the address); the cases with off = 1, 2, 3 run on the corrected predicate only.
Wall time of the module: 1.9 s (103 tests, fp64 references included; 1.2 s of it is the first launch, every other test takes
less than 0.1 s).
"""
import math
import time

import pytest
import torch

from tests.helpers import gemm_x6_cases as T
from tests.helpers.guard_bands import SENTINEL, untouched

pytestmark = pytest.mark.gpu

GUARD = 4096                 # elements of the band on either side of C: a multiple of 16 bytes
IMG_BAND = 4096              # bytes on either side of an image
IMG_FILL = 0xA5
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print("\nworst |err| / sum|terms| per case group (bf16x6 / fp32 kernel on the same operands, case):")
    for k in T.GROUPS + ("scaled", "call sites x6", "call sites fp32"):
        if k in WORST:
            v = WORST[k]
            print(f"  {k:16s} {v[0]:.2e} / {v[1]:.2e}   at {v[2]}")
    print(f"wall time of the module: {time.time() - t0:.1f} s")


def note(group, r, r32, name):
    if not r <= WORST.get(group, (-1.0,))[0]:
        WORST[group] = (r, r32, name)


def make_image(ops, src_d, ad, V, K, role):
    """the image of X[V][K] between two bands; returns (image bytes, the whole allocation)"""
    from buctd_amd import _C
    need = _C.lib().buctd_x6_image_bytes(V, K, role)
    big = torch.full((2 * IMG_BAND + need,), IMG_FILL, dtype=torch.uint8, device=src_d.device)
    view = big[IMG_BAND:]
    out = ops.x6_image(src_d, V, K, role, vs=ad.vs, ks=ad.ks, vg=ad.vg, vgs=ad.vgs, kg=ad.kg, kgs=ad.kgs, off=ad.off, out=view)
    assert out.data_ptr() == view.data_ptr() and view.data_ptr() % 16 == 0
    return view[:need], big


def image_bands_intact(big):
    return bool((big[:IMG_BAND] == IMG_FILL).all()) and bool((big[-IMG_BAND:] == IMG_FILL).all())


def run(ops, dev, c, b, a_buf=None, b_buf=None):
    """both images and the product of case c into a banded allocation; returns the allocation on the CPU"""
    a_d, b_d = (b.a_buf if a_buf is None else a_buf).to(dev), (b.b_buf if b_buf is None else b_buf).to(dev)
    assert a_d.data_ptr() % 16 == 0 and b_d.data_ptr() % 16 == 0
    a_img, a_big = make_image(ops, a_d, c.a, c.M, c.K, 0)
    b_img, b_big = make_image(ops, b_d, c.b, c.N, c.K, 1)
    big = torch.full((2 * GUARD + b.c_len,), SENTINEL, dtype=torch.float32, device=dev)
    big[(GUARD + b.c_addr).reshape(-1).to(dev)] = float("nan")
    e = c.epi
    ops.x6_gemm(a_img, b_img, big[GUARD:], c.M, c.N, c.K, ldc=e.ldc, Nc=e.Nc, gsc=e.gsc,
                bias=None if b.bias is None else b.bias.to(dev), bias_axis=e.bias_axis or 0, alpha=e.alpha, c_off=e.c_off)
    out = big.cpu()
    assert image_bands_intact(a_big) and image_bands_intact(b_big), f"{T.case_id(c)}: a launch wrote outside an operand image"
    return out


def fp32_kernel(ops, dev, c, b):
    """the same product on the exact-fp32 kernel, dense"""
    out = torch.full((c.M, c.N), float("nan"), device=dev)
    ops.matmul(b.A.to(dev), b.B.to(dev), out, batch=1, M=c.M, N=c.N, K=c.K, a_layout=0, b_layout=1, lda=c.K, ldb=c.N, ldc=c.N,
               alpha=c.epi.alpha, bias=None if b.bias is None else b.bias.to(dev), bias_axis=c.epi.bias_axis or 0)
    return out.cpu()


def reference(c, b):
    """fp64 result and the sum of the absolute values of each element's terms"""
    A, B = b.A.double(), b.B.double()
    ref, mag = c.epi.alpha * (A @ B), abs(c.epi.alpha) * (A.abs() @ B.abs())
    if b.bias is not None:
        bv = b.bias.double().view(1, c.N) if c.epi.bias_axis == 0 else b.bias.double().view(c.M, 1)
        ref, mag = ref + bv, mag + bv.abs()
    return ref, mag


def worst_of(r, mask=None):
    rr = r if mask is None else torch.where(mask, r, torch.zeros((), dtype=r.dtype))
    return float(rr.max()), tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))


def check_ratios(name, group, got, got32, ref, mag, subsets):
    r = (got.double() - ref).abs() / mag.clamp_min(1e-300)
    r32 = (got32.double() - ref).abs() / mag.clamp_min(1e-300)
    whole, at = worst_of(r)
    whole32, _ = worst_of(r32)
    print(f"{name}: error / sum|terms| {whole:.3e} at {at} (fp32 kernel {whole32:.3e}, bar {min(2e-6, 3 * whole32 + 2e-7):.3e})")
    note(group, whole, whole32, name)
    for where, m in subsets.items():
        w_, a_ = worst_of(r, m)
        w32, _ = worst_of(r32, m)
        bar = min(2e-6, 3 * w32 + 2e-7)
        assert w_ <= bar, (f"{name} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at (m, n) = {a_}: got {float(got[a_])!r}, fp64 "
                           f"{float(ref[a_])!r} (fp32 kernel on these elements {w32:.3e}; worst of the result {whole:.3e} at {at})")


@pytest.mark.parametrize("c", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_against_fp64(dev, c):
    from buctd_amd import ops
    name = T.case_id(c)
    b = T.build(c)
    pl = T.plan(c.M, c.N, c.K)
    assert pl is not None and (c.grid is None or (pl["gx"], pl["gy"], pl["row_major"]) == c.grid), f"{name}: not on the order under test: {pl}"

    out = run(ops, dev, c, b)
    at_c = (GUARD + b.c_addr).reshape(-1)
    got = out[at_c].view(c.M, c.N)
    assert torch.isfinite(got).all(), (f"{name}: {int((~torch.isfinite(got)).sum())} elements are not finite (never written, or an "
                                       f"operand read outside A / B), the first at (m, n) = "
                                       f"{tuple(int(v) for v in torch.nonzero(~torch.isfinite(got))[0])}; plan {pl}")
    ref, mag = reference(c, b)
    m, n = torch.arange(c.M).view(-1, 1), torch.arange(c.N).view(1, -1)
    subsets = {"whole result": None,
               "last row tile": (m // T.BM == (c.M - 1) // T.BM).expand(c.M, c.N),
               "last column tile": (n // T.BN == (c.N - 1) // T.BN).expand(c.M, c.N)}
    check_ratios(name, c.group, got, fp32_kernel(ops, dev, c, b), ref, mag, subsets)

    # everything outside the write set keeps the sentinel, bit for bit
    assert untouched(out, GUARD, b.c_len), f"{name}: the launch wrote in front of or behind C"
    outside = torch.ones(out.numel(), dtype=torch.bool)
    outside[at_c] = False
    bits = out.view(torch.int32)
    want = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32)
    hit = torch.nonzero(outside & (bits != want)).flatten()
    assert hit.numel() == 0, (f"{name}: {hit.numel()} elements outside the write set were written, the first at element "
                              f"{int(hit[0]) - GUARD} of C (value {float(out[hit[0]])!r}); plan {pl}")
    again = run(ops, dev, c, b)
    assert torch.equal(again.view(torch.int32), bits), f"{name}: two runs differ"


# ---- the images on their own ---------------------------------------------------------------------------------------------------
def image_sources():
    """every (address function, V, K) of the table, by role, once"""
    seen = {}
    for c in T.CASES:
        seen.setdefault((0, c.a, c.M, c.K), T.case_id(c))
        seen.setdefault((1, c.b, c.N, c.K), T.case_id(c))
    return seen


def operand(kind, V, K, g):
    if kind == "hard":
        return T.hard_operands((V, K), g, -12, 12)
    x = torch.randn(V, K, generator=g)
    return x * 2.0 ** {"normal": 0, "2^60": 60, "2^-60": -60}[kind]


@pytest.mark.parametrize("role", (0, 1), ids=("A", "B"))
@pytest.mark.parametrize("kind", ("normal", "hard", "2^60", "2^-60"))
def test_image_decodes_to_the_source_exactly(dev, kind, role):
    from buctd_amd import ops
    g = torch.Generator().manual_seed(17 + role)
    n = 0
    for (r, ad, V, K), name in image_sources().items():
        if r != role:
            continue
        n += 1
        X = operand(kind, V, K, g)
        img, big = make_image(ops, T.source(X, ad).to(dev), ad, V, K, role)
        val, bits = T.decode_image(img, V, K, role)
        assert image_bands_intact(big), f"{name} role {role}: the image kernel wrote outside buctd_x6_image_bytes"
        total = val[0] + val[1] + val[2]
        bad = torch.nonzero(total[:V, :K] != X.double())
        assert bad.numel() == 0, (f"{name} role {role} {ad}: h + m + l differs from the source at {bad.shape[0]} elements, the first "
                                  f"(v, k) = {tuple(int(v) for v in bad[0])}: {float(total[tuple(bad[0])])!r} for "
                                  f"{float(X[tuple(bad[0])])!r}")
        pad = torch.ones(bits.shape[1:], dtype=torch.bool)
        pad[:V, :K] = False
        bad = torch.nonzero((bits != 0).any(0) & pad)
        assert bad.numel() == 0, (f"{name} role {role} {ad}: {bad.shape[0]} padding slots are not +0, the first (v, k) = "
                                  f"{tuple(int(v) for v in bad[0])}")
    assert n >= 30


# ---- A * 2^s and B * 2^-s: the split is exact and the accumulation is fp32, so C keeps its bits -----------------------------------
SCALED = [c for c in T.CASES if (c.group, c.M, c.N, c.K) in (("tail", 129, 193, 7), ("tail", 33, 20, 257), ("hard", 129, 193, 257),
                                                            ("fc_o", 160, 60, 160))]


@pytest.mark.parametrize("c", SCALED, ids=[T.case_id(c) for c in SCALED])
def test_power_of_two_scaling_keeps_every_bit(dev, c):
    from buctd_amd import ops
    b = T.build(c)
    base = run(ops, dev, c, b)
    for s in (-40, 40):
        out = run(ops, dev, c, b, T.source(b.A * 2.0 ** s, c.a), T.source(b.B.t().contiguous() * 2.0 ** -s, c.b))
        diff = torch.nonzero(out.view(torch.int32) != base.view(torch.int32)).flatten()
        assert diff.numel() == 0, (f"{T.case_id(c)} s = {s}: {diff.numel()} elements differ from the unscaled product, the first at "
                                   f"element {int(diff[0]) - GUARD} of C: {float(out[diff[0]])!r} for {float(base[diff[0]])!r}")


def test_scaled_cases_cover_both_operand_kinds():
    assert len(SCALED) >= 5 and {c.hard for c in SCALED} == {0, 1}


# ---- the call sites: the three fc_o products of ops.ChannelAttention at the smallest shape that takes them ------------------------
def channel_attention_fp64(qn, yn, W, bias, dout):
    """out and the gradients in fp64 (h = 1, no dropout), each with the sum of the absolute values of the terms of the
    contraction that forms it"""
    qn, yn, W, bias, dout = (x.double() for x in (qn, yn, W, bias, dout))
    Tn = qn.shape[1]
    scale = 1.0 / math.sqrt(Tn)
    A = torch.softmax(torch.einsum("btc,btd->bcd", qn, yn) * scale, -1)
    on = torch.einsum("btd,bcd->btc", yn, A)
    out = torch.einsum("pt,btc->bpc", W, on) + bias[None, :, None]
    don = torch.einsum("pt,bpc->btc", W, dout)
    dA = torch.einsum("btc,btd->bcd", don, yn)
    dL = A * (dA - (A * dA).sum(-1, keepdim=True)) * scale
    res = {
        "out": (out, torch.einsum("pt,btc->bpc", W.abs(), on.abs()) + bias.abs()[None, :, None]),
        "d fc_w": (torch.einsum("bpc,btc->pt", dout, on), torch.einsum("bpc,btc->pt", dout.abs(), on.abs())),
        "d fc_b": (dout.sum((0, 2)), dout.abs().sum((0, 2))),
        "d qn": (torch.einsum("btd,bcd->btc", yn, dL), torch.einsum("btd,bcd->btc", yn.abs(), dL.abs())),
        "d yn": (torch.einsum("btc,bcd->btd", don, A) + torch.einsum("btc,bcd->btd", qn, dL),
                 torch.einsum("btc,bcd->btd", don.abs(), A.abs()) + torch.einsum("btc,bcd->btd", qn.abs(), dL.abs())),
    }
    # the restatement against autograd on the same fp64 graph
    leaves = [x.clone().requires_grad_(True) for x in (qn, yn, W, bias)]
    A2 = torch.softmax(torch.einsum("btc,btd->bcd", leaves[0], leaves[1]) * scale, -1)
    o2 = torch.einsum("pt,btc->bpc", leaves[2], torch.einsum("btd,bcd->btc", leaves[1], A2)) + leaves[3][None, :, None]
    o2.backward(dout)
    for k, x in zip(("d qn", "d yn", "d fc_w", "d fc_b"), leaves):
        assert float((x.grad - res[k][0]).abs().max()) <= 1e-11 * float(res[k][1].max()), k
    return res


def test_channel_attention_takes_the_x6_products_and_both_routes_meet_the_bar(dev, monkeypatch):
    from buctd_amd import ops
    assert ops.get_conv_math() == "bf16x6"
    Bn, Tn, Cn = 2, 512, 96
    assert ops.fc_o_x6_ok(Tn, Bn * Cn) and not ops.fc_o_x6_ok(Tn - 1, Bn * Cn) and not ops.fc_o_x6_ok(Tn, Bn * Cn - 1)
    g = torch.Generator().manual_seed(23)
    qn, yn, dout = (torch.randn(Bn, Tn, Cn, generator=g) for _ in range(3))
    W = torch.randn(Tn, Tn, generator=g) * Tn ** -0.5
    bias = torch.randn(Tn, generator=g)
    want = channel_attention_fp64(qn, yn, W, bias, dout)

    calls = []
    real = ops.x6_gemm
    monkeypatch.setattr(ops, "x6_gemm", lambda *a, **kw: (calls.append((a[3:6], kw)), real(*a, **kw))[1])

    def route():
        leaves = [x.clone().to(dev).requires_grad_(True) for x in (qn, yn, W, bias)]
        out = ops.ChannelAttention.apply(*leaves, 1, 0.0, False)
        out.backward(dout.to(dev))
        return {"out": out.detach().cpu(), "d qn": leaves[0].grad.cpu(), "d yn": leaves[1].grad.cpu(), "d fc_w": leaves[2].grad.cpu(),
                "d fc_b": leaves[3].grad.cpu()}

    x6 = route()
    assert [c[0] for c in calls] == [(Tn, Bn * Cn, Tn), (Tn, Tn, Bn * Cn), (Tn, Bn * Cn, Tn)], "forward, weight gradient, data gradient"
    assert calls[0][1].get("bias") is not None and calls[0][1]["bias_axis"] == 1 and calls[2][1].get("bias") is None
    monkeypatch.setattr(ops, "fc_o_x6_ok", lambda T_, rows: False)
    f32 = route()
    assert len(calls) == 3, "the fp32 route made a bf16x6 product"
    for k, (ref, mag) in want.items():
        r = float(((x6[k].double() - ref).abs() / mag.clamp_min(1e-300)).max())
        r32 = float(((f32[k].double() - ref).abs() / mag.clamp_min(1e-300)).max())
        print(f"ChannelAttention {k}: error / sum|terms| bf16x6 route {r:.3e}, fp32 route {r32:.3e}")
        note("call sites x6", r, r32, k)
        note("call sites fp32", r32, r32, k)
        assert r32 <= 2e-6, f"{k}: fp32 route {r32:.3e} > 2e-6"
        assert r <= min(2e-6, 3 * r32 + 2e-7), f"{k}: bf16x6 route {r:.3e} > {min(2e-6, 3 * r32 + 2e-7):.3e} (fp32 route {r32:.3e})"
