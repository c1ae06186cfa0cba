"""The streaming kernels between the matrix kernels - csrc/bn.hip, the soft-max / LayerNorm part of csrc/attention.hip,
csrc/elementwise.hip - against float64 references, one parametrised test per kernel family, one case per code path
(tests/helpers/stream_cases.py names the paths; tests/test_stream_cases_cover.py shows that every path has a case).

Every call runs twice through the C interface: once with each read-only operand between NaN bands and each output (and
workspace) between sentinel bands, once on plain tensors.  The bands must be intact, no NaN may be picked up and the two
results must be bit-equal; where a case names an ops.* entry, that wrapper must give the same bits again.

Bars (all against fp64, none taken from the kernels):
  bit-exact     add, relu, relu_bwd, mul, scale by 2^k, add_n (left to right), copy_channels, add_bcast, both transposes,
                max-pool values / indices (first maximum wins), max-pool backward where at most one output names an input,
                dres, fuse_sum (every prefix of its left-to-right sum of at most two terms is one fp32 addition)
  reductions    |err| <= (n_seq + 8) 2^-24 sum |terms|: colsum, classic BN mean / dgamma / dbeta, LayerNorm dgamma / dbeta
                (n_seq per path: stream_cases.py)
  project bars  accumulator path (test_gpu_bn_acc.py), soft-max 2e-6, LayerNorm y 5e-6, dx 2e-5 (test_gpu_ops.py `close`)
  measured      classic invstd (long rows) / dz, bn_apply, bn_fold, resize, fuse_sum(_bwd) beyond two terms: the same formula
                in fp32 on the CPU is measured against fp64; bar = max(4 x that, 2^-23), relative as stated per test

Worst figures of the MI355X run, per family: kernel error / bar [error of the fp32 CPU formula], case
  bn_apply                           7.260e-08 / 2.904e-07 [7.260e-08]  at (65, 3, 0, 0)
  bn_apply_acc_group invstd          9.895e-08 / 3.000e-07  at (2, 6, 5, 192, 'none', 0, 0)
  bn_apply_acc_group mean            5.359e-08 / 2.478e-06  at (2, 24, 18, 48, 'y', 1, 0)
  bn_apply_acc_group running_mean    1.178e-07 / 2.354e-06  at (2, 12, 9, 96, 'beta', 0, 1)
  bn_apply_acc_group running_var     6.021e-08 / 1.000e-06  at (2, 6, 5, 192, 'none', 0, 0)
  bn_apply_acc_group y               6.081e-07 / 1.090e-04  at (2, 6, 5, 192, 'none', 0, 0)
  bn_bwd C=1024 dbeta                1.184e-08 / 4.292e-06  at ('direct', 4100, 1024, 'none', 1, 1)
  bn_bwd C=1024 dgamma               1.834e-08 / 4.292e-06  at ('direct', 4100, 1024, 'beta', 1, 0)
  bn_bwd C=1024 dz                   1.052e-07 / 4.208e-07 [1.052e-07]  at ('direct', 4100, 1024, 'beta', 1, 0)
  bn_bwd C=2048 dbeta                9.100e-08 / 4.292e-06  at ('ops', 130, 2048, 'beta', 1, 1)
  bn_bwd C=2048 dgamma               1.411e-07 / 4.292e-06  at ('ops', 130, 2048, 'y', 1, 0)
  bn_bwd C=2048 dz                   7.963e-08 / 3.185e-07 [7.963e-08]  at ('ops', 130, 2048, 'y', 1, 0)
  bn_bwd C=3 dbeta                   4.416e-08 / 4.292e-06  at ('ops', 105, 3, 'y', 0, 0)
  bn_bwd C=3 dgamma                  6.125e-08 / 4.292e-06  at ('ops', 105, 3, 'beta', 0, 0)
  bn_bwd C=3 dz                      9.420e-08 / 3.768e-07 [9.420e-08]  at ('ops', 105, 3, 'y', 0, 0)
  bn_bwd C=48 dbeta                  8.126e-09 / 1.907e-06  at ('direct', 4100, 48, 'beta', 1, 0)
  bn_bwd C=48 dgamma                 1.192e-08 / 1.907e-06  at ('direct', 4100, 48, 'y', 1, 1)
  bn_bwd C=48 dz                     8.856e-08 / 3.529e-07 [8.822e-08]  at ('direct', 4100, 48, 'y', 1, 1)
  bn_bwd_acc dbeta                   8.093e-05 / 1.462e-02  at (12, 96, 72, 48, 'none')
  bn_bwd_acc dgamma                  9.634e-05 / 1.382e-02  at (12, 96, 72, 48, 'none')
  bn_bwd_acc dz                      1.257e-06 / 1.057e-04  at (12, 96, 72, 48, 'y')
  bn_bwd_acc_group dbeta             2.414e-06 / 3.753e-04  at (2, 6, 5, 192, 'none', 0, 0)
  bn_bwd_acc_group dgamma            2.744e-06 / 4.617e-04  at (2, 6, 5, 192, 'none', 0, 0)
  bn_bwd_acc_group dz                5.870e-07 / 6.227e-05  at (2, 24, 18, 48, 'y', 1, 0)
  bn_bwd_from_partials dbeta         7.715e-09 / 1.907e-06  at (4100, 48, 'y', 1, 0)
  bn_bwd_from_partials dgamma        1.114e-08 / 1.907e-06  at (4100, 48, 'y', 1, 0)
  bn_bwd_from_partials dz            8.856e-08 / 3.529e-07 [8.822e-08]  at (4100, 48, 'y', 1, 0)
  bn_fold scale                      7.168e-08 / 2.867e-07 [7.168e-08]  at 1
  bn_fold shift                      1.762e-07 / 7.048e-07 [1.762e-07]  at 256
  bn_stats invstd                    1.944e-07 / 2.146e-06  at (64, 300, 0)
  bn_stats invstd (long rows)        3.928e-08 / 1.571e-07 [3.928e-08]  at (131651, 3, 0)
  bn_stats mean                      3.845e-07 / 4.292e-06  at (64, 300, 0)
  bn_stats running_mean              2.857e-01 / 1.000e+00  at (1, 300, 0)
  bn_stats running_var               1.127e-07 / 1.000e-06  at (64, 300, 0)
  colsum                             3.627e-07 / 4.292e-06  at (70, 300, 0)
  fuse_sum                           5.944e-08 / 2.377e-07 [5.944e-08]  at (2, 8, 16, 8, (0, 1), 0)
  fuse_sum_bwd                       9.587e-08 / 3.835e-07 [9.587e-08]  at (2, 8, 16, 8, 1, 0)
  layernorm dbeta                    1.573e-07 / 4.292e-06  at (65, 63)
  layernorm dgamma                   2.028e-07 / 4.292e-06  at (3, 512)
  layernorm dx                       8.496e-07 / 9.358e-05  at (64, 112)
  layernorm invstd                   1.200e-07 / 9.537e-07  at (65, 65)
  layernorm mean                     1.427e-07 / 1.311e-06  at (130, 300)
  layernorm y                        9.554e-07 / 2.802e-05  at (64, 300)
  maxpool dx (shared argmax)         6.900e-08 / 7.153e-07  at (2, 7, 7, 3, 1)
  resize_bilinear                    3.729e-08 / 1.492e-07 [3.729e-08]  at (2, 5, 1, 3, 7, 5, 14, 10)
  softmax dropout ds                 6.181e-09 / 2.000e-06  at (5, 64, 3.0)
  softmax ds                         1.270e-08 / 2.000e-06  at (5, 65, 3.0)
  softmax p                          2.301e-08 / 2.000e-06  at (8, 64, 3.0)
bit-equal in every case: add, add+relu, add_bcast, add_layernorm_fwd invstd, add_layernorm_fwd mean, add_layernorm_fwd sum, add_layernorm_fwd y, add_n, bn_apply_acc_group member invstd, bn_apply_acc_group member mean, bn_apply_acc_group member rm, bn_apply_acc_group member rv, bn_apply_acc_group member y, bn_bwd C=1024 dres, bn_bwd C=2048 dres, bn_bwd C=3 dres, bn_bwd C=48 dres, bn_bwd_acc dres, bn_bwd_acc_group dres, bn_bwd_acc_group member dbeta, bn_bwd_acc_group member dgamma, bn_bwd_acc_group member dres, bn_bwd_acc_group member dz, bn_bwd_from_partials dres, copy_channels, fuse_sum (<= 2 terms), fuse_sum_bwd shift 0, maxpool idx, maxpool y, mul, nchw_to_nhwc, nhwc_to_nchw, relu, relu_bwd, scale, scale (device scalar), softmax dropout dseed ds, softmax dropout dseed p, softmax dropout dseed pd, softmax dropout pd
"""
import ctypes as C
import functools

import pytest
import torch

from tests.helpers import stream_cases as S
from tests.helpers.guard_bands import Bands

pytestmark = pytest.mark.gpu

WORST = {}
M32 = float(torch.tensor(0.1, dtype=torch.float32))        # the momentum and eps the kernels receive (float arguments)
EPS32 = float(torch.tensor(S.EPS, dtype=torch.float32))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst figures per family (kernel error / bar [fp32 CPU error], case):")
    for k in sorted(WORST):
        err, bar, e32, case = WORST[k]
        print(f"  {k:34s} {err:.3e} / {bar:.3e}" + (f" [{e32:.3e}]" if e32 is not None else "") + f"  at {case}")


def note(fam, err, bar, case, e32=None):
    err, bar = float(err), float(bar)
    if fam not in WORST or err / max(bar, 1e-300) > WORST[fam][0] / max(WORST[fam][1], 1e-300):
        WORST[fam] = (err, bar, e32, case)
    print(f"{fam} {case}: {err:.3e} / {bar:.3e}" + (f" [fp32 {e32:.3e}]" if e32 is not None else ""))
    return err <= bar


def measured(fam, got, ref64, ref32, scale, case):
    """the measured bar: error of `got` and of the fp32 CPU formula against fp64, both divided by `scale`"""
    err = ((got.double() - ref64).abs() / scale).max().item() if got.numel() else 0.0
    e32 = ((ref32.double() - ref64).abs() / scale).max().item() if got.numel() else 0.0
    bar = max(4 * e32, S.FLOOR)
    assert note(fam, err, bar, case, e32), f"{fam} {case}: error {err:.3e} > bar {bar:.3e} (fp32 CPU formula: {e32:.3e})"


def reduction(fam, got, ref64, mag, n_seq, case):
    """|err| <= (n_seq + 8) 2^-24 sum |terms| per output element"""
    ratio = ((got.double() - ref64).abs() / mag.clamp_min(1e-300)).max().item()
    bar = (n_seq + 8) * S.U
    assert note(fam, ratio, bar, case), f"{fam} {case}: error / sum|terms| {ratio:.3e} > ({n_seq} + 8) 2^-24 = {bar:.3e}"


def close(fam, got, ref64, tol, case):
    """the `close` metric of test_gpu_ops.py: max |err| <= tol max(1, max |ref|)"""
    err = (got.double() - ref64).abs().max().item()
    bar = tol * max(1.0, ref64.abs().max().item())
    assert note(fam, err, bar, case), f"{fam} {case}: max abs err {err:.3e} > {bar:.3e}"


def exact(fam, got, ref, case):
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{fam} {case}: {got.dtype} {tuple(got.shape)}"
    same = torch.equal(got, ref)
    note(fam, 0.0 if same else 1.0, 0.0, case)
    assert same, f"{fam} {case}: not bit-equal, {(got != ref).sum().item()} of {got.numel()} elements differ"


def both(dev, run, what):
    """run(mem) -> {name: device tensor}; between bands and plain: intact bands, no NaN, the same bits -> CPU tensors"""
    mem = Bands(dev, True)
    a = run(mem)
    torch.cuda.synchronize()
    mem.check(what)
    b = run(Bands(dev, False))
    torch.cuda.synchronize()
    out = {}
    for k, v in a.items():
        if v is None:
            assert b[k] is None
            out[k] = None
            continue
        assert not (v.dtype.is_floating_point and bool(torch.isnan(v).any())), f"{what}: NaN in {k}"
        assert torch.equal(v, b[k]), f"{what}: {k} between guard bands differs from the plain call"
        out[k] = v.cpu()
    return out


def lib_ops():
    from buctd_amd import _C, ops
    return _C.lib(), _C, ops


def ok(rc, what):
    from buctd_amd import _C
    _C.check(rc, what)


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    from buctd_amd import _C
    return _C.stream_ptr()


# ---- BatchNorm backward, classic path ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def bwd_setup(rows, Cn, form):
    z, dy, mean, invstd, gamma, beta, y, mask = S.bn_bwd_operands("bn_bwd", (rows, Cn, form), rows, Cn, form)
    ref64 = S.bn_bwd_ref(dy, z, mean, invstd, gamma, mask)
    dz32 = S.bn_bwd_ref(dy, z, mean, invstd, gamma, mask, torch.float32)[0]
    g = S.case_gen("bn_bwd_prior", (rows, Cn))
    prior = (torch.randn(Cn, generator=g), torch.randn(Cn, generator=g))
    return (z, dy, mean, invstd, gamma, beta, y), ref64, dz32, prior


def run_bn_bwd(mem, lib, opnd, prior, rows, Cn, form, dres, acc, keep_ws=None):
    z, dy, mean, invstd, gamma, beta, y = opnd
    relu = form != "none"
    d = {k: mem.ro(v) for k, v in (("z", z), ("dy", dy), ("mean", mean), ("invstd", invstd), ("gamma", gamma))}
    yb = mem.ro(y) if form == "y" else None
    bb = mem.ro(beta) if form == "beta" else None
    dz = mem.new((rows, Cn), "dz")
    dr = mem.new((rows, Cn), "dres") if dres else None
    nan = torch.full((Cn,), float("nan"))
    dg = mem.out(prior[0] if acc else nan, "dgamma")
    db = mem.out(prior[1] if acc else nan, "dbeta")
    need = lib.buctd_bn_bwd_workspace(rows, Cn)
    ws = mem.new((need // 4,), "the workspace")
    ok(lib.buctd_bn_bwd(P(d["dy"]), P(yb), P(d["z"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]), P(bb), int(relu), rows, Cn,
                        P(dz), P(dr), P(dg), P(db), acc, P(ws), need, stream()), "bn_bwd")
    if keep_ws is not None:
        keep_ws.append(ws)
    return {"dz": dz, "dres": dr, "dgamma": dg, "dbeta": db}


def check_bn_bwd(fam, got, ref64, dz32, prior, acc, n_seq, case):
    dz64, g64, s1, s2, m1, m2 = ref64
    if got["dres"] is not None:
        exact(fam + " dres", got["dres"], g64.float(), case)
    p0, p1 = (prior[0].double(), prior[1].double()) if acc else (torch.zeros_like(s1), torch.zeros_like(s1))
    reduction(fam + " dgamma", got["dgamma"], s2 + p0, m2 + p0.abs(), n_seq, case)
    reduction(fam + " dbeta", got["dbeta"], s1 + p1, m1 + p1.abs(), n_seq, case)
    measured(fam + " dz", got["dz"], dz64, dz32, max(1.0, dz64.abs().max().item()), case)


def bwd_n_seq(rows, Cn):
    if Cn % 4 == 0 and Cn // 4 <= 256:
        return S.chain(S.bwd2_blocks(rows)[1], 256 // (Cn // 4))
    return S.BWD_ROWS


@pytest.mark.parametrize("case", S.BN_BWD, ids=str)
def test_bn_bwd_classic(dev, case):
    lib, _C, ops = lib_ops()
    entry, rows, Cn, form, dres, acc = case
    opnd, ref64, dz32, prior = bwd_setup(rows, Cn, form)
    got = both(dev, lambda mem: run_bn_bwd(mem, lib, opnd, prior, rows, Cn, form, dres, acc), f"bn_bwd {case}")
    if entry == "ops":
        assert not ops.bn_acc_ok(Cn), "ops.bn_bwd would take the accumulator path"
        z, dy, mean, invstd, gamma, beta, y = (None if t is None else t.to(dev) for t in opnd)
        dg = (prior[0] if acc else torch.zeros(Cn)).to(dev)
        db = (prior[1] if acc else torch.zeros(Cn)).to(dev)
        dz, dr = ops.bn_bwd(dy, y if form == "y" else None, z, mean, invstd, gamma, form != "none", bool(dres), dg, db, acc,
                            beta=beta if form == "beta" else None)
        for name, t in (("dz", dz), ("dres", dr), ("dgamma", dg), ("dbeta", db)):
            assert (t is None and got[name] is None) or torch.equal(t.cpu(), got[name]), f"ops.bn_bwd {case}: {name} differs"
    check_bn_bwd("bn_bwd C=%d" % Cn, got, ref64, dz32, prior, acc, bwd_n_seq(rows, Cn), case)


@pytest.mark.parametrize("case", S.BN_BWD_PARTIALS, ids=str)
def test_bn_bwd_from_partials(dev, case):
    """the partial sums of buctd_bn_bwd's own reduce kernel, handed to buctd_bn_bwd_from_partials: the same bits"""
    lib, _C, ops = lib_ops()
    rows, Cn, form, dres, acc = case
    opnd, ref64, dz32, prior = bwd_setup(rows, Cn, form)
    keep = []
    first = run_bn_bwd(Bands(dev, False), lib, opnd, prior, rows, Cn, form, dres, acc, keep)
    nparts = S.bwd2_blocks(rows)[0]
    part = keep[0][:nparts * 2 * Cn].clone()
    z, dy, mean, invstd, gamma, beta, y = opnd
    relu = form != "none"

    def run(mem):
        d = {k: mem.ro(v) for k, v in (("z", z), ("dy", dy), ("mean", mean), ("invstd", invstd), ("gamma", gamma))}
        yb = mem.ro(y) if form == "y" else None
        bb = mem.ro(beta) if form == "beta" else None
        pb = mem.ro(part.cpu())
        dz, dr = mem.new((rows, Cn), "dz"), mem.new((rows, Cn), "dres")
        nan = torch.full((Cn,), float("nan"))
        dg, db = mem.out(prior[0] if acc else nan, "dgamma"), mem.out(prior[1] if acc else nan, "dbeta")
        ws = mem.new((2 * Cn,), "the workspace")
        ok(lib.buctd_bn_bwd_from_partials(P(d["dy"]), P(yb), P(d["z"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]), P(bb),
                                          int(relu), rows, Cn, P(pb), nparts, P(dz), P(dr), P(dg), P(db), acc, P(ws), 8 * Cn,
                                          stream()), "bn_bwd_from_partials")
        return {"dz": dz, "dres": dr, "dgamma": dg, "dbeta": db}
    got = both(dev, run, f"bn_bwd_from_partials {case}")
    for k, v in got.items():
        exact("bn_bwd_from_partials " + k, v, first[k].cpu(), case)
    check_bn_bwd("bn_bwd_from_partials", got, ref64, dz32, prior, acc, bwd_n_seq(rows, Cn), case)
    assert lib.buctd_bn_bwd_from_partials(P(first["dz"]), None, P(first["dz"]), P(first["dgamma"]), P(first["dgamma"]),
                                          P(first["dgamma"]), None, 0, rows, Cn, P(part), nparts, P(first["dz"]), None, None,
                                          None, 0, P(part), 8 * Cn - 4, stream()) != 0, "a workspace of 2 C - 1 floats is refused"


# ---- BatchNorm statistics, apply, fold ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.BN_STATS, ids=str)
def test_bn_stats_and_finalize(dev, case):
    lib, _C, ops = lib_ops()
    rows, Cn, explicit = case
    g = S.case_gen("bn_stats", (rows, Cn))
    z = S.channel_data(g, rows, Cn)
    rm0, rv0 = torch.randn(Cn, generator=g), 0.5 + torch.rand(Cn, generator=g)
    ng = S.ceil_div(rows, S.STAT_ROWS)
    counts = torch.full((ng,), S.STAT_ROWS, dtype=torch.int32)
    counts[-1] = rows - (ng - 1) * S.STAT_ROWS

    def run(mem):
        zb = mem.ro(z)
        part = mem.new((ng, Cn, 2), "the partials")
        ngo, rpg = C.c_int(0), C.c_int(0)
        ok(lib.buctd_bn_stats(P(zb), rows, Cn, P(part), C.byref(ngo), C.byref(rpg), stream()), "bn_stats")
        assert (ngo.value, rpg.value) == (ng, S.STAT_ROWS)
        cb = mem.ro(counts) if explicit else None
        mean, invstd = mem.new((Cn,), "mean"), mem.new((Cn,), "invstd")
        rm, rv = mem.out(rm0, "running_mean"), mem.out(rv0, "running_var")
        ok(lib.buctd_bn_finalize(P(part), P(cb), ng, S.STAT_ROWS, rows, Cn, S.EPS, 0.1, P(mean), P(invstd), P(rm), P(rv), stream()),
           "bn_finalize")
        return {"mean": mean, "invstd": invstd, "rm": rm, "rv": rv, "part": part}
    got = both(dev, run, f"bn_stats {case}")
    if not explicit:
        part, info = ops.bn_stats(z.to(dev))
        assert torch.equal(part.view(-1)[:ng * Cn * 2].cpu(), got["part"].view(-1)), "ops.bn_stats: other partials"
    mu, var, mag = S.bn_stats_ref(z)
    inv = 1.0 / torch.sqrt(var + EPS32)
    reduction("bn_stats mean", got["mean"], mu, mag, S.STAT_ROWS, case)
    z32 = z.float()
    mu32 = z32.sum(0) / rows
    inv32 = 1.0 / torch.sqrt(((z32 - mu32) ** 2).sum(0) / rows + S.EPS)
    if rows > 131072:
        measured("bn_stats invstd (long rows)", got["invstd"], inv, inv32, inv, case)
    else:
        # var is a sum of non-negative terms: relative error <= (64 + 8) 2^-24, half of it in invstd
        rel = ((got["invstd"].double() - inv).abs() / inv).max().item()
        assert note("bn_stats invstd", rel, 0.5 * (S.STAT_ROWS + 8) * S.U, case), f"bn_stats {case}: invstd off by {rel:.3e}"
    rm = (1.0 - M32) * rm0.double() + M32 * mu
    unb = var * rows / (rows - 1) if rows > 1 else var
    rv = (1.0 - M32) * rv0.double() + M32 * unb
    err = ((got["rm"].double() - rm).abs() / (M32 * mag * (S.STAT_ROWS + 8) * S.U + 2 * S.U * rm.abs())).max().item()
    assert note("bn_stats running_mean", err, 1.0, case), f"bn_stats {case}: running_mean {err:.3f} of its bound"
    rel = ((got["rv"].double() - rv).abs() / rv).max().item()
    assert note("bn_stats running_var", rel, 1e-6, case), f"bn_stats {case}: running_var off by {rel:.3e}"


@pytest.mark.parametrize("case", S.BN_APPLY, ids=str)
def test_bn_apply(dev, case):
    lib, _C, ops = lib_ops()
    rows, Cn, with_res, relu = case
    g = S.case_gen("bn_apply", (rows, Cn))
    z = S.channel_data(g, rows, Cn)
    gamma, beta = S.bn_params(g, Cn)
    res = torch.randn(rows, Cn, generator=g) if with_res else None
    mu, var, _ = S.bn_stats_ref(z)
    mean, invstd = mu.float(), (1.0 / torch.sqrt(var + S.EPS)).float()

    def run(mem):
        y = mem.new((rows, Cn), "y")
        ok(lib.buctd_bn_apply(P(mem.ro(z)), P(mem.ro(mean)), P(mem.ro(invstd)), P(mem.ro(gamma)), P(mem.ro(beta)),
                              P(mem.ro(res)), relu, P(y), rows, Cn, stream()), "bn_apply")
        return {"y": y}
    got = both(dev, run, f"bn_apply {case}")
    y2 = ops.bn_apply(z.to(dev), mean.to(dev), invstd.to(dev), gamma.to(dev), beta.to(dev), None if res is None else res.to(dev), relu)
    assert torch.equal(y2.cpu(), got["y"]), "ops.bn_apply: other bits"
    ref = S.bn_apply_ref(z, mean, invstd, gamma, beta, res, relu)
    ref32 = S.bn_apply_ref(z, mean, invstd, gamma, beta, res, relu, torch.float32)
    measured("bn_apply", got["y"], ref, ref32, max(1.0, ref.abs().max().item()), case)


@pytest.mark.parametrize("Cn", S.BN_FOLD)
def test_bn_fold(dev, Cn):
    lib, _C, ops = lib_ops()
    g = S.case_gen("bn_fold", Cn)
    gamma, beta = S.bn_params(g, Cn)
    rm, rv = torch.randn(Cn, generator=g), 0.1 + torch.rand(Cn, generator=g)

    def run(mem):
        sc, sh = mem.new((Cn,), "scale"), mem.new((Cn,), "shift")
        ok(lib.buctd_bn_fold(P(mem.ro(gamma)), P(mem.ro(beta)), P(mem.ro(rm)), P(mem.ro(rv)), S.EPS, Cn, P(sc), P(sh), stream()),
           "bn_fold")
        return {"scale": sc, "shift": sh}
    got = both(dev, run, f"bn_fold {Cn}")

    def ref(dt):
        sc = gamma.to(dt) / torch.sqrt(rv.to(dt) + (EPS32 if dt == torch.float64 else S.EPS))
        return sc, beta.to(dt) - rm.to(dt) * sc
    (sc, sh), (sc32, sh32) = ref(torch.float64), ref(torch.float32)
    measured("bn_fold scale", got["scale"], sc, sc32, sc.abs(), Cn)
    measured("bn_fold shift", got["shift"], sh, sh32, beta.double().abs() + (rm.double() * sc).abs(), Cn)


# ---- accumulator path -------------------------------------------------------------------------------------------------------
def acc_bwd_call(lib, mem, ops, dev, opnd, rows, Cn, form, want_dres, accumulate, prior, acc_ptr=None, ready=0):
    z, dy, mean, invstd, gamma, beta, y = opnd
    d = {k: mem.ro(v) for k, v in (("z", z), ("dy", dy), ("mean", mean), ("invstd", invstd), ("gamma", gamma))}
    yb = mem.ro(y) if form == "y" else None
    bb = mem.ro(beta) if form == "beta" else None
    dz = mem.new((rows, Cn), "dz")
    dr = mem.new((rows, Cn), "dres") if want_dres else None
    nan = torch.full((Cn,), float("nan"))
    dg, db = mem.out(prior[0] if accumulate else nan, "dgamma"), mem.out(prior[1] if accumulate else nan, "dbeta")
    if acc_ptr is None:
        acc_ptr = ops.AccRef(Cn, dev).ptr
    args = (P(d["dy"]), P(yb), P(d["z"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]), P(bb), int(form != "none"), rows, Cn,
            P(dz), P(dr), P(dg), P(db), accumulate, acc_ptr, ready)
    return args, {"dz": dz, "dres": dr, "dgamma": dg, "dbeta": db}, (d, yb, bb)


def check_acc_bwd(fam, got, ref64, prior, accumulate, case):
    dz64, g64, s1, s2, m1, m2 = ref64
    p0, p1 = (prior[0].double(), prior[1].double()) if accumulate else (0.0, 0.0)
    if got["dres"] is not None:
        exact(fam + " dres", got["dres"], g64.float(), case)
    close(fam + " dz", got["dz"], dz64, 1e-5, case)
    close(fam + " dgamma", got["dgamma"], s2 + p0, 2e-5, case)
    close(fam + " dbeta", got["dbeta"], s1 + p1, 2e-5, case)


@pytest.mark.parametrize("case", S.BN_ACC_BWD, ids=str)
def test_bn_bwd_accumulator_long(dev, case):
    lib, _C, ops = lib_ops()
    ops.step_boundary(dev)
    N, H, W, Cn, form = case
    rows = N * H * W
    opnd, ref64, dz32, prior = bwd_setup(rows, Cn, form)

    def run(mem):
        args, outs, keep = acc_bwd_call(lib, mem, ops, dev, opnd, rows, Cn, form, 1, 1, prior)
        ok(lib.buctd_bn_bwd_acc(*args, stream()), "bn_bwd_acc")
        return outs
    got = both(dev, run, f"bn_bwd_acc {case}")
    z, dy, mean, invstd, gamma, beta, y = (None if t is None else t.to(dev) for t in opnd)
    dg, db = prior[0].to(dev), prior[1].to(dev)
    dz, dr = ops.bn_bwd(dy, y if form == "y" else None, z, mean, invstd, gamma, form != "none", True, dg, db, 1,
                        beta=beta if form == "beta" else None)
    for name, t in (("dz", dz), ("dres", dr), ("dgamma", dg), ("dbeta", db)):
        assert torch.equal(t.cpu(), got[name]), f"ops.bn_bwd {case}: {name} differs from the direct call"
    check_acc_bwd("bn_bwd_acc", got, ref64, prior, 1, case)


@pytest.mark.parametrize("case", S.BN_ACC_GROUP, ids=lambda c: "x".join(str(m[3]) for m in c))
def test_bn_acc_group_backward(dev, case):
    """every member of a group launch is bit-equal to its own single launch (one member's sums are already in its accumulator)"""
    lib, _C, ops = lib_ops()
    ops.step_boundary(dev)
    plain = Bands(dev, False)
    singles, setups, accs = [], [], []
    for (N, H, W, Cn, form, res, ready) in case:
        rows = N * H * W
        opnd, ref64, dz32, prior = bwd_setup(rows, Cn, form)
        args, outs, keep = acc_bwd_call(lib, plain, ops, dev, opnd, rows, Cn, form, 1, ready, prior)
        ok(lib.buctd_bn_bwd_acc(*args, stream()), "bn_bwd_acc")
        torch.cuda.synchronize()
        singles.append({k: v.cpu() for k, v in outs.items()})
        setups.append((opnd, ref64, prior, rows))
        accs.append(args[15] if ready else None)            # the single launch left this member's sums in its accumulator

    def run(mem):
        items = (_C.BnBwdItem * len(case))()
        outs, keep = {}, []
        for k, (N, H, W, Cn, form, res, ready) in enumerate(case):
            opnd, ref64, prior, rows = setups[k]
            args, o, kp = acc_bwd_call(lib, mem, ops, dev, opnd, rows, Cn, form, 1, ready, prior, accs[k], ready)
            keep.append(kp)
            it = items[k]
            (it.dy, it.y, it.z, it.mean, it.invstd, it.gamma, it.beta, it.relu, it.rows, it.C, it.dz, it.dres, it.dgamma,
             it.dbeta, it.accumulate, it.acc, it.acc_ready) = args
            outs.update({f"{k}.{n}": t for n, t in o.items()})
        ok(lib.buctd_bn_bwd_acc_group(len(case), items, stream()), "bn_bwd_acc_group")
        return outs
    got = both(dev, run, f"bn_bwd_acc_group {case}")
    for k, member in enumerate(case):
        mine = {n: got[f"{k}.{n}"] for n in ("dz", "dres", "dgamma", "dbeta")}
        for n, t in mine.items():
            exact("bn_bwd_acc_group member " + n, t, singles[k][n], member)
        check_acc_bwd("bn_bwd_acc_group", mine, setups[k][1], setups[k][2], member[6], member)


@pytest.mark.parametrize("case", S.BN_ACC_GROUP, ids=lambda c: "x".join(str(m[3]) for m in c))
def test_bn_acc_group_forward(dev, case):
    """accumulators filled by the 3x3 convolution; group launch of bn_apply_acc against the single launches and fp64"""
    lib, _C, ops = lib_ops()
    ops.set_conv_math("bf16x6")
    ops.step_boundary(dev)
    members = []
    for (N, H, W, Cn, form, with_res, ready) in case:
        g = S.case_gen("bn_acc_fwd", (N, H, W, Cn))
        x = (torch.randn(N, H, W, Cn, generator=g) + 0.5).to(dev)
        w = (torch.randn(Cn, Cn, 3, 3, generator=g) * (Cn * 9) ** -0.5).contiguous(memory_format=torch.channels_last).to(dev)
        z, acc, info = ops.conv_fwd(x, w, None, 1, 1, stats="acc")
        assert info[0] == "acc", f"{N}x{H}x{W}x{Cn}: the convolution did not fill an accumulator"
        gamma, beta = S.bn_params(g, Cn)
        res = torch.randn(N, H, W, Cn, generator=g) if with_res else None
        rm0, rv0 = torch.randn(Cn, generator=g), 0.5 + torch.rand(Cn, generator=g)
        members.append((z, acc.ptr, gamma, beta, res, rm0, rv0, N * H * W, Cn, int(form != "none")))
    torch.cuda.synchronize()

    def fill(mem, m, st):
        z, accp, gamma, beta, res, rm0, rv0, rows, Cn, relu = m
        o = {"y": mem.new(tuple(z.shape), "y"), "mean": mem.new((Cn,), "mean"), "invstd": mem.new((Cn,), "invstd"),
             "rm": mem.out(rm0, "running_mean"), "rv": mem.out(rv0, "running_var")}
        st.acc, st.rows, st.eps, st.momentum = accp, rows, S.EPS, 0.1
        st.mean_out, st.invstd_out, st.running_mean, st.running_var = P(o["mean"]), P(o["invstd"]), P(o["rm"]), P(o["rv"])
        return o, (mem.ro(z.cpu()), mem.ro(gamma), mem.ro(beta), mem.ro(res))

    singles = []
    for m in members:
        st = _C.BnAccIn()
        o, (zb, gb, bb, rb) = fill(Bands(dev, False), m, st)
        ok(lib.buctd_bn_apply_acc(P(zb), C.byref(st), P(gb), P(bb), P(rb), m[9], P(o["y"]), m[7], m[8], stream()), "bn_apply_acc")
        torch.cuda.synchronize()
        singles.append({k: v.cpu() for k, v in o.items()})

    def run(mem):
        items = (_C.BnApplyItem * len(members))()
        outs, keep = {}, []
        for k, m in enumerate(members):
            o, (zb, gb, bb, rb) = fill(mem, m, items[k].st)
            keep.append((zb, gb, bb, rb))
            it = items[k]
            it.z, it.gamma, it.beta, it.residual, it.relu, it.y, it.rows, it.C = P(zb), P(gb), P(bb), P(rb), m[9], P(o["y"]), m[7], m[8]
            outs.update({f"{k}.{n}": t for n, t in o.items()})
        ok(lib.buctd_bn_apply_acc_group(len(members), items, stream()), "bn_apply_acc_group")
        return outs
    got = both(dev, run, f"bn_apply_acc_group {case}")
    for k, m in enumerate(members):
        z, accp, gamma, beta, res, rm0, rv0, rows, Cn, relu = m
        mine = {n: got[f"{k}.{n}"] for n in ("y", "mean", "invstd", "rm", "rv")}
        for n, t in mine.items():
            exact("bn_apply_acc_group member " + n, t, singles[k][n], case[k])
        zd = z.cpu().reshape(rows, Cn)
        mu, var, _ = S.bn_stats_ref(zd)
        inv = 1.0 / torch.sqrt(var + EPS32)
        y = S.bn_apply_ref(zd, mu, inv, gamma, beta, None if res is None else res.reshape(rows, Cn), relu)
        close("bn_apply_acc_group mean", mine["mean"], mu, 2e-6, case[k])
        rel = ((mine["invstd"].double() - inv).abs() / inv).max().item()
        assert note("bn_apply_acc_group invstd", rel, 3e-7, case[k]), f"invstd off by {rel:.3e}"
        close("bn_apply_acc_group y", mine["y"].reshape(rows, Cn), y, 2e-5, case[k])
        rv = (1.0 - M32) * rv0.double() + M32 * var * rows / (rows - 1)
        rel = ((mine["rv"].double() - rv).abs() / rv).max().item()
        assert note("bn_apply_acc_group running_var", rel, 1e-6, case[k]), f"running_var off by {rel:.3e}"
        close("bn_apply_acc_group running_mean", mine["rm"], (1.0 - M32) * rm0.double() + M32 * mu, 1e-6, case[k])


# ---- soft-max ---------------------------------------------------------------------------------------------------------------
def softmax_logits(case):
    rows, L, spread = case
    g = S.case_gen("softmax", case)
    if spread == 3.0:
        s = torch.randn(rows, L, generator=g) * 3.0
    else:
        s = -(1.5 * spread / S.SOFTMAX_SCALE) * torch.rand(rows, L, generator=g)
    return s, torch.randn(rows, L, generator=g), g


def seed_table(dev, seed):
    return torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.int64, device=dev)


def run_softmax(lib, mem, s, dp, rows, L, p_drop, seed, inplace, dseed, dev):
    table = seed_table(dev, seed) if dseed else None
    sarg = P(table) if dseed else seed
    fwd = lib.buctd_softmax_dropout_fwd_dseed if dseed else lib.buctd_softmax_dropout_fwd
    bwd = lib.buctd_softmax_dropout_bwd_dseed if dseed else lib.buctd_softmax_dropout_bwd
    if inplace:
        p = mem.out(s, "p (in place)")
        src = p
    else:
        src, p = mem.ro(s), mem.new((rows, L), "p")
    pd = mem.new((rows, L), "pd") if p_drop > 0 else p
    ok(fwd(P(src), rows, L, S.SOFTMAX_SCALE, p_drop, sarg, P(p), P(pd), stream()), "softmax_dropout_fwd")
    if inplace:
        ds = mem.out(dp, "ds (in place)")
        gsrc = ds
    else:
        gsrc, ds = mem.ro(dp), mem.new((rows, L), "ds")
    ok(bwd(P(gsrc), P(p), rows, L, S.SOFTMAX_SCALE, p_drop, sarg, P(ds), stream()), "softmax_dropout_bwd")
    return {"p": p, "pd": pd, "ds": ds}


@pytest.mark.parametrize("case", S.SOFTMAX, ids=str)
def test_softmax_fwd_bwd(dev, case):
    lib, _C, ops = lib_ops()
    rows, L, spread = case
    s, dp, g = softmax_logits(case)
    res = {}
    for inplace in (0, 1):
        for dseed in (0, 1):
            res[inplace, dseed] = both(dev, lambda mem: run_softmax(lib, mem, s, dp, rows, L, 0.0, 1234567, inplace, dseed, dev),
                                       f"softmax {case} inplace={inplace} dseed={dseed}")
    for key, r in res.items():
        for k in ("p", "ds"):
            assert torch.equal(r[k], res[0, 0][k]), f"softmax {case}: {k} of (inplace, dseed) = {key} differs from the plain entry"
    for inplace in (True, False):
        sd, dd = s.to(dev), dp.to(dev)
        p, pd = ops.softmax_dropout_fwd(sd, L, S.SOFTMAX_SCALE, 0.0, 5, inplace=inplace)
        ds = ops.softmax_dropout_bwd(dd, p, L, S.SOFTMAX_SCALE, 0.0, 5, inplace=inplace)
        assert torch.equal(p.cpu(), res[0, 0]["p"]) and torch.equal(ds.cpu(), res[0, 0]["ds"]), f"ops.softmax {case}: other bits"
        assert pd is p and (p is sd) == inplace and (ds is dd) == inplace
    got = res[0, 0]
    # the backward takes the kernel's own p (what the product feeds it); the reference is the fp64 chain
    p64, ds64 = S.softmax_ref(s, S.SOFTMAX_SCALE32, dp)
    close("softmax p", got["p"], p64, 2e-6, case)
    close("softmax ds", got["ds"], ds64, 2e-6, case)
    assert ((got["p"].double().sum(-1) - 1.0).abs() <= (L + 8) * S.U).all()


@pytest.mark.parametrize("case", S.SOFTMAX_DROP, ids=str)
def test_softmax_dropout_entries_agree(dev, case):
    """p = 0.3: the value-seed and device-seed entries give the same bits, and the backward regenerates the forward's mask"""
    lib, _C, ops = lib_ops()
    rows, L, spread = case
    s, dp, g = softmax_logits(case)
    pdrop, seed = 0.3, 0x9E3779B97F4A7C15
    a = both(dev, lambda mem: run_softmax(lib, mem, s, dp, rows, L, pdrop, seed, 0, 0, dev), f"softmax dropout {case}")
    b = both(dev, lambda mem: run_softmax(lib, mem, s, dp, rows, L, pdrop, seed, 0, 1, dev), f"softmax dropout dseed {case}")
    for k in a:
        exact("softmax dropout dseed " + k, b[k], a[k], case)
    p, pd, ds = a["p"], a["pd"], a["ds"]
    keep = pd != 0
    inv_keep = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(pdrop, dtype=torch.float32)))
    exact("softmax dropout pd", pd, torch.where(keep, p * inv_keep, torch.zeros_like(p)), case)
    frac = 1.0 - keep.double().mean().item()
    n = rows * L
    assert abs(frac - pdrop) <= 5 * (pdrop * (1 - pdrop) / n) ** 0.5 + 1.0 / n, f"{case}: dropped fraction {frac:.3f}"
    # the backward with the forward's mask, in fp64 on the kernel's own p
    gm = torch.where(keep, dp.double() * inv_keep, torch.zeros_like(dp, dtype=torch.float64))
    ds64 = S.SOFTMAX_SCALE32 * p.double() * (gm - (gm * p.double()).sum(-1, keepdim=True))
    close("softmax dropout ds", ds, ds64, 2e-6, case)
    sd = s.to(dev)
    assert lib.buctd_softmax_dropout_fwd(P(sd), rows, L, S.SOFTMAX_SCALE, pdrop, seed, P(sd), P(sd), stream()) != 0, "p == pd with dropout is refused"


def test_softmax_refuses_rows_longer_than_8192(dev):
    lib, _C, ops = lib_ops()
    t = torch.zeros(8193, device=dev)
    assert lib.buctd_softmax_dropout_fwd(P(t), 1, 8193, 1.0, 0.0, 0, P(t), P(t), stream()) != 0
    assert b"8193" in lib.buctd_last_error()
    assert lib.buctd_softmax_dropout_bwd(P(t), P(t), 1, 8193, 1.0, 0.0, 0, P(t), stream()) != 0


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.LAYERNORM, ids=str)
def test_layernorm_fwd_bwd(dev, case):
    lib, _C, ops = lib_ops()
    rows, Cn = case
    g = S.case_gen("layernorm", case)
    a = S.channel_data(g, Cn, rows).t().contiguous()        # a per-ROW mean of a few sigma: the axis LayerNorm normalises
    b = torch.randn(rows, Cn, generator=g)
    x = a + b                                               # one fp32 addition: what add_layernorm_fwd forms itself
    gamma, beta = S.bn_params(g, Cn)
    dy = torch.randn(rows, Cn, generator=g)
    prior = (torch.randn(Cn, generator=g), torch.randn(Cn, generator=g))
    eps = 1e-5

    def fwd(mem, fused, keep_sum):
        y, mean, invstd = mem.new((rows, Cn), "y"), mem.new((rows,), "mean"), mem.new((rows,), "invstd")
        out = {"y": y, "mean": mean, "invstd": invstd}
        if fused:
            sm = mem.new((rows, Cn), "sum") if keep_sum else None
            ok(lib.buctd_add_layernorm_fwd(P(mem.ro(a)), P(mem.ro(b)), P(mem.ro(gamma)), P(mem.ro(beta)), rows, Cn, eps, P(sm), P(y),
                                           P(mean), P(invstd), stream()), "add_layernorm_fwd")
            out["sum"] = sm
        else:
            ok(lib.buctd_layernorm_fwd(P(mem.ro(x)), P(mem.ro(gamma)), P(mem.ro(beta)), rows, Cn, eps, P(y), P(mean), P(invstd),
                                       stream()), "layernorm_fwd")
        return out
    got = both(dev, lambda mem: fwd(mem, False, False), f"layernorm_fwd {case}")
    for keep_sum in (True, False):
        fused = both(dev, lambda mem: fwd(mem, True, keep_sum), f"add_layernorm_fwd {case} keep_sum={keep_sum}")
        for k in ("y", "mean", "invstd"):
            exact("add_layernorm_fwd " + k, fused[k], got[k], case)
        if keep_sum:
            exact("add_layernorm_fwd sum", fused["sum"], x, case)
        y2, m2, i2, s2 = ops.add_layernorm_fwd(a.to(dev), b.to(dev), gamma.to(dev), beta.to(dev), eps, keep_sum=keep_sum)
        assert torch.equal(y2.cpu(), got["y"]) and torch.equal(m2.cpu(), got["mean"]) and (s2 is not None) == keep_sum
    y64, mu64, inv64 = S.layernorm_ref(x, gamma, beta, EPS32)
    close("layernorm y", got["y"], y64, 5e-6, case)
    # mean: 8 additions per lane and 6 in the shuffle tree, then one division
    reduction("layernorm mean", got["mean"], mu64, x.double().abs().sum(-1) / Cn, 14, case)
    # var: non-negative terms, (14 + 4) 2^-24 relative (squares, division, eps); invstd: half of it plus rsqrtf's 2 ulp
    rel = ((got["invstd"].double() - inv64).abs() / inv64).max().item()
    assert note("layernorm invstd", rel, 16 * S.U, case), f"layernorm {case}: invstd off by {rel:.3e}"

    mean, invstd = mu64.float(), inv64.float()              # the backward's operands: the fp64 statistics, rounded once

    def bwd(mem, accumulate):
        dx = mem.new((rows, Cn), "dx")
        nan = torch.full((Cn,), float("nan"))
        dg, db = mem.out(prior[0] if accumulate else nan, "dgamma"), mem.out(prior[1] if accumulate else nan, "dbeta")
        need = lib.buctd_layernorm_bwd_workspace(rows, Cn)
        ws = mem.new((need // 4,), "the workspace")
        ok(lib.buctd_layernorm_bwd(P(mem.ro(dy)), P(mem.ro(x)), P(mem.ro(mean)), P(mem.ro(invstd)), P(mem.ro(gamma)), rows, Cn, P(dx),
                                   P(dg), P(db), accumulate, P(ws), need, stream()), "layernorm_bwd")
        return {"dx": dx, "dgamma": dg, "dbeta": db}
    dx64, dg64, db64, mg, mb = S.layernorm_bwd_ref(dy, x, mean, invstd, gamma)
    for accumulate in (0, 1):
        r = both(dev, lambda mem: bwd(mem, accumulate), f"layernorm_bwd {case} accumulate={accumulate}")
        p0, p1 = (prior[0].double(), prior[1].double()) if accumulate else (torch.zeros(Cn, dtype=torch.float64),) * 2
        close("layernorm dx", r["dx"], dx64, 2e-5, case)
        reduction("layernorm dgamma", r["dgamma"], dg64 + p0, mg + p0.abs(), S.LN_ROWS, case)
        reduction("layernorm dbeta", r["dbeta"], db64 + p1, mb + p1.abs(), S.LN_ROWS, case)


def test_layernorm_refuses_more_than_512_columns(dev):
    lib, _C, ops = lib_ops()
    t = torch.zeros(2 * 513, device=dev)
    with pytest.raises(_C.BuctdHipError, match="C 513 > 512 unsupported"):
        ops.layernorm_fwd(t.view(2, 513), t[:513], t[:513], 1e-5)
    with pytest.raises(_C.BuctdHipError, match="C 513 > 512 unsupported"):
        ops.add_layernorm_fwd(t.view(2, 513), t.view(2, 513), t[:513], t[:513], 1e-5)
    assert lib.buctd_layernorm_bwd(P(t), P(t), P(t), P(t), P(t), 2, 513, P(t), P(t), P(t), 0, P(t), 1 << 20, stream()) != 0
    assert lib.buctd_layernorm_bwd(P(t), P(t), P(t), P(t), P(t), 2, 512, P(t), P(t), P(t), 0, P(t), 16, stream()) != 0, "workspace too small"


# ---- element-wise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.EW_N)
def test_add_mul_relu_scale(dev, n):
    lib, _C, ops = lib_ops()
    g = S.case_gen("ew", n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y = torch.relu(a)                                       # a forward output with exact zeros
    dsc = torch.tensor([4.0])
    every = n <= S.EW_ALL           # the long size: one entry per kernel (add and relu are add_kernel; scale twice the same)
    names = ("add_relu", "mul", "relu_bwd", "scale") + (("add", "relu", "scale_dev") if every else ())

    def run(mem):
        ab, bb = mem.ro(a), mem.ro(b)
        o = {k: mem.new((n,), k) for k in names}
        ok(lib.buctd_add(P(ab), P(bb), P(o["add_relu"]), n, 1, stream()), "add")
        ok(lib.buctd_mul(P(ab), P(bb), P(o["mul"]), n, stream()), "mul")
        ok(lib.buctd_relu_bwd(P(bb), P(mem.ro(y)), P(o["relu_bwd"]), n, stream()), "relu_bwd")
        ok(lib.buctd_scale(P(ab), None, 0.125, P(o["scale"]), n, stream()), "scale")
        if every:
            ok(lib.buctd_add(P(ab), P(bb), P(o["add"]), n, 0, stream()), "add")
            ok(lib.buctd_add(P(ab), None, P(o["relu"]), n, 1, stream()), "add")
            ok(lib.buctd_scale(P(ab), P(mem.ro(dsc)), 0.5, P(o["scale_dev"]), n, stream()), "scale")
        return o
    got = both(dev, run, f"element-wise n={n}")
    exact("add+relu", got["add_relu"], torch.relu(a + b), n)
    exact("mul", got["mul"], a * b, n)
    exact("relu_bwd", got["relu_bwd"], torch.where(y > 0, b, torch.zeros_like(b)), n)
    exact("scale", got["scale"], a * 0.125, n)
    if every:
        exact("add", got["add"], a + b, n)
        exact("relu", got["relu"], torch.relu(a), n)
        exact("scale (device scalar)", got["scale_dev"], a * 2.0, n)
        ad, bd = a.to(dev), b.to(dev)
        assert torch.equal(ops.add(ad, bd).cpu(), got["add"]) and torch.equal(ops.mul(ad, bd).cpu(), got["mul"])
        assert torch.equal(ops.relu_bwd(bd, y.to(dev)).cpu(), got["relu_bwd"])


@pytest.mark.parametrize("case", S.ADD_N, ids=str)
def test_add_n_left_to_right(dev, case):
    lib, _C, ops = lib_ops()
    n, k = case
    g = S.case_gen("add_n", case)
    # magnitudes that make the order visible: (a0 + a1) + a2 differs from a0 + (a1 + a2) on most elements
    terms = [torch.randn(n, generator=g) * s for s in (1.0, 1e3, -1e3, 1e-3)[:k]]
    if k >= 3:
        terms[2] = -terms[1] + torch.randn(n, generator=g)

    def run(mem):
        tb = [mem.ro(t) for t in terms]
        out = mem.new((n,), "the sum")
        arr = (C.c_void_p * k)(*[P(t) for t in tb])
        ok(lib.buctd_add_n(arr, k, P(out), n, stream()), "add_n")
        return {"out": out}
    got = both(dev, run, f"add_n {case}")
    ref = terms[0] + terms[1]
    for t in terms[2:]:
        ref = ref + t
    exact("add_n", got["out"], ref, case)


@pytest.mark.parametrize("case", S.COLSUM, ids=str)
def test_colsum(dev, case):
    lib, _C, ops = lib_ops()
    rows, Cn, accumulate = case
    g = S.case_gen("colsum", (rows, Cn))
    x = S.channel_data(g, rows, Cn)
    prior = torch.randn(Cn, generator=g)

    def run(mem):
        out = mem.out(prior if accumulate else torch.full((Cn,), float("nan")), "the sums")
        need = lib.buctd_colsum_workspace(rows, Cn)
        ws = mem.new((max(1, need // 4),), "the workspace")
        ok(lib.buctd_colsum(P(mem.ro(x)), rows, Cn, P(out), accumulate, P(ws), need, stream()), "colsum")
        return {"out": out}
    got = both(dev, run, f"colsum {case}")
    o2 = ops.colsum(x.to(dev), Cn, (prior if accumulate else torch.zeros(Cn)).to(dev), accumulate)
    assert torch.equal(o2.cpu(), got["out"]), "ops.colsum: other bits"
    cr = S.colsum_chunk_rows(rows)
    n_seq = S.chain(cr, 256 // min(Cn, 256))
    p = prior.double() if accumulate else torch.zeros(Cn, dtype=torch.float64)
    reduction("colsum", got["out"], x.double().sum(0) + p, x.double().abs().sum(0) + p.abs(), n_seq, case)
    assert lib.buctd_colsum(P(o2), rows, Cn, P(o2), 0, P(o2), max(0, lib.buctd_colsum_workspace(rows, Cn) - 4), stream()) != 0


@pytest.mark.parametrize("case", S.FUSE_SUM, ids=str)
def test_fuse_sum(dev, case):
    lib, _C, ops = lib_ops()
    N, H, W, Cn, shifts, relu = case
    g = S.case_gen("fuse_sum", case)
    terms = [torch.randn(N, H >> s, W >> s, Cn, generator=g) for s in shifts]

    def run(mem):
        tb = [mem.ro(t) for t in terms]
        out = mem.new((N, H, W, Cn), "the sum")
        arr = (C.c_void_p * len(tb))(*[P(t) for t in tb])
        ok(lib.buctd_fuse_sum(arr, (C.c_int * len(tb))(*shifts), len(tb), N, H, W, Cn, relu, P(out), stream()), "fuse_sum")
        return {"out": out}
    got = both(dev, run, f"fuse_sum {case}")
    ref = S.fuse_sum_ref(terms, shifts, relu)
    ref32 = S.fuse_sum_ref(terms, shifts, relu, torch.float32)
    mag = sum(S.nearest_up(t.double().abs(), s) for t, s in zip(terms, shifts))
    measured("fuse_sum", got["out"], ref, ref32, mag, case)
    if len(shifts) <= 2:
        exact("fuse_sum (<= 2 terms)", got["out"], ref32, case)
    if 0 in shifts:
        o2 = ops.fuse_sum([t.to(dev) for t in terms], list(shifts), bool(relu))
        assert torch.equal(o2.cpu(), got["out"]), "ops.fuse_sum: other bits"


@pytest.mark.parametrize("case", S.FUSE_SUM_BWD, ids=str)
def test_fuse_sum_bwd(dev, case):
    lib, _C, ops = lib_ops()
    N, H, W, Cn, s, with_y = case
    g = S.case_gen("fuse_sum_bwd", case)
    dy = torch.randn(N, H, W, Cn, generator=g)
    y = torch.relu(torch.randn(N, H, W, Cn, generator=g)) if with_y else None

    def run(mem):
        out = mem.new((N, H >> s, W >> s, Cn), "the gradient")
        ok(lib.buctd_fuse_sum_bwd(P(mem.ro(dy)), P(mem.ro(y)), s, N, H, W, Cn, P(out), stream()), "fuse_sum_bwd")
        return {"g": out}
    got = both(dev, run, f"fuse_sum_bwd {case}")
    ref, mag = S.fuse_sum_bwd_ref(dy, y, s)
    ref32, _ = S.fuse_sum_bwd_ref(dy, y, s, torch.float32)
    measured("fuse_sum_bwd", got["g"], ref, ref32, mag.clamp_min(1e-30), case)
    if s == 0:
        exact("fuse_sum_bwd shift 0", got["g"], ref32, case)
    assert torch.equal(ops.fuse_sum_bwd(dy.to(dev), None if y is None else y.to(dev), s).cpu(), got["g"])


@pytest.mark.parametrize("case", S.COPY_CHANNELS, ids=str)
def test_copy_channels(dev, case):
    lib, _C, ops = lib_ops()
    rows, Cs, cs0, Cd, cd0, Cc = case
    g = S.case_gen("copy_channels", case)
    src, dst0 = torch.randn(rows, Cs, generator=g), torch.randn(rows, Cd, generator=g)

    def run(mem):
        dst = mem.out(dst0, "dst")
        ok(lib.buctd_copy_channels(P(mem.ro(src)), rows, Cs, cs0, P(dst), Cd, cd0, Cc, stream()), "copy_channels")
        return {"dst": dst}
    got = both(dev, run, f"copy_channels {case}")
    ref = dst0.clone()
    ref[:, cd0:cd0 + Cc] = src[:, cs0:cs0 + Cc]
    exact("copy_channels", got["dst"], ref, case)


@pytest.mark.parametrize("case", S.ADD_BCAST, ids=str)
def test_add_bcast(dev, case):
    lib, _C, ops = lib_ops()
    batch, n = case
    g = S.case_gen("add_bcast", case)
    a, v = torch.randn(batch, n, generator=g), torch.randn(n, generator=g)

    def run(mem):
        out = mem.new((batch, n), "out")
        ok(lib.buctd_add_bcast(P(mem.ro(a)), P(mem.ro(v)), P(out), batch, n, stream()), "add_bcast")
        return {"out": out}
    exact("add_bcast", both(dev, run, f"add_bcast {case}")["out"], a + v, case)


@pytest.mark.parametrize("case", S.TRANSPOSE, ids=str)
def test_layout_transposes(dev, case):
    lib, _C, ops = lib_ops()
    N, Ct, c0, Cc, H, W = case
    g = S.case_gen("transpose", case)
    x = torch.randn(N, Ct, H, W, generator=g)
    xh = torch.randn(N, H, W, Cc, generator=g)

    def run(mem):
        y, back = mem.new((N, H, W, Cc), "the NHWC output"), mem.new((N, Cc, H, W), "the NCHW output")
        ok(lib.buctd_nchw_to_nhwc(P(mem.ro(x)), N, Ct, c0, Cc, H, W, P(y), stream()), "nchw_to_nhwc")
        ok(lib.buctd_nhwc_to_nchw(P(mem.ro(xh)), N, Cc, H, W, P(back), stream()), "nhwc_to_nchw")
        return {"y": y, "back": back}
    got = both(dev, run, f"transposes {case}")
    exact("nchw_to_nhwc", got["y"], x[:, c0:c0 + Cc].permute(0, 2, 3, 1).contiguous(), case)
    exact("nhwc_to_nchw", got["back"], xh.permute(0, 3, 1, 2).contiguous(), case)
    assert torch.equal(ops.nchw_to_nhwc(x.to(dev), c0, Cc).cpu(), got["y"]) and torch.equal(ops.nhwc_to_nchw(xh.to(dev)).cpu(), got["back"])


@pytest.mark.parametrize("case", S.RESIZE, ids=str)
def test_resize_bilinear(dev, case):
    lib, _C, ops = lib_ops()
    N, Ct, c0, Cc, H, W, Ho, Wo = case
    g = S.case_gen("resize", case)
    x = torch.randn(N, Ct, H, W, generator=g)

    def run(mem):
        y = mem.new((N, Ho, Wo, Cc), "y")
        ok(lib.buctd_resize_bilinear(P(mem.ro(x)), N, Ct, c0, Cc, H, W, Ho, Wo, P(y), stream()), "resize_bilinear")
        return {"y": y}
    got = both(dev, run, f"resize {case}")
    ref, mag = S.resize_ref(x, c0, Cc, Ho, Wo)
    ref32, _ = S.resize_ref(x, c0, Cc, Ho, Wo, torch.float32)
    # the weights themselves carry the rounding of the source coordinate: the error is taken relative to the sum of
    # |weight x value| plus the largest neighbour value (a coordinate off by one ulp moves weight between neighbours)
    measured("resize_bilinear", got["y"], ref, ref32, mag + x[:, c0:c0 + Cc].abs().max().item(), case)
    assert torch.equal(ops.resize_bilinear_from_nchw(x.to(dev), c0, Cc, Ho, Wo).cpu(), got["y"])


@pytest.mark.parametrize("case", S.MAXPOOL, ids=str)
def test_maxpool(dev, case):
    lib, _C, ops = lib_ops()
    N, H, W, Cn, ties = case
    g = S.case_gen("maxpool", case)
    x = torch.randn(N, H, W, Cn, generator=g)
    if ties:
        x = torch.round(x)                                  # a handful of levels: most windows hold their maximum twice
    Ho, Wo = S.pool_out(H), S.pool_out(W)
    dy = torch.randn(N, Ho, Wo, Cn, generator=g)

    def run(mem):
        y, idx = mem.new((N, Ho, Wo, Cn), "y"), mem.new((N, Ho, Wo, Cn), "idx", torch.int32)
        ok(lib.buctd_maxpool3x3s2_fwd(P(mem.ro(x)), N, H, W, Cn, P(y), P(idx), stream()), "maxpool_fwd")
        dx = mem.new((N, H, W, Cn), "dx")
        ok(lib.buctd_maxpool3x3s2_bwd(P(mem.ro(dy)), P(idx), N, H, W, Cn, P(dx), stream()), "maxpool_bwd")
        return {"y": y, "idx": idx, "dx": dx}
    got = both(dev, run, f"maxpool {case}")
    y, idx = S.maxpool_ref(x)
    exact("maxpool y", got["y"], y, case)
    exact("maxpool idx", got["idx"], idx, case)
    dx64, hits = S.maxpool_bwd_ref(dy, idx, (N, H, W, Cn))
    single = hits <= 1
    assert torch.equal(got["dx"][single], dx64.float()[single]), f"maxpool_bwd {case}: an input named by one output is not exact"
    mag, _ = S.maxpool_bwd_ref(dy.abs(), idx, (N, H, W, Cn))
    reduction("maxpool dx (shared argmax)", got["dx"], dx64, mag.clamp_min(1e-30), 4, case)
