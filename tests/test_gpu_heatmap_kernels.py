"""The kernels that open and close a training step and a validation batch - csrc/loss_decode.hip (joints MSE, arg-max decode
with and without the quarter offsets, Gaussian target, condition render, flip-back merge, Adam, SGD) and csrc/nms.hip -
against float64 / exact references, one parametrised test per kernel family, one case per code path
(tests/helpers/heatmap_cases.py names the paths; tests/test_heatmap_cases_cover.py shows that every path has a case and that
the references reproduce the goldens).

Every call runs twice through the C interface: once with each read-only operand between NaN bands and each output (and
workspace) between sentinel bands, once on plain tensors.  The bands must be intact, no NaN may be picked up and the two
results must be bit-equal; the ops.* wrapper (nms: nms.gpu_nms) must give the same bits again.

Bars (all against fp64, none taken from the kernels):
  bit-exact     arg-max index, preds, maxvals, quarter offsets, the pinned-host preds_out form against the device form;
                Gaussian-target weights (and zeros where nothing is painted); flipback_avg (one fp32 addition, an exact
                halving); adam_step with zero gradient and state; NMS keep list, count and the suppression words the sweep reads;
                sgd_step against the same formula in fp32 on the CPU in the kernel's order (the build uses -ffp-contract=off)
  reductions    MSE loss: |err| <= (n_seq + 8) 2^-24 sum |terms|, n_seq = ceil(HW / 256) + 19 (heatmap_cases.py)
  project bar   Gaussian-target values: 2e-7 absolute (test_gpu_ops.py)
  measured      MSE gradient (relative to each element), Adam m, v (relative to the largest element) and p (relative to
                |p| before + the updates so far) after one step and after three: the same formula in fp32 on the CPU is measured
                against fp64; bar = max(4 x that, 2^-23)
  cond_render   |err| <= 2 (cnt + 40) 2^-24 ref + 255 * 2^-23 (every term is non-negative; cnt = impulse pixels of the image);
                with truncate, trunc(ref) exactly wherever ref is further than that from a whole number, one off at most
                elsewhere

Worst figures of the MI355X run, per family: kernel error / bar [error of the fp32 CPU formula], case
  adam_step m after one step         3.412e-08 / 1.365e-07 [3.412e-08]  at (5, 1, 1.0, 'one')
  adam_step m after three steps      7.724e-08 / 3.089e-07 [7.724e-08]  at (1023, 1, 1.0, 'three')
  adam_step p after one step         1.078e-07 / 4.313e-07 [1.078e-07]  at (4, 1, 1.0, 'one')
  adam_step p after three steps      1.591e-07 / 6.365e-07 [1.591e-07]  at (1023, 1, 1.0, 'three')
  adam_step v after one step         3.316e-08 / 1.326e-07 [3.316e-08]  at (1, 1, 1.0, 'one')
  adam_step v after three steps      9.661e-08 / 3.864e-07 [9.661e-08]  at (1023, 1, 1.0, 'three')
  cond_render                        3.851e-02 / 1.000e+00  at (3, 9, 4, 64, 3, 0, 1)
  cond_render truncate (in the band) 1.000e+00 / 1.000e+00  at (2, 2, 3, 17, 3, 1, 0)
  gaussian_target                    3.001e-08 / 2.000e-07  at (5, 4, 4.0, 4.0, 3.0)
  joints_mse grad                    9.811e-08 / 3.924e-07 [9.811e-08]  at (2, 3, 1, 'w', 1, 1.0)
  joints_mse loss                    8.957e-08 / 1.729e-06  at (2, 3, 257, 'w', 1, 1.0)
  sgd_step buf against fp64          2.992e-08 / 1.197e-07 [2.992e-08]  at (1, 0.9, 0, 0.0001, 0, 1.0, 0)
  sgd_step p against fp64            3.834e-08 / 1.533e-07 [3.834e-08]  at (255, 0.0, 0, 0.0, 0, 1.0, 0)
bit-equal in every case: adam_step zero gradient and state: m, v, adam_step zero gradient and state: p, argmax idx, argmax
  idx (refined), argmax maxvals, argmax maxvals (refined), argmax preds, argmax preds (refined), argmax preds_out (pinned
  host), argmax quarter, flipback_avg, gaussian_target weight, nms keep list and count, nms mask words the sweep reads,
  sgd_step buf, sgd_step p
"""
import pytest
import torch

from tests.helpers import heatmap_cases as S
from tests.helpers.guard_bands import Bands

pytestmark = pytest.mark.gpu

WORST = {}
GAP_FILL = -777.25             # what the gaps between the images of buctd_cond_render_into hold before the call
CHUNK = 1 << 20                # elements of the optimizer vectors compared at a time


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst figures per family (kernel error / bar [fp32 CPU error], case):")
    for k in sorted(WORST):
        err, bar, e32, case = WORST[k]
        if bar > 0:
            print(f"  {k:34s} {err:.3e} / {bar:.3e}" + (f" [{e32:.3e}]" if e32 is not None else "") + f"  at {case}")
    print("bit-equal in every case: " + ", ".join(k for k in sorted(WORST) if WORST[k][1] == 0 and WORST[k][0] == 0))


def note(fam, err, bar, case, e32=None):
    err, bar = float(err), float(bar)
    if fam not in WORST or err / max(bar, 1e-300) > WORST[fam][0] / max(WORST[fam][1], 1e-300):
        WORST[fam] = (err, bar, e32, case)
    print(f"{fam} {case}: {err:.3e} / {bar:.3e}" + (f" [fp32 {e32:.3e}]" if e32 is not None else ""))
    return err <= bar


def measured(fam, err, e32, case):
    """the measured bar: the error of the kernel and of the fp32 CPU formula against fp64, on one scale"""
    bar = max(4 * e32, S.FLOOR)
    assert note(fam, err, bar, case, e32), f"{fam} {case}: error {err:.3e} > bar {bar:.3e} (fp32 CPU formula: {e32:.3e})"


def rel(x, ref64, scale):
    return ((x.double() - ref64).abs() / scale).max().item() if x.numel() else 0.0


def exact(fam, got, ref, case, rows=None):
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{fam} {case}: {got.dtype} {tuple(got.shape)}"
    same = torch.equal(got, ref)
    note(fam, 0.0 if same else 1.0, 0.0, case)
    if not same:
        bad = (got != ref).view(got.shape[0], -1).any(1).nonzero().view(-1).tolist()
        where = [f"{r} ({rows[r]})" for r in bad[:8]] if rows else bad[:8]
        raise AssertionError(f"{fam} {case}: not bit-equal, {(got != ref).sum().item()} of {got.numel()} elements differ; "
                             f"first rows: {where}; got {got.view(got.shape[0], -1)[bad[0]].tolist()[:4]} "
                             f"for {ref.view(ref.shape[0], -1)[bad[0]].tolist()[:4]}")


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


def P(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def stream():
    from buctd_amd import _C
    return _C.stream_ptr()


def D(t, dev):
    return None if t is None else t.to(dev)


# ---- joints MSE -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.MSE, ids=str)
def test_joints_mse(dev, case):
    lib, _C, ops = lib_ops()
    N, K, HW, wmode, want, gscale = case
    pred, gt, w = S.mse_operand(case)

    def run(mem):
        loss = mem.new((1,), "the loss")
        grad = mem.new((N, K, HW), "the gradient") if want else None
        ws = mem.new((N * K,), "the workspace")
        ok(lib.buctd_joints_mse(P(mem.ro(pred)), P(mem.ro(gt)), P(mem.ro(w)), N, K, HW, P(loss), P(grad), gscale, P(ws), N * K * 4,
                                stream()), "joints_mse")
        return {"loss": loss, "grad": grad}
    got = both(dev, run, f"joints_mse {case}")
    l2, g2 = ops.joints_mse(pred.to(dev), gt.to(dev), D(w, dev), bool(want), gscale)
    assert torch.equal(l2.cpu().view(1), got["loss"]), "ops.joints_mse: another loss"
    assert (g2 is None and got["grad"] is None) or torch.equal(g2.cpu(), got["grad"]), "ops.joints_mse: another gradient"
    loss64, grad64 = S.mse_ref(pred, gt, w, gscale)
    # every term is non-negative: the sum of |terms| is the loss itself
    ratio = abs(got["loss"].double().item() - loss64.item()) / loss64.item()
    bar = (S.mse_n_seq(case) + 8) * S.U
    assert note("joints_mse loss", ratio, bar, case), f"joints_mse {case}: loss off by {ratio:.3e} of it > {bar:.3e}"
    if want:
        grad32 = S.mse_ref(pred, gt, w, gscale, torch.float32)[1]
        scale = grad64.abs().clamp_min(1e-300)
        measured("joints_mse grad", rel(got["grad"], grad64, scale), rel(grad32, grad64, scale), case)
        if wmode == "zero-rows":
            assert not got["grad"][0].any() and not got["grad"][:, ::3].any(), "rows of zero weight have a zero gradient"
    t = torch.zeros(N * K * HW, device=dev)
    assert lib.buctd_joints_mse(P(t), P(t), None, N, K, HW, P(t), None, 1.0, P(t), N * K * 4 - 4, stream()) != 0, \
        "a workspace of N K - 1 floats is refused"


# ---- arg-max decode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ARGMAX, ids=str)
def test_argmax_decode_plain_and_refined(dev, case):
    lib, _C, ops = lib_ops()
    H, W, kind = case
    hm, names = S.argmax_operand(case)
    rows = hm.shape[0]

    def run(mem, refined, with_idx=True):
        h = mem.ro(hm)
        o = {"preds": mem.new((rows, 2), "preds"), "maxvals": mem.new((rows,), "maxvals"),
             "idx": mem.new((rows,), "idx", torch.int32) if with_idx else None}
        if refined:
            o["quarter"] = mem.new((rows, 2), "quarter")
            ok(lib.buctd_argmax_decode_refined(P(h), rows, H, W, P(o["preds"]), P(o["maxvals"]), P(o["idx"]), P(o["quarter"]),
                                               stream()), "argmax_decode_refined")
        else:
            ok(lib.buctd_argmax_decode(P(h), rows, H, W, P(o["preds"]), P(o["maxvals"]), P(o["idx"]), stream()), "argmax_decode")
        return o
    plain = both(dev, lambda mem: run(mem, False), f"argmax_decode {case}")
    fine = both(dev, lambda mem: run(mem, True), f"argmax_decode_refined {case}")
    noidx = both(dev, lambda mem: run(mem, True, False), f"argmax_decode_refined {case} idx = NULL")
    idx, preds, mx, quarter = S.argmax_ref(hm, H, W)
    for tag, r in (("", plain), (" (refined)", fine)):
        exact("argmax idx" + tag, r["idx"], idx, case, names)
        exact("argmax preds" + tag, r["preds"], preds, case, names)
        exact("argmax maxvals" + tag, r["maxvals"], mx, case, names)
    exact("argmax quarter", fine["quarter"], quarter, case, names)
    assert torch.equal(noidx["preds"], preds) and torch.equal(noidx["quarter"], quarter), "idx = NULL changes the result"
    # the wrapper: device form, and preds written straight into pinned host memory (core/function.py, core/inference.py)
    hd = hm.view(1, rows, H, W).to(dev)
    p, m, i = ops.argmax_decode(hd)
    assert torch.equal(p.cpu()[0], preds) and torch.equal(m.cpu().view(-1), mx) and torch.equal(i.cpu()[0], idx)
    p, m, i, q = ops.argmax_decode(hd, refine=True)
    assert torch.equal(p.cpu()[0], preds) and torch.equal(q.cpu()[0], quarter) and torch.equal(i.cpu()[0], idx)
    for refine in (False, True):
        pin = torch.full((1, rows, 2), -1.0).pin_memory()
        res = ops.argmax_decode(hd, refine=refine, preds_out=pin)
        torch.cuda.synchronize()
        assert res[0] is pin
        exact("argmax preds_out (pinned host)", pin[0], preds, case, names)
        assert torch.equal(res[1].cpu().view(-1), mx) and (not refine or torch.equal(res[3].cpu()[0], quarter))


# ---- Gaussian target --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.GAUSS, ids=str)
def test_gaussian_target(dev, case):
    lib, _C, ops = lib_ops()
    Hh, Wh, sx, sy, sigma = case
    joints, vis = S.gauss_operand(case)
    B, K = vis.shape
    what = [f"{j[0]} ({j[1]}, {j[2]}) vis {j[3]}" for j in S.gauss_joints(case)]

    def run(mem):
        target, weight = mem.new((B, K, Hh, Wh), "the target"), mem.new((B, K), "the weights")
        ok(lib.buctd_gaussian_target(P(mem.ro(joints)), P(mem.ro(vis)), B, K, Hh, Wh, sx, sy, sigma, P(target), P(weight), stream()),
           "gaussian_target")
        return {"target": target, "weight": weight}
    got = both(dev, run, f"gaussian_target {case}")
    t2, w2 = ops.gaussian_target(joints.to(dev), vis.to(dev), (Wh, Hh), (Wh * sx, Hh * sy), sigma)
    assert torch.equal(t2.cpu(), got["target"]) and torch.equal(w2.cpu().view(B, K), got["weight"]), "ops.gaussian_target: other bits"
    t64, w = S.gauss_ref(joints, vis, case)
    exact("gaussian_target weight", got["weight"].view(B * K, 1), w.view(B * K, 1), case, what)
    err = (got["target"].double() - t64).abs().view(B * K, -1).max(1).values
    k = int(err.argmax())
    assert note("gaussian_target", err[k].item(), 2e-7, case), f"gaussian_target {case}: {err[k].item():.3e} at joint {k}: {what[k]}"
    painted = (t64 != 0).view(B * K, -1)
    wrong = ((got["target"] != 0).view(B * K, -1) != painted).any(1).nonzero().view(-1).tolist()
    assert not wrong, f"gaussian_target {case}: other pixels painted for {[what[r] for r in wrong[:6]]}"


# ---- condition render -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.COND, ids=str)
def test_cond_render(dev, case):
    lib, _C, ops = lib_ops()
    H, W, Cc, K, js, trunc, into = case
    B = S.COND_B
    joints, colors = S.cond_operand(case), S.cond_colors(Cc, K)
    per = Cc * H * W
    stride = per + (S.COND_GAP if into else 0)
    need = lib.buctd_cond_render_workspace(B, Cc, H, W)
    assert need == (B * per + B) * 4

    def run(mem):
        out = mem.out(torch.full((B, stride), GAP_FILL), "the condition images")
        ws = mem.new((need // 4,), "the workspace")
        j, c = mem.ro(joints), mem.ro(colors)
        if into:
            ok(lib.buctd_cond_render_into(P(j), js, P(c), B, K, Cc, H, W, trunc, P(out), stride, P(ws), need, stream()), "cond_render_into")
        else:
            ok(lib.buctd_cond_render(P(j), js, P(c), B, K, Cc, H, W, trunc, P(out), P(ws), need, stream()), "cond_render")
        return {"cond": out}
    got = both(dev, run, f"cond_render {case}")["cond"]
    assert bool((got[:, per:] == GAP_FILL).all()), f"cond_render_into {case}: the gap between two images was written"
    img = got[:, :per].reshape(B, Cc, H, W)
    o2 = ops.cond_render(joints.to(dev), D(colors, dev), H, W, truncate=bool(trunc))
    assert torch.equal(o2.cpu(), img), "ops.cond_render: other bits"
    ref, cnt = S.cond_ref(joints, colors, case)
    bar = S.cond_bar(ref, cnt)
    assert not img[1].any(), "a member whose key points are all rejected is a zero image"
    assert bool(((ref == 0) == (img == 0)).all()) or trunc, f"cond_render {case}: zero and non-zero pixels differ"
    if not trunc:
        ratio = ((img.double() - ref).abs() / bar).max().item()
        assert note("cond_render", ratio, 1.0, case), f"cond_render {case}: {ratio:.3f} of 2 (cnt + 40) 2^-24 ref + 255 * 2^-23"
        return
    want = torch.trunc(ref)
    band = S.cond_band(ref, cnt)
    d = (img.double() - want).abs()
    assert bool((d[~band] == 0).all()), f"cond_render {case}: {int((d[~band] != 0).sum())} truncated pixels differ outside the band"
    assert note("cond_render truncate (in the band)", d.max().item(), 1.0, case), f"cond_render {case}: off by {d.max().item()}"
    print(f"cond_render {case}: {int(band.sum())} pixels in the band, {int((d != 0).sum())} of them one off")


def test_cond_render_refuses_65_key_points_without_a_launch(dev):
    lib, _C, ops = lib_ops()
    j = torch.full((1, 65, 2), 3.0, device=dev)
    out = torch.full((8 * 8 + 5,), GAP_FILL, device=dev)
    need = lib.buctd_cond_render_workspace(1, 1, 8, 8)
    ws = torch.full((need // 4,), GAP_FILL, device=dev)
    assert lib.buctd_cond_render(P(j), 2, None, 1, 65, 1, 8, 8, 0, P(out), P(ws), need, stream()) != 0
    assert b"K<=64" in lib.buctd_last_error()
    assert lib.buctd_cond_render_into(P(j), 2, None, 1, 64, 1, 8, 8, 0, P(out), 63, P(ws), need, stream()) != 0
    assert b"batch stride" in lib.buctd_last_error()
    assert lib.buctd_cond_render(P(j), 2, None, 1, 64, 1, 8, 8, 0, P(out), P(ws), need - 4, stream()) != 0
    with pytest.raises(_C.BuctdHipError, match="K<=64"):
        ops.cond_render(j, None, 8, 8)
    torch.cuda.synchronize()
    assert bool((out == GAP_FILL).all()) and bool((ws == GAP_FILL).all()), "a refused call wrote"


# ---- flip-back merge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.FLIP, ids=str)
def test_flipback_avg(dev, case):
    lib, _C, ops = lib_ops()
    N, K, H, W, kind, shift = case
    a, b = S.flip_operand(case)
    perm = S.flip_perm(K, kind)
    pt = torch.tensor(perm, dtype=torch.int32)

    def run(mem):
        out = mem.new((N, K, H, W), "the merged heat-maps")
        ok(lib.buctd_flipback_avg(P(mem.ro(a)), P(mem.ro(b)), P(mem.ro(pt)), N, K, H, W, shift, P(out), stream()), "flipback_avg")
        return {"out": out}
    got = both(dev, run, f"flipback_avg {case}")["out"]
    assert torch.equal(ops.flipback_avg(a.to(dev), b.to(dev), pt.to(dev), shift).cpu(), got), "ops.flipback_avg: other bits"
    exact("flipback_avg", got.view(N * K, -1), S.flip_ref(a, b, perm, shift).view(N * K, -1), case)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.ADAM, ids=str)
def test_adam_step(dev, case):
    lib, _C, ops = lib_ops()
    n, step0, gscale, mode = case
    p0, m0, v0, grads = S.adam_operand(case)
    lr, b1, b2, eps = S.ADAM_HYPER
    last = len(grads) - 1

    def run(mem, via_ops=False):
        p, m, v = mem.out(p0, "p"), mem.out(m0, "m"), mem.out(v0, "v")
        o = {}
        for k, g in enumerate(grads):
            gb = mem.ro(g)
            if via_ops:
                ops.adam_step(p, gb, m, v, lr, b1, b2, eps, step0 + k, gscale)
            else:
                ok(lib.buctd_adam_step(P(p), P(gb), P(m), P(v), n, lr, b1, b2, eps, step0 + k, gscale, stream()), "adam_step")
            if k == 0 and last > 0:
                o.update({"p1": p.clone(), "m1": m.clone(), "v1": v.clone()})
        o.update({"p": p, "m": m, "v": v})
        return o
    got = both(dev, run, f"adam_step {case}")
    again = run(Bands(dev, False), via_ops=True)
    for k, t in got.items():
        assert torch.equal(again[k].cpu(), t), f"ops.adam_step {case}: {k} differs"
    if mode == "zero":
        exact("adam_step zero gradient and state: p", got["p"].view(-1, 1), p0.view(-1, 1), case)
        exact("adam_step zero gradient and state: m, v", torch.stack([got["m"], got["v"]]), torch.zeros(2, n), case)
        return
    figs = {}
    for s in range(0, n, CHUNK):
        sl = slice(s, s + CHUNK)
        st64 = st32 = (p0[sl], m0[sl], v0[sl])
        moved = torch.zeros(st64[0].shape, dtype=torch.float64)
        for k, g in enumerate(grads):
            was = st64[0].double()
            st64 = S.adam_ref(st64[0], g[sl], st64[1], st64[2], step0 + k, gscale, torch.float64)
            st32 = S.adam_ref(st32[0], g[sl], st32[1], st32[2], step0 + k, gscale, torch.float32)
            moved = moved + (st64[0] - was).abs()
            for tag in ([""] if k == last else []) + (["1"] if k == 0 and last > 0 else []):
                # p is a difference: its error is taken relative to the sizes of its terms, |p| before and the updates so far
                scales = (p0[sl].double().abs() + moved, st64[1].abs().max().clamp_min(1e-300), st64[2].abs().max().clamp_min(1e-300))
                for name, r64, r32, sc in zip("pmv", st64, st32, scales):
                    f = figs.setdefault((name, tag), [0.0, 0.0])
                    f[0] = max(f[0], rel(got[name + tag][sl], r64, sc))
                    f[1] = max(f[1], rel(r32, r64, sc))
    for (name, tag), (err, e32) in sorted(figs.items()):
        steps = "one step" if (tag == "1" or last == 0) else "three steps"
        measured(f"adam_step {name} after {steps}", err, e32, case)


# ---- SGD --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.SGD, ids=str)
def test_sgd_step(dev, case):
    lib, _C, ops = lib_ops()
    n, mu, nesterov, wd, first, gscale, off = case
    p0, g0, buf0 = S.sgd_operand(case)
    lead = torch.full((off,), 7.5)

    def run(mem, via_ops=False):
        # the slice starts `off` elements into its allocation, as the runs of FusedSGD.step do in the arena: in bounds
        p, g = mem.out(torch.cat([lead, p0]), "p"), mem.ro(torch.cat([lead, g0]))
        buf = mem.out(torch.cat([lead, buf0]), "the momentum buffer") if mu != 0.0 else None
        if via_ops:
            ops.sgd_step(p[off:], g[off:], None if buf is None else buf[off:], S.SGD_LR, mu, wd, nesterov, first, gscale)
        else:
            ok(lib.buctd_sgd_step(P(p, off), P(g, off), P(buf, off), n, S.SGD_LR, mu, wd, nesterov, first, gscale, stream()), "sgd_step")
        return {"p": p, "buf": buf}
    got = both(dev, run, f"sgd_step {case}")
    again = run(Bands(dev, False), via_ops=True)
    assert torch.equal(again["p"].cpu(), got["p"]) and (mu == 0.0 or torch.equal(again["buf"].cpu(), got["buf"])), "ops.sgd_step: other bits"
    p32, b32 = S.sgd_ref(p0, g0, buf0, case, torch.float32)
    p64, b64 = S.sgd_ref(p0, g0, buf0, case, torch.float64)
    for name, g_, r32, r64 in (("p", got["p"], p32, p64), ("buf", got["buf"], b32, b64)):
        if g_ is None:
            assert r32 is None
            continue
        assert bool((g_[:off] == 7.5).all()), f"sgd_step {case}: the elements in front of the slice were written ({name})"
        exact("sgd_step " + name, g_[off:].view(-1, 1), r32.view(-1, 1), case)
        sc = r64.abs().max().clamp_min(1e-300)
        measured("sgd_step %s against fp64" % name, rel(g_[off:], r64, sc), rel(r32, r64, sc), case)
    assert lib.buctd_sgd_step(P(again["p"]), P(again["p"]), None, n, 0.1, 0.9, 0.0, 0, 0, 1.0, stream()) != 0, \
        "momentum without a buffer is refused"


# ---- NMS --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.NMS, ids=str)
def test_nms(dev, case):
    lib, _C, ops = lib_ops()
    import buctd_amd.nms.nms as pn
    n, dim, kind, thresh = case
    boxes = S.nms_boxes(case)
    want = S.nms_ref(boxes, thresh)
    need = lib.buctd_nms_workspace(n)
    assert need == n * S.ceil_div(n, 64) * 8

    def run(mem):
        keep, num = mem.new((n,), "keep", torch.int32), mem.new((1,), "the count", torch.int32)
        ws = mem.new((need // 4,), "the mask")
        ok(lib.buctd_nms(P(keep), P(num), P(mem.ro(boxes)), n, dim, thresh, P(ws), need, stream()), "nms")
        return {"keep": keep, "num": num, "mask": ws.view(torch.int64).view(n, -1)}
    got = both(dev, run, f"nms {case}")
    words, read = S.nms_mask_ref(boxes, thresh)
    exact("nms mask words the sweep reads", torch.where(read, got["mask"], torch.zeros_like(words)), words, case)
    k = got["num"].item()
    same = k == len(want) and got["keep"][:k].tolist() == want
    note("nms keep list and count", 0.0 if same else 1.0, 0.0, case)
    assert same, f"nms {case}: kept {k} boxes {got['keep'][:k].tolist()[:12]}..., the exact rule keeps {len(want)}: {want[:12]}..."
    assert bool((got["keep"][k:] == -7).all()), "entries behind the count were written"
    if dim == 5:
        assert pn.gpu_nms(boxes.numpy(), thresh, 0) == want, f"nms.gpu_nms {case}"
    t = boxes.to(dev)
    assert lib.buctd_nms(P(t), P(t), P(t), n, dim, thresh, P(t), need - 8, stream()) != 0, "a workspace one word short is refused"
