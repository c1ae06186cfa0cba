"""The kernels of the bf16 inference mode (csrc/conv_bf16.hip) against float64, one case per code path
(tests/helpers/bf16_cases.py names the paths; tests/test_bf16_cases_cover.py shows that every path - all 18
bf16_conv_kernel<MT, NT, VEC> instances among them - has a case).  The calls go through the C interface, so every tensor
can sit between guard bands.

Every call runs twice: once with each read-only operand between NaN bands and each output between sentinel bands, once
on plain tensors.  The bands must be intact, no NaN may be picked up and the two results must be bit-equal.

Bars (all against fp64 on the same bf16-rounded operands, none taken from the kernels; bf16_cases.py derives them):
  conv, random operands    |err| <= (Kt + 8) 2^-24 (sum |x||w| + |bias| + |res|), + 2^-8 |ref| for a bf16 output
  conv, integer operands   bit-equal: the fp32 head to the integer reference, the bf16 output to its one rounding
  conv, poisoned pixel     an inf activation reaches the outputs whose window holds it and no other (K padding reads nothing)
  from_f32, pack           bit-equal to torch's rounding / to the host fold of tests/test_gpu_bf16_inference.py
  fuse                     |err| <= (nterms + 1) 2^-24 sum |terms| + 2^-8 |ref|
  refusals                 -1 before any launch: no output byte changes, buctd_last_error names the reason

Worst error / bar of the MI355X run per instance, random operands.  With a bf16 output the 2^-8 |ref| of the one stored
rounding carries the bar, hence the figures just below 1; the fp32 head (MT4-NT2-gather) shows the accumulation alone, and
the integer operands are bit-equal in every case:
  MT1-NT2-vec 0.976  MT1-NT2-gather 0.959  MT1-NT3-vec 0.948  MT1-NT3-gather 0.958  MT1-NT4-vec 0.958  MT1-NT4-gather 0.919
  MT2-NT2-vec 0.993  MT2-NT2-gather 0.995  MT2-NT3-vec 0.993  MT2-NT3-gather 0.989  MT2-NT4-vec 0.993  MT2-NT4-gather 0.996
  MT4-NT2-vec 0.996  MT4-NT2-gather 0.055  MT4-NT3-vec 0.996  MT4-NT3-gather 0.996  MT4-NT4-vec 0.996  MT4-NT4-gather 0.995
  fuse 0.996

Mutations of conv_bf16.hip tried on a scratch copy: `c += 24` for `c += 32` (:87) fails every vector case of more than one K
step (12 of test_conv_matches_fp64, the first (3, 1, 1, 8, 32, 1, 7, 5, 1, 1, 0)); `kv = true` (:77) fails
test_conv_k_padding_reads_no_activation on its three vector cases and nothing else - with finite activations a padded K lane
only multiplies what it loaded by a zero of the filter image.  Dropping the min(..., Co - 1) of :67 changes no output (the
columns it re-reads are never stored, :135); its only effect is a load past the filter image, which no test here provokes.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import bf16_cases as B
from tests.helpers.guard_bands import BandsAny

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

WORST = {}          # conv instance -> (worst error / bar, case)
RAN = {}            # kernel -> worst error / bar


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error / bar per bf16_conv_kernel instance (random operands), case:")
    for mt in (1, 2, 4):
        for nt in (2, 3, 4):
            for vec in (True, False):
                name = B.inst_name(mt, nt, vec)
                ratio, case = WORST.get(name, (float("nan"), "did not run"))
                print(f"  {name:22s} {ratio:.3f}  at {case}")
    for k in sorted(RAN):
        print(f"  {k:22s} {RAN[k]:.3f}")


def lib():
    from buctd_amd import _C
    return _C.lib()


def ok(rc, what):
    from buctd_amd import _C
    _C.check(rc, what)


def stream():
    from buctd_amd import _C
    return _C.stream_ptr()


def P(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def both(dev, run, what, nan_ok=False):
    """run(mem) -> {name: device tensor}; between bands and plain: intact bands, no NaN, the same bits -> CPU tensors"""
    mem = BandsAny(dev, True)
    a = run(mem)
    torch.cuda.synchronize()
    mem.check(what)
    b = run(BandsAny(dev, False))
    torch.cuda.synchronize()
    out = {}
    for k, v in a.items():
        assert nan_ok or not bool(torch.isnan(v).any()), f"{what}: NaN in {k}"
        assert torch.equal(bits(v), bits(b[k])), f"{what}: {k} between guard bands differs from the plain call"
        out[k] = v.cpu()
    return out


# ---- convolution ----------------------------------------------------------------------------------------------------------------
def run_conv(mem, case, x, wimg, bias, r):
    R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
    M, Ho, Wo, _, _ = B.conv_geom(case)
    xd, wd, bd, rd = mem.ro(x), mem.ro(wimg), mem.ro(bias), mem.ro(r)
    y = mem.new((N, Co, Ho, Wo), "y", torch.float32) if head else mem.new((N, Ho, Wo, Co), "y", BF16)
    ok(lib().buctd_bf16_conv(P(xd), N, H, W, Ci, P(wd), P(bd), Co, R, stride, pad, P(rd), relu, head, P(y), None, 0, stream()),
       "bf16_conv")
    return {"y": y}


@pytest.mark.parametrize("case", B.CONV, ids=str)
def test_conv_matches_fp64(dev, case):
    head = case[10]
    inst = B.inst_name(*B.conv_instance(case))
    # random operands: the accumulation bar
    x, w, bias, r = B.conv_operands(case, "randn")
    got = both(dev, lambda mem: run_conv(mem, case, x, B.filter_image(w), bias, r), f"conv {case}")["y"]
    assert got.dtype == (torch.float32 if head else BF16)
    ref, mag = B.conv_ref(case, x, w, bias, r)
    assert got.shape == ref.shape
    err = (got.double() - ref).abs()
    del got
    ratio = float((err / B.conv_bar(case, ref, mag)).max())
    print(f"conv {inst} {case}: max |err| {float(err.max()):.3e}, worst error / bar {ratio:.3f}")
    if inst not in WORST or ratio > WORST[inst][0]:
        WORST[inst] = (ratio, case)
    del err, ref, mag
    # integer operands: exact whatever the order of the additions
    x, w, bias, r = B.conv_operands(case, "int")
    goti = both(dev, lambda mem: run_conv(mem, case, x, B.filter_image(w), bias, r), f"conv (integers) {case}")["y"]
    refi = B.conv_ref(case, x, w, bias, r, magnitude=False)[0].float()
    want = refi if head else refi.to(BF16)
    same = torch.equal(bits(goti), bits(want))
    assert same, (f"conv (integers) {inst} {case}: {int((bits(goti) != bits(want)).sum())} of {want.numel()} outputs differ, "
                  f"max |d| {float((goti.double() - want.double()).abs().max())}")
    assert ratio <= 1.0, f"conv {inst} {case}: error / bar {ratio:.3f}"


@pytest.mark.parametrize("case", B.CONV_POISON, ids=str)
def test_conv_k_padding_reads_no_activation(dev, case):
    """K lanes from Kt to Kp meet zeros of the filter image, but 0 * inf is NaN: the kernel must not load an activation for
    them (conv_bf16.hip:77, :98).  The last two rows of x are +inf: the taps from R*R on point below a window (r >= R), into
    those rows for the last output row whose window is clear of them.  Outputs whose window holds an inf are non-finite,
    every other output is within the bar of the reference computed with zeros in their place."""
    R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
    x, w, bias, r = B.conv_operands(case, "randn")
    hot = torch.zeros(N, H, W, 1)
    hot[:, H - 2:] = 1.0
    x0 = torch.where(hot.bool(), torch.zeros_like(x), x)
    xp = torch.where(hot.bool(), torch.full_like(x, float("inf")), x)
    w = torch.where(w == 0, torch.ones_like(w), w)       # no zero weight: every product with an inf is +-inf
    got = both(dev, lambda mem: run_conv(mem, case, xp, B.filter_image(w), bias, r), f"conv (inf pixel) {case}", nan_ok=True)["y"]
    ref, mag = B.conv_ref(case, x0, w, bias, r)
    touched = F.conv2d(hot.permute(0, 3, 1, 2).double(), torch.ones(1, 1, R, R, dtype=torch.float64), None, stride, pad) > 0
    touched = touched.expand(N, Co, *touched.shape[2:])
    if not head:
        touched = touched.permute(0, 2, 3, 1)
    assert bool(touched.any()) and not bool(touched.all())
    gd = got.double()
    assert not bool(torch.isfinite(gd[touched]).any()), "an output whose window holds an inf is finite"
    leaked = ~torch.isfinite(gd) & ~touched
    assert not bool(leaked.any()), f"{int(leaked.sum())} outputs whose windows hold no inf are not finite"
    err = torch.where(touched, torch.zeros_like(gd), (gd - ref).abs())
    assert bool((err <= B.conv_bar(case, ref, mag)).all())


# ---- fp32 -> bf16 ---------------------------------------------------------------------------------------------------------------
def run_cvt(mem, x):
    xd = mem.ro(x)
    y = mem.new(x.shape, "y", BF16)
    ok(lib().buctd_bf16_from_f32(P(xd), x.numel(), P(y), stream()), "bf16_from_f32")
    return {"y": y}


@pytest.mark.parametrize("case", B.FROM_F32, ids=str)
def test_from_f32_is_torch_rounding(dev, case):
    if case == "specials":
        x = B.bits_to_f32(B.CVT_SPECIALS)
    else:
        x = B.cvt_operand(case)
    assert bool(torch.isnan(x).sum() == 0)
    got = both(dev, lambda mem: run_cvt(mem, x), f"from_f32 {case}")["y"]
    want = x.to(BF16)
    assert torch.equal(bits(got), bits(want)), [(hex(b & 0xFFFFFFFF), hex(g & 0xFFFF), hex(t & 0xFFFF)) for b, g, t in zip(
        bits(x).tolist(), bits(got).tolist(), bits(want).tolist()) if g != t][:8]
    if case == "specials":
        # a NaN stays a NaN of its sign.  The kernel keeps the upper payload bits and sets the quiet bit (conv_bf16.hip:26);
        # torch writes the one pattern 0x7FC0 - so only NaN-ness and the sign bit are compared
        xn = B.bits_to_f32(B.CVT_NANS)
        gn = both(dev, lambda mem: run_cvt(mem, xn), "from_f32 NaNs", nan_ok=True)["y"]
        assert bool(torch.isnan(gn).all())
        assert torch.equal(bits(gn) < 0, bits(xn) < 0)


# ---- filter image ---------------------------------------------------------------------------------------------------------------
def run_pack(mem, case, w, cbias, bn, eps):
    Ci, Co, R, _, _, cl = case
    if cl:          # the channels-last storage [Co][R][R][Ci], read through its strides
        wd = mem.ro(w.permute(0, 2, 3, 1).contiguous())
        s = (R * R * Ci, 1, R * Ci, Ci)
    else:
        wd = mem.ro(w.contiguous())
        s = (Ci * R * R, R * R, R, 1)
    cb = mem.ro(cbias)
    g, b, rm, rv = (mem.ro(t) for t in bn) if bn is not None else (None,) * 4
    wimg = mem.new((Co, B.image_k(Ci, R)), "the filter image", BF16)
    bias = mem.new((Co,), "the folded bias", torch.float32)
    ok(lib().buctd_bf16_pack_conv(P(wd), s[0], s[1], s[2], s[3], Co, Ci, R, P(cb), P(g), P(b), P(rm), P(rv),
                                  eps, P(wimg), P(bias), stream()), "bf16_pack_conv")
    return {"wimg": wimg, "bias": bias}


@pytest.mark.parametrize("case", B.PACK, ids=str)
def test_pack_is_the_host_fold(dev, case):
    from tests.test_gpu_bf16_inference import _host_fold, _image_as_oihw, _random_conv_bn
    Ci, Co, R, cbias, bn, cl = case
    conv, b = _random_conv_bn(Ci, Co, R, 1, seed=Ci + 7 * Co + R, conv_bias=bool(cbias), bn=bool(bn))
    w_ref, b_ref = _host_fold(conv, b)
    w = conv.weight.detach()
    bnt = (b.weight.detach(), b.bias.detach(), b.running_mean, b.running_var) if b is not None else None
    eps = float(b.eps) if b is not None else 0.0
    got = both(dev, lambda mem: run_pack(mem, case, w, conv.bias.detach() if cbias else None, bnt, eps), f"pack {case}")
    img = got["wimg"]
    assert torch.equal(bits(_image_as_oihw(img, Ci, R).contiguous()), bits(w_ref.contiguous()))
    assert not bits(img[:, R * R * Ci:]).any(), "K padding of the image must be zero"
    assert torch.equal(got["bias"], b_ref)


# ---- fuse row -------------------------------------------------------------------------------------------------------------------
def run_fuse(mem, case, terms):
    N, H, W, Cn, shifts, relu = case
    td = [mem.ro(t) for t in terms]
    y = mem.new((N, H, W, Cn), "y", BF16)
    arr = (C.c_void_p * len(td))(*[t.data_ptr() for t in td])
    sh = (C.c_int * len(td))(*shifts)
    ok(lib().buctd_bf16_fuse_sum(arr, sh, len(td), N, H, W, Cn, relu, P(y), stream()), "bf16_fuse_sum")
    return {"y": y}


@pytest.mark.parametrize("case", B.FUSE, ids=str)
def test_fuse_matches_fp64(dev, case):
    shifts, relu = case[4], case[5]
    terms = B.fuse_operands(case)
    got = both(dev, lambda mem: run_fuse(mem, case, terms), f"fuse {case}")["y"]
    ref, mag = B.fuse_ref(terms, shifts, relu)
    err = (got.double() - ref).abs()
    ratio = float((err / B.fuse_bar(len(shifts), ref, mag).clamp_min(1e-300)).max())
    print(f"fuse {case}: max |err| {float(err.max()):.3e}, worst error / bar {ratio:.3f}")
    RAN["fuse"] = max(RAN.get("fuse", 0.0), ratio)
    assert ratio <= 1.0, f"fuse {case}: error / bar {ratio:.3f}"


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_alone(dev):
    L = lib()
    x = torch.zeros(1, 8, 8, 8, dtype=BF16, device=dev)
    wimg = torch.zeros(16, 5 * 5 * 8 + 24, dtype=BF16, device=dev)      # large enough for every refused form below
    bias = torch.zeros(16, device=dev)
    r = torch.zeros(1, 8, 8, 16, dtype=BF16, device=dev)
    y = torch.full((32768,), 7.0, device=dev)                           # larger than the output of any form below
    keep = y.clone()

    def conv(R, stride, pad, res=None, head=0):
        return L.buctd_bf16_conv(P(x), 1, 8, 8, 8, P(wimg), P(bias), 16, R, stride, pad, P(res), 1, head, P(y), None, 0, stream())

    def fuse(nterms, shifts, H=32, W=32, Cn=8):
        t = torch.zeros(1, H, W, 8, dtype=BF16, device=dev)
        arr = (C.c_void_p * nterms)(*[t.data_ptr()] * nterms)
        rc = L.buctd_bf16_fuse_sum(arr, (C.c_int * nterms)(*shifts), nterms, 1, H, W, Cn, 1, P(y), stream())
        torch.cuda.synchronize()
        return rc

    for what, call, reason in [
            ("R = 5", lambda: conv(5, 1, 2), b"R must be 1 or 3"),
            ("stride 3", lambda: conv(3, 3, 1), b"stride 1 or 2"),
            ("pad = R", lambda: conv(3, 1, 3), b"0 <= pad < R"),
            ("pad = R (1x1)", lambda: conv(1, 1, 1), b"0 <= pad < R"),
            ("residual with the fp32 head", lambda: conv(3, 1, 1, r, 1), b"no residual"),
            ("C % 8 != 0", lambda: fuse(1, [0], Cn=12), b"multiple of 8"),
            ("5 terms", lambda: fuse(5, [0] * 5), b"1..4 terms"),
            ("shift 6", lambda: fuse(2, [0, 6], H=64, W=64), b"bad term 1"),
            ("H not divisible by 2^shift", lambda: fuse(2, [0, 3], H=12, W=16), b"not divisible by 2^shift for term 1")]:
        rc = call()
        torch.cuda.synchronize()
        msg = L.buctd_last_error()
        assert rc == -1, f"{what}: returned {rc}"
        assert reason in msg, f"{what}: {msg}"
        assert torch.equal(y, keep), f"{what}: the refused call wrote to the output"
