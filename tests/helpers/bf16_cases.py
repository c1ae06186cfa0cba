"""Cases, code paths and fp64 references for the kernels of the bf16 inference mode: csrc/conv_bf16.hip, reached through
buctd_bf16_conv, buctd_bf16_pack_conv, buctd_bf16_fuse_sum and buctd_bf16_from_f32.  CPU only: the case tables are plain
tuples, path_of() restates the dispatch conditions of the host functions (conv_bf16.hip:line next to each), the references
are explicit float64 formulas on the bf16-rounded operands.  tests/test_bf16_cases_cover.py checks the tables against PATHS,
tests/test_gpu_bf16_kernels.py runs them.

Bars (none taken from the kernels):
  conv      |err| <= (Kt + 8) 2^-24 (sum |x||w| + |bias| + |res|)  (+ 2^-8 |ref| for a bf16 output).  Every product of two
            bf16 numbers is exact in fp32, so only the additions round: Kt of them in sequence is the worst case of any
            accumulation order of the MFMA; the 8 is the project's allowance for the bias, the residual and the stored roundings.
  integers  x, w in [-4, 4], bias in [-16, 16], residual in [-8, 8]: every partial sum is an integer below 2^24 (Kt <= 3456:
            3456 * 16 + 24 < 2^16), exact in fp32 in any order -> the fp32 output is bit-equal, the bf16 one is one rounding.
  fuse      (nterms + 1) 2^-24 sum |terms| + 2^-8 |ref|
  pack, from_f32   bit-equal

fp64 reference of the largest conv case on the CPU (16 threads): LARGEST_REF_SECONDS, next to the table.
"""
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
U32 = 2.0 ** -24               # unit round-off of fp32
U16 = 2.0 ** -8                # the issue's bf16 store term

# ---- constants of the host functions, restated ------------------------------------------------------------------------------
KSTEP = 32                     # conv_bf16.hip:113 (one 16x16x32 MFMA per K step), :198
MIN_BLOCKS = 1024              # conv_bf16.hip:168, :170 (4 blocks per CU, 256 CUs)
PACK_GRID_CAP = 4096           # conv_bf16.hip:248
FUSE_GRID_CAP = 8192           # conv_bf16.hip:304
CVT_GRID_CAP = 4096            # conv_bf16.hip:319
FUSE_MAX_TERMS, FUSE_MAX_SHIFT = 4, 5      # conv_bf16.hip:290, :298


def ceil_div(a, b):
    return -(-a // b)


def conv_out(n, R, stride, pad):           # conv_bf16.hip:194-195
    return (n + 2 * pad - R) // stride + 1


def conv_geom(case):
    """-> M, Ho, Wo, Kt, Kp of a conv case"""
    R, stride, pad, Ci, Co, N, H, W = case[:8]
    Ho, Wo = conv_out(H, R, stride, pad), conv_out(W, R, stride, pad)
    Kt = R * R * Ci                        # conv_bf16.hip:197
    return N * Ho * Wo, Ho, Wo, Kt, ceil_div(Kt, KSTEP) * KSTEP         # :198


def conv_nt(Co):                           # conv_bf16.hip:203-208
    return 2 if Co <= 32 else 3 if (Co % 64 != 0 and Co % 48 == 0) else 4


def conv_mt(M, Co):                        # conv_bf16.hip:167-173
    nN = ceil_div(Co, conv_nt(Co) * 16)
    if ceil_div(M, 256) * nN >= MIN_BLOCKS:
        return 4
    if ceil_div(M, 128) * nN >= MIN_BLOCKS:
        return 2
    return 1


def conv_vec(Ci):                          # conv_bf16.hip:158
    return Ci % 8 == 0


def conv_instance(case):
    M = conv_geom(case)[0]
    return conv_mt(M, case[4]), conv_nt(case[4]), conv_vec(case[3])


def image_k(Ci, R):                        # conv_bf16.hip:246 (the pack kernel's Kp, the same rule as :198)
    return ceil_div(R * R * Ci, KSTEP) * KSTEP


def grid_trips(items, cap):
    """trips of the busiest thread of a grid-stride loop over `items` work items: conv_bf16.hip:223, :266, :314"""
    return ceil_div(items, min(cap, ceil_div(items, 256)) * 256)


# ---- case tables ------------------------------------------------------------------------------------------------------------
# conv: (R, stride, pad, Ci, Co, N, H, W, residual, relu, fp32 NCHW head)
# MT = 1: small maps, one case per edge of the entry point's arguments
CONV_SMALL = [
    (3, 1, 1, 8, 32, 1, 7, 5, 1, 1, 0),        # NT 2; four taps per K step; Kt = 72 padded to 96; the block's 4th wave idle
    (3, 1, 0, 16, 48, 2, 9, 8, 0, 0, 0),       # NT 3; pad 0 with R = 3; two blocks of pixels
    (3, 2, 2, 24, 80, 1, 10, 9, 1, 1, 0),      # NT 4 with an idle channel tile; pad 2; a K step covers 1 1/3 taps
    (1, 1, 0, 8, 20, 1, 5, 3, 0, 1, 0),        # Kp = 32: no prefetch; ragged Co with the bf16 store; M = 15 < one tile
    (3, 1, 1, 40, 100, 1, 6, 5, 1, 0, 0),      # Ci = 40: K steps straddle taps; Co = 100 ragged, two channel blocks
    (3, 1, 1, 32, 64, 1, 8, 8, 0, 1, 0),       # everything whole: M = 64, Co = 64, Kt = 288
    (1, 1, 0, 32, 17, 2, 6, 5, 0, 0, 1),       # fp32 head, ragged Co, batch 2 (the NCHW index), Kp = Kt = 32
    (3, 1, 1, 64, 96, 1, 12, 9, 0, 1, 1),      # fp32 head, NT 3
    (1, 2, 0, 64, 256, 1, 9, 7, 1, 1, 0),      # 1x1 stride 2
    (3, 1, 1, 384, 48, 1, 4, 3, 0, 0, 0),      # the longest K of the networks (3456)
    (3, 2, 0, 72, 144, 3, 9, 11, 0, 1, 0),     # stride 2 without padding, Ci = 72
    (3, 2, 1, 3, 16, 2, 11, 9, 0, 1, 0),       # gather, the stem's Ci = 3; NT 2 with an idle channel tile
    (3, 1, 1, 5, 48, 1, 6, 7, 1, 0, 0),        # gather NT 3, Ci = 5
    (3, 1, 0, 17, 64, 1, 7, 6, 0, 1, 0),       # gather NT 4, Ci = 17
    (3, 1, 2, 37, 33, 1, 5, 4, 1, 1, 0),       # gather Ci >= 32, pad 2, ragged Co
    (1, 1, 0, 1, 3, 1, 4, 4, 0, 0, 1),         # gather Ci = 1, fp32 head
    (1, 2, 0, 44, 48, 2, 7, 9, 0, 1, 0),       # gather Ci = 44 (a multiple of 4, not of 8), 1x1 stride 2
    (3, 1, 1, 3, 70, 1, 13, 11, 0, 0, 1),      # gather, fp32 head, three pixel blocks and two channel blocks
]
# MT = 2 / 4: the smallest M that meets the block threshold of the instance's nN, with Ci = 8 / 16 (vector) or <= 17 (gather).
# pad = R // 2 throughout: tests/test_gpu_bf16_inference.py runs the same shapes through ops_bf16.conv
CONV_LARGE = [
    (1, 1, 0, 8, 512, 1, 181, 180, 0, 1, 0),       # MT4-NT4-vec     nN 8, M 32,580 >= 32,513
    (3, 2, 1, 8, 512, 1, 257, 253, 1, 1, 0),       # MT2-NT4-vec     nN 8, M 16,383 >= 16,257
    (3, 1, 1, 3, 512, 1, 181, 180, 0, 1, 0),       # MT4-NT4-gather
    (1, 2, 0, 5, 512, 1, 257, 253, 1, 0, 0),       # MT2-NT4-gather
    (1, 1, 0, 16, 336, 3, 113, 111, 0, 0, 0),      # MT4-NT3-vec     nN 7, M 37,629 >= 37,377
    (3, 1, 1, 8, 336, 2, 97, 98, 1, 1, 0),         # MT2-NT3-vec     nN 7, M 19,012 >= 18,689
    (3, 1, 1, 1, 336, 1, 194, 193, 1, 1, 0),       # MT4-NT3-gather
    (3, 2, 1, 17, 336, 1, 279, 273, 0, 0, 0),      # MT2-NT3-gather
    (1, 1, 0, 8, 24, 2, 362, 362, 1, 1, 0),        # MT4-NT2-vec     nN 1, M 262,088 >= 261,889
    (3, 2, 1, 8, 32, 1, 725, 723, 0, 1, 0),        # MT2-NT2-vec     nN 1, M 131,406 >= 130,945
    (3, 1, 1, 3, 12, 1, 512, 512, 0, 1, 1),        # MT4-NT2-gather  fp32 head
    (3, 2, 1, 3, 32, 1, 725, 723, 1, 0, 0),        # MT2-NT2-gather
]
CONV = CONV_SMALL + CONV_LARGE
CONV_MAX_MACS = 2e9            # M * Co * Kt of any case
CONV_MAX_BYTES = 512e6
# F.conv2d in float64 of the case with the most multiply-adds ((3, 2, 1, 17, 336, 1, 279, 273, ...): 9.9e8), measured once on
# a 16-thread CPU: reference plus magnitude convolution together.  The slowest case, (3, 1, 1, 1, 336, 1, 194, 193, ...) with
# its 12.6 M outputs, took 0.21 s; all 30 cases together, operands and integer references included, 4.0 s
LARGEST_REF_SECONDS = 0.04

# K padding must read no activation (conv_bf16.hip:77 `kv`, :98 `k < a.Kt`): cases with Kt % 32 != 0 for the poisoned-pixel test
CONV_POISON = [(3, 1, 1, 8, 32, 1, 9, 6, 0, 0, 0), (1, 1, 0, 8, 16, 1, 6, 4, 0, 0, 1), (3, 1, 1, 3, 32, 1, 9, 6, 0, 0, 0),
               (3, 2, 0, 24, 48, 1, 11, 7, 0, 0, 0)]

# pack: (Ci, Co, R, conv bias, BatchNorm, channels-last weight)
PACK = [(384, 384, 3, 0, 1, 0), (24, 40, 3, 1, 1, 1), (8, 16, 1, 1, 0, 0), (5, 7, 3, 0, 0, 1), (32, 33, 1, 0, 1, 1),
        (3, 64, 3, 1, 1, 0)]
# fuse: (N, H, W, C, shifts, relu)
FUSE_LONG = (1, 128, 128, 1032, (1, 2), 1)         # 16,384 pixels x 129 pieces of 8 channels > 8192 x 256
FUSE = [(2, 8, 16, 8, (0,), 0), (1, 8, 12, 24, (1, 0), 1), (2, 8, 8, 16, (0, 3, 2), 0), (1, 16, 8, 8, (3, 2, 1, 0), 1),
        (1, 32, 64, 8, (0, 4, 5), 0), (1, 32, 32, 40, (5, 0, 4, 1), 1), FUSE_LONG]
# from_f32: element counts, or "specials" for the table of bit patterns
CVT_LONG = CVT_GRID_CAP * 256 + 256 + 3
FROM_F32 = [1, 7, 255, 256, 1027, CVT_LONG, "specials"]


# ---- paths ------------------------------------------------------------------------------------------------------------------
def inst_name(mt, nt, vec):
    return "inst:MT%d-NT%d-%s" % (mt, nt, "vec" if vec else "gather")


def path_of(kernel, case):
    """-> the set of path names `case` takes through `kernel` (every name is listed in PATHS[kernel])"""
    if kernel == "conv":
        R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
        assert R in (1, 3) and stride in (1, 2) and 0 <= pad < R and not (res and head)      # conv_bf16.hip:183-186
        M, Ho, Wo, Kt, Kp = conv_geom(case)
        assert Ho > 0 and Wo > 0                                                              # :196
        mt, nt, vec = conv_instance(case)
        names = {inst_name(mt, nt, vec), "R:%d" % R, "stride:%d" % stride, "pad:%d" % pad, "res:%d" % res, "relu:%d" % relu,
                 "out:f32-nchw" if head else "out:bf16-nhwc"}                                 # :146-151
        tiles = ceil_div(Co, 16)
        if Co % 16:
            names.add("co:ragged16")                         # :135 `co >= a.Co`, :67 the re-read of row Co - 1
        if tiles % nt:
            names.add("co:idle-tile")                        # a whole 16-column tile of the last block is past Co
        if Co % 16 == 0 and tiles % nt == 0:
            names.add("co:full")
        if ceil_div(Co, nt * 16) > 1:
            names.add("co:blocks>1")                         # :45 blockIdx.y
        mtiles = ceil_div(M, 16)
        if M % 16:
            names.add("m:ragged16")                          # :55 `mv`, :142
        if ceil_div(mtiles, mt) % 4:
            names.add("m:idle-wave")                         # :44: a wave of the last block has m0 >= M
        if mtiles % mt:
            names.add("m:idle-tile")                         # a whole 16-row tile of the last wave is past M (MT > 1)
        if M % (64 * mt) == 0:
            names.add("m:full")
        if ceil_div(M, 64 * mt) > 1:
            names.add("m:blocks>1")                          # :43 blockIdx.x
        # :71, :87-88: how the (tap, channel) cursor of a lane moves over a K step of 32
        names.add("ci:taps-per-step>1" if Ci < 32 else "ci:32-multiple" if Ci % 32 == 0 else "ci:step-straddles-tap")
        names.add("k:padded" if Kt % KSTEP else "k:whole")   # :77, :98
        if Kp == KSTEP:
            names.add("k:single-step")                       # :115-116: `more` is never true, nothing is prefetched
        if not vec:
            names.add("gather:ci<8" if Ci < 8 else "gather:ci>=32" if Ci >= 32 else "gather:ci8..31")
        return names
    if kernel == "pack":
        Ci, Co, R, cbias, bn, cl = case
        Kt, Kp = R * R * Ci, image_k(Ci, R)
        names = {"bn:%d" % bn, "bias:%d" % cbias, "strides:channels-last" if cl else "strides:contiguous",
                 "k:padded" if Kt % KSTEP else "k:whole"}
        names.add("pack:second-trip" if grid_trips(Co * Kp, PACK_GRID_CAP) > 1 else "pack:one-trip")
        return names
    if kernel == "fuse":
        N, H, W, C, shifts, relu = case
        assert C % 8 == 0 and 1 <= len(shifts) <= FUSE_MAX_TERMS                              # :290-291
        assert all(0 <= s <= FUSE_MAX_SHIFT and H % (1 << s) == 0 and W % (1 << s) == 0 for s in shifts)    # :298-300
        names = {"fuse:terms-%d" % len(shifts), "relu:%d" % relu} | {"fuse:shift-%d" % s for s in shifts}
        names.add("fuse:second-trip" if grid_trips(N * H * W * C // 8, FUSE_GRID_CAP) > 1 else "fuse:one-trip")
        return names
    if kernel == "from_f32":
        if case == "specials":
            return {"cvt:specials", "cvt:one-trip"}
        return {"cvt:second-trip" if grid_trips(case, CVT_GRID_CAP) > 1 else "cvt:one-trip"}
    raise KeyError(kernel)


TABLES = {"conv": CONV, "pack": PACK, "fuse": FUSE, "from_f32": FROM_F32}

PATHS = {
    "conv": [inst_name(mt, nt, vec) for mt in (1, 2, 4) for nt in (2, 3, 4) for vec in (True, False)] + [
        "R:1", "R:3", "stride:1", "stride:2", "pad:0", "pad:1", "pad:2", "res:0", "res:1", "relu:0", "relu:1",
        "out:bf16-nhwc", "out:f32-nchw", "co:ragged16", "co:idle-tile", "co:full", "co:blocks>1", "m:ragged16", "m:idle-wave",
        "m:idle-tile", "m:full", "m:blocks>1", "ci:taps-per-step>1", "ci:step-straddles-tap", "ci:32-multiple", "k:padded",
        "k:whole", "k:single-step", "gather:ci<8", "gather:ci8..31", "gather:ci>=32"],
    "pack": ["bn:0", "bn:1", "bias:0", "bias:1", "strides:contiguous", "strides:channels-last", "k:padded", "k:whole",
             "pack:one-trip", "pack:second-trip"],
    "fuse": ["fuse:terms-1", "fuse:terms-2", "fuse:terms-3", "fuse:terms-4", "fuse:shift-0", "fuse:shift-1", "fuse:shift-2",
             "fuse:shift-3", "fuse:shift-4", "fuse:shift-5", "relu:0", "relu:1", "fuse:one-trip", "fuse:second-trip"],
    "from_f32": ["cvt:one-trip", "cvt:second-trip", "cvt:specials"],
}

# the cases that exist to reach a second loop trip: (kernel, case filter, path name)
SECOND_TRIPS = [
    ("pack", lambda c: c[:3] == (384, 384, 3), "pack:second-trip"),
    ("fuse", lambda c: c == FUSE_LONG, "fuse:second-trip"),
    ("from_f32", lambda c: c == CVT_LONG, "cvt:second-trip"),
]


def conv_macs(case):
    M, _, _, Kt, _ = conv_geom(case)
    return M * case[4] * Kt


def case_bytes(kernel, case):
    """bytes of all operands and outputs of the plain and the banded call and of the references kept for the comparison;
    temporaries of the reference formulas are not counted"""
    h, f, d = 2, 4, 8
    if kernel == "conv":
        R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
        M, _, _, _, Kp = conv_geom(case)
        dev = N * H * W * Ci * h + Co * Kp * h + Co * f + (M * Co * h if res else 0) + M * Co * (f if head else h)
        return 2 * dev + M * Co * 3 * d                      # reference, magnitude, the result as fp64
    if kernel == "pack":
        Ci, Co, R = case[:3]
        return 2 * (Co * Ci * R * R * f + Co * image_k(Ci, R) * h) + Co * image_k(Ci, R) * h + 12 * Co * f
    if kernel == "fuse":
        N, H, W, C, shifts, relu = case
        n = N * H * W * C
        terms = sum(n >> (2 * s) for s in shifts)
        return 2 * (terms + n) * h + n * 3 * d
    if kernel == "from_f32":
        n = 64 if case == "specials" else case
        return 2 * n * (f + h) + n * h
    raise KeyError(kernel)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def case_gen(kernel, case):
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(kernel))

    def walk(c):
        nonlocal seed
        for k in c:
            if isinstance(k, (tuple, list)):
                walk(k)
            else:
                seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) & 0x7FFFFFFF
    walk(case if isinstance(case, (tuple, list)) else (case,))
    return torch.Generator().manual_seed(seed)


def conv_operands(case, kind):
    """-> x [N][H][W][Ci] bf16, w [Co][Ci][R][R] bf16, bias [Co] fp32, residual [N][Ho][Wo][Co] bf16 or None.
    kind "randn": unit normal activations, filters scaled to unit output variance; kind "int": small integers (see the
    module's bars: every partial sum is exact in fp32)"""
    R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
    M, Ho, Wo, Kt, _ = conv_geom(case)
    g = case_gen("conv-" + kind, case)
    if kind == "int":
        x = torch.randint(-4, 5, (N, H, W, Ci), generator=g).to(BF16)
        w = torch.randint(-4, 5, (Co, Ci, R, R), generator=g).to(BF16)
        bias = torch.randint(-16, 17, (Co,), generator=g).float()
        r = torch.randint(-8, 9, (N, Ho, Wo, Co), generator=g).to(BF16) if res else None
    else:
        x = torch.randn(N, H, W, Ci, generator=g).to(BF16)
        w = (torch.randn(Co, Ci, R, R, generator=g) / Kt ** 0.5).to(BF16)
        bias = torch.randn(Co, generator=g) * 0.1
        r = torch.randn(N, Ho, Wo, Co, generator=g).to(BF16) if res else None
    return x, w, bias, r


def filter_image(w):
    """[Co][Ci][R][R] bf16 -> the image [Co][Kp] of conv_bf16.hip:3-5: K = (r * R + s) * Ci + ci, zero from R*R*Ci to Kp"""
    Co, Ci, R, _ = w.shape
    img = torch.zeros(Co, image_k(Ci, R), dtype=w.dtype)
    img[:, :R * R * Ci] = w.permute(0, 2, 3, 1).reshape(Co, R * R * Ci)
    return img


# ---- fp64 references --------------------------------------------------------------------------------------------------------
def conv_ref(case, x, w, bias, r, magnitude=True):
    """-> reference and magnitude (sum |x||w| + |bias| + |res|), fp64, in the layout of the output: [N][Ho][Wo][Co], or
    [N][Co][Ho][Wo] for the fp32 head"""
    R, stride, pad, Ci, Co, N, H, W, res, relu, head = case
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(xd, wd, bias.double(), stride, pad)
    mag = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), stride, pad) if magnitude else None
    if r is not None:
        rd = r.double().permute(0, 3, 1, 2)
        ref = ref + rd
        mag = mag + rd.abs() if magnitude else None
    if relu:
        ref = ref.clamp_min(0)
    if not head:
        ref = ref.permute(0, 2, 3, 1).contiguous()
        mag = mag.permute(0, 2, 3, 1).contiguous() if magnitude else None
    return ref, mag


def conv_bar(case, ref, mag):
    Kt = conv_geom(case)[3]
    bar = (Kt + 8) * U32 * mag
    return bar if case[10] else bar + U16 * ref.abs()


def nearest_up(t, s):
    """[N, h, w, C] -> [N, h << s, w << s, C]: out[h][w] = t[h >> s][w >> s]"""
    f = 1 << s
    return t.repeat_interleave(f, 1).repeat_interleave(f, 2)


def fuse_operands(case):
    N, H, W, C, shifts, relu = case
    g = case_gen("fuse", case)
    return [torch.randn(N, H >> s, W >> s, C, generator=g).to(BF16) for s in shifts]


def fuse_ref(terms, shifts, relu):
    """-> reference, sum of |terms| (fp64)"""
    ref = mag = None
    for t, s in zip(terms, shifts):
        u = nearest_up(t.double(), s)
        ref = u if ref is None else ref + u
        mag = u.abs() if mag is None else mag + u.abs()
    return (ref.clamp_min(0) if relu else ref), mag


def fuse_bar(nterms, ref, mag):
    return (nterms + 1) * U32 * mag + U16 * ref.abs()


# fp32 bit patterns for buctd_bf16_from_f32.  A bf16 keeps the upper 16 bits; the lower 16 decide the rounding.
CVT_SPECIALS = [
    0x00000000, 0x80000000,                          # +-0
    0x3F800000, 0xBF800000,                          # +-1
    0x3F808000, 0xBF808000,                          # a tie above an even bf16: down to 0x3F80
    0x3F818000, 0xBF818000,                          # a tie above an odd bf16: up to 0x3F82
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # one bit either side of both ties
    0x3FFF8000, 0x3FFFFFFF,                          # the carry of the rounding runs into the exponent
    0x7F7F0000, 0x7F7F7FFF, 0xFF7F7FFF,              # the largest finite bf16, and the largest fp32 that still rounds to it
    0x7F7F8000, 0xFF7F8000, 0x7F7FFFFF, 0xFF7FFFFF,  # the first value that rounds to inf (a tie above an odd bf16), FLT_MAX
    0x7F800000, 0xFF800000,                          # +-inf
    0x00000001, 0x80000001, 0x00007FFF, 0x00008000,  # denormals that round to +-0 (the tie at 0x8000 goes to the even 0)
    0x00008001, 0x00010000, 0x80010000, 0x00018000,  # the smallest bf16 denormal, and a tie above it
    0x007FFFFF, 0x807FFFFF, 0x00800000,              # the largest denormal rounds up to the smallest normal
]
CVT_NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F810000, 0xFFA5A5A5]


def bits_to_f32(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def cvt_operand(case):
    """finite fp32 values over the whole exponent range (random bit patterns, NaN / inf exponents replaced)"""
    g = case_gen("from_f32", (case,))
    b = torch.randint(-(1 << 31), (1 << 31) - 1, (case,), generator=g, dtype=torch.int64).to(torch.int32)
    nonfinite = (b & 0x7F800000) == 0x7F800000
    return torch.where(nonfinite, b & ~0x40000000, b).view(torch.float32)
