"""The case table of the exact-fp32 thin-channel convolution tests (csrc/conv.hip: conv_fwd_thin_kernel,
conv_fwd_thin_px4_kernel, conv_dgrad_thin_kernel, conv_dgrad_thin_px4_kernel, conv_dgrad_thin_s2_kernel,
conv3x3_thin_in_fwd_kernel, conv3x3_thin_in_wgrad_kernel, conv_wgrad_thin_kernel, conv_wgrad_thin_rows_kernel), as data.

A case is (N, H, W, Ci, Co, k, stride, pad) of the FORWARD convolution, as in conv2d_cases.py.  Next to each case stands the
route buctd_conv2d_plan must report (and, for a weight gradient, its nsplit).  What the plan query does not say - which
template instance runs and which of its loops and ragged branches the case takes - is the INSTANCE KEY, which key() below
computes from the descriptor with the tile constants stated here once (test_conv_thin_plan_cover.py checks them against the
source text, and nsplit_of() against the library's own nsplit).

tests/test_conv_thin_plan_cover.py (host only) proves that every (direction, route, key) of the search grid below is the key
of a table case, and that no two cases share one: remove a case and its key is reported missing.
tests/test_gpu_conv_thin_routes.py runs every case against fp64.

Every case is the smallest shape that still has its property: a thin route needs N*H*W >= 4096 (N*Ho*Wo for the thin-input
routes), so most cases are one image of 70x61 - whose last 8-row tile has 6 rows and whose last 32-column tile has 29
columns, so that the four pixels of a px4 thread straddle W - or two of 37x59, for the image index; the loop cases use many
small images.  No tensor of a case exceeds 8M floats."""
from tests.helpers.conv2d_cases import BIAS, DGRAD, FWD, RELU, RESIDUAL, SCALE, STATS, WGRAD, case_id, desc, out_hw, plan  # noqa: F401

# the tile constants of conv.hip that the keys use
THIN_TH, THIN_TW = 8, 32        # one pixel per thread: 8 x 32 pixel tiles (forward 3, data gradient 4, weight gradient 2)
THIN4_T, THIN4_CH = 32, 8       # four pixels per thread: 32 x 32 pixel tiles, 8-channel chunks (forward 2)
THIN_SPLITS = 1024              # most workgroups (= slabs) of conv_wgrad_thin_kernel
THIN_IN_WG = 1024               # most workgroups (= slabs) of conv3x3_thin_in_wgrad_kernel
TR_W = 32                       # columns of a strip of conv_wgrad_thin_rows_kernel
CONSTANTS = ("THIN_TH", "THIN_TW", "THIN4_T", "THIN4_CH", "THIN_SPLITS", "THIN_IN_WG", "TR_W")

ROUTE_NAMES = {
    (FWD, 1): "px4, 4-channel pixels", (FWD, 2): "px4, 8-channel chunks", (FWD, 3): "one pixel per thread", (FWD, 4): "thin input",
    (DGRAD, 1): "stride 2", (DGRAD, 2): "px4 transposed", (DGRAD, 3): "px4", (DGRAD, 4): "one pixel per thread",
    (WGRAD, 1): "rolling rows", (WGRAD, 2): "tiles", (WGRAD, 3): "thin input",
}


def ceil_div(a, b):
    return -(-a // b)


def rows_geo(case):
    """(strips, segments, rows per segment) of conv_wgrad_thin_rows_kernel: thin_rows_geo of conv.hip"""
    N, H, W = case[:3]
    strips = ceil_div(W, TR_W)
    sg = max(1, min(ceil_div(768, N * strips), max(H // 16, 1)))
    rps = ceil_div(H, sg)
    return strips, ceil_div(H, rps), rps


def wgrad_tiles(case):
    N, H, W = case[:3]
    return N * ceil_div(H, THIN_TH) * ceil_div(W, THIN_TW)


def nsplit_of(case, route):
    """the slabs (= workgroups) of a thin weight gradient, from the constants above"""
    N = case[0]
    if route == 1:
        strips, segs, _ = rows_geo(case)
        return N * strips * segs
    if route == 2:
        return min(wgrad_tiles(case), THIN_SPLITS)
    assert route == 3
    return min(N * out_hw(case)[0], THIN_IN_WG)


def _chunks16(c):
    """('one' | 'several' 16-channel chunks, 'full' | 'partial' last chunk) of the one-pixel-per-thread kernels"""
    return ("several" if c > 16 else "one", "partial" if c % 16 else "full")


def _loop(n, cap):
    """a grid-stride loop over n items on min(n, cap) workgroups: every workgroup one item, or some of them more"""
    return "one pass" if n <= cap else "loop"


def key(case, direction, route, flags=0):
    """the instance key of a case on a thin route: what the plan query leaves open"""
    N, H, W, Ci, Co, k, s, p = case
    if direction == FWD:
        if route == 1:      # conv_fwd_thin_px4_kernel<7, Co, 4, false>: 16-byte staging at Ci = 4, scalar below
            return (f"CO={Co}", "16-byte staging" if Ci == 4 else "scalar staging")
        if route == 2:      # conv_fwd_thin_px4_kernel<7, Co, 8, false>
            return (f"CO={Co}", "one chunk" if Ci == THIN4_CH else "several chunks")
        if route == 3:      # conv_fwd_thin_kernel<7>: four accumulators of which Co are stored; qn < 4 in a partial chunk
            return ("Co=4" if Co == 4 else "Co<4", "Ci%4==0" if Ci % 4 == 0 else "Ci%4!=0") + _chunks16(Ci)
        if route == 4:      # conv3x3_thin_in_fwd_kernel<Ci, stride>
            return (f"CI={Ci}", f"ST={s}", "statistics" if flags & STATS else "plain")
    if direction == DGRAD:
        if route == 1:      # conv_dgrad_thin_s2_kernel: the taps a pixel takes follow the parities of its row and column
            return (f"Ci={Ci}", "Co=4" if Co == 4 else "Co=256" if Co == 256 else "4<Co<256", f"H%2={H % 2}", f"W%2={W % 2}")
        if route == 2:      # conv_fwd_thin_px4_kernel<7, Ci, 4, true>: its input pixels are dy's Co channels
            return (f"CO={Ci}", f"Ci={Co}", "16-byte staging" if Co == 4 else "scalar staging")
        if route == 3:      # conv_dgrad_thin_px4_kernel<7>
            return (f"Co={Co}", "one chunk" if Ci == 16 else "several chunks")
        if route == 4:      # conv_dgrad_thin_kernel<7>: the Co > 3 branch, 16-byte against scalar stores
            return ("Co=4" if Co == 4 else "Co<4", "Ci%4==0" if Ci % 4 == 0 else "Ci%4!=0") + _chunks16(Ci)
    if direction == WGRAD:
        if route == 1:      # conv_wgrad_thin_rows_kernel
            strips, segs, rps = rows_geo(case)
            seg = "one segment" if segs == 1 else "short last segment" if H % rps else "equal segments"
            return (f"Co={Co}", seg, "narrow last strip" if W % TR_W else "full strips", "H<=6" if H <= 6 else "H>6")
        if route == 2:      # conv_wgrad_thin_kernel<k, wide side on dy>
            wide_dy = Co > Ci
            wide = Co if wide_dy else Ci
            chunks = ("wide<16" if wide < 16 else "one chunk" if wide == 16 else "ragged last chunk" if wide % 16 else
                      "four chunks" if wide == 64 else "full chunks")
            return (f"<{k},{'true' if wide_dy else 'false'}>", chunks, _loop(wgrad_tiles(case), THIN_SPLITS))
        if route == 3:      # conv3x3_thin_in_wgrad_kernel<Ci, stride>
            return (f"CI={Ci}", f"ST={s}", _loop(N * out_hw(case)[0], THIN_IN_WG))
    raise ValueError(f"{case} direction {direction} route {route}: not a thin route")


def tile_of(direction, route, case):
    """(rows, columns) of the pixel tile of a forward / data-gradient route; the stride-2 data gradient has 256 pixels of the
    flat [N][H][W] order per workgroup (reported as (0, 256)), the thin-input forward a quarter output row per wavefront"""
    if direction == FWD and route == 4:
        return 1, out_hw(case)[1] // 4
    if direction == DGRAD and route == 1:
        return 0, 256
    if (direction, route) in ((FWD, 3), (DGRAD, 4)):
        return THIN_TH, THIN_TW
    return THIN4_T, THIN4_T


# ---- forward: (case, route) -----------------------------------------------------------------------------------------------
FWD_CASES = [
    # route 1: px4 with 4-channel pixels, CO = 1..3; Ci = 4 stages in 16-byte pieces, Ci < 4 scalar
    ((1, 70, 61, 4, 1, 7, 1, 3), 1),
    ((1, 70, 61, 3, 1, 7, 1, 3), 1),
    ((2, 37, 59, 4, 2, 7, 1, 3), 1),
    ((1, 70, 61, 1, 2, 7, 1, 3), 1),
    ((1, 70, 61, 4, 3, 7, 1, 3), 1),
    ((2, 37, 59, 3, 3, 7, 1, 3), 1),        # the condition branch's 3 -> 3
    # route 2: px4 with 8-channel chunks, one chunk (Ci = 8) against several (24, 64)
    ((1, 70, 61, 8, 1, 7, 1, 3), 2),
    ((1, 70, 61, 24, 1, 7, 1, 3), 2),
    ((2, 37, 59, 8, 2, 7, 1, 3), 2),
    ((1, 70, 61, 64, 2, 7, 1, 3), 2),
    ((1, 70, 61, 8, 3, 7, 1, 3), 2),
    ((2, 37, 59, 64, 3, 7, 1, 3), 2),       # the preNet's 64 -> 3
    # route 3: one pixel per thread.  Co = 4 takes every Ci, Co < 4 what px4 leaves (Ci > 4, no multiple of 8)
    ((1, 70, 61, 3, 4, 7, 1, 3), 3),        # Ci % 4, one partial chunk (qn = 1)
    ((1, 70, 61, 12, 4, 7, 1, 3), 3),       # 16-byte loads, one partial chunk (qn = 3)
    ((2, 37, 59, 16, 4, 7, 1, 3), 3),       # one full chunk
    ((1, 70, 61, 17, 4, 7, 1, 3), 3),       # two chunks, the second with one channel, scalar loads
    ((1, 70, 61, 20, 4, 7, 1, 3), 3),       # two chunks, the second with qn = 1, 16-byte loads
    ((1, 70, 61, 64, 4, 7, 1, 3), 3),       # four full chunks
    ((1, 70, 61, 5, 3, 7, 1, 3), 3),
    ((2, 37, 59, 12, 2, 7, 1, 3), 3),
    ((1, 70, 61, 17, 1, 7, 1, 3), 3),
    ((1, 70, 61, 20, 3, 7, 1, 3), 3),
    # route 4: thin input to 64 channels, CI = 1..4, stride 1 and 2; each runs without and with statistics
    ((1, 64, 64, 1, 64, 3, 1, 1), 4),       # exactly 4096 pixels
    ((2, 33, 80, 2, 64, 3, 1, 1), 4),
    ((2, 33, 80, 3, 64, 3, 1, 1), 4),
    ((1, 4, 1264, 4, 64, 3, 1, 1), 4),      # the LDS cap of fwd_thin_in_ok: (W + 3) * Ci = 5068 of 5120
    ((4, 34, 128, 1, 64, 3, 2, 1), 4),
    ((1, 128, 128, 2, 64, 3, 2, 1), 4),
    ((4, 34, 128, 3, 64, 3, 2, 1), 4),
    ((2, 66, 160, 4, 64, 3, 2, 1), 4),
]

# ---- data gradient: (case, route) ------------------------------------------------------------------------------------------
DGRAD_CASES = [
    # route 1 (stride 2): Ci = 1..4 x {Co = 4, 4 < Co < 256} x the four parities of (H, W), and Co = 256 (the largest filter
    # image in LDS) on every parity.  65 x 63 pixels = 4095: two images.
    *[((N, H, W, Ci, Co, 3, 2, 1), 1)
      for (N, H, W) in ((1, 64, 64), (1, 64, 65), (1, 65, 64), (2, 65, 63))
      for Ci in (1, 2, 3, 4) for Co in (4, 12)],
    ((1, 64, 64, 3, 256, 3, 2, 1), 1),
    ((1, 64, 65, 1, 256, 3, 2, 1), 1),
    ((1, 65, 64, 4, 256, 3, 2, 1), 1),
    ((2, 65, 63, 2, 256, 3, 2, 1), 1),
    # route 2 (px4 transposed): every (Ci, Co) of 1..3 x 1..4; at Co = 4 the kernel's pixels are 4-channel, 16-byte staging
    *[(((1, 70, 61) if (Ci + Co) % 2 else (2, 37, 59)) + (Ci, Co, 7, 1, 3), 2) for Ci in (1, 2, 3) for Co in (1, 2, 3, 4)],
    # route 3 (px4): one chunk against several
    ((1, 70, 61, 16, 1, 7, 1, 3), 3),
    ((1, 70, 61, 48, 1, 7, 1, 3), 3),
    ((2, 37, 59, 16, 2, 7, 1, 3), 3),
    ((1, 70, 61, 64, 2, 7, 1, 3), 3),
    ((1, 70, 61, 16, 3, 7, 1, 3), 3),
    ((2, 37, 59, 64, 3, 7, 1, 3), 3),       # the preNet's 64 -> 3
    # route 4 (one pixel per thread): Co = 4 with every Ci > 3, Co < 4 with Ci no multiple of 16
    ((1, 70, 61, 4, 4, 7, 1, 3), 4),
    ((1, 70, 61, 5, 4, 7, 1, 3), 4),
    ((2, 37, 59, 16, 4, 7, 1, 3), 4),
    ((1, 70, 61, 17, 4, 7, 1, 3), 4),
    ((1, 70, 61, 20, 4, 7, 1, 3), 4),
    ((1, 70, 61, 64, 4, 7, 1, 3), 4),
    ((1, 70, 61, 8, 1, 7, 1, 3), 4),
    ((1, 70, 61, 5, 3, 7, 1, 3), 4),
    ((2, 37, 59, 17, 2, 7, 1, 3), 4),
    ((1, 70, 61, 20, 3, 7, 1, 3), 4),
]

# ---- weight gradient: (case, route, nsplit) --------------------------------------------------------------------------------
WGRAD_CASES = [
    # route 1 (rolling rows, Ci = 64), per Co = 1..3: (strips, segments, rows per segment) in the comment
    *[((N, H, W, 64, Co, 7, 1, 3), 1, ns) for Co in (1, 2, 3) for (N, H, W, ns) in (
        (1, 64, 64, 8),         # (2, 4, 16): equal segments, full strips
        (1, 64, 65, 12),        # (3, 4, 16): equal segments, a last strip of one column
        (4, 16, 64, 8),         # (2, 1, 16): one segment
        (1, 6, 700, 22),        # (22, 1, 6): H = 6, every halo row above or below lies outside the image; a strip of 28 columns
        (17, 12, 40, 34),       # (2, 1, 12): one segment, a strip of 8 columns, the image index
        (1, 65, 64, 8),         # (2, 4, 17): the last segment has 14 rows
        (1, 70, 61, 8),         # (2, 4, 18): the last segment has 16 rows, the last strip 29 columns
    )],
    # route 2 (8 x 32 tiles, at most 1024 workgroups): <7, true> = 7x7 with the wide side on dy, <k, false> with it on x.
    # 70 x 61 has 18 tiles, 2 x 37 x 59 has 20; 260 x 12 x 40 has 1040 tiles (2 x 2 per image, ragged in rows and columns) of
    # which 16 workgroups take two; 1030 x 5 x 7 has 1030 (6 workgroups take two)
    ((1, 70, 61, 2, 5, 7, 1, 3), 2, 18),            # <7,true> wide < 16: groups = 2
    ((260, 12, 40, 3, 5, 7, 1, 3), 2, 1024),
    ((2, 37, 59, 4, 16, 7, 1, 3), 2, 20),           # <7,true> one chunk
    ((260, 12, 40, 1, 16, 7, 1, 3), 2, 1024),
    ((1, 70, 61, 2, 17, 7, 1, 3), 2, 18),           # <7,true> ragged second chunk
    ((260, 12, 40, 3, 17, 7, 1, 3), 2, 1024),       #          the cross-tile barrier is also the cross-chunk barrier
    ((1, 70, 61, 4, 48, 7, 1, 3), 2, 18),           # <7,true> three full chunks
    ((1030, 5, 7, 1, 48, 7, 1, 3), 2, 1024),
    ((2, 37, 59, 2, 64, 7, 1, 3), 2, 20),           # <7,true> four chunks
    ((1030, 5, 7, 3, 64, 7, 1, 3), 2, 1024),
    ((1, 70, 61, 5, 4, 7, 1, 3), 2, 18),            # <7,false> wide < 16
    ((260, 12, 40, 3, 3, 7, 1, 3), 2, 1024),        #           the condition branch's 3 -> 3: groups = 1
    ((1, 70, 61, 16, 2, 7, 1, 3), 2, 18),           # <7,false> one chunk
    ((260, 12, 40, 16, 3, 7, 1, 3), 2, 1024),
    ((2, 37, 59, 17, 4, 7, 1, 3), 2, 20),           # <7,false> ragged second chunk
    ((260, 12, 40, 17, 1, 7, 1, 3), 2, 1024),
    ((1, 70, 61, 48, 2, 7, 1, 3), 2, 18),           # <7,false> three full chunks
    ((1030, 5, 7, 48, 3, 7, 1, 3), 2, 1024),
    ((1, 70, 61, 64, 4, 7, 1, 3), 2, 18),           # <7,false> four chunks: Ci = 64 with Co = 4, which route 1 does not take
    ((1030, 5, 7, 64, 4, 7, 1, 3), 2, 1024),
    ((2, 37, 59, 5, 2, 3, 1, 1), 2, 20),            # <3,false> wide < 16
    ((260, 12, 40, 5, 3, 3, 1, 1), 2, 1024),
    ((1, 70, 61, 16, 4, 3, 1, 1), 2, 18),           # <3,false> one chunk
    ((260, 12, 40, 16, 1, 3, 1, 1), 2, 1024),
    ((1, 70, 61, 17, 2, 3, 1, 1), 2, 18),           # <3,false> ragged second chunk
    ((260, 12, 40, 17, 3, 3, 1, 1), 2, 1024),
    ((2, 37, 59, 48, 4, 3, 1, 1), 2, 20),           # <3,false> three full chunks
    ((1030, 5, 7, 48, 1, 3, 1, 1), 2, 1024),
    ((1, 70, 61, 64, 2, 3, 1, 1), 2, 18),           # <3,false> four chunks
    ((1030, 5, 7, 64, 3, 3, 1, 1), 2, 1024),
    # route 3 (thin input, one output row at a time, at most 1024 workgroups): 17 images of 64 output rows = 1088 rows
    ((1, 64, 64, 1, 64, 3, 1, 1), 3, 64),
    ((17, 64, 64, 1, 64, 3, 1, 1), 3, 1024),
    ((4, 34, 128, 1, 64, 3, 2, 1), 3, 68),
    ((17, 128, 128, 1, 64, 3, 2, 1), 3, 1024),
    ((2, 33, 80, 2, 64, 3, 1, 1), 3, 66),
    ((17, 64, 64, 2, 64, 3, 1, 1), 3, 1024),
    ((1, 128, 128, 2, 64, 3, 2, 1), 3, 64),
    ((17, 128, 128, 2, 64, 3, 2, 1), 3, 1024),
    ((1, 64, 64, 3, 64, 3, 1, 1), 3, 64),
    ((17, 64, 64, 3, 64, 3, 1, 1), 3, 1024),        # the preNet's 3 -> 64
    ((4, 34, 128, 3, 64, 3, 2, 1), 3, 68),
    ((17, 128, 128, 3, 64, 3, 2, 1), 3, 1024),      # the stem's 3 -> 64
    ((1, 4, 1264, 4, 64, 3, 1, 1), 3, 4),           # the LDS cap of fwd_thin_in_ok
    ((17, 64, 64, 4, 64, 3, 1, 1), 3, 1024),
    ((1, 128, 128, 4, 64, 3, 2, 1), 3, 64),
    ((17, 128, 128, 4, 64, 3, 2, 1), 3, 1024),
]


def is_loop_case(case, route):
    """a weight-gradient case whose workgroups take more than one tile (route 2) or output row (route 3)"""
    return route in (2, 3) and key(case, WGRAD, route)[-1] == "loop"

# ---- threshold pairs: (direction, case inside, its route, case outside, its route, the line) -------------------------------
THRESHOLDS = [
    (FWD, (1, 64, 64, 3, 3, 7, 1, 3), 1, (1, 63, 65, 3, 3, 7, 1, 3), 0, "fwd_thin_ok: 4096 pixels against 4095"),
    (DGRAD, (1, 64, 64, 64, 3, 7, 1, 3), 3, (1, 63, 65, 64, 3, 7, 1, 3), 0, "fwd_thin_ok: 4096 pixels against 4095"),
    (FWD, (1, 70, 61, 64, 4, 7, 1, 3), 3, (1, 70, 61, 68, 4, 7, 1, 3), 0, "fwd_thin_ok: Ci = 64 against 68"),
    (DGRAD, (1, 70, 61, 64, 4, 7, 1, 3), 4, (1, 70, 61, 68, 4, 7, 1, 3), 0, "fwd_thin_ok: Ci = 64 against 68"),
    (FWD, (1, 70, 61, 16, 4, 7, 1, 3), 3, (1, 70, 61, 16, 5, 7, 1, 3), 0, "fwd_thin_ok: Co = 4 against 5"),
    (DGRAD, (1, 64, 64, 3, 4, 3, 2, 1), 1, (1, 63, 65, 3, 4, 3, 2, 1), 0, "dgrad_thin_s2_ok: 4096 pixels against 4095"),
    (DGRAD, (1, 64, 64, 3, 256, 3, 2, 1), 1, (1, 64, 64, 3, 260, 3, 2, 1), 0, "dgrad_thin_s2_ok: Co = 256 against 260"),
    (DGRAD, (1, 64, 64, 4, 8, 3, 2, 1), 1, (1, 64, 64, 5, 8, 3, 2, 1), 0, "dgrad_thin_s2_ok: Ci = 4 against 5"),
    (FWD, (1, 64, 64, 3, 64, 3, 1, 1), 4, (1, 63, 64, 3, 64, 3, 1, 1), 0, "fwd_thin_in_ok: 4096 pixels against 4032"),
    (WGRAD, (1, 64, 64, 3, 64, 3, 1, 1), 3, (1, 63, 64, 3, 64, 3, 1, 1), 0, "fwd_thin_in_ok: 4096 pixels against 4032"),
    (FWD, (2, 64, 64, 3, 64, 3, 1, 1), 4, (2, 86, 48, 3, 64, 3, 1, 1), 0, "fwd_thin_in_ok: Wo = 64 against 48"),
    (WGRAD, (2, 64, 64, 3, 64, 3, 1, 1), 3, (2, 86, 48, 3, 64, 3, 1, 1), 0, "fwd_thin_in_ok: Wo = 64 against 48"),
    (FWD, (2, 64, 128, 3, 64, 3, 2, 1), 4, (2, 65, 128, 3, 64, 3, 2, 1), 0, "fwd_thin_in_ok: stride 2 on an even H against an odd one"),
    (FWD, (1, 4, 1264, 4, 64, 3, 1, 1), 4, (1, 4, 1280, 4, 64, 3, 1, 1), 0, "fwd_thin_in_ok: the LDS cap, W = 1264 against 1280"),
    (WGRAD, (1, 4, 1264, 4, 64, 3, 1, 1), 3, (1, 4, 1280, 4, 64, 3, 1, 1), 0, "fwd_thin_in_ok: the LDS cap, W = 1264 against 1280"),
    (WGRAD, (1, 64, 64, 3, 3, 7, 1, 3), 2, (1, 63, 65, 3, 3, 7, 1, 3), 0, "wgrad_thin_ok: 4096 pixels against 4095"),
    (WGRAD, (1, 64, 64, 64, 3, 7, 1, 3), 1, (1, 63, 65, 64, 3, 7, 1, 3), 0, "wgrad_thin_rows_ok: 4096 pixels against 4095"),
    (WGRAD, (1, 70, 61, 64, 4, 7, 1, 3), 2, (1, 70, 61, 68, 4, 7, 1, 3), 0, "wgrad_thin_ok: wide = 64 against 68"),
    (WGRAD, (1, 70, 61, 4, 64, 7, 1, 3), 2, (1, 70, 61, 4, 68, 7, 1, 3), 0, "wgrad_thin_ok: wide = 64 against 68, on dy"),
    (WGRAD, (1, 70, 61, 16, 4, 7, 1, 3), 2, (1, 70, 61, 16, 5, 7, 1, 3), 0, "wgrad_thin_ok: thin = 4 against 5"),
    (WGRAD, (1, 70, 61, 64, 3, 3, 1, 1), 2, (1, 70, 61, 3, 64, 3, 1, 1), 0, "wgrad_thin_ok: 3x3 with the thin side on dy against on x"),
    (WGRAD, (1, 70, 61, 64, 3, 7, 1, 3), 1, (1, 70, 61, 64, 4, 7, 1, 3), 2, "wgrad_thin_rows_ok: Co = 3 against 4"),
    (WGRAD, (1, 70, 61, 64, 3, 7, 1, 3), 1, (1, 70, 61, 48, 3, 7, 1, 3), 2, "wgrad_thin_rows_ok: Ci = 64 against 48"),
]

# ---- flags that must leave the thin routes: (direction, case, route without the flag, flags, route with them) --------------
FLAG_CASES = [
    (FWD, (1, 70, 61, 3, 3, 7, 1, 3), 1, BIAS | RELU, 0),
    (FWD, (1, 70, 61, 64, 3, 7, 1, 3), 2, BIAS | SCALE, 0),
    (FWD, (1, 70, 61, 17, 4, 7, 1, 3), 3, RESIDUAL, 0),
    (FWD, (1, 70, 61, 3, 3, 7, 1, 3), 1, BIAS | STATS, 0),
    (FWD, (1, 70, 61, 64, 3, 7, 1, 3), 2, STATS, 0),
    (FWD, (1, 70, 61, 17, 4, 7, 1, 3), 3, BIAS | STATS, 0),
    (FWD, (1, 64, 64, 3, 64, 3, 1, 1), 4, BIAS | RELU, 0),
    (FWD, (1, 64, 64, 3, 64, 3, 1, 1), 4, BIAS | STATS, 4),
    (DGRAD, (1, 64, 64, 3, 64, 3, 2, 1), 1, BIAS, 0),
    (DGRAD, (1, 70, 61, 3, 3, 7, 1, 3), 2, STATS, 0),
    (DGRAD, (1, 70, 61, 64, 3, 7, 1, 3), 3, BIAS | STATS, 0),
    (DGRAD, (1, 70, 61, 17, 4, 7, 1, 3), 4, BIAS, 0),
]
# thin input with statistics AND an epilogue: the plan query (and the launch) return an error
REFUSED = [(FWD, (1, 64, 64, 3, 64, 3, 1, 1), STATS | RELU), (FWD, (4, 34, 128, 3, 64, 3, 2, 1), BIAS | STATS | SCALE)]

# ---- guard bands: the most ragged case of each route -----------------------------------------------------------------------
GUARD_CASES = [
    (FWD, (2, 37, 59, 3, 3, 7, 1, 3), 1),           # 3-channel pixels read scalar, 5 rows and 27 columns in the last tiles
    (FWD, (2, 37, 59, 64, 3, 7, 1, 3), 2),
    (FWD, (1, 70, 61, 17, 4, 7, 1, 3), 3),          # one channel in the second chunk
    (FWD, (1, 4, 1264, 4, 64, 3, 1, 1), 4),         # the longest row in LDS; with statistics
    (FWD, (4, 34, 128, 3, 64, 3, 2, 1), 4),         # stride 2, 3-channel pixels; with statistics
    (DGRAD, (2, 65, 63, 3, 12, 3, 2, 1), 1),        # odd H and W, 8190 = 31 * 256 + 254 pixels
    (DGRAD, (2, 37, 59, 3, 3, 7, 1, 3), 2),
    (DGRAD, (2, 37, 59, 64, 3, 7, 1, 3), 3),
    (DGRAD, (1, 70, 61, 17, 4, 7, 1, 3), 4),
    (WGRAD, (1, 70, 61, 64, 3, 7, 1, 3), 1),        # short last segment, narrow last strip
    (WGRAD, (260, 12, 40, 3, 17, 7, 1, 3), 2),      # the tile loop with a ragged second chunk
    (WGRAD, (17, 128, 128, 3, 64, 3, 2, 1), 3),     # the row loop at stride 2
]

# ---- hard operands (all 24 mantissa bits set, exponents spread over 2^40 inside a reduction): one per kernel and direction --
HARD_CASES = [
    (FWD, (2, 37, 59, 3, 3, 7, 1, 3), 1),
    (FWD, (2, 37, 59, 64, 3, 7, 1, 3), 2),
    (FWD, (1, 70, 61, 17, 4, 7, 1, 3), 3),
    (FWD, (2, 33, 80, 3, 64, 3, 1, 1), 4),
    (FWD, (4, 34, 128, 3, 64, 3, 2, 1), 4),
    (DGRAD, (2, 65, 63, 3, 12, 3, 2, 1), 1),
    (DGRAD, (2, 37, 59, 3, 3, 7, 1, 3), 2),
    (DGRAD, (2, 37, 59, 64, 3, 7, 1, 3), 3),
    (DGRAD, (1, 70, 61, 17, 4, 7, 1, 3), 4),
]

# ---- the search grid of the closure test -----------------------------------------------------------------------------------
GRID_N = [1, 2, 3, 17, 32, 260]
GRID_HW = [(384, 288), (256, 192), (70, 61), (37, 59), (64, 64), (64, 65), (65, 64), (65, 63), (33, 80), (34, 128), (12, 40),
           (4, 1264), (6, 700), (128, 128)]
GRID_C = [1, 2, 3, 4, 5, 8, 12, 16, 17, 20, 24, 32, 48, 64]
GRID_GEO = [(3, 1, 1), (3, 2, 1), (7, 1, 3)]        # (k, stride, pad)
MAX_FLOATS = 8 << 20


def tensor_floats(case):
    """the largest tensor of a case, in floats"""
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    return max(N * H * W * Ci, N * Ho * Wo * Co)
