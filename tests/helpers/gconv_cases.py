"""The case table of the gathered bf16x6 convolution tests (csrc/conv_gather_x6.hip, csrc/conv_gather_wgrad.hip), as data.

A convolution case is (kind, dir, N, H, W, Ci, Co) exactly as the C interface takes it: kind 1 = 1x1 / stride 1 / pad 0,
kind 2 = 3x3 / stride 2 / pad 1; (H, W) are the INPUT dims of the forward convolution Ci -> Co; dir 0 runs that forward
convolution, dir 1 its data gradient (the launch then reads Co channels and writes Ci).  A weight-gradient case is
(kind, N, H, W, Ci, Co).

tests/test_gconv_plan_cover.py (host only) proves through buctd_gconv_x6_plan / buctd_gconv_wgrad_x6_plan that every case
takes the route the table names and that the table reaches every plan the search grid can see;
tests/test_gpu_gconv_plan_cover.py runs every case x option set against fp64."""
import ctypes as C

FWD, DGRAD = 0, 1
# flags of buctd_gconv_x6_plan: which optional arguments the call carries
BIAS, SCALE, RELU, PARTIALS, ACC, RES = 1, 2, 4, 8, 16, 32
MODE_GENERAL, MODE_PLAIN, C3M_STATS, C3M_RES = -1, 0, 2, 4      # the epilogue (csrc/c3_lean.h)

# option set -> flags.  "general" is two calls (bias; scale / shift + residual + relu), both on the general epilogue.
FWD_SETS = {"general": BIAS, "general-affine": SCALE | RES | RELU, "plain": 0, "STATS": ACC, "partials": PARTIALS, "fwd-RES": RES}
DGRAD_SETS = {"plain": 0, "RES": RES}
# the row-streaming kernel has no scale / shift, relu or partial sums: those calls go to the tiled kernel whatever the size
ROWS_FWD_SETS = {"plain": 0, "bias": BIAS, "RES": RES, "STATS": ACC, "STATS+bias": ACC | BIAS}
ROWS_DGRAD_SETS = {"plain": 0, "RES": RES}

PLAN_FIELDS = ("route", "MF", "NF", "WM", "WN", "BM", "BN", "mode", "ncls")
WGRAD_FIELDS = ("CF", "TPG", "ntg", "nsplit", "q", "rem", "ksteps", "qrem")


def plan(case, flags=0):
    """buctd_gconv_x6_plan as a dict (cls = [(ntaps, nhs, nsteps)] of the ncls classes), or None where it refuses"""
    from buctd_amd import _C
    out = (C.c_int * 25)()
    kind, direction, N, H, W, Ci, Co = case
    if _C.lib().buctd_gconv_x6_plan(kind, direction, N, H, W, Ci, Co, flags, out) != 0:
        return None
    v = list(out)
    pl = dict(zip(PLAN_FIELDS, v[:9]))
    pl["cls"] = [tuple(v[9 + 3 * c:12 + 3 * c]) for c in range(pl["ncls"])]
    pl["tiles"], pl["ncol"], pl["NFT"], pl["ksteps"] = v[21:25]
    return pl


def wgrad_plan(case):
    from buctd_amd import _C
    out = (C.c_int * 8)()
    if _C.lib().buctd_gconv_wgrad_x6_plan(*case, out) != 0:
        return None
    return dict(zip(WGRAD_FIELDS, out))


def positions(case):
    """P of the tiled launch: the zero-padded flattened positions of its grid (per class for a stride-2 data gradient)"""
    kind, direction, N, H, W, Ci, Co = case
    Hg, Wg = (H, W) if kind == 1 else (H // 2, W // 2)
    return N * (Hg + 1) * (Wg + 2) + Wg + 2


def out_shape(case):
    """NHWC shape of what the launch writes"""
    kind, direction, N, H, W, Ci, Co = case
    if direction == DGRAD:
        return (N, H, W, Ci)
    return (N, H, W, Co) if kind == 1 else (N, H // 2, W // 2, Co)


def in_shape(case):
    """NHWC shape of what the launch reads"""
    kind, direction, N, H, W, Ci, Co = case
    if direction == FWD:
        return (N, H, W, Ci)
    return (N, H, W, Co) if kind == 1 else (N, H // 2, W // 2, Co)


# ---- the tiled kernel: (case, tile width BN of the plan) ----------------------------------------------------------------------
# One case per (tile plan) x (kind 1 fwd, kind 1 dgrad, kind 2 fwd, kind 2 dgrad); the position tiles are ragged everywhere
# (P % 128 != 0).  Comment: half-steps / steps per class - what the step loop (unrolled by two, A pieces two steps ahead) sees.
PLAN_CASES = [
    ((1, FWD, 3, 12, 9, 16, 192), 96),        # nhs 1, nsteps 1: the whole contraction is the prologue; dead half-step; 2 column tiles
    ((1, DGRAD, 2, 7, 5, 96, 32), 96),        # nhs 2, nsteps 1
    ((2, FWD, 2, 12, 10, 16, 96), 96),        # nhs 9, nsteps 5: odd both, kind 2 forward with a dead last half-step
    ((2, DGRAD, 2, 12, 10, 96, 48), 96),      # classes nhs 3 / 6 / 6 / 12, nsteps 2 / 3 / 3 / 6: class 0 ends on a dead half-step
    ((1, FWD, 5, 96, 72, 64, 256), 128),      # 34560 rows: 281 x 2 workgroups >= 512; nhs 4
    ((1, DGRAD, 5, 96, 72, 256, 64), 128),    # its data-gradient twin
    ((2, FWD, 5, 192, 144, 16, 256), 128),    # nhs 9
    ((2, DGRAD, 5, 192, 144, 256, 16), 128),  # classes nhs 1 / 2 / 2 / 4: class 0 is nsteps 1 with a dead half-step
    ((1, FWD, 2, 24, 18, 48, 64), 64),        # nhs 3, nsteps 2: odd nhs on kind 1, even steps
    ((1, DGRAD, 3, 9, 7, 64, 80), 64),        # nhs 5, nsteps 3
    ((2, FWD, 2, 20, 14, 48, 128), 64),       # nhs 27, nsteps 14; 128 outputs on a small map stay on the 64-wide tiles, 2 column tiles
    ((2, DGRAD, 2, 20, 14, 64, 32), 64),      # classes nhs 2 / 4 / 4 / 8: every class ends on a live half-step
    ((1, FWD, 3, 1, 1, 64, 48), 48),          # 1x1 input (three rows: statistics need more than one); nhs 4, nsteps 2
    ((1, DGRAD, 3, 12, 9, 48, 96), 48),       # nhs 6, nsteps 3: even nhs, odd steps
    ((2, FWD, 3, 2, 2, 32, 48), 48),          # 2x2 input (H/2 = W/2 = 1); nhs 18
    ((2, DGRAD, 2, 16, 12, 144, 16), 48),     # three 48-wide column tiles; classes nhs 1 / 2 / 2 / 4
]
EDGE_CASES = [
    ((2, DGRAD, 2, 2, 2, 48, 32), 48),        # 2x2 input of a stride-2 data gradient: a 1x1 grid per class; class 0 live (nhs 2)
    ((1, FWD, 1, 257, 257, 160, 128), 128),   # 66049 rows that the row kernel cannot take (the image of 160 inputs exceeds its LDS)
    ((1, FWD, 1, 255, 257, 32, 64), 64),      # 65535 rows: one below the row kernel's threshold
    ((2, FWD, 1, 2, 6, 16, 64), 64),          # H/2 = 1
    ((2, FWD, 1, 6, 2, 16, 64), 64),          # W/2 = 1
]
TILED_CASES = PLAN_CASES + EDGE_CASES

# ---- the row-streaming 1x1 kernel: (case, NFT, K steps) -------------------------------------------------------------------------
# rows >= 65536, 64 / 128 / 256 outputs of the launch, inputs a multiple of 32 up to what the filter image leaves of the LDS
# (256 / 128 / 64 inputs).  256 x 256 = 65536 rows exactly; 257 x 257 = 66049 rows end in a block of one row.
ROW_CASES = [
    ((1, FWD, 1, 256, 256, 32, 64), 4, 1),
    ((1, FWD, 1, 257, 257, 256, 64), 4, 8),       # the largest input count for 64 outputs
    ((1, DGRAD, 1, 257, 257, 128, 32), 8, 1),
    ((1, FWD, 1, 256, 256, 128, 128), 8, 4),      # the largest for 128
    ((1, FWD, 1, 257, 257, 32, 256), 16, 1),
    ((1, DGRAD, 1, 256, 256, 256, 64), 16, 2),    # the largest for 256
    ((1, DGRAD, 1, 257, 257, 64, 256), 4, 8),
    ((1, FWD, 2, 257, 257, 64, 256), 16, 2),      # more row blocks (4129) than waves of the persistent grid (2048)
]

# ---- hard operands (all mantissa bits set): one per kind and direction ------------------------------------------------------------
HARD_CASES = [(1, FWD, 2, 9, 7, 48, 48), (1, DGRAD, 2, 9, 7, 48, 48), (2, FWD, 2, 10, 6, 48, 48), (2, DGRAD, 2, 10, 6, 48, 48)]

# ---- prepared-image pad: odd nhs on kind 1 forward, kind 2 forward and (class 0) kind 2 data gradient -----------------------------
PAD_CASES = [(1, FWD, 2, 24, 18, 48, 64), (2, FWD, 2, 12, 10, 16, 96), (2, DGRAD, 2, 12, 10, 96, 48)]

# ---- weight gradient: (case, key, nsplit) with key = (kind, CF, nsplit == 1, rem == 0, Q % 32 == 0) -------------------------------
# nsplit = min(ceil(768 / (chunk pairs x tap groups)), ceil(k-steps / 16)): the 192 x 192 case (9 pairs) is bounded by the first
WGRAD_CASES = [
    ((1, 1, 1, 2, 32, 32), (1, 2, True, True, False), 1),          # Wo = 2: one ragged k-step of two pixels
    ((1, 1, 8, 4, 32, 64), (1, 2, True, True, True), 1),
    ((1, 16, 7, 5, 64, 64), (1, 2, False, True, False), 2),
    ((1, 5, 16, 8, 32, 64), (1, 2, False, True, True), 2),
    ((1, 5, 12, 9, 32, 64), (1, 2, False, False, False), 2),
    ((1, 2, 24, 18, 64, 32), (1, 2, False, False, True), 2),
    ((1, 1, 1, 2, 48, 48), (1, 3, True, True, False), 1),
    ((1, 1, 8, 4, 96, 96), (1, 3, True, True, True), 1),           # CF 3 although both channel counts are multiples of 32 too
    ((1, 16, 7, 5, 48, 48), (1, 3, False, True, False), 2),
    ((1, 5, 16, 8, 96, 48), (1, 3, False, True, True), 2),
    ((1, 5, 12, 9, 48, 96), (1, 3, False, False, False), 2),
    ((1, 2, 24, 18, 96, 192), (1, 3, False, False, True), 2),      # ... again
    ((1, 1, 256, 256, 64, 128), (1, 4, False, True, True), 128),     # CF 4: 65536 rows exactly
    ((1, 2, 255, 257, 64, 64), (1, 4, False, True, False), 256),
    ((1, 1, 256, 256, 192, 192), (1, 4, False, False, True), 86),
    ((1, 1, 257, 257, 128, 64), (1, 4, False, False, False), 130),   # last k-step: one pixel
    ((2, 1, 2, 4, 32, 32), (2, 2, True, True, False), 1),          # Wo = 2
    ((2, 1, 16, 8, 64, 32), (2, 2, True, True, True), 1),
    ((2, 16, 14, 10, 32, 32), (2, 2, False, True, False), 2),
    ((2, 1, 48, 48, 32, 64), (2, 2, False, True, True), 2),
    ((2, 5, 24, 18, 32, 64), (2, 2, False, False, False), 2),
    ((2, 3, 36, 32, 64, 32), (2, 2, False, False, True), 2),
    ((2, 1, 2, 4, 48, 48), (2, 3, True, True, False), 1),          # Wo = 2
    ((2, 1, 16, 8, 96, 48), (2, 3, True, True, True), 1),
    ((2, 16, 14, 10, 48, 48), (2, 3, False, True, False), 2),
    ((2, 1, 48, 48, 48, 96), (2, 3, False, True, True), 2),
    ((2, 5, 24, 18, 48, 96), (2, 3, False, False, False), 2),
    ((2, 3, 36, 32, 96, 192), (2, 3, False, False, True), 2),
]
WGRAD_HARD = [(1, 2, 9, 7, 48, 48), (2, 2, 10, 6, 48, 48)]

# ---- guard bands: one ragged shape per tile plan, per row-kernel instance, per weight-gradient CF ---------------------------------
GUARD_TILED = [(2, DGRAD, 2, 12, 10, 96, 48), (1, FWD, 5, 96, 72, 64, 256), (2, FWD, 2, 20, 14, 48, 128), (1, DGRAD, 3, 12, 9, 48, 96)]
GUARD_ROWS = [(1, FWD, 1, 257, 257, 256, 64), (1, DGRAD, 1, 257, 257, 128, 32), (1, FWD, 1, 257, 257, 32, 256)]
GUARD_WGRAD = [(2, 5, 24, 18, 32, 64), (1, 5, 12, 9, 48, 96), (1, 1, 257, 257, 128, 64)]

# ---- the search grid of the closure test ------------------------------------------------------------------------------------------
GRID_N = [1, 2, 3, 5, 16]
GRID_HW = [(1, 1), (1, 2), (2, 2), (2, 4), (6, 4), (7, 5), (8, 4), (12, 9), (14, 10), (16, 8), (24, 16), (24, 18), (32, 32), (36, 32), (48, 48),
           (96, 72), (192, 144), (255, 257), (256, 256), (257, 257), (258, 256), (259, 257)]
GRID_C = [16, 32, 48, 64, 80, 96, 128, 144, 160, 192, 256, 384]
GRID_KINDS = [1, 2]


def case_id(case):
    if len(case) == 7:
        return f"k{case[0]}{'dgrad' if case[1] else 'fwd'}-" + "x".join(str(v) for v in case[2:])
    return f"k{case[0]}-" + "x".join(str(v) for v in case[1:])
