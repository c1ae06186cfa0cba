"""The case table of the exact-fp32 implicit-GEMM convolution tests (csrc/conv.hip: conv_gemm_kernel, conv_wgrad_kernel,
splitk_reduce_kernel), as data.

A case is (N, H, W, Ci, Co, k, stride, pad) of the FORWARD convolution x [N][H][W][Ci] -> y [N][Ho][Wo][Co]; a data-gradient
case runs the data gradient of that convolution (rows N*H*W, columns Ci, reduction k*k*Co), a weight-gradient case its weight
gradient.  Next to each case stands the plan it must reach, as buctd_conv2d_plan reports it - the GPU test asserts it before it
runs, so a dispatch change cannot move a case off the kernel under test without a failure that says so.

tests/test_conv2d_plan_cover.py (host only) proves that the table reaches every implicit-GEMM plan the routing can pick on the
search grid below; tests/test_gpu_conv2d_fp32.py runs every case against fp64 in the fp32 math mode."""
import ctypes as C

# the flag bits of buctd_conv2d_plan (include/buctd_hip.h)
BIAS, SCALE, RESIDUAL, RELU, STATS = 1, 2, 4, 8, 16
FWD, DGRAD, WGRAD = 0, 1, 2
PLAN_FIELDS = ("route", "tile", "BM", "BN", "WM", "MF", "vec", "par", "nsplit", "pix_per_split", "vec_reduce")

# the option sets the GPU test runs per direction (and the closure test enumerates)
FWD_FLAGS = {"bias": BIAS, "scale/shift/residual/relu": BIAS | SCALE | RESIDUAL | RELU, "stats": BIAS | STATS}
DGRAD_FLAGS = {"plain": 0, "bias+stats": BIAS | STATS}        # (residual= is an elementwise add behind the plain launch)

# ---- forward: (case, tile id) -------------------------------------------------------------------------------------------
# 64-row tiles at M = 2*11*9 = 198 = 3 * 64 + 6: the last row tile has 6 rows, so three of its four wavefronts (16 rows each,
# tiles 3 and 5) own no valid row at all; M = 297 = 256 + 41 for the 256-row tile
FWD_CASES = [
    ((2, 9, 7, 20, 30, 3, 1, 1), 0),        # scalar loads (Ci % 16): 128x64, M = 126 (one ragged tile), K = 180 = 11 * 16 + 4
    ((1, 7, 5, 3, 5, 7, 1, 3), 0),          # scalar loads, 7x7, K = 147 = 9 * 16 + 3, 5 of 64 columns
    ((3, 11, 9, 16, 14, 1, 1, 0), 1),       # 256x16, 14 of 16 columns, two row tiles
    ((2, 11, 9, 32, 17, 1, 1, 0), 2),       # 128x32, 17 of 32 columns (one column of the second 16-column fragment)
    ((2, 11, 9, 48, 48, 3, 1, 1), 3),       # 64x48
    ((1, 223, 220, 16, 40, 1, 1, 0), 4),    # 128x48: M = 49060 -> 384 row tiles (the last with 36 rows), 40 of 48 columns
    ((2, 11, 9, 32, 64, 3, 1, 1), 5),       # 64x64
    ((1, 223, 220, 16, 64, 1, 1, 0), 6),    # 128x64
    ((2, 11, 9, 16, 80, 3, 1, 1), 7),       # 64x96, 80 of 96 columns
    ((1, 223, 220, 16, 96, 1, 1, 0), 8),    # 128x96 (the largest case: 49060 x 96 floats = 19 MB)
    ((2, 11, 9, 32, 160, 3, 1, 1), 9),      # 64x128, two column tiles, the second with 32 columns
    ((2, 113, 109, 16, 128, 1, 1, 0), 10),  # 128x128: M = 24634 -> 193 row tiles (the last with 58 rows)
    ((2, 13, 9, 48, 192, 3, 2, 1), 7),      # stride 2 on an odd size, two 96-column tiles
    ((2, 8, 6, 32, 32, 4, 2, 1), 2),        # the deconvolution geometry of pose_resnet (4x4 / s2 / p1)
    ((2, 9, 7, 64, 48, 7, 1, 3), 3),        # 7x7, K = 3136
    ((2, 12, 9, 384, 384, 3, 1, 1), 7),     # the largest reduction: K = 3456, four 96-column tiles
]

# ---- data gradient: (case, tile id, par) -------------------------------------------------------------------------------
# vector loads need Co % 16 == 0 and Ci % 4 == 0; the tile follows Ci (the columns of dx) and M = N * H * W
DGRAD_CASES = [
    ((2, 9, 7, 20, 30, 3, 1, 1), 0, 0),        # scalar loads, K = 270 = 16 * 16 + 14, 20 of 64 columns
    ((1, 7, 5, 3, 5, 7, 1, 3), 0, 0),          # scalar loads, 7x7, 3 columns
    ((3, 11, 9, 12, 16, 1, 1, 0), 1, 0),       # 256x16, 12 of 16 columns
    ((2, 11, 9, 20, 32, 1, 1, 0), 2, 0),       # 128x32, 20 of 32 columns
    ((2, 11, 9, 48, 48, 3, 1, 1), 3, 0),       # 64x48
    ((1, 223, 220, 40, 16, 1, 1, 0), 4, 0),    # 128x48, 40 of 48 columns
    ((2, 11, 9, 64, 32, 3, 1, 1), 5, 0),       # 64x64
    ((1, 223, 220, 64, 16, 1, 1, 0), 6, 0),    # 128x64
    ((2, 11, 9, 80, 16, 3, 1, 1), 7, 0),       # 64x96, 80 of 96 columns
    ((1, 223, 220, 96, 16, 1, 1, 0), 8, 0),    # 128x96
    ((2, 11, 9, 160, 32, 3, 1, 1), 9, 0),      # 64x128, two column tiles
    ((2, 113, 109, 128, 16, 1, 1, 0), 10, 0),  # 128x128
    ((2, 8, 6, 32, 32, 4, 2, 1), 2, 0),        # deconvolution geometry: the transposed-convolution forward of pose_resnet
    ((2, 9, 7, 48, 64, 7, 1, 3), 3, 0),        # 7x7, K = 3136
    ((2, 12, 9, 384, 384, 3, 1, 1), 7, 0),     # the largest reduction: K = 3456
    # stride-2 3x3 split by output-pixel parity (3x3 / s2 / p1, vector loads): the four combinations of odd / even H and W, and
    # every tile (the 128-row ones take M = N * H * W of the whole gradient, not of a class)
    ((2, 13, 8, 48, 96, 3, 2, 1), 3, 1),       # H odd, W even
    ((2, 13, 9, 16, 160, 3, 2, 1), 1, 1),      # H odd, W odd
    ((2, 12, 9, 32, 32, 3, 2, 1), 2, 1),       # H even, W odd
    ((1, 6, 6, 64, 16, 3, 2, 1), 5, 1),        # H even, W even; 9 rows per class
    ((1, 1, 5, 96, 16, 3, 2, 1), 7, 1),        # H = 1: the two odd-row classes are empty
    ((2, 13, 9, 160, 48, 3, 2, 1), 9, 1),      # two column tiles
    ((1, 223, 220, 40, 16, 3, 2, 1), 4, 1),    # 128-row tiles: 12320 / 12210 / 12320 / 12210 rows per class
    ((1, 223, 220, 64, 16, 3, 2, 1), 6, 1),
    ((1, 223, 220, 96, 16, 3, 2, 1), 8, 1),
    ((2, 113, 109, 128, 16, 3, 2, 1), 10, 1),
]
# the parity cases with statistics must leave the parity split (the Welford groups are rows of the whole gradient)
DGRAD_STATS_PAR0 = (2, 13, 8, 48, 96, 3, 2, 1)

# ---- weight gradient: (case, configuration, nsplit) ----------------------------------------------------------------------
# configuration 0 = 64x64 scalar loads (Ci % 4 or Co % 4), 1..4 = 48 / 64 / 96 / 128 x 64 vector loads; key of the closure
# test: (configuration, nsplit == 1, last split ragged, float4 slab reduction)
WGRAD_CASES = [
    ((2, 9, 7, 20, 30, 3, 1, 1), 0, 1),        # generic, one ragged split (126 pixels), float4 reduction (Co*9*Ci % 4 == 0)
    ((1, 7, 5, 3, 5, 7, 1, 3), 0, 1),          # generic, 735 elements: the scalar slab reduction; 147 columns = 2 * 64 + 19
    ((1, 8, 6, 3, 5, 3, 1, 1), 0, 1),          # generic, one exact split (48 pixels), scalar reduction
    ((1, 8, 6, 6, 10, 3, 1, 1), 0, 1),         # generic, one exact split, float4 reduction
    ((2, 23, 17, 3, 5, 7, 1, 3), 0, 4),        # generic, ragged last split, scalar reduction
    ((2, 16, 16, 3, 5, 3, 1, 1), 0, 2),        # generic, exact splits, scalar reduction
    ((2, 23, 17, 20, 30, 3, 1, 1), 0, 4),      # generic, ragged last split, float4 reduction
    ((2, 16, 16, 6, 10, 3, 1, 1), 0, 2),       # generic, exact splits, float4 reduction
    ((2, 11, 9, 48, 40, 3, 1, 1), 1, 1),       # 48x64, Co = 40 ragged against 48, one ragged split
    ((1, 8, 6, 16, 48, 1, 1, 0), 1, 1),        # 48x64, one exact split, 16 of 64 columns
    ((1, 223, 220, 16, 40, 1, 1, 0), 1, 192),  # 48x64, 192 splits of 256 pixels, the last with 164
    ((2, 16, 16, 32, 48, 3, 1, 1), 1, 2),      # 48x64, exact splits
    ((2, 11, 9, 32, 64, 3, 1, 1), 2, 1),       # 64x64, one ragged split
    ((1, 8, 6, 32, 64, 1, 1, 0), 2, 1),        # 64x64, one exact split
    ((2, 23, 17, 36, 52, 3, 1, 1), 2, 4),      # 64x64, Co = 52 ragged against 64, 324 columns = 5 * 64 + 4, ragged last split
    ((2, 16, 16, 16, 64, 3, 1, 1), 2, 2),      # 64x64, exact splits
    ((2, 11, 9, 16, 96, 3, 1, 1), 3, 1),       # 96x64, one ragged split
    ((1, 8, 6, 16, 96, 1, 1, 0), 3, 1),        # 96x64, one exact split
    ((1, 223, 220, 16, 96, 1, 1, 0), 3, 192),  # 96x64, 192 splits, ragged last
    ((2, 16, 16, 16, 192, 3, 1, 1), 3, 2),     # 96x64, two row tiles, exact splits
    ((2, 11, 9, 32, 80, 3, 1, 1), 4, 1),       # 128x64, Co = 80 ragged against 128, one ragged split
    ((1, 8, 6, 16, 128, 1, 1, 0), 4, 1),       # 128x64, one exact split
    ((2, 13, 9, 48, 160, 3, 2, 1), 4, 1),      # 128x64, stride 2 on an odd size, two row tiles, the second with 32 rows
    ((2, 113, 109, 16, 128, 1, 1, 0), 4, 97),  # 128x64, 97 splits, ragged last
    ((2, 16, 16, 16, 128, 3, 1, 1), 4, 2),     # 128x64, exact splits
    ((2, 8, 6, 32, 32, 4, 2, 1), 1, 1),        # deconvolution geometry
    ((2, 12, 9, 384, 384, 3, 1, 1), 3, 1),     # 216 output columns tiles x 4 row tiles, one split
]

# ---- all 24 mantissa bits set, exponents spread over 2^40 inside a reduction (forward and data gradient) ---------------------
HARD_CASE = ((2, 9, 7, 48, 48, 3, 1, 1), 3)

# ---- guard bands: the C entry point writes into a slice of a sentinel-filled buffer ----------------------------------------
GUARD_FWD = (2, 9, 7, 20, 30, 3, 1, 1)          # scalar loads, ragged row and column tile
GUARD_DGRAD = (2, 13, 9, 16, 160, 3, 2, 1)      # parity classes, odd H and W
GUARD_WGRAD = (2, 23, 17, 36, 52, 3, 1, 1)      # four splits, ragged in Co, columns and pixels

# ---- the search grid of the closure test -----------------------------------------------------------------------------------
GRID_N = [1, 2, 3, 8, 32]
GRID_HW = [(1, 1), (1, 5), (6, 6), (7, 5), (8, 6), (11, 9), (12, 9), (13, 8), (16, 16), (23, 17), (64, 48), (113, 109), (160, 154)]
GRID_C = [3, 14, 16, 17, 20, 32, 40, 48, 64, 80, 96, 128, 160, 192, 256, 384]
GRID_GEO = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (7, 1, 3), (4, 2, 1)]        # (k, stride, pad)


def case_id(case):
    N, H, W, Ci, Co, k, s, p = case
    return f"{N}x{H}x{W}x{Ci}-{Co}k{k}s{s}p{p}"


def out_hw(case):
    N, H, W, Ci, Co, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def desc(case):
    from buctd_amd import _C
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = out_hw(case)
    return _C.ConvDesc(N, H, W, Ci, Co, k, k, s, p, Ho, Wo)


def plan(case, direction, flags=0):
    """buctd_conv2d_plan as a dict of PLAN_FIELDS, or None where the launch would refuse the call"""
    from buctd_amd import _C
    out = (C.c_int * len(PLAN_FIELDS))()
    d = desc(case)
    if _C.lib().buctd_conv2d_plan(C.byref(d), direction, flags, out) != 0:
        return None
    return dict(zip(PLAN_FIELDS, out))


def rows_of(case, direction):
    """rows of the GEMM (forward / data gradient) or reduction length (weight gradient)"""
    N, H, W = case[:3]
    Ho, Wo = out_hw(case)
    return N * H * W if direction == DGRAD else N * Ho * Wo
