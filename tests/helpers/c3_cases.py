"""The case table of the 3x3 / stride-1 / pad-1 bf16x6 convolution tests, as data.

A shape is (N, H, W, Ci, Co) of ONE kernel call: x [N][H][W][Ci] -> y [N][H][W][Co].  A forward option set runs it as the
convolution Ci -> Co, a data-gradient option set as the data gradient of a convolution Co -> Ci (dy has Ci channels, dx has
Co), so every option set of a case runs the tile plan that buctd_conv3x3_bf16x6_plan reports for the case.

tests/test_conv3x3_plan_cover.py (host only) proves that the table reaches every kernel variant the plan functions can pick;
tests/test_gpu_conv3x3_plan_cover.py runs every case x option set against fp64."""

# the train-mode option sets as the C3M_* mask of csrc/c3_lean.h; -1: none of them (bias / eval scale / partial sums / plain)
C3M_IN_BN, C3M_STATS, C3M_RES, C3M_BS_REBUILD, C3M_BS_Y = 1, 2, 4, 8, 16
OPTION_SETS = {
    "general": -1,
    "STATS": C3M_STATS,
    "STATS|IN_BN": C3M_STATS | C3M_IN_BN,
    "BS_REBUILD": C3M_BS_REBUILD,
    "RES|BS_Y": C3M_RES | C3M_BS_Y,
    "RES": C3M_RES,
}

# bench.py: --batch defaults to 32 images per GPU, and --step-graph captures the same batch
BENCH_BATCH = 32

# ---- the shapes the models run: every 3x3 / s1 / p1 convolution of HRNet-W48 at 384x288 and HRNet-W32 at 256x192 ----------
MODEL_CASES = [
    (BENCH_BATCH, 96, 72, 48, 48),     # W48 branch 0 (448-position single-buffer tiles)
    (BENCH_BATCH, 48, 36, 96, 96),     # W48 branch 1
    (BENCH_BATCH, 24, 18, 192, 192),   # W48 branch 2
    (BENCH_BATCH, 12, 9, 384, 384),    # W48 branch 3 (32-column tiles, column-major grid)
    (BENCH_BATCH, 64, 48, 32, 32),     # W32 branch 0
    (BENCH_BATCH, 32, 24, 64, 64),     # W32 branch 1
    (BENCH_BATCH, 16, 12, 128, 128),   # W32 branch 2
    (BENCH_BATCH, 8, 6, 256, 256),     # W32 branch 3
    (BENCH_BATCH, 96, 72, 64, 64),     # layer 1 Bottleneck conv2 at 384x288
    (BENCH_BATCH, 64, 48, 64, 64),     # layer 1 Bottleneck conv2 at 256x192
    (BENCH_BATCH, 96, 72, 256, 48),    # transition 1 -> W48 branch 0
    (BENCH_BATCH, 64, 48, 256, 32),    # transition 1 -> W32 branch 0
]

# ---- one small shape per kernel variant, ragged position tiles (N * H * W is no multiple of BM anywhere) -------------------
# comment: MF NF WMxWN [col = column-major grid] -> kernel for the train-mode option sets (general = conv3x3_x6_kernel)
VARIANT_CASES = [
    (2, 1, 37, 32, 16),       # 1 1 4x1, general only; H = 1, Ci > Co
    (3, 29, 1, 16, 48),       # 1 3 4x1, general only; W = 1
    (17, 31, 25, 16, 128),    # 1 4 2x2, general only
    (36, 31, 25, 32, 16),     # 2 1 4x1, general only
    (21, 3, 73, 16, 384),     # 2 3 2x2, general only
    (21, 3, 73, 192, 384),    # 2 3 2x2 col, general only
    (36, 31, 25, 16, 48),     # 2 3 4x1, general only
    (36, 47, 35, 32, 16),     # 4 1 4x1, general only
    (33, 96, 72, 16, 48),     # 8 3 4x1 single buffer (512-position tiles), general only
    (2, 7, 5, 16, 32),        # 1 2 4x1 -> family 1 variant 3
    (1, 7, 5, 384, 192),      # 1 2 4x1 col -> family 1 variant 3; Ci > Co
    (33, 31, 25, 16, 64),     # 1 4 4x1 -> family 1 variant 1
    (33, 1, 37, 16, 256),     # 2 2 4x1 -> family 0 variant 2; H = 1
    (33, 29, 1, 192, 384),    # 2 2 4x1 col -> family 0 variant 2; W = 1
    (33, 23, 19, 16, 128),    # 2 4 2x2 -> family 1 variant 5
    (33, 3, 73, 384, 256),    # 2 4 2x2 col -> family 1 variant 5; Ci > Co
    (36, 31, 25, 16, 64),     # 2 4 4x1 -> family 1 variant 4
    (33, 2, 74, 16, 192),     # 4 2 4x1 -> family 0 variant 4; W = 74 = MAX_SW - 1
    (17, 2, 74, 192, 384),    # 4 2 4x1 col -> family 0 variant 4; W = 74
    (36, 31, 25, 96, 96),     # 4 3 2x2 -> family 0 variant 1
    (33, 2, 74, 192, 384),    # 4 3 2x2 col -> family 0 variant 1; W = 74
    (36, 47, 35, 16, 48),     # 4 3 4x1 -> family 0 variant 3
    (21, 95, 71, 16, 48),     # 7 3 4x1 single buffer (448-position tiles) -> family 0 variant 0
]

CASES = MODEL_CASES + VARIANT_CASES

# ---- weight gradient: (N, H, W, Ci, Co) of the forward convolution; key (CF, nsplit == 1, rem == 0) ------------------------
WGRAD_MODEL_CASES = list(MODEL_CASES)
WGRAD_VARIANT_CASES = [
    (1, 6, 5, 32, 64),        # CF 2, one split
    (2, 7, 5, 64, 32),        # CF 2, even splits
    (20, 3, 73, 32, 192),     # CF 2, ragged splits
    (1, 6, 5, 96, 48),        # CF 3, one split
    (3, 7, 5, 48, 96),        # CF 3, even splits
    (17, 2, 74, 64, 48),      # CF 3 with a ragged last input chunk (Ci = 64), ragged splits; W = 74
    (5, 1, 37, 48, 48),       # H = 1
]
WGRAD_CASES = WGRAD_MODEL_CASES + WGRAD_VARIANT_CASES

# ---- guard bands: one ragged shape per kernel family (train-mode family 0, family 1, the general kernel), and per CF --------
GUARD_CASES = [(33, 2, 74, 16, 192), (33, 23, 19, 16, 128), (21, 3, 73, 16, 384)]
GUARD_WGRAD_CASES = [(20, 3, 73, 32, 192), (17, 2, 74, 96, 48)]     # CF 2, CF 3 (whole input chunks: x_bn)


# ---- the search grid of the closure test -----------------------------------------------------------------------------------
GRID_N = [1, 2, 3, 4, 8, 16, 20, 32, 36, 64]          # 36: the 512-position tiles need 229376 < P <= 262144 padded positions
GRID_HW = [(1, 1), (3, 73), (6, 5), (8, 6), (12, 9), (16, 12), (17, 13), (24, 18), (32, 24), (48, 36), (64, 48), (96, 72)]
GRID_C = [16, 32, 48, 64, 96, 128, 192, 256, 384]


def case_id(shape):
    return "x".join(str(v) for v in shape)
