"""Cases, code paths and fp64 references for the kernels that open and close a training step and a validation batch:
csrc/loss_decode.hip (joints MSE, arg-max decode, Gaussian target, condition render, flip-back merge, Adam, SGD) and
csrc/nms.hip.  CPU only: the case tables are plain tuples, path_of() restates the loop bounds and branches of the kernels
(file:line next to each), the operands are built from the case alone, the references are explicit float64 / integer
formulas that do not import buctd_amd.  tests/test_heatmap_cases_cover.py checks the tables against PATHS and the
references against the goldens, tests/test_gpu_heatmap_kernels.py runs them.

Longest chain of sequential fp32 additions of the MSE loss (n_seq of its bar, (n_seq + 8) 2^-24 of the sum of terms):
  mse_partial_kernel  ceil(HW / 256) per thread, 6 + 3 in block_sum_256, 1 product with w^2     loss_decode.hip:18-24
  mse_final_kernel    fp64 per thread, then 6 + 3 in block_sum_256                              loss_decode.hip:30-32
the 8: p - g enters squared (2), the square, w * w, fp64 -> fp32, 0.5 / denom, the product with it, and one to spare.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from tests.helpers.stream_cases import FLOOR, U, case_gen, ceil_div  # noqa: F401  (FLOOR, U: re-exported for the tests)


def f32(x):
    """the value a `float` argument of the C interface has"""
    return float(np.float32(x))


# ---- constants of the host functions, restated ------------------------------------------------------------------------------
BLOCK = 256
FLIP_GRID_CAP = 4096           # loss_decode.hip:613
ADAM_GRID_CAP = 4096           # loss_decode.hip:661 (workgroups of 256 float4)
SGD_GRID_CAP = 8192            # loss_decode.hip:690
COND_MAX_K = 64                # loss_decode.hip:554
NMS_COLS = 64                  # nms.hip:34: boxes per column block (one wavefront)

# ---- case tables ------------------------------------------------------------------------------------------------------------
# joints_mse: (N, K, HW, w: "w" | "null" | "zero-rows", grad wanted, gscale)
MSE = ([(2, 3, HW, "w", 1, 1.0) for HW in (1, 255, 256, 257, 432)] +
       [(1, 1, 40, "null", 0, 1.0), (16, 16, 5, "w", 1, 0.125), (257, 1, 3, "null", 1, 1.0), (3, 86, 35, "w", 0, 0.125),
        (3, 86, 257, "zero-rows", 1, 1.0), (5, 14, 432, "zero-rows", 1, 0.125)])

# arg-max (plain and refined entry on every case): (H, W, kind)
ARGMAX_SHAPES = ((1, 1), (5, 8), (10, 10), (16, 16), (1, 257), (257, 1), (24, 18), (7, 5))
ARGMAX = ([(H, W, kind) for (H, W) in ARGMAX_SHAPES for kind in ("random", "ties", "special") if H * W > 1 or kind != "ties"] +
          [(H, W, "quarter") for (H, W) in ((24, 18), (7, 5), (16, 16), (5, 8), (4, 4), (3, 9), (9, 3))])

# gaussian_target: (Hh, Wh, stride_x, stride_y, sigma)
GAUSS = [(Hh, Wh, sx, sy, sg) for (Hh, Wh) in ((5, 4), (16, 12), (24, 18)) for (sx, sy) in ((4.0, 4.0), (4.0, 8.0))
         for sg in (1.0, 2.0, 3.0, 1.5)]
GAUSS_VIS = (0.0, 0.3, 0.5, 0.51, 1.0)

# cond_render: (H, W, Cc, K, js, truncate, into: 0 = buctd_cond_render, 1 = buctd_cond_render_into with a gap of 37 floats)
COND_B = 3                     # batch members: key points everywhere / every key point rejected / the border set alone
COND_GAP = 37
COND = [(2, 2, 1, 1, 2, 0, 0), (2, 2, 3, 17, 3, 1, 0),
        (3, 9, 3, 1, 2, 0, 0), (3, 9, 4, 64, 3, 0, 1), (3, 9, 1, 17, 2, 1, 0),
        (8, 8, 1, 17, 2, 1, 1), (8, 8, 4, 17, 3, 0, 0),
        (15, 16, 3, 17, 2, 0, 0), (15, 16, 1, 64, 2, 1, 0),
        (33, 31, 3, 64, 3, 0, 1), (33, 31, 1, 17, 2, 1, 0), (33, 31, 4, 1, 2, 0, 0),
        (64, 48, 3, 17, 2, 0, 0), (64, 48, 1, 64, 3, 1, 1), (64, 48, 4, 64, 2, 0, 0), (64, 48, 3, 17, 2, 1, 0)]

# flipback_avg: (N, K, H, W, perm: "identity" | "swapped", shift)
FLIP_LONG_N = 174              # x 14 x 24 x 18 = 1052352 elements, just over 4096 * 256
FLIP = [(1, 1, 1, 1, "identity", 0), (2, 1, 3, 1, "identity", 1), (3, 1, 5, 2, "identity", 1), (1, 14, 2, 2, "swapped", 1),
        (1, 14, 3, 1, "swapped", 0), (2, 14, 24, 18, "swapped", 1), (2, 14, 24, 18, "swapped", 0), (2, 14, 24, 18, "identity", 0),
        (FLIP_LONG_N, 14, 24, 18, "swapped", 1)]

# adam_step: (n, first step number, gscale, mode: "one" step | "three" chained steps | "zero" gradient and state)
ADAM_LONG = 4 * ADAM_GRID_CAP * 256 + 4 * 256 + 3
ADAM = ([(n, 1, 1.0, "one") for n in (1, 3, 4, 5, 1023, 1027, ADAM_LONG)] +
        [(5, 2, 0.25, "one"), (1027, 1000, 0.25, "one"), (1023, 1, 1.0, "three"), (1027, 2, 0.25, "three"),
         (3, 1000, 1.0, "zero"), (1027, 1, 0.25, "zero")])
ADAM_HYPER = (1e-3, 0.9, 0.999, 1e-8)          # lr, beta1, beta2, eps: torch.optim.Adam's defaults, the BUCTD recipe

# sgd_step: (n, mu, nesterov, wd, first, gscale, element offset of the slice in its allocation)
SGD_LONG = SGD_GRID_CAP * 256 + 259
SGD_FORMS = ((0.0, 0, 0.0, 0, 1.0), (0.9, 0, 1e-4, 1, 1.0), (0.9, 0, 1e-4, 0, 1.0), (0.9, 1, 0.0, 0, 1.0), (0.9, 1, 1e-2, 0, 0.5))
SGD = ([(n,) + f + (0,) for n in (1, 255, 257) for f in SGD_FORMS] +
       [(SGD_LONG,) + SGD_FORMS[4] + (0,), (SGD_LONG,) + SGD_FORMS[0] + (0,)] +
       [(257,) + SGD_FORMS[2] + (3,), (255,) + SGD_FORMS[4] + (1,), (1,) + SGD_FORMS[0] + (5,)])
SGD_LR = 0.05

# nms: (n, boxes_dim, kind, thresh)
NMS_N = (1, 63, 64, 65, 129, 200)
NMS = ([(n, 4 + (i % 2), "disjoint", 0.5) for i, n in enumerate(NMS_N)] +
       [(n, 5 - (i % 2), "identical", 0.5) for i, n in enumerate(NMS_N)] +
       [(n, 5, "chain", 0.5) for n in (63, 65, 129, 200)] +
       [(n, 4 + (i % 2), "threshold", 0.5) for i, n in enumerate((63, 64, 65, 129, 200))] +
       [(n, 5, "random", t) for n, t in ((63, 0.3), (64, 0.5), (65, 0.7), (129, 0.3), (200, 0.5), (200, 0.7))])


# ---- arg-max operands -------------------------------------------------------------------------------------------------------
def tie_pairs(HW):
    """(i, j, name), i < j < HW: the two positions of one row that hold the same maximum (block_argmax_256,
    loss_decode.hip:215-241: thread t reads t, t + 256, ...; lanes of a wave meet in the shuffles, waves in LDS)"""
    want = [(0, 256, "tie:same-thread"), (HW - 257, HW - 1, "tie:same-thread"), (1, 2, "tie:same-wave"), (3, 40, "tie:same-wave"),
            (0, 63, "tie:same-wave"), (63, 64, "tie:across-waves"), (5, 69, "tie:across-waves"), (70, 200, "tie:across-waves"),
            (10, 300, "tie:across-trips"), (255, 256, "tie:across-trips"), (0, HW - 1, "tie:first-and-last")]
    out = []
    for i, j, name in want:
        if 0 <= i < j < HW and (i, j) not in [(a, b) for a, b, _ in out]:
            out.append((i, j, name))
    return out


def quarter_rows(H, W):
    """(py, px, horizontal, vertical): peaks next to every border, neighbours equal / higher on one side"""
    xs = sorted({v for v in (1, 2, W - 2, W - 1) if 0 <= v < W})
    ys = sorted({v for v in (1, 2, H - 2, H - 1) if 0 <= v < H})
    rows = []
    for a, py in enumerate(ys):
        for b, px in enumerate(xs):
            for c, hor in enumerate(("equal", "left", "right")):
                rows.append((py, px, hor, ("up", "equal", "down")[(a + b + c) % 3]))
    return rows


def quarter_eligible(H, W, py, px):            # loss_decode.hip:275, reference core/inference.py:68-77
    return 1 < px < W - 1 and 1 < py < H - 1


def argmax_operand(case):
    """-> hm [rows, H * W] fp32 and, per row, the name of what the row is for"""
    H, W, kind = case
    HW = H * W
    g = case_gen("argmax", case)
    rows, names = [], []

    def base(lo, hi):
        return torch.rand(HW, generator=g) * (hi - lo) + lo
    if kind == "random":
        for k in range(6):
            rows.append(torch.randn(HW, generator=g))
            names.append("random")
    elif kind == "ties":
        for i, j, name in tie_pairs(HW):
            r = base(-1.0, 0.5)
            r[i] = r[j] = 2.0
            rows.append(r)
            names.append(name)
            r = base(-1.0, 0.5)                 # not a tie: the later, higher one wins
            r[i], r[j] = 2.0, 3.0
            rows.append(r)
            names.append("later-higher")
    elif kind == "special":
        p, q = HW // 3, (2 * HW) // 3 + (1 if HW > 3 else 0)
        q = min(q, HW - 1)
        rows.append(torch.full((HW,), 0.5)); names.append("row:constant")
        r = base(-1.0, -0.1); r[p] = 0.0; r[q] = 0.0
        rows.append(r); names.append("row:max-zero")
        r = base(-3.0, -0.5); r[q] = -0.25
        rows.append(r); names.append("row:max-negative")
        rows.append(torch.full((HW,), float("-inf"))); names.append("row:all-neg-inf")
        r = base(-1.0, 1.0); r[p] = float("inf"); r[q] = float("inf")
        rows.append(r); names.append("row:pos-inf")
    else:
        for py, px, hor, ver in quarter_rows(H, W):
            r = base(0.0, 0.3).view(H, W)
            r[py, px] = 1.0
            lo, hi = {"equal": (0.5, 0.5), "left": (0.7, 0.4), "right": (0.4, 0.7)}[hor]
            if px - 1 >= 0:
                r[py, px - 1] = lo
            if px + 1 < W:
                r[py, px + 1] = hi
            lo, hi = {"equal": (0.5, 0.5), "up": (0.7, 0.4), "down": (0.4, 0.7)}[ver]
            if py - 1 >= 0:
                r[py - 1, px] = lo
            if py + 1 < H:
                r[py + 1, px] = hi
            rows.append(r.reshape(-1)); names.append("quarter")
        r = base(-1.0, -0.5).view(H, W)         # a masked peak: every value <= 0, the neighbours differ
        py, px = min(2, H - 1), min(2, W - 1)
        r[py, px] = -0.1
        if px + 1 < W:
            r[py, px + 1] = -0.2
        if py + 1 < H:
            r[py + 1, px] = -0.2
        rows.append(r.reshape(-1)); names.append("quarter:masked")
    return torch.stack(rows).contiguous(), names


def argmax_ref(hm, H, W):
    """get_max_preds (reference core/inference.py:19-47) and the quarter offsets of get_final_preds (:68-77) -> idx int32
    [rows], preds fp32 [rows, 2], maxvals fp32 [rows], quarter fp32 [rows, 2]; comparisons only, so exact"""
    x = hm.double().numpy()
    idx = x.argmax(1)
    mx = x.max(1)
    keep = (mx > 0.0)
    preds = np.stack([idx % W, idx // W], 1).astype(np.float64) * keep[:, None]
    quarter = np.zeros_like(preds)
    for r in range(x.shape[0]):
        px, py = int(math.floor(preds[r, 0] + 0.5)), int(math.floor(preds[r, 1] + 0.5))
        if 1 < px < W - 1 and 1 < py < H - 1:
            m = x[r].reshape(H, W)
            quarter[r] = np.sign([m[py, px + 1] - m[py, px - 1], m[py + 1, px] - m[py - 1, px]]) * 0.25
    return (torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(preds.astype(np.float32)),
            torch.from_numpy(mx.astype(np.float32)), torch.from_numpy(quarter.astype(np.float32)))


# ---- Gaussian target operands and reference ---------------------------------------------------------------------------------
def gauss_box(mu, tmp):
    """ul, br of the reference (JointsDataset.py:411-412): int() truncates toward zero, tmp = sigma * 3 need not be whole"""
    return int(mu - tmp), int(mu + tmp + 1)


def gauss_joints(case):
    """-> [(name, jx, jy, vis)]: every integer centre along the middle row and the middle column from well outside one border
    to well outside the other (so each side is clipped, just inside its "outside" test and just outside it), the corners,
    negative coordinates that truncate toward zero, every visibility, and centres off the stride grid.  All coordinates are
    multiples of 1/8: fp32 and fp64 agree on every int(x / stride + 0.5)."""
    Hh, Wh, sx, sy, sigma = case
    reach = int(sigma * 3) + 4
    cx, cy = Wh // 2, Hh // 2
    out = []
    for mx in range(-reach, Wh + reach + 1):
        out.append(("sweep-x", mx * sx, cy * sy, 1.0))
    for my in range(-reach, Hh + reach + 1):
        out.append(("sweep-y", cx * sx, my * sy, 1.0))
    for mx in (0, Wh - 1):
        for my in (0, Hh - 1):
            out.append(("corner", mx * sx, my * sy, 1.0))
    # x / s + 0.5 in (-1, 0): int() gives 0 where floor would give -1; in (-2, -1): -1 where floor would give -2
    out += [("trunc", -0.75 * sx, -0.625 * sy, 1.0), ("trunc", -1.75 * sx, cy * sy, 1.0), ("trunc", cx * sx, -1.625 * sy, 1.0)]
    for v in GAUSS_VIS:
        out.append(("vis", cx * sx, cy * sy, v))
        out.append(("vis-outside", (Wh + reach) * sx, cy * sy, v))
    out += [("off-grid", cx * sx + 1.125, cy * sy - 0.875, 1.0), ("off-grid", cx * sx - 0.5 * sx, cy * sy + 0.5 * sy - 0.125, 0.51)]
    if len(out) % 2:
        out.append(("vis", cx * sx, cy * sy, 1.0))
    return out


def gauss_operand(case):
    """-> joints fp32 [2, K, 3], vis fp32 [2, K]"""
    js = gauss_joints(case)
    joints = torch.tensor([[j[1], j[2], 0.0] for j in js], dtype=torch.float32).view(2, -1, 3)
    assert torch.equal(joints * 8, torch.round(joints * 8)), "coordinates are multiples of 1/8"
    return joints.contiguous(), torch.tensor([j[3] for j in js], dtype=torch.float32).view(2, -1).contiguous()


def gauss_ref(joints, vis, case):
    """generate_target (reference JointsDataset.py:397-453) in float64, one map at a time -> target [B, K, Hh, Wh] fp64,
    weight [B, K] fp32 (exact)"""
    Hh, Wh, sx, sy, sigma = case
    B, K = vis.shape
    target = np.zeros((B, K, Hh, Wh))
    weight = vis.numpy().astype(np.float32).copy()
    tmp = sigma * 3
    size = 2 * tmp + 1
    c0 = size // 2
    ax = np.arange(0, size, 1, dtype=np.float64)
    gauss = np.exp(-((ax[None, :] - c0) ** 2 + (ax[:, None] - c0) ** 2) / (2 * sigma ** 2))
    for b in range(B):
        for k in range(K):
            mu_x = int(float(joints[b, k, 0]) / sx + 0.5)
            mu_y = int(float(joints[b, k, 1]) / sy + 0.5)
            (ulx, brx), (uly, bry) = gauss_box(mu_x, tmp), gauss_box(mu_y, tmp)
            if ulx >= Wh or uly >= Hh or brx < 0 or bry < 0:
                weight[b, k] = 0
                continue
            gx0, gx1 = max(0, -ulx), min(brx, Wh) - ulx
            gy0, gy1 = max(0, -uly), min(bry, Hh) - uly
            ix0, ix1 = max(0, ulx), min(brx, Wh)
            iy0, iy1 = max(0, uly), min(bry, Hh)
            if weight[b, k] > 0.5:
                target[b, k, iy0:iy1, ix0:ix1] = gauss[gy0:gy1, gx0:gx1]
    return torch.from_numpy(target), torch.from_numpy(weight)


# ---- condition render operands and reference --------------------------------------------------------------------------------
def cond_taps():
    """cv2.getGaussianKernel(15, 0): sigma 0.3 * ((15 - 1) * 0.5 - 1) + 0.8, normalised to sum 1, float64"""
    sigma = 0.3 * ((15 - 1) * 0.5 - 1) + 0.8
    x = np.arange(15, dtype=np.float64) - 7
    k = np.exp(-(x * x) / (2 * sigma * sigma))
    return k / k.sum()


def reflect101(i, n):
    """BORDER_REFLECT_101 as a closed form: the extension has period 2 (n - 1)"""
    if n == 1:
        return 0
    m = i % (2 * (n - 1))
    return m if m < n else 2 * (n - 1) - m


def blur_matrix(n):
    """[n, n] float64: row o holds the taps of output o, folded back at the borders"""
    A = np.zeros((n, n))
    for o in range(n):
        for d, t in zip(range(-7, 8), cond_taps()):
            A[o, reflect101(o + d, n)] += t
    return A


def cond_colors(Cc, K):
    """[K, Cc] fp32, whole numbers in 13..255 (None for the mono form)"""
    if Cc == 1:
        return None
    g = case_gen("cond_colors", (Cc, K))
    return torch.randint(13, 256, (K, Cc), generator=g).float()


def cond_operand(case):
    """-> joints fp32 [3, K, js].  Member 0: the border / corner / duplicate / rejected set, then random points; member 1:
    every key point rejected; member 2: the first of the set alone (K = 1), or the set in reverse (so the colour that wins a
    shared pixel is another one)."""
    H, W, Cc, K, js, trunc, into = case
    g = case_gen("cond", case)
    xm, ym = max(1, W // 2), max(1, H // 2)
    special = [(1.0, 1.0), (W - 1.0, H - 1.0), (1.9, H - 1.0), (W - 1.0, 1.5),             # the four corners (px 0 / W - 2)
               (xm + 0.25, 1.0), (xm + 0.5, H - 1.0), (1.0, ym + 0.75), (W - 1.0, ym + 0.125),     # one on each border
               (min(4.0, W - 1.0), min(5.0, H - 1.0)), (max(1.0, W - 5.0), max(1.0, H - 3.0)),     # within 7 px of two borders
               (xm + 0.0, ym + 0.0), (xm + 0.9, ym + 0.9),                                  # duplicates on one pixel
               (0.4, ym + 0.0), (W + 0.0, ym + 0.0), (xm + 0.0, 0.99), (xm + 0.0, H + 0.5),        # rejected: kx <= 0, kx >= W, ...
               (-3.5, ym + 0.0), (-0.5, -0.5), (xm + 0.0, -2.0)]
    rejected = [(0.4, 1.0), (W + 0.0, 1.0), (1.0, H + 3.0), (-3.5, 1.0), (-0.5, -0.5), (1.0, 0.0), (W + 9.0, -7.0)]
    pts = np.zeros((COND_B, K, js), dtype=np.float32)
    rnd = torch.rand(K, 2, generator=g).numpy() * np.array([W + 1.0, H + 1.0]) - 0.5
    for k in range(K):
        pts[0, k, :2] = special[k] if k < len(special) else rnd[k]
        pts[1, k, :2] = rejected[k % len(rejected)]
    pts[2, :, :2] = pts[0, ::-1, :2]
    if js > 2:
        pts[:, :, 2:] = torch.rand(COND_B, K, js - 2, generator=g).numpy()      # scores: not read by the kernel
    return torch.from_numpy(pts)


def cond_accept(joints_b, H, W):
    """the reference's acceptance rule (JointsDataset.py:500-543): np.array(kpts).astype(int) truncates toward zero, a key
    point counts when 0 < kx < W and 0 < ky < H and is written at [ky - 1][kx - 1] -> [(k, py, px)] in key-point order"""
    out = []
    for k, kp in enumerate(np.asarray(joints_b)):
        kx, ky = int(kp[0]), int(kp[1])
        if 0 < kx < W and 0 < ky < H:
            out.append((k, ky - 1, kx - 1))
    return out


def cond_ref(joints, colors, case):
    """-> ref fp64 [B, Cc, H, W] (the dense 15-tap separable reflect-101 blur of the impulse image, peak-normalised to 255 per
    batch member over all channels; an empty image stays zero), cnt [B]: distinct impulse pixels per member"""
    H, W, Cc, K, js, trunc, into = case
    AH, AW = blur_matrix(H), blur_matrix(W)
    B = joints.shape[0]
    ref = np.zeros((B, Cc, H, W))
    cnt = []
    col = None if colors is None else colors.double().numpy()
    for b in range(B):
        z = np.zeros((Cc, H, W))
        hit = set()
        for k, py, px in cond_accept(joints[b].numpy(), H, W):
            z[:, py, px] = 255.0 if col is None else col[k]      # a later key point overwrites the colour
            hit.add((py, px))
        cnt.append(len(hit))
        blurred = np.einsum("oy,cyx,px->cop", AH, z, AW)
        am = blurred.max()
        ref[b] = blurred if am == 0 else blurred / (am / 255)
    return torch.from_numpy(ref), cnt


def cond_bar(ref, cnt):
    """|err| <= 2 (cnt + 40) 2^-24 ref + 255 * 2^-23: every term is non-negative; a tap response is the sum of at most 15
    fp32 taps (twice), the products, cnt additions, and the same again in the maximum the image is divided by"""
    c = torch.tensor(cnt, dtype=torch.float64).view(-1, 1, 1, 1)
    return 2 * (c + 40) * U * ref + 255 * FLOOR


def cond_band(ref, cnt):
    """pixels whose truncated value may differ by one: non-zero and within the bar of a whole number"""
    return (ref != 0) & ((ref - torch.round(ref)).abs() <= cond_bar(ref, cnt))


def cond_band_fraction():
    """over all truncate cases together: the fraction of pixels in the band (every non-empty image has its peak of exactly 255
    in it, which is most of it)"""
    band = total = 0
    for case in COND:
        if case[5]:
            j = cond_operand(case)
            ref, cnt = cond_ref(j, cond_colors(case[2], case[3]), case)
            band += int(cond_band(ref, cnt).sum())
            total += ref.numel()
    return band / total


# ---- flip-back --------------------------------------------------------------------------------------------------------------
FLIP_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]         # CrowdPose (reference dataset/crowdpose.py:49-50)


def flip_perm(K, kind):
    perm = list(range(K))
    if kind == "swapped":
        for a, b in FLIP_PAIRS:
            if b < K:
                perm[a], perm[b] = b, a
    return perm


def flip_operand(case):
    """a, b fp32 [N, K, H, W] with |x| in [2^-20, 16): the fp64 sum of two of them is exact, so its rounding to fp32 is the
    one fp32 addition of the kernel"""
    N, K, H, W, kind, shift = case
    g = case_gen("flip", case)

    def one():
        t = torch.randn(N, K, H, W, generator=g).clamp(-15.0, 15.0)
        return torch.where(t.abs() < 2.0 ** -20, torch.full_like(t, 2.0 ** -20), t)
    return one(), one()


def flip_ref(a, b, perm, shift):
    """the flip-test merge (reference core/function.py:226-236, utils/transforms.py:16-30) -> fp32, exact"""
    fb = b.double().flip(3)[:, perm]            # flip_back: mirror, then out[:, a] <-> out[:, b]: out[:, k] = mirrored[:, perm[k]]
    if shift:
        sh = fb.clone()
        sh[:, :, :, 1:] = fb[:, :, :, :-1]
        fb = sh
    return ((a.double() + fb) * 0.5).float()


# ---- Adam / SGD -------------------------------------------------------------------------------------------------------------
def adam_operand(case):
    """-> p, m, v and one gradient per step (fp32).  p is small, so that the update (about lr) is a visible part of it."""
    n, step, gscale, mode = case
    g = case_gen("adam", (n, step, mode))
    p = torch.randn(n, generator=g) * 0.01
    steps = 3 if mode == "three" else 1
    if mode == "zero":
        return p, torch.zeros(n), torch.zeros(n), [torch.zeros(n)]
    if step > 1:
        m, v = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, m, v, [torch.randn(n, generator=g) for _ in range(steps)]


def adam_bias(step, b1, b2):
    """what buctd_adam_step passes on (loss_decode.hip:658-663): bc1, sqrt(bc2) from the fp32 betas, in fp64"""
    return 1.0 - f32(b1) ** step, math.sqrt(1.0 - f32(b2) ** step)


def adam_ref(p, g, m, v, step, gscale, dtype):
    """torch.optim.Adam (no amsgrad, no weight decay) in the kernel's order (loss_decode.hip:637-640) -> p, m, v in `dtype`.
    float64: the fp32-rounded lr, betas, eps, gscale the kernel receives, everything else in fp64; float32: its own steps"""
    lr, b1, b2, eps = (f32(x) for x in ADAM_HYPER)
    bc1, bc2s = adam_bias(step, b1, b2)
    if dtype == torch.float32:
        S = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
        bc1, bc2s = S(bc1), S(bc2s)
        lr, b1, b2, eps, gs, one = S(lr), S(b1), S(b2), S(eps), S(f32(gscale)), S(1.0)
        step_size = lr / bc1
    else:
        gs, one = f32(gscale), 1.0
        step_size = lr / bc1
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    gg = g * gs
    m = b1 * m + (one - b1) * gg
    v = b2 * v + (one - b2) * gg * gg
    denom = torch.sqrt(v) / bc2s + eps
    return p - step_size * (m / denom), m, v


def sgd_operand(case):
    n = case[0]
    g = case_gen("sgd", (n, case[6]))
    return torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)


def sgd_ref(p, g, buf, case, dtype):
    """torch.optim.SGD (dampening 0) in the kernel's order (loss_decode.hip:676-683) -> p, buf (None without momentum)"""
    n, mu, nesterov, wd, first, gscale, off = case
    if dtype == torch.float32:
        S = lambda x: torch.tensor(f32(x), dtype=torch.float32)      # noqa: E731
    else:
        S = f32
    lr, mu_, wd_, gs = S(SGD_LR), S(mu), S(wd), S(gscale)
    p, g, buf = (t.to(dtype) for t in (p, g, buf))
    gg = g * gs + wd_ * p
    if mu != 0.0:
        b = gg if first else mu_ * buf + gg
        gg = gg + mu_ * b if nesterov else b
    else:
        b = None
    return p - lr * gg, b


# ---- NMS --------------------------------------------------------------------------------------------------------------------
def nms_chains(n):
    """index triples (A, B, C), A < B < C: A kills B, so C - which only B would have killed - survives"""
    out = [(64 * m - 2, 64 * m - 1, 64 * m) for m in range(1, 4) if 64 * m < n]
    if n >= 8:
        out.append((1, 3, 6))
    if n >= 140:
        out.append((20, 21, 139))               # B and C two column blocks apart
    return out


def nms_boxes(case):
    """-> boxes fp32 [n, dim], whole-number coordinates, scores (dim 5) strictly descending"""
    n, dim, kind, thresh = case
    b = np.zeros((n, 4), dtype=np.int64)
    cell = lambda i: (40 * (i % 16), 40 * (i // 16))      # noqa: E731  disjoint 40 x 40 cells
    if kind in ("disjoint", "chain", "threshold"):
        for i in range(n):
            x, y = cell(i)
            b[i] = (x, y, x + 9, y + 9)
    if kind == "identical":
        b[:] = (3, 5, 40, 27)
    elif kind == "chain":
        for A, B, C in nms_chains(n):
            x, y = cell(A)
            b[A] = (x, y, x + 9, y + 9)
            b[B] = (x, y + 2, x + 9, y + 11)     # IoU(A, B) = 80 / 120
            b[C] = (x, y + 5, x + 9, y + 14)     # IoU(B, C) = 70 / 130, IoU(A, C) = 50 / 150
    elif kind == "threshold":
        for i in range(1, n - 1, 2):             # pairs (1, 2), (3, 4), ... (63, 64), ...: the second lies inside the first
            x, y = cell(i)
            b[i] = (x, y, x + 9, y + 9)
            b[i + 1] = (x, y, x + 9, y + 4) if (i // 2) % 3 != 2 else (x, y, x + 9, y + 5)     # IoU exactly 1/2 | 6/10
    elif kind == "random":
        rng = np.random.RandomState(1000 * n + int(thresh * 10))
        c = rng.randint(0, 120, size=(n, 2))
        wh = rng.randint(8, 60, size=(n, 2))
        b = np.concatenate([c, c + wh], 1).astype(np.int64)
    out = np.zeros((n, dim), dtype=np.float32)
    out[:, :4] = b
    if dim == 5:
        out[:, 4] = 1.0 - np.arange(n, dtype=np.float32) / (n + 1)
    return torch.from_numpy(out)


def nms_over(boxes, thresh):
    """[n, n] bool: box j overlaps box i by more than thresh, decided in exact integer arithmetic: inter * den > num * union with
    thresh = num / den the fp32 value the kernel receives (the device rule is `>`, nms.hip:49).  Asserts that no pair lies
    within 1e-6 of the threshold without being exactly on it."""
    b = boxes[:, :4].numpy().astype(np.int64)
    assert np.array_equal(b, boxes[:, :4].numpy()), "whole-number coordinates"
    t = Fraction(f32(thresh))
    x1, y1, x2, y2 = (b[:, i] for i in range(4))
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    w = np.clip(np.minimum(x2[:, None], x2[None, :]) - np.maximum(x1[:, None], x1[None, :]) + 1, 0, None)
    h = np.clip(np.minimum(y2[:, None], y2[None, :]) - np.maximum(y1[:, None], y1[None, :]) + 1, 0, None)
    inter = w * h
    union = area[:, None] + area[None, :] - inter
    lhs, rhs = inter * t.denominator, union * t.numerator
    near = np.abs(inter / union - float(t)) < 1e-6
    assert not (near & (lhs != rhs)).any(), "a pair lies within 1e-6 of the threshold"
    return lhs > rhs


def nms_ref(boxes, thresh):
    """greedy suppression by descending score (the order of the rows) on nms_over() -> keep list"""
    over = nms_over(boxes, thresh)
    n = over.shape[0]
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if not dead[i]:
            keep.append(i)
            dead[i + 1:] |= over[i, i + 1:]
    return keep


def nms_mask_ref(boxes, thresh):
    """the suppression words the sweep reads (nms.hip:28-29, :68: word c of row r for c >= r / 64): bit i of mask[r][c] is set
    when box 64 c + i comes after box r and overlaps it by more than thresh -> int64 [n, col_blocks], bool [n, col_blocks]: read"""
    over = nms_over(boxes, thresh)
    n = over.shape[0]
    cb = ceil_div(n, NMS_COLS)
    later = np.triu(over, 1)
    bits = np.zeros((n, cb * NMS_COLS), dtype=np.uint64)
    bits[:, :n] = later
    words = (bits.reshape(n, cb, NMS_COLS) << np.arange(NMS_COLS, dtype=np.uint64)).sum(2, dtype=np.uint64)
    read = np.arange(cb)[None, :] >= (np.arange(n) // NMS_COLS)[:, None]
    return torch.from_numpy(words.view(np.int64).copy()), torch.from_numpy(read)


# ---- joints MSE -------------------------------------------------------------------------------------------------------------
def mse_operand(case):
    N, K, HW, wmode, grad, gscale = case
    g = case_gen("mse", case)
    pred, gt = torch.randn(N, K, HW, generator=g), torch.rand(N, K, HW, generator=g)
    if wmode == "null":
        return pred, gt, None
    w = 0.25 + torch.rand(N, K, generator=g)
    if wmode == "zero-rows":
        w[:, ::3] = 0.0
        w[0] = 0.0
    return pred, gt, w


def mse_ref(pred, gt, w, gscale, dtype=torch.float64):
    """JointsMSELoss (reference core/loss.py:23-41) in closed form: L = 0.5 / (K N HW) sum w^2 (p - g)^2 and its gradient
    times gscale, in the kernel's order (loss_decode.hip:19-24, :44-49) -> loss, grad"""
    N, K, HW = pred.shape
    d = pred.to(dtype) - gt.to(dtype)
    w2 = torch.ones(N, K, dtype=dtype) if w is None else w.to(dtype) * w.to(dtype)
    loss = 0.5 * (w2[:, :, None] * d * d).sum() / (K * N * HW)
    if dtype == torch.float32:
        gcoef = torch.tensor(f32(gscale), dtype=dtype) / torch.tensor(float(K * N * HW), dtype=dtype)
    else:
        gcoef = f32(gscale) / (K * N * HW)
    return loss, (gcoef * w2)[:, :, None] * d


def mse_n_seq(case):
    return ceil_div(case[2], BLOCK) + 9 + 1 + 9


# ---- paths ------------------------------------------------------------------------------------------------------------------
def grid_trips(items, cap):
    """trips of the busiest thread of a grid-stride loop of min(cap, ceil(items / 256)) workgroups"""
    return ceil_div(items, max(1, min(cap, ceil_div(items, BLOCK))) * BLOCK)


def _row_loop(n, what):        # a 256-thread loop `for (i = threadIdx.x; i < n; i += 256)`
    if n < BLOCK:
        return what + ":idle-threads"
    return what + (":one-trip" if n == BLOCK else ":tail-trip" if n % BLOCK else ":whole-trips")


def _grid(items, cap):
    return "grid:partial-block" if items < BLOCK else "grid:one-trip" if grid_trips(items, cap) == 1 else "grid:second-trip"


def path_of(kernel, case):
    """-> the set of path names `case` takes through `kernel` (every name is listed in PATHS[kernel])"""
    if kernel == "joints_mse":
        N, K, HW, wmode, grad, gscale = case
        return {_row_loop(HW, "partial"),                              # loss_decode.hip:18
                _row_loop(N * K, "final").replace("tail-trip", "second-trip"),       # loss_decode.hip:30
                "w:" + wmode, "grad:%d" % grad, "gscale:%g" % gscale}     # :15, :21, :46
    if kernel == "argmax":
        H, W, kind = case
        HW = H * W
        names = {"kind:" + kind,                                       # loss_decode.hip:215: the row loop, by waves
                 "hw:1" if HW == 1 else "hw:part-wave" if HW < 64 else "hw:idle-waves" if HW < 192 else _row_loop(HW, "hw")}
        names.add("shape:W=1" if W == 1 and H > 1 else "shape:H=1" if H == 1 and W > 1 else "shape:square" if H == W else "shape:non-square")
        if kind == "ties":
            names |= {name for _, _, name in tie_pairs(HW)} | {"later-higher"}      # :217, :226, :238
        if kind == "special":
            names |= {"row:constant", "row:max-zero", "row:max-negative", "row:all-neg-inf", "row:pos-inf"}     # :251, :273
        if kind == "quarter":                                          # loss_decode.hip:275-280
            names.add("quarter:masked")
            if H < 4 or W < 4:
                names.add("quarter:map-below-4")
            for py, px, hor, ver in quarter_rows(H, W):
                if quarter_eligible(H, W, py, px):
                    names |= {"quarter:eligible", "quarter:x-" + hor, "quarter:y-" + ver}
                    names |= {"quarter:px=2"} if px == 2 else set()
                    names |= {"quarter:px=W-2"} if px == W - 2 else set()
                    names |= {"quarter:py=2"} if py == 2 else set()
                    names |= {"quarter:py=H-2"} if py == H - 2 else set()
                else:
                    for v, lim, ax in ((px, W, "px"), (py, H, "py")):
                        if v <= 1:
                            names.add("quarter:%s<=1" % ax)
                        if v >= lim - 1:
                            names.add("quarter:%s=%s-1" % (ax, "W" if ax == "px" else "H"))
        return names
    if kernel == "gaussian_target":
        Hh, Wh, sx, sy, sigma = case
        tmp = sigma * 3
        names = {"sigma:%g" % sigma, "stride:square" if sx == sy else "stride:non-square",
                 _row_loop(Hh * Wh, "pixels")}                         # loss_decode.hip:429
        for name, jx, jy, vis in gauss_joints(case):
            fx, fy = jx / sx + 0.5, jy / sy + 0.5
            mu_x, mu_y = int(fx), int(fy)
            if (fx < 0 and fx != math.floor(fx)) or (fy < 0 and fy != math.floor(fy)):
                names.add("mu:truncates-toward-zero")                  # :423
            (ulx, brx), (uly, bry) = gauss_box(mu_x, tmp), gauss_box(mu_y, tmp)
            out = [n for n, c in (("outside:ulx>=W", ulx >= Wh), ("outside:uly>=H", uly >= Hh), ("outside:brx<0", brx < 0),
                                  ("outside:bry<0", bry < 0)) if c]      # :425
            names |= set(out)
            names.add("vis:%g" % vis if not out else "vis:any-outside")
            if out:
                continue
            names |= {n for n, c in (("edge:brx==0", brx == 0), ("edge:bry==0", bry == 0), ("edge:ulx==W-1", ulx == Wh - 1),
                                     ("edge:uly==H-1", uly == Hh - 1), ("clip:left", ulx < 0 < brx), ("clip:top", uly < 0 < bry),
                                     ("clip:right", ulx < Wh - 1 and brx > Wh), ("clip:bottom", uly < Hh - 1 and bry > Hh),
                                     ("inside:whole", ulx >= 0 and uly >= 0 and brx <= Wh and bry <= Hh)) if c}      # :432
        return names
    if kernel == "cond_render":
        H, W, Cc, K, js, trunc, into = case
        names = {"Cc:%d" % Cc, "K:%d" % K, "js:%d" % js, "truncate:%d" % trunc, "entry:into-gap-37" if into else "entry:plain",
                 "colors:null" if Cc == 1 else "colors:given",
                 "reflect:repeats" if min(H, W) < 8 else "reflect:once",            # loss_decode.hip:461: 7 > n - 1
                 "pixels:below-256" if H * W < BLOCK else "pixels:%d-blocks-of-4-trips" % ceil_div(H * W, 4 * BLOCK)}      # :506, :579
        if min(H, W) >= 15:
            names.add("reject:far-from-border")                          # :512-513 can skip a point
        j = cond_operand(case)
        for b in range(COND_B):
            acc = cond_accept(j[b].numpy(), H, W)
            names.add("member:every-point-rejected" if not acc else "member:points")      # :538 am == 0
            if len({(py, px) for _, py, px in acc}) < len(acc):
                names.add("points:duplicate-pixel")                      # :493-494
            if len(acc) < K:
                names.add("points:some-rejected")                        # :490
            for _, py, px in acc:
                if (px in (0, W - 2)) and (py in (0, H - 2)):
                    names.add("points:corner")
                elif px in (0, W - 2) or py in (0, H - 2):
                    names.add("points:border")
        return names
    if kernel == "flipback_avg":
        N, K, H, W, kind, shift = case
        return {"W:%s" % (W if W <= 2 else "n"), "K:%s" % (1 if K == 1 else "n"), "perm:" + kind, "shift:%d" % shift,
                _grid(N * K * H * W, FLIP_GRID_CAP)}                      # loss_decode.hip:595, :603, :613
    if kernel == "adam_step":
        n, step, gscale, mode = case
        n4 = n >> 2
        names = {"body:none" if n4 == 0 else "body", "tail:%d" % (n % 4), "step:%d" % step, "gscale:%g" % gscale, "mode:" + mode}
        if n4 and grid_trips(n4, ADAM_GRID_CAP) > 1:                      # loss_decode.hip:630, :646, :661
            names.add("body:second-trip")
        return names
    if kernel == "sgd_step":
        n, mu, nesterov, wd, first, gscale, off = case
        return {_grid(n, SGD_GRID_CAP), "mu:0-null-buffer" if mu == 0.0 else "mu:>0", "nesterov:%d" % nesterov,     # :675, :678-681
                "wd:0" if wd == 0.0 else "wd:>0", "first:%d" % first, "gscale:%g" % gscale,
                "slice:aligned" if off % 4 == 0 else "slice:odd-offset"}
    if kernel == "nms":
        n, dim, kind, thresh = case
        cb = ceil_div(n, NMS_COLS)
        names = {"dim:%d" % dim, "kind:" + kind, "blocks:%d%s" % (cb, "" if n % NMS_COLS == 0 else "-ragged")}    # nms.hip:34, :88
        if n == 1:
            names.add("n:1")
        if kind == "chain":
            for A, B, C in nms_chains(n):
                names.add("chain:in-block" if A // 64 == C // 64 else "chain:crosses-block" if C // 64 - B // 64 == 1 else "chain:far-block")
        if kind == "threshold" and n > 64:
            names.add("threshold:pair-straddles-block")
        return names
    raise KeyError(kernel)


TABLES = {"joints_mse": MSE, "argmax": ARGMAX, "gaussian_target": GAUSS, "cond_render": COND, "flipback_avg": FLIP,
          "adam_step": ADAM, "sgd_step": SGD, "nms": NMS}

# every path a kernel has; each must be taken by at least one case of its table
PATHS = {
    "joints_mse": ["partial:idle-threads", "partial:one-trip", "partial:tail-trip", "final:idle-threads", "final:one-trip",
                   "final:second-trip", "w:w", "w:null", "w:zero-rows", "grad:0", "grad:1", "gscale:1", "gscale:0.125"],
    "argmax": ["kind:random", "kind:ties", "kind:special", "kind:quarter", "hw:1", "hw:part-wave", "hw:idle-waves", "hw:one-trip",
               "hw:tail-trip", "shape:W=1", "shape:H=1", "shape:square", "shape:non-square", "tie:same-thread", "tie:same-wave",
               "tie:across-waves", "tie:across-trips", "tie:first-and-last", "later-higher", "row:constant", "row:max-zero",
               "row:max-negative", "row:all-neg-inf", "row:pos-inf", "quarter:masked", "quarter:map-below-4", "quarter:eligible",
               "quarter:x-equal", "quarter:x-left", "quarter:x-right", "quarter:y-equal", "quarter:y-up", "quarter:y-down",
               "quarter:px=2", "quarter:px=W-2", "quarter:py=2", "quarter:py=H-2", "quarter:px<=1", "quarter:px=W-1",
               "quarter:py<=1", "quarter:py=H-1"],
    "gaussian_target": ["sigma:1", "sigma:2", "sigma:3", "sigma:1.5", "stride:square", "stride:non-square", "pixels:idle-threads",
                        "pixels:tail-trip", "mu:truncates-toward-zero", "outside:ulx>=W", "outside:uly>=H", "outside:brx<0",
                        "outside:bry<0", "edge:brx==0", "edge:bry==0", "edge:ulx==W-1", "edge:uly==H-1", "clip:left", "clip:top",
                        "clip:right", "clip:bottom", "inside:whole", "vis:0", "vis:0.3", "vis:0.5", "vis:0.51", "vis:1",
                        "vis:any-outside"],
    "cond_render": ["Cc:1", "Cc:3", "Cc:4", "K:1", "K:17", "K:64", "js:2", "js:3", "truncate:0", "truncate:1", "entry:plain",
                    "entry:into-gap-37", "colors:null", "colors:given", "reflect:repeats", "reflect:once", "pixels:below-256",
                    "pixels:1-blocks-of-4-trips", "pixels:3-blocks-of-4-trips", "reject:far-from-border", "member:every-point-rejected", "member:points",
                    "points:duplicate-pixel", "points:some-rejected", "points:corner", "points:border"],
    "flipback_avg": ["W:1", "W:2", "W:n", "K:1", "K:n", "perm:identity", "perm:swapped", "shift:0", "shift:1",
                     "grid:partial-block", "grid:one-trip", "grid:second-trip"],
    "adam_step": ["body:none", "body", "body:second-trip", "tail:0", "tail:1", "tail:3", "step:1", "step:2", "step:1000",
                  "gscale:1", "gscale:0.25", "mode:one", "mode:three", "mode:zero"],
    "sgd_step": ["grid:partial-block", "grid:one-trip", "grid:second-trip", "mu:0-null-buffer", "mu:>0", "nesterov:0",
                 "nesterov:1", "wd:0", "wd:>0", "first:0", "first:1", "gscale:1", "gscale:0.5", "slice:aligned",
                 "slice:odd-offset"],
    "nms": ["n:1", "dim:4", "dim:5", "kind:disjoint", "kind:identical", "kind:chain", "kind:threshold", "kind:random",
            "blocks:1-ragged", "blocks:1", "blocks:2-ragged", "blocks:3-ragged", "blocks:4-ragged", "chain:in-block",
            "chain:crosses-block", "chain:far-block", "threshold:pair-straddles-block"],
}

# the cases that exist to reach a later loop trip, and the trip they must reach: (kernel, case filter, path name)
SECOND_TRIPS = [
    ("joints_mse", lambda c: c[0] * c[1] > 256, "final:second-trip"),
    ("joints_mse", lambda c: c[2] in (257, 432), "partial:tail-trip"),
    ("argmax", lambda c: c[0] * c[1] in (257, 432), "hw:tail-trip"),
    ("flipback_avg", lambda c: c[0] == FLIP_LONG_N, "grid:second-trip"),
    ("adam_step", lambda c: c[0] == ADAM_LONG, "body:second-trip"),
    ("sgd_step", lambda c: c[0] == SGD_LONG, "grid:second-trip"),
    ("nms", lambda c: c[0] == 200, "blocks:4-ragged"),
]


def case_bytes(kernel, case):
    """bytes of all operands and outputs (fp32 / int32) and of the references kept for the comparison (fp64, or fp32 where the
    bar is bit-exact) of one case; the long Adam and SGD vectors are compared a million elements at a time"""
    f, d = 4, 8
    if kernel == "joints_mse":
        return case[0] * case[1] * case[2] * (3 * f + 2 * d + f)
    if kernel == "argmax":
        rows = argmax_operand(case)[0].shape[0]
        return rows * case[0] * case[1] * (f + d) + rows * 12 * f
    if kernel == "gaussian_target":
        return len(gauss_joints(case)) * (case[0] * case[1] * (f + d) + 5 * f)
    if kernel == "cond_render":
        H, W, Cc, K = case[:4]
        return COND_B * (Cc * H * W * (2 * f + 2 * d) + COND_GAP * f + K * case[4] * f)
    if kernel == "flipback_avg":
        return math.prod(case[:4]) * 4 * f
    if kernel == "adam_step":
        return case[0] * (4 * f + 3 * f) + (1 << 20) * 3 * (d + f)
    if kernel == "sgd_step":
        return (case[0] + case[6]) * (3 * f + 2 * f) + (1 << 20) * 2 * (d + f)
    if kernel == "nms":
        n = case[0]
        return n * case[1] * f + n * ceil_div(n, 64) * 8 + 2 * n * n * 8
    raise KeyError(kernel)
