"""Restatement of the two debug pictures of buctd_amd/utils/vis.py (csrc/vis.hip) from their definitions in
include/buctd_hip.h, in numpy: float32 operation by operation where the definition names fp32, Python integers
elsewhere.  It draws the way the reference's save_batch_heatmaps / save_batch_image_with_joints do - shrink the image,
paint marker after marker onto it, blend, paint again - and shares no code with the package.

Images are float32 [B, 3, H, W] arrays in logical NCHW order, whatever the memory layout of the tensor under test."""
import numpy as np

F = np.float32
RED, GREEN, BLUE = (255, 0, 0), (0, 255, 0), (0, 0, 255)


def min_max(image):
    return F(image.min()), F(image.max())


def max_preds(heatmaps):
    """get_max_preds: (x, y) of the first largest value per map, (0, 0) where that value is <= 0.  float32 [B, K, 2]."""
    B, K, Hh, Wh = heatmaps.shape
    preds = np.zeros((B, K, 2), dtype=F)
    for b in range(B):
        for j in range(K):
            flat = heatmaps[b, j].reshape(-1)
            at = int(np.argmax(flat))
            if flat[at] > 0:
                preds[b, j] = (at % Wh, at // Wh)
    return preds


def image_bytes(image, lohi):
    """[B, 3, H, W] float32 -> int [B, 3, H, W]: u = (v - lo) / ((hi - lo) + 1e-5f) (u = v without lohi), u * 255 clamped
    to [0, 255] and truncated."""
    u = image.astype(F)
    if lohi is not None:
        lo, hi = F(lohi[0]), F(lohi[1])
        u = (u - lo) / ((hi - lo) + F(1e-5))
    assert u.dtype == F
    return np.clip(u * F(255.0), F(0.0), F(255.0)).astype(np.int64)


def tap(x, n, m):
    fx = (F(x) + F(0.5)) * (F(n) / F(m)) - F(0.5)
    fl = np.floor(fx)
    a = fx - fl
    x0 = int(fl)
    x1 = x0 + 1
    if x0 < 0:
        x0, x1, a = 0, min(1, n - 1), F(0.0)
    if x0 >= n - 1:
        x0, x1, a = n - 1, n - 1, F(0.0)
    assert type(a) is F
    return x0, x1, int(np.rint(a * F(2048.0)))


def shrink(plane, Hh, Wh):
    """int [H, W] bytes -> int [Hh, Wh]: bilinear, half-pixel centres, 11-bit weights."""
    H, W = plane.shape
    out = np.zeros((Hh, Wh), dtype=np.int64)
    for y in range(Hh):
        y0, y1, wb = tap(y, H, Hh)
        for x in range(Wh):
            x0, x1, wa = tap(x, W, Wh)
            p00, p01, p10, p11 = int(plane[y0, x0]), int(plane[y0, x1]), int(plane[y1, x0]), int(plane[y1, x1])
            out[y, x] = ((p00 * (2048 - wa) + p01 * wa) * (2048 - wb) + (p10 * (2048 - wa) + p11 * wa) * wb + (1 << 21)) >> 22
    return out


def heat_byte(h):
    return int(min(max(F(h) * F(255.0), F(0.0)), F(255.0)))


def jet(byte):
    t = F(byte) / F(255.0)
    rgb = []
    for centre in (F(3.0), F(2.0), F(1.0)):
        c = min(max(F(1.5) - abs(F(4.0) * t - centre), F(0.0)), F(1.0))
        assert type(c) is F
        rgb.append(int(np.floor(c * F(255.0) + F(0.5))))
    return tuple(rgb)


def draw_marker(tile, px, py):
    """the four pixels at Manhattan distance 1 from (int(px), int(py)), clipped to the tile, pure red"""
    cx, cy = int(float(px)), int(float(py))
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        x, y = cx + dx, cy + dy
        if 0 <= x < tile.shape[1] and 0 <= y < tile.shape[0]:
            tile[y, x] = RED


def heatmap_grid(image, heatmaps, peaks, normalize=True, bgr=True):
    """uint8 [B*Hh, (K+1)*Wh, 3] RGB"""
    B, K, Hh, Wh = heatmaps.shape
    by = image_bytes(image[:, :3], min_max(image[:, :3]) if normalize else None)
    grid = np.zeros((B * Hh, (K + 1) * Wh, 3), dtype=np.uint8)
    for i in range(B):
        order = (2, 1, 0) if bgr else (0, 1, 2)
        resized = np.stack([shrink(by[i, c], Hh, Wh) for c in order], axis=-1)     # [Hh, Wh, 3] RGB
        for j in range(K):
            draw_marker(resized, peaks[i, j, 0], peaks[i, j, 1])
            masked = np.zeros((Hh, Wh, 3), dtype=np.int64)
            for y in range(Hh):
                for x in range(Wh):
                    colour = jet(heat_byte(heatmaps[i, j, y, x]))
                    for c in range(3):
                        masked[y, x, c] = (7 * colour[c] + 3 * int(resized[y, x, c])) // 10
            draw_marker(masked, peaks[i, j, 0], peaks[i, j, 1])
            grid[i * Hh:(i + 1) * Hh, (j + 1) * Wh:(j + 2) * Wh] = masked
        grid[i * Hh:(i + 1) * Hh, 0:Wh] = resized
    return grid


def _paint(cell, x, y, colour):
    if 0 <= x < cell.shape[1] and 0 <= y < cell.shape[0]:
        cell[y, x] = colour


def joint_grid(image, pred, pred_vis, gt, gt_vis, cond=None, cond_vis=None, nrow=8, padding=2, bgr=True):
    """uint8 [Hg, Wg, 3] RGB.  pred / gt / cond [B, K, 2]; the visibilities [B, K] (cond_vis: the sum)."""
    B, _, H, W = image.shape
    K = pred.shape[1]
    by = image_bytes(image[:, :3], min_max(image[:, :3]))
    xmaps = min(nrow, B)
    ymaps = (B + xmaps - 1) // xmaps
    grid = np.zeros((ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3), dtype=np.uint8)
    k = 0
    for yc in range(ymaps):
        for xc in range(xmaps):
            if k >= B:
                break
            top, left = yc * (H + padding) + padding, xc * (W + padding) + padding
            cell = grid[top:top + H, left:left + W]                               # a view: marks clip to it
            for c, src in enumerate((2, 1, 0) if bgr else (0, 1, 2)):
                cell[:, :, c] = by[k, src]
            for j in range(K):
                if pred_vis[k, j] != 0:
                    cx, cy = int(float(pred[k, j, 0])), int(float(pred[k, j, 1]))
                    for dy in range(-3, 4):
                        for dx in range(-3, 4):
                            if dx * dx + dy * dy <= 8:
                                _paint(cell, cx + dx, cy + dy, RED)
                if gt_vis[k, j] != 0:
                    cx, cy = int(float(gt[k, j, 0])), int(float(gt[k, j, 1]))
                    for d in range(-2, 3):
                        _paint(cell, cx + d, cy, BLUE)
                        _paint(cell, cx, cy + d, BLUE)
                if cond is not None and cond_vis[k, j] > 0 and cond[k, j, 0] > 0 and cond[k, j, 1] > 0:
                    cx, cy = int(float(cond[k, j, 0])), int(float(cond[k, j, 1]))
                    for d in range(-2, 3):
                        _paint(cell, cx + d, cy + d, GREEN)
                        _paint(cell, cx + d, cy - d, GREEN)
            k += 1
    return grid
