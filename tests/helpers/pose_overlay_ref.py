"""Restatement of the pose overlay (buctd_vis_pose_overlay, csrc/vis_pose.hip) from the rules in include/buctd_hip.h, in
numpy: int64 throughout, one vectorised mask per primitive, painted one after the other in the stated order, then the
integer blend.  It shares no code with the package and none with the reference.

A canvas is a uint8 [H, W, 3] array; poses are [P, K, 2 or 3] (x, y, score; a missing score counts as 1) and are read as
float32; a limb is (a0, a1, b0, b1, colour index or -1)."""
import numpy as np

LO, HI = -8192, 8191


def floor_mid(a, b):
    """floor midpoint of two integers (Python's >> is arithmetic, = numpy's // 2)"""
    return (int(a) + int(b)) >> 1


def _pixels(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return xs.astype(np.int64), ys.astype(np.int64)


def segment_mask(H, W, p, q, t):
    """pixels X with 4 d(X, segment p-q)^2 <= t^2"""
    xs, ys = _pixels(H, W)
    px, py, qx, qy, t = int(p[0]), int(p[1]), int(q[0]), int(q[1]), int(t)
    vx, vy = qx - px, qy - py
    wx, wy = xs - px, ys - py
    c1 = wx * vx + wy * vy
    c2 = vx * vx + vy * vy
    ww = wx * wx + wy * wy
    uu = (xs - qx) ** 2 + (ys - qy) ** 2
    before = c1 <= 0
    after = ~before & (c1 >= c2)
    between = ~before & ~after
    return (before & (4 * ww <= t * t)) | (after & (4 * uu <= t * t)) | (between & (4 * (ww * c2 - c1 * c1) <= t * t * c2))


def disc_mask(H, W, z, r):
    xs, ys = _pixels(H, W)
    return (xs - int(z[0])) ** 2 + (ys - int(z[1])) ** 2 <= int(r) * int(r)


def ring_mask(H, W, z, r, t):
    xs, ys = _pixels(H, W)
    d4 = 4 * ((xs - int(z[0])) ** 2 + (ys - int(z[1])) ** 2)
    r, t = int(r), int(t)
    mask = d4 <= (2 * r + t) ** 2
    if 2 * r > t:
        mask &= d4 >= (2 * r - t) ** 2
    return mask


def joint_pixel(joint, offset, score_thresh):
    """(x, y) integers or None: finite x, y, score, score > thresh, truncation toward zero, offset, range"""
    x, y = np.float32(joint[0]), np.float32(joint[1])
    s = np.float32(joint[2]) if len(joint) > 2 else np.float32(1.0)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(s)) or not (s > np.float32(score_thresh)):
        return None
    ix, iy = int(np.trunc(x)) + int(offset[0]), int(np.trunc(y)) + int(offset[1])
    if not (LO <= ix <= HI and LO <= iy <= HI):
        return None
    return ix, iy


def end_point(pose, j0, j1, offset, score_thresh):
    a, b = joint_pixel(pose[j0], offset, score_thresh), joint_pixel(pose[j1], offset, score_thresh)
    if a is None or b is None:
        return None
    return floor_mid(a[0], b[0]), floor_mid(a[1], b[1])


def primitives(pose, limbs, palette, colour, style, thickness, radius, offset, score_thresh):
    """the (mask function, colour) list of one person, in paint order"""
    out = []
    if style == 'plain':
        for j in range(len(pose)):
            z = joint_pixel(pose[j], offset, score_thresh)
            if z is not None:
                out.append((lambda H, W, z=z: ring_mask(H, W, z, radius, thickness), colour))
        for a0, a1, b0, b1, _ in limbs:
            A, B = end_point(pose, a0, a1, offset, score_thresh), end_point(pose, b0, b1, offset, score_thresh)
            if A is not None and B is not None:
                out.append((lambda H, W, A=A, B=B: segment_mask(H, W, A, B, thickness), colour))
    elif style == 'pretty':
        for a0, a1, b0, b1, ci in limbs:
            col = colour if ci < 0 else tuple(int(v) for v in palette[ci])
            A, B = end_point(pose, a0, a1, offset, score_thresh), end_point(pose, b0, b1, offset, score_thresh)
            if A is not None and B is not None:
                out.append((lambda H, W, A=A, B=B: segment_mask(H, W, A, B, thickness), col))
            if A is not None:
                out.append((lambda H, W, A=A: disc_mask(H, W, A, radius), col))
            if B is not None:
                out.append((lambda H, W, B=B: disc_mask(H, W, B, radius), col))
    else:
        raise ValueError(style)
    return out


def draw_poses(canvas, poses, limbs, colours, palette=None, style='plain', thickness=2, radius=3, score_thresh=-1.0,
               alpha256=256, offsets=None, clips=None):
    """-> a new uint8 [H, W, 3]: the persons of `poses` painted in order onto a copy of `canvas`.  colours [P, 3];
    offsets [P, 2] or None; clips [P, 4] = x0, y0, x1, y1 or None (the whole canvas)."""
    H, W = canvas.shape[:2]
    poses = np.asarray(poses, dtype=np.float32)
    xs, ys = _pixels(H, W)
    covered = np.zeros((H, W), dtype=bool)
    paint = np.zeros((H, W, 3), dtype=np.int64)
    for p, pose in enumerate(poses):
        offset = (0, 0) if offsets is None else offsets[p]
        x0, y0, x1, y1 = (0, 0, W, H) if clips is None else (int(v) for v in clips[p])
        inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        colour = tuple(int(v) for v in colours[p])
        for mask_of, col in primitives(pose, limbs, palette, colour, style, thickness, radius, offset, score_thresh):
            mask = mask_of(H, W) & inside
            paint[mask] = col
            covered |= mask
    out = canvas.astype(np.int64)
    blended = (out * (256 - int(alpha256)) + paint * int(alpha256) + 128) >> 8
    out[covered] = blended[covered]
    return out.astype(np.uint8)
