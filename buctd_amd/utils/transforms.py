"""Flip-test helpers and the crop <-> image affine - drop-in for reference lib/utils/transforms.py:16-118.
numpy entry points keep the reference names and signatures; *_device variants run on the GPU."""
import numpy as np
import torch

from .. import ops


def _swap_table(count, matched_parts):
    """Channel permutation that exchanges every left/right pair."""
    table = np.arange(count)
    for left, right in matched_parts:
        table[left], table[right] = right, left
    return table


def flip_back(output_flipped, matched_parts):
    """Undo a horizontal flip on heat-maps [N, K, H, W]: mirror the width axis, exchange left/right joints."""
    if output_flipped.ndim != 4:
        raise AssertionError('output_flipped should be [batch_size, num_joints, height, width]')
    table = _swap_table(output_flipped.shape[1], matched_parts)
    return np.ascontiguousarray(output_flipped[:, table, :, ::-1])


def flip_perm(num_joints, matched_parts, device):
    return torch.as_tensor(_swap_table(num_joints, matched_parts), dtype=torch.int32, device=device)


def flip_merge_device(output, output_flipped, matched_parts, shift):
    """(output + shift(flip_back(output_flipped))) * 0.5 in one kernel (reference core/function.py:226-236)."""
    perm = flip_perm(output.shape[1], matched_parts, output.device)
    return ops.flipback_avg(output.contiguous(), output_flipped.contiguous(), perm, shift)


def fliplr_joints(joints, joints_vis, width, matched_parts):
    """Mirror key points [K, 3] about the vertical axis of a `width`-pixel image (in place, like the reference)
    and exchange left/right rows; invisible joints come back zeroed."""
    joints[:, 0] = width - joints[:, 0] - 1
    table = _swap_table(joints.shape[0], matched_parts)
    joints[:] = joints[table]
    joints_vis[:] = joints_vis[table]
    return joints * joints_vis, joints_vis


def mirror_condition(cond_joints, cond_joints_vis, width, matched_parts):
    """The condition coordinates of the mirrored half of a flip-test input, as the renderer takes them: fliplr_joints per
    sample on copies (x' = (width - x) - 1 in float64, partners exchanged, joints times their visibility), then
    np.array(kpts).astype(int) as floats (dataset.pipeline.trunc_condition).  cond_joints [B, K, >=2], cond_joints_vis
    [B, K, 3] or None for all ones -> float32 [B, K, 2].  trunc(width - 1 - x) is not width - 1 - trunc(x) for a
    non-integer x: this takes the untruncated crop coordinates.  The CPU statement of buctd_cond_mirror."""
    kp = np.array(cond_joints, dtype=np.float64)
    vis = np.ones(kp.shape[:2] + (3,)) if cond_joints_vis is None else np.array(cond_joints_vis, dtype=np.float64)
    if kp.shape[2] == 2:
        vis = vis[:, :, :2].copy()
    mirrored = np.stack([fliplr_joints(kp[b], vis[b], width, matched_parts)[0] for b in range(kp.shape[0])])
    return np.ascontiguousarray(np.trunc(mirrored[:, :, :2]).astype(np.float32))


def flip_hm(heatmap, dataset, cond_joints, cond_joints_vis):
    """Condition flip for the flip test (reference 33-58): a 3-channel condition is re-rendered (colored) from the
    mirrored key points - on the GPU here; a stacked one is mirrored with left/right channels exchanged."""
    channels = heatmap.shape[1]
    if channels == 3:
        width, height = int(dataset.image_size[0]), int(dataset.image_size[1])
        kp = cond_joints.detach().cpu().numpy().copy()
        vis = cond_joints_vis.detach().cpu().numpy().copy()
        mirrored = [fliplr_joints(kp[b], vis[b], width, dataset.flip_pairs)[0] for b in range(kp.shape[0])]
        pts = torch.from_numpy(np.ascontiguousarray(np.stack(mirrored))).float().to(heatmap.device)
        colors = torch.tensor(dataset.kpt_colors, dtype=torch.float32, device=heatmap.device)
        return ops.cond_render(pts, colors, height, width)
    mirrored = heatmap.flip(3)
    if channels > 3:
        table = torch.as_tensor(_swap_table(channels, dataset.flip_pairs), device=heatmap.device)
        mirrored = mirrored.index_select(1, table)
    return mirrored.contiguous()


# ---------------------------------------------------------------------------------------------- affine ----
def get_dir(src_point, rot_rad):
    """src_point rotated by rot_rad (counter-clockwise in image coordinates with y down)."""
    s, c = np.sin(rot_rad), np.cos(rot_rad)
    x, y = src_point[0], src_point[1]
    return [x * c - y * s, x * s + y * c]


def get_3rd_point(a, b):
    """Third corner of the right-angled isosceles triangle on the segment a-b (float32 like the reference)."""
    dx, dy = a[0] - b[0], a[1] - b[1]
    return b + np.array([-dy, dx], dtype=np.float32)


def _triangle(origin, arm):
    """The three float32 control points the reference feeds to cv2.getAffineTransform."""
    pts = np.zeros((3, 2), dtype=np.float32)
    pts[0] = origin
    pts[1] = origin + arm
    pts[2] = get_3rd_point(pts[0], pts[1])
    return pts


def get_affine_transform(center, scale, rot, output_size, shift=np.array([0, 0], dtype=np.float32), inv=0):
    """2x3 matrix mapping the person box (center, scale*200 px, rotated by rot degrees) onto an output_size crop
    (inv=1: the reverse).  cv2.getAffineTransform solves the 3-point system in float64; so does this."""
    if not isinstance(scale, (np.ndarray, list)):
        scale = np.array([scale, scale])
    box = np.asarray(scale) * 200.0
    out_w, out_h = output_size[0], output_size[1]
    offset = box * shift
    box_pts = _triangle(center + offset, np.asarray(get_dir([0, box[0] * -0.5], np.pi * rot / 180)))
    crop_pts = _triangle(np.array([out_w * 0.5, out_h * 0.5]), np.array([0, out_w * -0.5], np.float32))
    frm, to = (crop_pts, box_pts) if inv else (box_pts, crop_pts)
    system = np.hstack([frm.astype(np.float64), np.ones((3, 1))])
    return np.linalg.solve(system, to.astype(np.float64)).T


def crop_affine_closed_form(center, scale, output_size, inv=0):
    """get_affine_transform(center, scale, 0, output_size, inv=inv) for float32 center / scale and an integer output_size,
    without the solve: with rot = 0 the three control points are the corners of an axis-parallel right-angled triangle, so
    the matrix is diagonal.  The float32 roundings of the box triangle are those of _triangle / get_3rd_point; everything
    after them is float64, one rounding per operation.  buctd_refine_step (csrc/sample.hip, crop_affine) restates these
    lines; the solve differs from them by its own rounding only (tests/test_refine_closed_form.py: <= 1e-9)."""
    cx, cy = np.float32(center[0]), np.float32(center[1])
    box = np.float32(scale[0]) * np.float32(200.0)                       # scale * 200.0 in float32; only box[0] is used
    p1y = np.float32(np.float64(cy) + np.float64(box * np.float32(-0.5)))  # pts[1] = origin + arm, stored as float32
    dy = cy - p1y                                                        # get_3rd_point: float32 differences
    p2x = cx - dy
    # box triangle (cx, cy), (cx, p1y), (p2x, p1y) <-> crop triangle (a, b), (a, b - a), (0, b - a)
    ex, ey = np.float64(cx) - np.float64(p2x), np.float64(cy) - np.float64(p1y)
    a, b = np.float64(output_size[0]) * 0.5, np.float64(output_size[1]) * 0.5
    t = np.zeros((2, 3), dtype=np.float64)
    if inv:
        t[0, 0], t[1, 1] = ex / a, ey / a
        t[0, 2], t[1, 2] = np.float64(cx) - t[0, 0] * a, np.float64(cy) - t[1, 1] * b
    else:
        t[0, 0], t[1, 1] = a / ex, a / ey
        t[0, 2], t[1, 2] = a - t[0, 0] * np.float64(cx), b - t[1, 1] * np.float64(cy)
    return t


def _two_sum(a, b):
    """a + b = s + e exactly (Knuth), float64."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    """a = h + l with 26-bit halves (Veltkamp)."""
    c = 134217729.0 * a
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker: no fused multiply-add), float64."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _cross(a, u, b, v):
    """a * (u[0] + u[1]) - b * (v[0] + v[1]) with the cancellation of the two leading products done exactly."""
    p1, e1 = _two_prod(a, u[0])
    p2, e2 = _two_prod(b, v[0])
    s, es = _two_sum(p1, -p2)
    return s + ((es + (e1 - e2)) + (a * u[1] - b * v[1]))


def crop_affine_rot_closed_form(center, scale, sn, cs, output_size):
    """get_affine_transform(center, scale, rot, output_size) for any rotation, without the solve; sn, cs = sin and cos of
    pi * rot / 180 in float64.  center is float32; scale keeps its dtype (float32 records, float64 after the train path's
    scale draw: numpy multiplies a float32 array by a float64 scalar in float64), as `scale * 200.0` does there.

    The box triangle P0, P1, P2 is the one _triangle / get_3rd_point build, with their float32 roundings; the crop
    triangle is (a, b), (a, b - a), (0, b - a) with a, b = half the crop size, exact in float32.  The 2x2 part A solves
    A (P1 - P0) = (0, -a) and A (P2 - P1) = (-a, 0):

        A = [[a * d1y, -a * d1x], [-a * d2y, a * d2x]] / det,   d1 = P1 - P0, d2 = P2 - P1, det = d1x * d2y - d2x * d1y

    (d2 is d1 turned by a right angle up to the float32 roundings, so the two products of det have the same sign and
    nothing cancels).  The translation (a, b) - A P0 cancels: evaluated from the rounded A its error is |dA| |P0|, thousands
    of ulp of a small translation.  It is therefore written over the same denominator,

        tx = a * (d1x * (d2y + cy) - d1y * (d2x + cx)) / det
        ty = (d2y * (b * d1x + a * cx) - d2x * (b * d1y + a * cy)) / det

    with the two differences of products taken exactly (_two_sum / _two_prod, which need no fused multiply-add).
    Everything after the float32 triangle is float64, one rounding per operation.  buctd_sample_geometry
    (csrc/sample.hip, crop_affine_rot) restates these lines.  tests/test_sample_geometry.py measures this form and the
    solve against the exact rational solution."""
    cx, cy = np.float32(center[0]), np.float32(center[1])
    box = np.asarray(scale).reshape(-1)[0] * 200.0                       # only box[0] is used
    y = box * -0.5
    ax, ay = -(y * np.float64(sn)), y * np.float64(cs)                   # get_dir([0, y], rot): 0 * c - y * s, 0 * s + y * c
    p1x, p1y = np.float32(np.float64(cx) + ax), np.float32(np.float64(cy) + ay)   # pts[1] = origin + arm, stored as float32
    dx, dy = cx - p1x, cy - p1y                                          # get_3rd_point: float32 differences
    p2x, p2y = p1x - dy, p1y + dx
    cx, cy = np.float64(cx), np.float64(cy)
    d1x, d1y = np.float64(p1x) - cx, np.float64(p1y) - cy
    d2x, d2y = np.float64(p2x) - np.float64(p1x), np.float64(p2y) - np.float64(p1y)
    det = d1x * d2y - d2x * d1y
    if det == 0.0:
        raise np.linalg.LinAlgError("crop_affine_rot_closed_form: the box has no extent")
    a, b = np.float64(output_size[0]) * 0.5, np.float64(output_size[1]) * 0.5
    t = np.zeros((2, 3), dtype=np.float64)
    t[0, 0], t[0, 1] = (a * d1y) / det, -(a * d1x) / det
    t[1, 0], t[1, 1] = -(a * d2y) / det, (a * d2x) / det
    t[0, 2] = (a * _cross(d1x, _two_sum(d2y, cy), d1y, _two_sum(d2x, cx))) / det
    qx, fx = _two_prod(b, d1x)
    qy, fy = _two_prod(b, d1y)
    wx, gx = _two_sum(qx, a * cx)                                        # a * cx, a * cy: exact (a float32 times a half-integer)
    wy, gy = _two_sum(qy, a * cy)
    t[1, 2] = _cross(d2y, (wx, gx + fx), d2x, (wy, gy + fy)) / det
    return t


def affine_transform(pt, t):
    return t[:, :2] @ np.array([pt[0], pt[1]], dtype=np.float64) + t[:, 2]


def transform_preds(coords, center, scale, output_size):
    """Heat-map coordinates [K, >=2] -> image coordinates through the inverse crop affine (rot = 0)."""
    t = get_affine_transform(center, scale, 0, output_size, inv=1)
    mapped = np.zeros(coords.shape)
    mapped[:, 0:2] = coords[:, 0:2].astype(np.float64) @ t[:, :2].T + t[:, 2]
    return mapped
