"""Host side of DeviceSamplePipeline(geometry_on_device=True): the rotated closed form of the crop affine against the exact
rational solution, the draw table against draw_augmentation, the keep-rectangle of DATASET.NEW_AUGMENTATION on the host
path against oracle.sample.warp_affine_u8, the scale dtype of the train path, and the crop of the closed-form matrix
against the crop of the solve's."""
import itertools
from fractions import Fraction as F

import numpy as np
import pytest

import geometry_cases as G


# ---- 1. the closed form -----------------------------------------------------------------------------------------------
def _control_points(center, scale, rot, size):
    """The float32 control points get_affine_transform hands to its solve (its lines before the solve)."""
    from buctd_amd.utils import transforms as T
    box = np.asarray(scale) * 200.0
    box_pts = T._triangle(center + box * np.array([0, 0], np.float32), np.asarray(T.get_dir([0, box[0] * -0.5], np.pi * rot / 180)))
    crop_pts = T._triangle(np.array([size[0] * 0.5, size[1] * 0.5]), np.array([0, size[0] * -0.5], np.float32))
    return box_pts, crop_pts


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _exact(box_pts, crop_pts):
    """The 2 x 3 matrix that maps the float32 box points onto the crop points, as Fractions (Cramer's rule)."""
    S = [[F(float(p[0])), F(float(p[1])), F(1)] for p in box_pts]
    d = _det3(S)
    out = [[None] * 3 for _ in range(2)]
    for r in range(2):
        q = [F(float(p[r])) for p in crop_pts]
        for c in range(3):
            M = [row[:] for row in S]
            for i in range(3):
                M[i][c] = q[i]
            out[r][c] = _det3(M) / d
    return out


ROTATIONS = [0, 0.01, -0.01, 30, -30, 59.9, -59.9, 60, -60]
WIDTHS = [10, 11, 37.3, 150, 640, 2000]
CENTRES = [(320, 240), (0, 0), (639, 479), (0.5, 479), (123.456, 77.7)]
SIZES = [(288, 384), (192, 256)]


def test_rotated_closed_form_against_the_exact_solution():
    """Measured over this grid (1080 cases, float32 and float64 scale): get_affine_transform is off by up to 2.64e-10, the
    closed form by up to 1.80e-12 and never by more than 2 ulp of the element.  (A closed form that ignores the float32
    roundings of the control points differs from both by ~1e-4 on 10-px boxes: a rounding of 3e-5 px at x = 640 against
    an arm of 5 px, times the magnification.  That is the naive form's error, not the solve's.)"""
    from buctd_amd.utils import transforms as T
    worst_a = worst_b = worst_b_ulp = 0.0
    for rot, w, c, size, wide in itertools.product(ROTATIONS, WIDTHS, CENTRES, SIZES, (False, True)):
        center = np.array(c, np.float32)
        scale = np.array([w / 200.0, w / 200.0 * size[1] / size[0]], np.float32)
        if wide:
            scale = scale * np.float64(1.0873)              # the train path: float32 scale * a float64 draw
        ex = _exact(*_control_points(center, scale, rot, size))
        a = T.get_affine_transform(center, scale, rot, np.array(size))
        b = T.crop_affine_rot_closed_form(center, scale, np.sin(np.pi * rot / 180), np.cos(np.pi * rot / 180), size)
        for r, k in itertools.product(range(2), range(3)):
            ea, eb = abs(float(F(float(a[r, k])) - ex[r][k])), abs(float(F(float(b[r, k])) - ex[r][k]))
            ulp = float(np.spacing(abs(float(ex[r][k])))) if ex[r][k] != 0 else 0.0
            worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
            if ulp:
                worst_b_ulp = max(worst_b_ulp, eb / ulp)
            assert eb <= ea or (ea < 4 * ulp and eb < 4 * ulp), (rot, w, c, size, wide, r, k, ea, eb, ulp)
    print(f"largest element error: solve {worst_a:.3e}, closed form {worst_b:.3e} ({worst_b_ulp:.2f} ulp)")
    assert worst_a <= G.SOLVE_ERR and worst_b <= G.CLOSED_ERR, (worst_a, worst_b)


def test_closed_form_with_rotation_zero_equals_the_diagonal_form():
    from buctd_amd.utils import transforms as T
    for c, w in itertools.product(CENTRES, WIDTHS):
        center, scale = np.array(c, np.float32), np.array([w / 200.0, w / 150.0], np.float32)
        a, b = T.crop_affine_closed_form(center, scale, (288, 384)), T.crop_affine_rot_closed_form(center, scale, 0.0, 1.0, (288, 384))
        assert np.abs(a - b).max() <= 4 * np.spacing(np.abs(a).max()) and b[0, 1] == 0 and b[1, 0] == 0
    with pytest.raises(np.linalg.LinAlgError):
        T.crop_affine_rot_closed_form(np.array([3, 4], np.float32), np.array([0, 0], np.float32), 0.0, 1.0, (288, 384))


# ---- 2. draws -----------------------------------------------------------------------------------------------------------
def test_draw_table_reproduces_draw_augmentation():
    over = {"PROB_HALF_BODY": 0.6, "FLIP": False, "BBOX_AUGMENTATION": True}
    recs = G.records(14, 16)
    a, b = G.pipe_for(14, seed=7, **over), G.pipe_for(14, seed=7, **over)
    table = a.draw_table(recs)
    ref = [b.draw_augmentation(r, np.array(r["center"], np.float32), np.array(r["scale"], np.float32)) for r in recs]
    assert a.np_rng.rand() == b.np_rng.rand() and a.py_rng.random() == b.py_rng.random(), "the generators ended elsewhere"
    half = table["flags"] & 4 != 0
    assert 2 <= half.sum() <= 14 and not (table["flags"] & 8).any()
    assert (table["bbox_draws"] >= 0).all() and (table["bbox_draws"] <= 20).all() and len(np.unique(table["bbox_draws"])) > 5
    for i, (r, (c, s, rot, flip)) in enumerate(zip(recs, ref)):
        c0, s0 = (table["half_body"][i, :2], table["half_body"][i, 2:]) if half[i] else (r["center"], r["scale"])
        assert np.array_equal(c, c0) and c.dtype == np.float32, i
        assert s.dtype == np.float64 and np.array_equal(s, np.asarray(s0, np.float32).astype(np.float64) * table["draws"][i, 0]), i
        assert table["draws"][i, 3] == rot and flip is False
        assert table["draws"][i, 1] == np.sin(np.pi * rot / 180) and table["draws"][i, 2] == np.cos(np.pi * rot / 180)
    assert len({float(v) for v in table["draws"][:, 3]}) > 5 and (table["draws"][:, 3] == 0).any()
    # a record without the BBOX_AUGMENTATION key draws what it drew before the key existed
    c, d = G.pipe_for(14, seed=7), G.pipe_for(14, seed=7)
    d.new_augmentation = False
    assert all(c.draw(r)["rot"] == d.draw(r)["rot"] for r in recs) and c.draw(recs[0])["bbox_aug"] is None


def test_train_scale_is_float64():
    """numpy >= 2 (NEP 50): float32 array * float64 numpy scalar -> float64.  The train path's get_affine_transform and
    meta['scale'] see a float64 scale; buctd_sample_geometry widens the float32 scale and multiplies in float64 likewise."""
    pipe = G.pipe_for(14, seed=3)
    r = G.records(14, 16)[0]
    g = pipe.geometry(dict(r, image=np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8)))
    assert g["scale"].dtype == np.float64 and g["center"].dtype == np.float32
    d = G.draws([r])[0]
    g = pipe.geometry(dict(r, image=np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8)), aug=d)
    assert g["scale"].dtype == np.float64 and np.array_equal(g["scale"], r["scale"].astype(np.float64) * d["scale_mul"])
    assert not np.array_equal(g["scale"], (r["scale"] * np.float32(d["scale_mul"])).astype(np.float64))


# ---- 3. the keep-rectangle on the host path ----------------------------------------------------------------------------
@pytest.mark.parametrize("bbox,bbox_draws,flip,rect", [
    ([30.7, 20.2, 60.9, 50.5], None, False, (30, 20, 60, 50)),                      # inside the image
    ([0.0, 37.6, 80.2, 82.4], None, False, (0, 37, 80, 82)),                        # touching two borders
    ([30.7, 20.2, 60.9, 50.5], (0, 0), False, (30, 20, 60, 50)),                    # BBOX_AUGMENTATION draws 0 ...
    ([30.7, 20.2, 60.9, 50.5], (20, 20), False, (0, 0, 300, 250)),                  # ... and 20: x - 120 <= 0 -> 0, w + 240
    ([30.7, 20.2, 60.9, 50.5], (3, 7), True, (12, 0, 96, 120)),                     # flipped, 60 * 3 // 10 = 18, 50 * 7 // 10 = 35
    ([-7.5, 10.2, 90.0, 70.0], None, True, (0, 10, 83, 70)),                        # origin left of the image: cut at 0
])
def test_keep_rectangle_on_the_host_path(bbox, bbox_draws, flip, rect):
    from oracle import sample as S
    from buctd_amd.dataset.pipeline import keep_rectangle
    assert keep_rectangle(bbox, bbox_draws) == rect
    r = G.records(14, 16)[7]
    rec = dict(r, image=np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8), bbox=bbox)
    d = dict(G.draws([r])[0], flip=flip, bbox_aug=bbox_draws, rot=17.5)
    pipe = G.pipe_for(14, BBOX_AUGMENTATION=bbox_draws is not None)
    g = pipe.geometry(rec, aug=d)
    assert g["keep_rect"] == rect
    # what the table's rectangle means: the reference zeroes the (mirrored) image outside the unmirrored box, then warps
    img = r["image_np"][:, ::-1] if flip else r["image_np"]
    x, y, w, h = np.array(bbox).astype(int)
    if bbox_draws is not None:                                       # JointsDataset.py:267-273
        xd, yd = w * bbox_draws[0] // 10, h * bbox_draws[1] // 10
        x, y, w, h = (int(x - xd) if x - xd > 0 else 0), (int(y - yd) if y - yd > 0 else 0), int(w + 2 * xd), int(h + 2 * yd)
    masked = np.zeros_like(img)
    masked[max(y, 0):y + h, max(x, 0):x + w] = img[max(y, 0):y + h, max(x, 0):x + w]
    ref = S.warp_affine_u8(masked, g["trans"], G.CROP)
    got = S.warp_affine_u8(r["image_np"], g["trans"], G.CROP, flip_src=flip, keep_rect=g["keep_rect"])
    assert np.array_equal(got, ref) and (ref == 0).mean() > 0.02 and ref.any()
    # no box, or the key switched off: no rectangle
    assert pipe.geometry(dict(rec, bbox=None) if False else {k: v for k, v in rec.items() if k != "bbox"}, aug=d)["keep_rect"] is None
    assert G.pipe_for(14, NEW_AUGMENTATION=False).geometry(rec, aug=d)["keep_rect"] is None


def test_bottom_up_box_is_the_rectangle_under_use_bu_bbox():
    from buctd_amd.dataset.pipeline import box_from_keypoints, keep_rectangle
    r = G.records(14, 16)[9]
    rec = dict(r, image=np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8), use_bu_bbox=True)
    assert "bbox" not in rec
    g = G.pipe_for(14).geometry(rec, aug=G.draws([r])[0])
    assert g["keep_rect"] == keep_rectangle(box_from_keypoints(r["cond_joints"], 25, G.IMG_W, G.IMG_H))


# ---- 4. the crop of the closed-form matrix against the crop of the solve's -----------------------------------------------
def pipeline_batch():
    """The batch of the flag-on / flag-off pipeline test: seven records, hand-made draws (rotations 90, -0.01, 0, -33.25,
    0, 0.01, -90; flips; one half-body override)."""
    recs = G.records(14, 16)
    return recs[4:11], G.draws(recs)[4:11]


def test_crops_of_both_matrices_stay_inside_the_pipeline_tests_cap():
    """tests/test_gpu_sample_geometry.py allows 0.1 % of the crop pixels to differ by one level between the flag-on and
    the flag-off pipeline.  Here: the oracle warp fed with the solve's matrix and with the closed form's, same samples.
    And the heat-map centres of that batch are clear of an integer step, so its targets must be equal.
    The sources are noise, where one step of the warp's 1/32-px source grid is worth up to 8 levels: the cap of one level
    holds as long as no source coordinate sits on a rounding tie of that grid, which the two matrices (they differ by
    ~1e-14) would resolve differently.  That was seen once while choosing the fixture (record 9 with a rotation of 17.5
    degrees and a scale draw of 0.85: 3 of 18432 values, by 6 levels); this batch has no such tie, at any of its rotations."""
    from oracle import sample as S
    from buctd_amd.utils import transforms as T
    recs, ds = pipeline_batch()
    pipe = G.pipe_for(14)
    differ = total = 0
    for r, d in zip(recs, ds):
        g = pipe.geometry(dict(r, image=np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8)), aug=d)
        m = T.crop_affine_rot_closed_form(g["center"], g["scale"], np.sin(np.pi * d["rot"] / 180), np.cos(np.pi * d["rot"] / 180), G.CROP)
        assert np.abs(m - g["trans"]).max() <= G.TOL
        a = S.warp_affine_u8(r["image_np"], g["trans"], G.CROP, flip_src=d["flip"], keep_rect=g["keep_rect"]).astype(int)
        b = S.warp_affine_u8(r["image_np"], m, G.CROP, flip_src=d["flip"], keep_rect=g["keep_rect"]).astype(int)
        assert np.abs(a - b).max() <= 1
        differ, total = differ + int((a != b).sum()), total + a.size
        q = g["joints"][:, :2] / 4.0 + 0.5
        assert not G.near_integer(q[g["joints_vis"][:, 0] > 0]).any()
    print(f"{differ} of {total} crop values differ between the two matrices")
    assert differ <= 1e-3 * total
    assert {d["rot"] for d in ds} >= {0, 0.01, -90.0, 90.0} and any(d["flip"] for d in ds) and any(d["half_body"] for d in ds)
