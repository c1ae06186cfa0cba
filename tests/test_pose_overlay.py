"""The pose overlay's restatement (tests/helpers/pose_overlay_ref.py) and the host tables of buctd_amd/utils/vis.py,
checked against properties of the pixel rules in include/buctd_hip.h and values worked by hand.  No GPU."""
import numpy as np
import pytest

from tests.helpers import pose_overlay_ref as ref

H, W = 29, 37
ENDS = [((5, 4), (30, 9)), ((30, 9), (5, 4)), ((6, 3), (11, 25)), ((20, 20), (3, 2)), ((2, 14), (33, 14)), ((18, 1), (18, 27)),
        ((-9, 5), (50, 21)), ((12, 12), (12, 12))]


@pytest.mark.parametrize("t", [1, 2, 3, 6])
def test_segment_mask_does_not_depend_on_the_order_of_its_ends(t):
    for p, q in ENDS:
        m = ref.segment_mask(H, W, p, q, t)
        assert np.array_equal(m, ref.segment_mask(H, W, q, p, t))
        if 0 <= p[0] < W and 0 <= p[1] < H:
            assert m[p[1], p[0]] and m.any()


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5])
def test_zero_length_segment_of_thickness_2r_is_the_disc_of_radius_r(r):
    for z in [(12, 12), (0, 0), (36, 28), (-1, 3)]:
        assert np.array_equal(ref.segment_mask(H, W, z, z, 2 * r), ref.disc_mask(H, W, z, r))


def test_masks_are_symmetric_under_mirroring_the_canvas():
    mx = lambda p: (W - 1 - p[0], p[1])
    my = lambda p: (p[0], H - 1 - p[1])
    for p, q in ENDS:
        for t in (1, 2, 3):
            m = ref.segment_mask(H, W, p, q, t)
            assert np.array_equal(m[:, ::-1], ref.segment_mask(H, W, mx(p), mx(q), t))
            assert np.array_equal(m[::-1], ref.segment_mask(H, W, my(p), my(q), t))
        assert np.array_equal(ref.disc_mask(H, W, p, 3)[:, ::-1], ref.disc_mask(H, W, mx(p), 3))
        assert np.array_equal(ref.ring_mask(H, W, p, 3, 2)[::-1], ref.ring_mask(H, W, my(p), 3, 2))


def test_masks_by_hand():
    # thickness 1: 4 d^2 <= 1, the pixels of the row itself; thickness 2: d <= 1, the rows beside it and the end caps
    m = ref.segment_mask(7, 9, (2, 3), (6, 3), 1)
    assert m.sum() == 5 and m[3, 2:7].all()
    m = ref.segment_mask(7, 9, (2, 3), (6, 3), 2)
    assert m.sum() == 5 * 3 + 2 and m[2:5, 2:7].all() and m[3, 1] and m[3, 7]
    assert ref.disc_mask(9, 9, (4, 4), 3).sum() == 29                      # x^2 + y^2 <= 9
    ring = ref.ring_mask(9, 9, (4, 4), 3, 2)                               # 16 <= 4 d^2 <= 64: 4 <= d^2 <= 16
    assert ring[4, 4 + 2] and ring[4, 4 + 4] and not ring[4, 4 + 1] and not ring[4, 4] and ring[4 + 2, 4 + 3]
    assert np.array_equal(ref.ring_mask(9, 9, (4, 4), 1, 2), ref.disc_mask(9, 9, (4, 4), 2))     # 2r <= t: no hole


def test_floor_midpoint_and_joint_pixel():
    assert ref.floor_mid(-3, 4) == 0 and ref.floor_mid(-3, -4) == -4 and ref.floor_mid(3, 4) == 3
    assert ref.floor_mid(-3, 4) == (np.int16(-3) + np.int16(4)) // 2 and ref.floor_mid(-3, -4) == (np.int16(-3) + np.int16(-4)) // 2
    assert ref.joint_pixel((-0.9, 2.9, 0.0), (0, 0), -1.0) == (0, 2)              # truncation toward zero
    assert ref.joint_pixel((-1.5, 2.0), (10, -3), 0.5) == (9, -1)                 # a missing score counts as 1
    assert ref.joint_pixel((1.0, 2.0, 0.5), (0, 0), 0.5) is None                  # score == threshold
    for bad in (np.nan, np.inf, -np.inf):
        assert ref.joint_pixel((bad, 2.0, 1.0), (0, 0), -1.0) is None
        assert ref.joint_pixel((1.0, bad, 1.0), (0, 0), -1.0) is None
        assert ref.joint_pixel((1.0, 2.0, bad), (0, 0), -1.0) is None
    assert ref.joint_pixel((8191.9, -8192.9, 1.0), (0, 0), -1.0) == (8191, -8192)
    assert ref.joint_pixel((8192.0, 0.0, 1.0), (0, 0), -1.0) is None
    assert ref.joint_pixel((0.0, -8193.0, 1.0), (0, 0), -1.0) is None
    assert ref.joint_pixel((8000.0, 0.0, 1.0), (192, 0), -1.0) is None            # the offset counts


def test_blend_and_paint_order_by_hand():
    canvas = np.full((5, 5, 3), 100, dtype=np.uint8)
    poses = [[[1, 2], [3, 2]], [[2, 1], [2, 3]]]                                   # a horizontal, then a vertical limb
    got = ref.draw_poses(canvas, poses, [(0, 0, 1, 1, -1)], [(255, 0, 0), (0, 0, 255)], style='pretty', thickness=1,
                         radius=0, alpha256=179)
    red = ((100 * 77 + 255 * 179 + 128) >> 8, (100 * 77 + 128) >> 8, (100 * 77 + 128) >> 8)
    assert tuple(got[2, 1]) == red and tuple(got[2, 3]) == red
    assert tuple(got[2, 2]) == red[::-1] and tuple(got[1, 2]) == red[::-1]        # the later person lies on top
    assert tuple(got[0, 0]) == (100, 100, 100) and (got != 100).any(-1).sum() == 5
    assert np.array_equal(ref.draw_poses(canvas, poses, [(0, 0, 1, 1, -1)], [(255, 0, 0)] * 2, alpha256=0), canvas)
    assert round(0.7 * 256) == 179


def test_skeleton_tables():
    from buctd_amd.utils import vis
    for name, sk in vis.SKELETONS.items():
        limbs = np.asarray(sk.limbs)
        assert limbs.shape[1] == 5 and 1 <= len(limbs) <= 64 and sk.num_joints <= 64, name
        assert limbs[:, :4].min() >= 0 and limbs[:, :4].max() < sk.num_joints, name
        n = 0 if sk.palette is None else len(sk.palette)
        assert limbs[:, 4].min() >= -1 and limbs[:, 4].max() < n, name
    assert vis.SKELETONS['coco'].num_joints == 17 and len(vis.SKELETONS['coco'].limbs) == 18
    assert vis.SKELETONS['crowdpose'].num_joints == 14 and len(vis.SKELETONS['crowdpose'].limbs) == 17
    pretty = vis.SKELETONS['coco_pretty']
    assert len(pretty.limbs) == 17 and pretty.palette.shape == (17, 3) and pretty.palette.dtype == np.uint8
    # mid-shoulder - nose and mid-shoulder - mid-hip come first, in the last two rainbow colours
    assert pretty.limbs[0] == (6, 5, 0, 0, 15) and pretty.limbs[1] == (6, 5, 12, 11, 16)
    assert [l[4] for l in pretty.limbs[2:]] == list(range(15))
    assert all(l[0] == l[1] and l[2] == l[3] for l in pretty.limbs[2:])
    assert pretty.limbs[2] == (1, 1, 2, 2, 0) and pretty.limbs[-1] == (12, 12, 11, 11, 14)
    assert vis.SKELETONS['coco'].limbs[4] == (3, 3, 5, 5, -1) and vis.SKELETONS['crowdpose'].limbs[-1] == (3, 3, 13, 13, -1)
    with pytest.raises(vis._C.BuctdHipError, match="buctd_vis_pose_overlay"):
        vis._skeleton_tables('coco', 16)                                           # a limb index >= K, before any upload
    with pytest.raises(vis._C.BuctdHipError):
        vis._skeleton_tables([(0, 0, 1, 1, 0)], 2)                                 # a colour without a palette


def test_palettes_by_hand():
    from buctd_amd.utils import vis
    pal = vis.rainbow_palette(17)
    assert tuple(pal[0]) == (128, 0, 255) and tuple(pal[-1]) == (255, 0, 0)       # |0 - 0.5|, sin 0, cos 0; |2 - 0.5| clipped
    assert vis.rainbow_palette(1).shape == (1, 3)
    wheel = vis.hsv_wheel(4)
    assert tuple(wheel[0]) == (255, 0, 0) and wheel.shape == (4, 3) and wheel.dtype == np.uint8
    assert vis.hsv_wheel(1).tolist() == [[255, 0, 0]] and vis.hsv_wheel(0).shape == (0, 3)


@pytest.mark.parametrize("n", [17, 2, 5, 18, 64])
def test_palettes_equal_matplotlib(n):
    mpl = pytest.importorskip("matplotlib")
    from buctd_amd.utils import vis
    cmap = mpl.colormaps['rainbow']
    want = np.rint(np.array([cmap(x)[:3] for x in np.linspace(0, 1, n)]) * 255).astype(np.uint8)
    assert np.array_equal(vis.rainbow_palette(n), want)
    hsv = mpl.colormaps['hsv'].resampled(n)
    want = np.rint(np.array([hsv(i)[:3] for i in range(n)]) * 255).astype(np.uint8)
    assert np.array_equal(vis.hsv_wheel(n), want)
