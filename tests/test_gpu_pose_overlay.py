"""GPU suite for the pose overlay (buctd_vis_pose_overlay in csrc/vis_pose.hip under buctd_amd/utils/vis.py:draw_poses)
against the restatement tests/helpers/pose_overlay_ref.py.

The bar is equality on every byte: coverage and blend are integer expressions, so there is no tolerance.  The shapes are
the smallest that still visit every path: a canvas that is no multiple of the 64 x 16 tile, segments through several
tiles, more primitives than one round of the workgroup examines, clipping, strided rows, several canvases per launch."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import pose_overlay_ref as ref
from tests.helpers import vis_ref
from tests.helpers.png_read import decode_png

pytestmark = pytest.mark.gpu
EINVAL = -1
PAIR = [(0, 0, 1, 1, -1)]                       # one limb between two joints, in the person's colour
COLOURS = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (250, 120, 10), (9, 99, 199),
           (128, 128, 128), (1, 2, 3), (77, 200, 50)]


@functools.lru_cache(maxsize=None)
def _canvas(H, W, seed=0):
    a = np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _both(dev, canvas, poses, limbs, colours, palette=None, device_poses=False, **kw):
    """(device picture, restatement) of one canvas; limbs with a palette go to the package as a Skeleton"""
    from buctd_amd.utils import vis
    img = torch.from_numpy(canvas.copy()).to(dev)
    poses = np.asarray(poses, dtype=np.float32)
    colours = np.asarray(colours)[:len(poses)]
    sk = vis.Skeleton(poses.shape[1], tuple(limbs), palette) if palette is not None else np.asarray(limbs)
    got = vis.draw_poses(img, torch.from_numpy(poses).to(dev) if device_poses else poses, skeleton=sk,
                         colors=colours, style=kw.get('style', 'plain'), thickness=kw.get('thickness', 2),
                         radius=kw.get('radius', 3), score_thresh=kw.get('score_thresh', -1.0),
                         alpha=kw.get('alpha256', 256) / 256, offsets=kw.get('offsets'), clips=kw.get('clips'))
    assert got is img
    want = ref.draw_poses(canvas, poses, limbs, colours, palette=palette, **kw)
    return got.cpu().numpy(), want


# one segment per octant, horizontal, vertical and zero-length, spread over the 37 x 29 canvas
SEGMENTS = [((3, 3), (12, 6)), ((3, 8), (7, 17)), ((16, 18), (13, 9)), ((22, 6), (14, 3)), ((24, 9), (16, 12)),
            ((30, 5), (27, 14)), ((20, 25), (23, 16)), ((26, 23), (35, 20)), ((2, 26), (15, 26)), ((33, 2), (33, 12)),
            ((30, 26), (30, 26))]


@pytest.mark.parametrize("style", ['plain', 'pretty'])
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_every_octant_on_a_canvas_that_is_no_multiple_of_the_tile(dev, thickness, style):
    octants = {(np.sign(q[0] - p[0]), np.sign(q[1] - p[1]), abs(q[0] - p[0]) > abs(q[1] - p[1])) for p, q in SEGMENTS}
    assert len(octants) == 11
    poses = [[p, q] for p, q in SEGMENTS]
    got, want = _both(dev, _canvas(29, 37), poses, PAIR, COLOURS, style=style, thickness=thickness, radius=0 if style == 'pretty' else 3)
    assert np.array_equal(got, want)
    assert (want != _canvas(29, 37)).any()


def test_end_points_far_outside_and_absent_joints(dev):
    canvas = _canvas(29, 37, 1)
    far = [[(-8191, -8191), (8191, 8191)], [(8191, -8000), (-8192, 8100)], [(-8191.9, 14.5), (8191.9, 14.5)], [(18, -8192), (18, 8191)]]
    got, want = _both(dev, canvas, far, PAIR, COLOURS, thickness=3)
    assert np.array_equal(got, want) and (want[14] != canvas[14]).any(-1).all()
    # one end at 8192 / 9000 / -8193 is an absent joint: the picture of the same person with that joint NaN
    for bad in (8192.0, 9000.0, -8193.0, 3e38):
        gone = [[(5, 10), (bad, 10)], [(20, bad), (20, 20)]]
        nan = [[(5, 10), (np.nan, 10)], [(20, np.nan), (20, 20)]]
        got, want = _both(dev, canvas, gone, PAIR, COLOURS)
        assert np.array_equal(got, want) and np.array_equal(want, ref.draw_poses(canvas, nan, PAIR, COLOURS))
        assert np.array_equal(want[10, 12:], canvas[10, 12:])
    # the offset counts: 8000 + 192 is out of range, 8000 + 191 is not
    for dx, drawn in ((192, False), (191, True)):
        got, want = _both(dev, canvas, [[(-8000, 9), (8000, 9)]], PAIR, COLOURS, offsets=[(dx, 0)])
        assert np.array_equal(got, want) and (want[9] != canvas[9]).any() == drawn


def test_segments_through_several_tiles(dev):
    canvas = _canvas(50, 150)                                   # 3 x 4 tiles, the last ones partial
    poses = [[(2, 3), (147, 47)], [(140, 1), (5, 49)], [(64, 0), (64, 49)], [(0, 16), (149, 16)], [(63, 15), (64, 16)]]
    for thickness in (1, 4):
        got, want = _both(dev, canvas, poses, PAIR, COLOURS, thickness=thickness, style='pretty', radius=5)
        assert np.array_equal(got, want)


def test_clip_rectangle_cuts_a_disc_and_strided_rows_keep_their_padding(dev):
    from buctd_amd.utils import vis
    canvas = _canvas(29, 37, 2)
    poses, clips = [[(10, 10), (20, 12)], [(30, 20), (30, 20)]], [(8, 6, 19, 12), (0, 0, 33, 29)]
    kw = dict(style='pretty', thickness=3, radius=6, clips=clips)
    got, want = _both(dev, canvas, poses, PAIR, COLOURS, **kw)
    assert np.array_equal(got, want)
    changed = (want != canvas).any(-1)
    assert changed[6:12, 8:19].any() and not changed[:, :8].any() and not changed[12:, :19].any() and not changed[:, 33:].any()
    assert changed[6, 8:15].all() and changed[20, 32]            # the cut runs through both discs
    # the same picture as a view of a wider buffer: row stride 3 * 50, the bytes beside it stay as they were
    wide = torch.full((29, 50, 3), 201, dtype=torch.uint8, device=dev)
    wide[:, 5:42] = torch.from_numpy(canvas.copy()).to(dev)
    view = wide[:, 5:42]
    assert view.stride(0) == 150 > 3 * 37
    vis.draw_poses(view, np.asarray(poses, dtype=np.float32), skeleton=np.asarray(PAIR), colors=np.asarray(COLOURS[:2]),
                   style='pretty', thickness=3, radius=6, clips=clips)
    out = wide.cpu().numpy()
    assert np.array_equal(out[:, 5:42], want) and (out[:, :5] == 201).all() and (out[:, 42:] == 201).all()


def test_paint_order_between_persons_and_within_a_person(dev):
    canvas = _canvas(29, 37, 3)
    cross = [[(4, 4), (32, 24)], [(4, 24), (32, 4)]]
    got, want = _both(dev, canvas, cross, PAIR, COLOURS[:2], thickness=3)
    swapped, want_swapped = _both(dev, canvas, cross[::-1], PAIR, COLOURS[:2][::-1], thickness=3)
    assert np.array_equal(got, want) and np.array_equal(swapped, want_swapped)
    assert tuple(got[14, 18]) == COLOURS[1] and tuple(swapped[14, 18]) == COLOURS[0] and not np.array_equal(got, swapped)
    # within a person: limb 1's segment runs through limb 0's disc at (18, 14) and, drawn later, lies on top of it
    chain = [[(6, 14), (18, 14), (14, 6), (24, 22)]]
    limbs = [(0, 0, 1, 1, 0), (2, 2, 3, 3, 1)]
    palette = np.array([(200, 10, 10), (10, 10, 200)], dtype=np.uint8)
    got, want = _both(dev, canvas, chain, limbs, COLOURS[:1], palette=palette, style='pretty', thickness=2, radius=4)
    assert np.array_equal(got, want)
    assert tuple(got[14, 19]) == (10, 10, 200) and tuple(got[14, 16]) == (200, 10, 10) and tuple(got[14, 12]) == (200, 10, 10)
    got, want = _both(dev, canvas, chain, limbs[::-1], COLOURS[:1], palette=palette, style='pretty', thickness=2, radius=4)
    assert np.array_equal(got, want) and tuple(got[14, 19]) == (200, 10, 10)      # the other way round: the disc on top


def test_more_primitives_than_one_round(dev):
    from buctd_amd import _C
    from buctd_amd.utils import vis
    sk = vis.SKELETONS['coco_pretty']
    persons = 40
    assert persons * 3 * len(sk.limbs) > 4 * _C.VIS_POSE_CHUNK
    rng = np.random.default_rng(40)
    poses = np.concatenate([rng.uniform(4, 60, (persons, 17, 1)), rng.uniform(4, 44, (persons, 17, 1)),
                            rng.uniform(0, 1, (persons, 17, 1))], axis=-1).astype(np.float32)
    colours = rng.integers(0, 256, (persons, 3))
    for style, thresh in (('pretty', 0.2), ('plain', -1.0)):
        got, want = _both(dev, _canvas(48, 64), poses, sk.limbs, colours, palette=sk.palette, style=style, score_thresh=thresh,
                          device_poses=True)
        assert np.array_equal(got, want)
    assert (want != _canvas(48, 64)).any(-1).mean() > 0.5       # the persons overlap all over the canvas


def test_validity_and_mid_points(dev):
    canvas = _canvas(29, 37, 4)
    nan, inf = np.nan, np.inf
    poses = [[(5, 5, 1.0), (nan, 9, 1.0), (20, 5, 1.0), (25, 9, 1.0)],          # NaN x
             [(5, 12, 1.0), (9, inf, 1.0), (20, 12, 1.0), (-inf, 16, 1.0)],     # +inf y, -inf x
             [(5, 19, nan), (12, 19, 1.0), (20, 19, 0.5), (28, 19, 0.75)],      # NaN score; score == threshold
             [(-3.7, 24, 0.9), (4.2, 27, 0.9), (-4.2, -4.5, 0.9), (11, 25, 0.9)],   # negative coordinates, odd sums
             [(31, 3, inf), (35, 8, 0.6), (33, 14, 0.6), (30, 20, 0.6)]]        # an infinite score is not finite
    limbs = [(0, 0, 1, 1, -1), (2, 2, 3, 3, -1), (0, 1, 2, 3, -1), (1, 2, 3, 3, -1)]
    for style in ('plain', 'pretty'):
        got, want = _both(dev, canvas, poses, limbs, COLOURS, style=style, score_thresh=0.5)
        assert np.array_equal(got, want)
    assert ref.end_point(np.float32(poses[3]), 0, 1, (0, 0), 0.5) == (0, 25)      # (-3 + 4) >> 1, (24 + 27) >> 1
    assert ref.end_point(np.float32(poses[3]), 0, 2, (0, 0), 0.5) == (-4, 10)     # (-3 - 4) >> 1, (24 - 4) >> 1
    assert ref.end_point(np.float32(poses[3]), 2, 3, (0, 0), 0.5) == (3, 10)
    # without a score column every joint counts, whatever the threshold below 1
    xy = [[(5, 5), (20, 9)], [(8, 20), (30, 22)]]
    got, want = _both(dev, canvas, xy, PAIR, COLOURS, score_thresh=0.99)
    assert np.array_equal(got, want) and (want != canvas).any()
    got, want = _both(dev, canvas, xy, PAIR, COLOURS, score_thresh=1.0)
    assert np.array_equal(got, want) and np.array_equal(want, canvas)


@pytest.mark.parametrize("radius,thickness", [(3, 2), (1, 2), (1, 3), (0, 1), (5, 1)])
def test_rings_and_their_degenerate_forms(dev, radius, thickness):
    poses = [[(10, 10), (25, 18)], [(0, 0), (36, 28)]]
    got, want = _both(dev, _canvas(29, 37, 5), poses, PAIR, COLOURS, radius=radius, thickness=thickness)
    assert np.array_equal(got, want)
    hole = ref.ring_mask(29, 37, (25, 18), radius, thickness)[18, 25]
    assert hole == (2 * radius <= thickness) and (want != _canvas(29, 37, 5)).any()


@pytest.mark.parametrize("alpha256", [0, 179, 256])
@pytest.mark.parametrize("style", ['plain', 'pretty'])
def test_several_canvases_in_one_launch(dev, alpha256, style):
    """four canvases of different sizes: one person-free, one with three persons, one laid out as a 2 x 2 grid of cells
    with offsets and clip rectangles (a limb that leaves its cell is cut at the border), one a single tile"""
    from buctd_amd.utils import vis
    canvases = [_canvas(29, 37, 6), _canvas(16, 16, 6), _canvas(44, 90, 6), _canvas(9, 70, 6)]
    sk = vis.SKELETONS['coco_pretty'] if style == 'pretty' else vis.SKELETONS['coco']
    rng = np.random.default_rng(6)
    pose = lambda n, w, h: np.concatenate([rng.uniform(-3, w + 3, (n, 17, 1)), rng.uniform(-3, h + 3, (n, 17, 1)),
                                           rng.uniform(0, 1, (n, 17, 1))], axis=-1).astype(np.float32)
    cw, ch, pad = 42, 19, 2
    cells = [(pad + (i % 2) * (cw + pad), pad + (i // 2) * (ch + pad)) for i in range(4)]
    poses = [pose(3, 37, 29), np.zeros((0, 17, 3), dtype=np.float32), pose(4, cw, ch), pose(2, 70, 9)]
    offsets = [None, None, np.array(cells), None]
    clips = [None, None, np.array([(x, y, x + cw, y + ch) for x, y in cells]), None]
    colours = [rng.integers(0, 256, (len(p), 3)) for p in poses]
    imgs = [torch.from_numpy(c.copy()).to(dev) for c in canvases]
    out = vis.draw_poses(imgs, [poses[0], poses[1], torch.from_numpy(poses[2]).to(dev), poses[3]], skeleton=sk,
                         colors=colours, style=style, alpha=alpha256 / 256, score_thresh=0.1, offsets=offsets, clips=clips)
    assert out is not None and len(out) == 4
    for i, (img, canvas) in enumerate(zip(imgs, canvases)):
        want = ref.draw_poses(canvas, poses[i], sk.limbs, colours[i], palette=sk.palette, style=style, score_thresh=0.1,
                              alpha256=alpha256, offsets=offsets[i], clips=clips[i])
        assert np.array_equal(img.cpu().numpy(), want), i
        if i == 1 or alpha256 == 0:
            assert np.array_equal(want, canvas)
        else:
            assert (want != canvas).any()
        if i == 2:                                              # nothing in the padding between the cells
            assert np.array_equal(want[:, pad + cw:2 * pad + cw], canvas[:, pad + cw:2 * pad + cw])
            assert np.array_equal(want[pad + ch:2 * pad + ch], canvas[pad + ch:2 * pad + ch])


def test_default_colours_and_panels(dev):
    from buctd_amd.utils import vis
    canvas = _canvas(40, 52, 7)
    rng = np.random.default_rng(7)
    cond = np.concatenate([rng.uniform(0, 52, (3, 14, 1)), rng.uniform(0, 40, (3, 14, 1))], axis=-1).astype(np.float32)
    pred = cond + rng.uniform(-2, 2, cond.shape).astype(np.float32)
    pred[1, 4] = np.nan                                         # a low-confidence joint, as tools/inference.py marks it
    image = torch.from_numpy(canvas.copy()).to(dev)
    out = vis.render_pose_panels(image, cond, torch.from_numpy(pred).to(dev), skeleton='crowdpose')
    assert tuple(out.shape) == (40, 104, 3) and out.dtype == torch.uint8 and out.is_cuda
    assert np.array_equal(image.cpu().numpy(), canvas)
    limbs = vis.SKELETONS['crowdpose'].limbs
    wheel = vis.hsv_wheel(3)
    assert np.array_equal(out[:, :52].cpu().numpy(), ref.draw_poses(canvas, cond, limbs, wheel))
    assert np.array_equal(out[:, 52:].cpu().numpy(), ref.draw_poses(canvas, pred, limbs, wheel))


JOINT_H, JOINT_W = 30, 22


@functools.lru_cache(maxsize=None)
def _batch_case(B=3):
    rng = np.random.default_rng(17)
    image = (rng.standard_normal((B, 3, JOINT_H, JOINT_W)) * 0.8).astype(np.float32)
    joints = np.concatenate([rng.uniform(-2, JOINT_W + 2, (B, 17, 1)), rng.uniform(-2, JOINT_H + 2, (B, 17, 1)),
                             np.zeros((B, 17, 1))], axis=-1)
    return image, joints


def _pretty_want(image, joints, nrow, padding, bgr):
    from buctd_amd.utils import vis
    B, K = joints.shape[:2]
    zeros, hidden = np.zeros((B, K, 2), dtype=np.float32), np.zeros((B, K), dtype=np.float32)
    grid = vis_ref.joint_grid(image, zeros, hidden, zeros, hidden, nrow=nrow, padding=padding, bgr=bgr)
    xmaps = min(nrow, B)
    cells = [((b % xmaps) * (JOINT_W + padding) + padding, (b // xmaps) * (JOINT_H + padding) + padding) for b in range(B)]
    sk = vis.SKELETONS['coco_pretty']
    poses = np.concatenate([joints[..., :2], np.zeros((B, K, 1))], axis=-1)
    return ref.draw_poses(grid, poses, sk.limbs, [(0, 0, 0)] * B, palette=sk.palette, style='pretty', thickness=2, radius=3,
                          score_thresh=-1.0, alpha256=179, offsets=cells,
                          clips=[(x, y, x + JOINT_W, y + JOINT_H) for x, y in cells])


def test_save_pretty_batch_image_with_joints(dev, tmp_path):
    from buctd_amd.utils import vis
    image, joints = _batch_case()
    path = str(tmp_path / 'pretty.png')
    vis.save_pretty_batch_image_with_joints(torch.from_numpy(image).to(dev), torch.from_numpy(joints), None, path, nrow=2)
    got = decode_png(path)
    want = _pretty_want(image, joints, 2, 2, True)
    assert got.shape == (2 * (JOINT_H + 2) + 2, 2 * (JOINT_W + 2) + 2, 3) and np.array_equal(got, want)
    assert not got[:, :2].any() and not got[JOINT_H + 4:, JOINT_W + 4:].any()         # padding and the unused cell
    with pytest.raises(vis._C.BuctdHipError, match="skeleton"):
        vis.save_pretty_batch_image_with_joints(torch.from_numpy(image).to(dev), joints[:, :5], None, path)
    five = vis.Skeleton(5, ((0, 1, 2, 2, -1), (2, 2, 3, 4, -1)), None)
    vis.save_pretty_batch_image_with_joints(torch.from_numpy(image).to(dev), joints[:, :5], None, path, skeleton=five)
    assert (decode_png(path) != vis_ref.joint_grid(image, np.zeros((3, 5, 2), np.float32), np.zeros((3, 5), np.float32),
                                                   np.zeros((3, 5, 2), np.float32), np.zeros((3, 5), np.float32))).any()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_save_pretty_debug_images_writes_the_files_its_flags_name(dev, tmp_path):
    from buctd_amd.config import cfg
    from buctd_amd.utils import vis
    image, joints = _batch_case()
    x = torch.from_numpy(image).to(dev)
    rng = np.random.default_rng(3)
    target = torch.from_numpy(rng.random((3, 17, 8, 6), dtype=np.float32)).to(dev)
    output = torch.from_numpy(rng.standard_normal((3, 17, 8, 6)).astype(np.float32)).to(dev)
    meta = {'joints': torch.from_numpy(joints), 'joints_vis': torch.ones(3, 17, 3)}
    pred = joints[:, :, :2] + 1.5
    c = cfg.clone()
    c.defrost()
    flags = ('SAVE_BATCH_IMAGES_GT', 'SAVE_BATCH_IMAGES_PRED', 'SAVE_HEATMAPS_GT', 'SAVE_HEATMAPS_PRED')
    for k in flags:
        c.DEBUG[k] = True
    c.DEBUG.DEBUG = False
    vis.save_pretty_debug_images(c, x, meta, target, pred, output, str(tmp_path / 'off'), 'e1')
    assert _files(tmp_path) == []
    c.DEBUG.DEBUG = True
    vis.save_pretty_debug_images(c, x, meta, target, pred, output, str(tmp_path / 'all'), 'e1')
    assert _files(tmp_path) == ['all_gt_e1.png', 'all_hm_gt_e1.png', 'all_hm_pred_e1.png', 'all_pred_e1.png']
    bgr = not c.DATASET.COLOR_RGB
    assert np.array_equal(decode_png(str(tmp_path / 'all_gt_e1.png')), _pretty_want(image, joints, 8, 2, bgr))
    assert np.array_equal(decode_png(str(tmp_path / 'all_pred_e1.png')), _pretty_want(image, pred, 8, 2, bgr))
    assert np.array_equal(decode_png(str(tmp_path / 'all_hm_pred_e1.png')), vis.render_batch_heatmaps(x, output, bgr=bgr).cpu().numpy())
    for k in flags:
        c.DEBUG[k] = k == 'SAVE_BATCH_IMAGES_PRED'
    vis.save_pretty_debug_images(c, x, meta, target, pred, output, str(tmp_path / 'one'))
    assert _files(tmp_path)[-2:] == ['all_pred_e1.png', 'one_pred_.png'] and len(_files(tmp_path)) == 5


def test_refusals(dev):
    from buctd_amd import _C
    from buctd_amd.utils import vis
    lib = _C.lib()
    img = torch.full((20, 30, 3), 9, dtype=torch.uint8, device=dev)
    canvases = np.zeros(1, dtype=vis._CANVAS_ROW)
    canvases[0] = (img.data_ptr(), 90, 20, 30)
    table = lambda a: torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy()).to(dev)
    t_canvas, t_off = table(canvases), table(np.array([0, 1], dtype=np.int32))
    t_person = table(np.array([[0, 0, 0, 0, 30, 20, 0xff]], dtype=np.int32))
    t_joints = torch.tensor([[[3.0, 3.0, 1.0], [20.0, 15.0, 1.0]]], device=dev)
    t_limbs, t_tiles = table(np.array([[0, 0, 1, 1, -1]], dtype=np.int32)), table(np.array([[0, 0, 0], [0, 0, 1]], dtype=np.int32))

    def call(**kw):
        f = dict(canvases=t_canvas.data_ptr(), person_offsets=t_off.data_ptr(), persons=t_person.data_ptr(),
                 joints=t_joints.data_ptr(), skeleton=t_limbs.data_ptr(), palette=None, tiles=t_tiles.data_ptr(), C=1, P=1,
                 K=2, L=1, n_palette=0, n_tiles=2, canvas_h_max=20, canvas_w_max=30, style=_C.VIS_POSE_PLAIN, thickness=2,
                 radius=3, score_thresh=-1.0, alpha256=256)
        f.update(kw)
        return lib.buctd_vis_pose_overlay(ctypes.byref(_C.VisPoseArgs(**f)), _C.stream_ptr())

    bad = [dict(canvases=None), dict(person_offsets=None), dict(persons=None), dict(joints=None), dict(skeleton=None),
           dict(tiles=None), dict(n_palette=1), dict(K=65), dict(K=0), dict(L=65), dict(L=0), dict(thickness=0),
           dict(thickness=-2), dict(radius=-1), dict(canvas_h_max=8193), dict(canvas_w_max=8193), dict(alpha256=-1),
           dict(alpha256=257), dict(style=2), dict(C=0), dict(P=-1), dict(n_tiles=-1)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b'buctd_vis_pose_overlay' in lib.buctd_last_error(), kw
    assert lib.buctd_vis_pose_overlay(None, _C.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert (img == 9).all()                                      # no refused call launched anything
    assert call(P=0) == 0 and call(n_tiles=0) == 0
    torch.cuda.synchronize()
    assert (img == 9).all()
    assert call() == 0
    want = ref.draw_poses(np.full((20, 30, 3), 9, dtype=np.uint8), [[(3, 3), (20, 15)]], PAIR, [(255, 0, 0)])
    assert np.array_equal(img.cpu().numpy(), want)
    # the host mirror: a limb index >= K is refused before anything is uploaded or drawn; so are the library's refusals
    before = img.clone()
    with pytest.raises(_C.BuctdHipError, match="buctd_vis_pose_overlay"):
        vis.draw_poses(img, np.zeros((1, 2, 2), np.float32), skeleton=[(0, 2)])
    with pytest.raises(_C.BuctdHipError, match="buctd_vis_pose_overlay.*alpha256"):
        vis.draw_poses(img, np.zeros((1, 2, 2), np.float32), skeleton=[(0, 1)], alpha=1.5)
    with pytest.raises(_C.BuctdHipError, match="buctd_vis_pose_overlay.*thickness"):
        vis.draw_poses(img, np.zeros((1, 2, 2), np.float32), skeleton=[(0, 1)], thickness=0)
    with pytest.raises(_C.BuctdHipError):
        vis.draw_poses(img.cpu(), np.zeros((1, 2, 2), np.float32), skeleton=[(0, 1)])
    assert torch.equal(img, before)
