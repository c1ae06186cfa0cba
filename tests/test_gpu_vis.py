"""GPU suite for the debug pictures (buctd_amd/utils/vis.py over buctd_vis_minmax / buctd_vis_heatmap_grid /
buctd_vis_joint_grid in csrc/vis.hip) against the restatement tests/helpers/vis_ref.py.

The bar is equality on every byte: each value is an integer expression of bytes or an fp32 expression fixed operation
by operation in a library built without contraction.  A restatement is computed once per case and shared by the memory
layouts it is compared under."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import vis_ref as ref
from tests.helpers.png_read import decode_png

pytestmark = pytest.mark.gpu
EINVAL = -1

# (B, K, H, W, Hh, Wh): ratio 4 on both axes; different ratios per axis, odd Wh; ratio 1; a non-integer ratio
HEAT_SHAPES = [(3, 5, 32, 24, 8, 6), (2, 17, 36, 28, 12, 7), (1, 1, 8, 8, 8, 8), (2, 3, 30, 20, 8, 6)]


@functools.lru_cache(maxsize=None)
def _heat_case(shape):
    """Image values beyond [0, 1], heat values below 0 and above 1; peaks in the four corners (the markers clip), two
    joints on one pixel, and for K = 17 one map without a positive value (its peak is reported as (0, 0))."""
    B, K, H, W, Hh, Wh = shape
    rng = np.random.default_rng(sum(shape))
    image = (rng.standard_normal((B, 3, H, W)) * 1.2 + 0.4).astype(np.float32)
    heat = (rng.standard_normal((B, K, Hh, Wh)) * 0.6 + 0.3).astype(np.float32)
    assert heat.min() < 0 and heat.max() > 1
    corners = [(0, 0), (Wh - 1, 0), (0, Hh - 1), (Wh - 1, Hh - 1), (Wh - 1, Hh - 1)]
    for b in range(B):
        for j in range(min(K, len(corners))):
            x, y = corners[(j + b) % len(corners)] if K >= len(corners) else corners[-1 - j]
            heat[b, j, y, x] = 5.0
    if K == 17:
        heat[:, 6] = -np.abs(heat[:, 6])
    return image, heat


@functools.lru_cache(maxsize=None)
def _heat_want(shape, normalize, bgr):
    image, heat = _heat_case(shape)
    return ref.heatmap_grid(image, heat, ref.max_preds(heat), normalize=normalize, bgr=bgr)


def _layout(image, dev, layout):
    t = torch.from_numpy(image).to(dev)
    if layout == 'nhwc':
        t = t.contiguous(memory_format=torch.channels_last)
        assert t.stride(1) == 1 or t.size(1) == 1
    return t


@pytest.mark.parametrize("layout", ['nchw', 'nhwc'])
@pytest.mark.parametrize("normalize,bgr", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("shape", HEAT_SHAPES)
def test_heatmap_grid_equals_restatement(dev, shape, normalize, bgr, layout):
    from buctd_amd.utils import vis
    image, heat = _heat_case(shape)
    got = vis.render_batch_heatmaps(_layout(image, dev, layout), torch.from_numpy(heat).to(dev), normalize=normalize, bgr=bgr)
    want = _heat_want(shape, normalize, bgr)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


def test_heat_cases_hold_what_they_claim():
    """the corner peaks, the shared pixel and the map without a positive value, read off the restatement's decode"""
    for shape in HEAT_SHAPES:
        B, K, H, W, Hh, Wh = shape
        peaks = ref.max_preds(_heat_case(shape)[1])
        corners = {(0.0, 0.0), (Wh - 1.0, 0.0), (0.0, Hh - 1.0), (Wh - 1.0, Hh - 1.0)}
        assert {tuple(p) for p in peaks.reshape(-1, 2)} & corners
        if K >= 5:
            assert {tuple(p) for p in peaks[:, :5].reshape(-1, 2)} == corners
            assert any(len({tuple(p) for p in peaks[b, :5]}) == 4 for b in range(B))      # 5 joints, 4 pixels
        if K == 3:
            assert tuple(peaks[0, 0]) == tuple(peaks[0, 1])
    assert (_heat_case(HEAT_SHAPES[1])[1][:, 6] <= 0).all()


def test_heatmap_grid_constant_image(dev):
    """hi == lo: u = 0 / 1e-5 = 0, every image byte is 0"""
    from buctd_amd.utils import vis
    shape = HEAT_SHAPES[0]
    _, heat = _heat_case(shape)
    image = np.full((shape[0], 3, shape[2], shape[3]), 0.37, dtype=np.float32)
    want = ref.heatmap_grid(image, heat, ref.max_preds(heat))
    got = vis.render_batch_heatmaps(torch.from_numpy(image).to(dev), torch.from_numpy(heat).to(dev))
    assert np.array_equal(got.cpu().numpy(), want)
    untouched = (want[:, :shape[5]] != ref.RED).any(-1)
    assert untouched.any() and not want[:, :shape[5]][untouched].any()


def _heatmap_entry(dev, image, heat, peaks, lohi=None, bgr=1):
    from buctd_amd import _C
    B, _, H, W = image.shape
    _, K, Hh, Wh = heat.shape
    out = torch.full((B * Hh, (K + 1) * Wh, 3), 77, dtype=torch.uint8, device=dev)
    rc = _C.lib().buctd_vis_heatmap_grid(_C.ptr(image), B, H, W, *image.stride(), _C.ptr(lohi), _C.ptr(heat), K, Hh, Wh,
                                         _C.ptr(peaks), bgr, _C.ptr(out), _C.stream_ptr())
    return rc, out


def test_heatmap_grid_fractional_and_outside_peaks(dev):
    """positions are truncated toward zero: (-0.6, 2.9) marks around (0, 2); a peak far outside leaves no marker.  The
    picture has 1 * 5 * 3 * 7 = 105 pixels - no multiple of 4, the last thread writes single bytes."""
    rng = np.random.default_rng(11)
    image = rng.random((1, 3, 10, 14), dtype=np.float32)
    heat = rng.random((1, 2, 5, 7), dtype=np.float32)
    peaks = np.array([[[-0.6, 2.9], [40.0, 1.0]]], dtype=np.float32)
    rc, out = _heatmap_entry(dev, torch.from_numpy(image).to(dev), torch.from_numpy(heat).to(dev),
                             torch.from_numpy(peaks).to(dev))
    assert rc == 0
    want = ref.heatmap_grid(image, heat, peaks, normalize=False)
    assert np.array_equal(out.cpu().numpy(), want)
    assert tuple(want[2, 1]) == ref.RED and (want[:, 14:] != ref.RED).any(-1).all()


@pytest.mark.parametrize("layout", ['nchw', 'nhwc', 'view'])
def test_minmax(dev, layout):
    """18000 elements: nine blocks meet in the two atomics"""
    from buctd_amd.utils import vis
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 5 if layout == 'view' else 3, 40, 50)).astype(np.float32))
    x = x.to(dev)
    if layout == 'nhwc':
        x = x.contiguous(memory_format=torch.channels_last)
    if layout == 'view':
        x[:, 3:] = 100.0          # behind the three channels of the picture: not read
    lohi = vis._minmax(x)
    assert lohi.tolist() == [float(x[:, :3].min()), float(x[:, :3].max())]


JOINT_K, JOINT_H, JOINT_W = 7, 14, 11


@functools.lru_cache(maxsize=None)
def _joint_case(B):
    """Per image seven joints: inside; on the far border; at (-0.6, -0.3), which truncates to (0, 0); outside the cell;
    invisible; predicted, ground-truth and condition mark on one pixel; a condition joint at x = 0 (not drawn)."""
    H, W, K = JOINT_H, JOINT_W, JOINT_K
    rng = np.random.default_rng(100 + B)
    image = (rng.standard_normal((B, 3, H, W)) * 0.8).astype(np.float32)
    pred = np.zeros((B, K, 3)); gt = np.zeros((B, K, 3)); cond = np.zeros((B, K, 3))
    pred_vis = np.ones((B, K, 3)); gt_vis = np.ones((B, K, 3)); cond_vis = np.ones((B, K, 3))
    for b in range(B):
        pred[b, 0, :2] = (3.7 + b % 3, 4.2); gt[b, 0, :2] = (6.1, 9.9 - b % 2); cond[b, 0, :2] = (8.5, 2.5)
        pred[b, 1, :2] = (W - 1, H - 1); gt[b, 1, :2] = (W - 1, 0.0); cond[b, 1, :2] = (0.5, H - 1)
        pred[b, 2, :2] = (-0.6, -0.3); gt[b, 2, :2] = (-0.9, 5.0); cond[b, 2, :2] = (5.0, 0.2)
        pred[b, 3, :2] = (W + 1, 3.0); gt[b, 3, :2] = (4.0, H + 1); cond[b, 3, :2] = (W + 7, H + 7)
        pred[b, 4, :2] = gt[b, 4, :2] = cond[b, 4, :2] = (5.0, 7.0)
        pred_vis[b, 4] = gt_vis[b, 4] = cond_vis[b, 4] = 0
        pred[b, 5, :2] = gt[b, 5, :2] = cond[b, 5, :2] = (2.0 + b % 4, 11.0)
        pred_vis[b, 6] = gt_vis[b, 6] = 0
        cond[b, 6, :2] = (0.0, 6.0)
    gt_vis[:, :, 1:] = 0          # only the first entry of a visibility row counts ...
    cond_vis[:, 1, 0] = 0         # ... but a condition's row is summed
    meta = {'joints': torch.from_numpy(gt), 'joints_vis': torch.from_numpy(gt_vis),
            'cond_joints': torch.from_numpy(cond), 'cond_joints_vis': torch.from_numpy(cond_vis)}
    return image, pred[:, :, :2].copy(), pred_vis, meta


@functools.lru_cache(maxsize=None)
def _joint_want(B, padding, with_cond, bgr):
    image, pred, pred_vis, meta = _joint_case(B)
    f = lambda a: np.asarray(a, dtype=np.float32)
    cond = f(meta['cond_joints'].numpy()[:, :, :2]) if with_cond else None
    cond_vis = f(meta['cond_joints_vis'].numpy().sum(-1)) if with_cond else None
    return ref.joint_grid(image, f(pred), f(pred_vis[:, :, 0]), f(meta['joints'].numpy()[:, :, :2]),
                          f(meta['joints_vis'].numpy()[:, :, 0]), cond, cond_vis, nrow=8, padding=padding, bgr=bgr)


@pytest.mark.parametrize("layout,bgr", [('nchw', True), ('nhwc', False)])
@pytest.mark.parametrize("with_cond", [True, False])
@pytest.mark.parametrize("padding", [2, 0])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_joint_grid_equals_restatement(dev, B, padding, with_cond, layout, bgr):
    from buctd_amd.utils import vis
    image, pred, pred_vis, meta = _joint_case(B)
    if not with_cond:
        meta = {k: v for k, v in meta.items() if not k.startswith('cond')}
    got = vis.render_batch_image_with_joints(_layout(image, dev, layout), pred, pred_vis, meta, nrow=8, padding=padding,
                                             bgr=bgr)
    want = _joint_want(B, padding, with_cond, bgr)
    xmaps, ymaps = min(8, B), -(-B // min(8, B))
    assert want.shape == (ymaps * (JOINT_H + padding) + padding, xmaps * (JOINT_W + padding) + padding, 3)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


def test_joint_case_holds_what_it_claims():
    want = _joint_want(9, 2, True, True)
    plain = _joint_want(9, 2, False, True)
    cell = want[2:2 + JOINT_H, 2:2 + JOINT_W]
    assert tuple(cell[11, 2]) == ref.GREEN and tuple(cell[11, 3]) == ref.BLUE and tuple(cell[9, 2]) == ref.BLUE
    assert tuple(cell[9, 4]) == ref.GREEN and tuple(cell[9, 3]) == ref.RED        # x over + over disc, joint 5
    assert tuple(plain[2 + 11, 2 + 2]) == ref.BLUE
    assert tuple(cell[0, 0]) == ref.RED                                              # (-0.6, -0.3) -> (0, 0)
    assert not (cell[4:9, 0] == ref.GREEN).all(-1).any()                             # the condition joint at x = 0
    assert (cell[:, JOINT_W - 1] == ref.RED).all(-1).any()                           # the disc of the joint outside, clipped
    assert not want[2 + JOINT_H:4 + JOINT_H].any() and not want[:, :2].any()         # padding
    assert not want[4 + JOINT_H:, 2 + JOINT_W + 2:].any()                            # the seven unused cells of row 2
    assert want[4 + JOINT_H:4 + 2 * JOINT_H, 2:2 + JOINT_W].any()


def test_entries_refuse_null_pointers_and_zero_extents(dev):
    from buctd_amd import _C
    lib = _C.lib()
    img = torch.zeros(1, 3, 8, 8, device=dev)
    lohi = torch.full((2,), 7.0, device=dev)
    hm = torch.zeros(1, 2, 4, 4, device=dev)
    xy = torch.zeros(1, 2, 2, device=dev)
    vis = torch.ones(1, 2, device=dev)
    out = torch.full((64, 64, 3), 9, dtype=torch.uint8, device=dev)
    st, p, s = _C.stream_ptr(), _C.ptr, img.stride()
    assert lib.buctd_vis_minmax(None, 1, 8, 8, *s, p(lohi), st) == EINVAL
    assert lib.buctd_vis_minmax(p(img), 1, 8, 8, *s, None, st) == EINVAL
    assert lib.buctd_vis_minmax(p(img), 1, 0, 8, *s, p(lohi), st) == EINVAL
    assert lib.buctd_vis_minmax(p(img), 0, 8, 8, *s, p(lohi), st) == EINVAL
    heat = lambda im, h, pk, o, K=2, Hh=4, Wh=4, H=8: lib.buctd_vis_heatmap_grid(im, 1, H, 8, *s, p(lohi), h, K, Hh, Wh, pk,
                                                                                   1, o, st)
    assert heat(p(img), p(hm), p(xy), p(out)) == 0
    assert heat(None, p(hm), p(xy), p(out)) == EINVAL
    assert heat(p(img), None, p(xy), p(out)) == EINVAL
    assert heat(p(img), p(hm), None, p(out)) == EINVAL
    assert heat(p(img), p(hm), p(xy), None) == EINVAL
    assert heat(p(img), p(hm), p(xy), p(out) + 1) == EINVAL
    for kw in ({'K': 0}, {'Hh': 0}, {'Wh': -1}, {'H': 0}):
        assert heat(p(img), p(hm), p(xy), p(out), **kw) == EINVAL
    assert b'buctd_vis_heatmap_grid' in lib.buctd_last_error()
    joint = lambda im, a, av, g, gv, c, cv, o, K=2, nrow=8, pad=2, W=8: lib.buctd_vis_joint_grid(
        im, 1, 8, W, *s, p(lohi), K, a, av, g, gv, c, cv, nrow, pad, 1, o, st)
    assert joint(p(img), p(xy), p(vis), p(xy), p(vis), None, None, p(out)) == 0
    assert joint(p(img), p(xy), p(vis), p(xy), p(vis), p(xy), p(vis), p(out)) == 0
    assert joint(None, p(xy), p(vis), p(xy), p(vis), None, None, p(out)) == EINVAL
    assert joint(p(img), None, p(vis), p(xy), p(vis), None, None, p(out)) == EINVAL
    assert joint(p(img), p(xy), None, p(xy), p(vis), None, None, p(out)) == EINVAL
    assert joint(p(img), p(xy), p(vis), None, p(vis), None, None, p(out)) == EINVAL
    assert joint(p(img), p(xy), p(vis), p(xy), None, None, None, p(out)) == EINVAL
    assert joint(p(img), p(xy), p(vis), p(xy), p(vis), p(xy), None, p(out)) == EINVAL
    assert joint(p(img), p(xy), p(vis), p(xy), p(vis), None, None, None) == EINVAL
    for kw in ({'K': 0}, {'nrow': 0}, {'pad': -1}, {'W': 0}):
        assert joint(p(img), p(xy), p(vis), p(xy), p(vis), None, None, p(out), **kw) == EINVAL
    torch.cuda.synchronize()
    assert lohi.tolist() == [7.0, 7.0]           # no refused call launched anything


def _debug_cfg(debug):
    from buctd_amd.config import cfg
    c = cfg.clone()
    c.defrost()
    c.DEBUG.DEBUG = debug
    for k in ('SAVE_BATCH_IMAGES_GT', 'SAVE_BATCH_IMAGES_PRED', 'SAVE_HEATMAPS_GT', 'SAVE_HEATMAPS_PRED'):
        c.DEBUG[k] = True
    return c


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_debug_hook_end_to_end(dev, tmp_path):
    from buctd_amd.core.function import _save_debug_images
    from buctd_amd.utils import vis
    image, pred, _, meta = _joint_case(3)
    x = torch.from_numpy(image).to(dev)
    rng = np.random.default_rng(8)
    target = torch.from_numpy(rng.random((3, JOINT_K, 7, 5), dtype=np.float32)).to(dev)
    output = torch.from_numpy(rng.standard_normal((3, JOINT_K, 7, 5)).astype(np.float32)).to(dev)
    keep = (x.clone(), target.clone(), output.clone())

    off = tmp_path / 'off'
    off.mkdir()
    _save_debug_images(_debug_cfg(False), x, meta, target, pred, output, str(off / 'val_0'), output_dir=str(off))
    assert _files(off) == []

    on = tmp_path / 'on'
    on.mkdir()
    cfg = _debug_cfg(True)
    bgr = not cfg.DATASET.COLOR_RGB
    _save_debug_images(cfg, x, meta, target, pred, output, str(on / 'val_0'), output_dir=str(on))
    assert _files(on) == ['val_0_hm_gt_.png', 'val_0_hm_pred_.png', os.path.join('val_0_pred', 'batch.png')]
    for t, k in zip((x, target, output), keep):
        assert torch.equal(t, k)
    want = {'val_0_hm_gt_.png': vis.render_batch_heatmaps(x, target, bgr=bgr),
            'val_0_hm_pred_.png': vis.render_batch_heatmaps(x, output, bgr=bgr),
            os.path.join('val_0_pred', 'batch.png'): vis.render_batch_image_with_joints(x, pred, meta['joints_vis'], meta,
                                                                                        bgr=bgr)}
    for name, picture in want.items():
        assert np.array_equal(decode_png(str(on / name)), picture.cpu().numpy()), name
    # meta['pred_joints_vis'] takes the place of meta['joints_vis'] for the predicted joints
    hidden = dict(meta, pred_joints_vis=torch.zeros(3, JOINT_K, 1))
    cfg.DEBUG.SAVE_HEATMAPS_GT = cfg.DEBUG.SAVE_HEATMAPS_PRED = False
    _save_debug_images(cfg, x, hidden, target, pred, output, str(on / 'val_1'))
    assert _files(on)[-1] == os.path.join('val_1_pred', 'batch.png') and len(_files(on)) == 4
    got = decode_png(str(on / 'val_1_pred' / 'batch.png'))
    assert np.array_equal(got, vis.render_batch_image_with_joints(x, pred, hidden['pred_joints_vis'], hidden,
                                                                  bgr=bgr).cpu().numpy())
    assert not (got == ref.RED).all(-1).any()
