"""Host checks of the debug pictures (buctd_amd/utils/vis.py): the PNG writer against the decoder of
tests/helpers/png_read.py, the restatement tests/helpers/vis_ref.py against values worked by hand, and the hook's
DEBUG.DEBUG gate.  No device."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import vis_ref as ref
from tests.helpers.png_read import decode_png


@pytest.mark.parametrize("shape", [(5, 7), (1, 1)])
def test_write_png_round_trip(tmp_path, shape):
    from buctd_amd.utils.vis import write_png
    img = np.random.default_rng(3).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    path = str(tmp_path / 'a.png')
    write_png(path, img)
    got = decode_png(path)
    assert got.shape == img.shape and np.array_equal(got, img)


def test_write_png_refuses_other_arrays(tmp_path):
    from buctd_amd.utils.vis import write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / 'bad.png'), bad)
    assert os.listdir(tmp_path) == []


def test_ref_jet_bytes():
    """c = clamp(1.5 - |4t - centre|, 0, 1), byte = floor(c * 255 + 0.5), t = byte / 255, centres 3, 2, 1 for r, g, b.
    0:   t = 0: r = g = 0, b = 0.5 -> floor(128.0) = 128.
    64:  4t = 256/255: g = 1.5 - 254/255 = 128.5/255, on 129.0 in real numbers; fp32's t = 64/255 is rounded up
         (0.25098041 > 0.250980392...), which here brings 4t closer to 2: 129.00002 -> 129; b = 1.5 - 1/255 -> 1 -> 255,
         r = 0.
    128: 4t = 512/255: r = 1.5 - 253/255 = 129.5/255 -> 130, g -> 1 -> 255; b = 1.5 - 257/255 = 125.5/255, exactly on
         126.0 in real numbers, but fp32's t = 128/255 is rounded up (0.50196081 > 0.501960784...), so 4t - 1 is a little
         larger, c * 255 + 0.5 = 125.99997 and the byte is 125.
    191: 4t = 764/255: r -> 1 -> 255, b = 1.5 - 509/255 < 0 -> 0; g = 1.5 - 254/255 = 128.5/255, on 129.0 in real
         numbers; fp32's t = 191/255 is rounded up as well (0.74901962 > 0.749019607...), 128.99998 -> 128.
    255: t = 1: r = 1.5 - 1 = 0.5 -> 128, g = 1.5 - 2 < 0 -> 0, b = 0."""
    assert float(np.float32(128) / np.float32(255)) > 128 / 255 and float(np.float32(191) / np.float32(255)) > 191 / 255
    assert ref.jet(0) == (0, 0, 128)
    assert ref.jet(64) == (0, 129, 255)
    assert ref.jet(128) == (130, 255, 125)
    assert ref.jet(191) == (255, 128, 0)
    assert ref.jet(255) == (128, 0, 0)


def test_ref_shrink_four_to_one():
    """fx = 0.5 * 4 - 0.5 = 1.5: taps 1 and 2, both weights 1024: ((10 + 20) * 1024 * 1024 + (30 + 41) * 1024 * 1024 +
    2^21) >> 22 = (101 + 2) >> 2 = 25."""
    plane = np.zeros((4, 4), dtype=np.int64)
    plane[1, 1], plane[1, 2], plane[2, 1], plane[2, 2] = 10, 20, 30, 41
    assert ref.tap(0, 4, 1) == (1, 2, 1024)
    assert ref.shrink(plane, 1, 1).tolist() == [[25]]
    # borders: ratio 1 is the identity, and a 2:1 shrink never leaves the image
    assert ref.tap(0, 8, 8) == (0, 1, 0) and ref.tap(7, 8, 8) == (7, 7, 0)
    assert ref.tap(3, 8, 4) == (6, 7, 1024)


def test_ref_image_bytes():
    img = np.array([-1.0, 0.0, 0.5, 1.0, 3.0], dtype=np.float32).reshape(1, 1, 1, 5)
    assert ref.image_bytes(img, None).reshape(-1).tolist() == [0, 0, 127, 255, 255]
    assert ref.image_bytes(img, (np.float32(-1), np.float32(3))).reshape(-1).tolist() == [0, 63, 95, 127, 254]
    assert ref.image_bytes(np.full((1, 1, 2, 2), 0.7, np.float32), (np.float32(0.7), np.float32(0.7))).max() == 0


def test_ref_heatmap_markers_accumulate():
    """Tile j+1 shows the markers of joints 0..j - joint j's in pure red, the earlier ones blended - and column block 0
    shows all of them."""
    B, K, Hh, Wh = 1, 3, 8, 8
    image = np.zeros((B, 3, 16, 16), dtype=np.float32)          # constant: every image byte is 0
    heat = np.zeros((B, K, Hh, Wh), dtype=np.float32)           # heat byte 0 -> colour (0, 0, 128)
    peaks = np.array([[[1, 1], [4, 4], [6, 2]]], dtype=np.float32)
    grid = ref.heatmap_grid(image, heat, peaks)
    assert grid.shape == (Hh, (K + 1) * Wh, 3) and grid.dtype == np.uint8

    def cross(j):
        cx, cy = int(peaks[0, j, 0]), int(peaks[0, j, 1])
        return [(cx + 1, cy), (cx - 1, cy), (cx, cy + 1), (cx, cy - 1)]

    plain = ((7 * 0 + 3 * 0) // 10, 0, (7 * 128 + 3 * 0) // 10)
    under = ((7 * 0 + 3 * 255) // 10, 0, (7 * 128 + 3 * 0) // 10)        # an earlier joint's red, blended
    for tile in range(K + 1):
        want = np.zeros((Hh, Wh, 3), dtype=np.int64)
        if tile == 0:
            for j in range(K):
                for x, y in cross(j):
                    want[y, x] = ref.RED
        else:
            want[:, :] = plain
            for j in range(tile - 1):
                for x, y in cross(j):
                    want[y, x] = under
            for x, y in cross(tile - 1):
                want[y, x] = ref.RED
        assert np.array_equal(grid[:, tile * Wh:(tile + 1) * Wh], want), tile
    # a peak in the corner: two of the four pixels fall off the tile
    corner = ref.heatmap_grid(image, heat[:, :1], np.zeros((1, 1, 2), np.float32))
    assert (corner[:, :Wh] == ref.RED).all(-1).sum() == 2 and tuple(corner[0, 1]) == ref.RED and tuple(corner[1, 0]) == ref.RED


def test_ref_joint_grid_layout_and_paint_order():
    B, K, H, W = 3, 1, 8, 6
    image = np.zeros((B, 3, H, W), dtype=np.float32)
    image[:, 0] = 1.0                                            # channel 0 at the maximum, the others at the minimum
    at = np.full((B, K, 2), 3.0, dtype=np.float32)
    ones, zeros = np.ones((B, K), np.float32), np.zeros((B, K), np.float32)
    grid = ref.joint_grid(image, at, zeros, at, zeros, nrow=2, padding=1, bgr=True)
    assert grid.shape == (2 * 9 + 1, 2 * 7 + 1, 3)
    byte = int(np.float32(1.0) / (np.float32(1.0) + np.float32(1e-5)) * np.float32(255.0))
    cell = np.zeros((H, W, 3), np.uint8)
    cell[:, :, 2] = byte                                         # bgr: channel 0 is blue
    want = np.zeros_like(grid)
    for k, (top, left) in enumerate([(1, 1), (1, 8), (10, 1)]):
        want[top:top + H, left:left + W] = cell
    assert np.array_equal(grid, want)                            # padding and the unused fourth cell stay 0
    # pred, gt and cond on one pixel: the x lies over the + lies over the disc
    g = ref.joint_grid(image[:1], at[:1], ones[:1], at[:1], ones[:1], at[:1], ones[:1], padding=0)
    assert tuple(g[3, 3]) == ref.GREEN and tuple(g[2, 2]) == ref.GREEN and tuple(g[3, 4]) == ref.BLUE
    assert tuple(g[1, 3]) == ref.BLUE and tuple(g[2, 4]) == ref.GREEN and tuple(g[5, 4]) == ref.RED
    assert tuple(g[6, 3]) == (0, 0, byte)                        # dy = 3: outside the disc
    # a condition joint at x = 0 is not drawn; an invisible joint is not drawn
    at0 = at[:1].copy()
    at0[0, 0, 0] = 0.0
    g = ref.joint_grid(image[:1], at[:1], zeros[:1], at[:1], zeros[:1], at0, ones[:1], padding=0)
    assert np.array_equal(g, cell)


def _debug_cfg(debug, flags=True):
    from buctd_amd.config import cfg
    c = cfg.clone()
    c.defrost()
    c.DEBUG.DEBUG = debug
    for k in ('SAVE_BATCH_IMAGES_GT', 'SAVE_BATCH_IMAGES_PRED', 'SAVE_HEATMAPS_GT', 'SAVE_HEATMAPS_PRED'):
        c.DEBUG[k] = flags
    return c


def test_hook_returns_at_once_without_debug(tmp_path):
    """DEBUG.DEBUG false: nothing is touched (CPU tensors, which every renderer refuses) and nothing is written."""
    from buctd_amd.core.function import _save_debug_images
    from buctd_amd.utils.vis import save_debug_images
    x, hm = torch.rand(2, 3, 8, 8), torch.rand(2, 4, 4, 4)
    meta = {'joints': torch.zeros(2, 4, 3), 'joints_vis': torch.ones(2, 4, 3)}
    keep = (x.clone(), hm.clone())
    prefix = str(tmp_path / 'train_0')
    assert save_debug_images(_debug_cfg(False), x, meta, hm, np.zeros((2, 4, 2)), hm, prefix) is None
    assert _save_debug_images(_debug_cfg(False), x, meta, hm, np.zeros((2, 4, 2)), hm, prefix, output_dir=str(tmp_path)) is None
    assert os.listdir(tmp_path) == []
    assert torch.equal(x, keep[0]) and torch.equal(hm, keep[1])


def test_renderers_refuse_cpu_tensors():
    from buctd_amd import _C
    from buctd_amd.utils import vis
    with pytest.raises(_C.BuctdHipError):
        vis.render_batch_heatmaps(torch.rand(1, 3, 8, 8), torch.rand(1, 2, 4, 4))
