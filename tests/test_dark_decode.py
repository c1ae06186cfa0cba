"""get_final_preds(use_dark=True) on numpy heat-maps (the DARK decoder, reference lib/core/inference.py:90-151) against a
loop-by-loop restatement of the reference and against hand-derived cases.  No GPU."""
import numpy as np
import pytest

from oracle import core as oc

from buctd_amd.core.inference import _dark_taps, get_final_preds


class Cfg:
    class TEST:
        POST_PROCESS = True       # ignored by the DARK decoder


def _ref_taylor(hm, coord):
    """reference taylor (90-110); the derivatives in float64, the inverse by np.linalg.inv."""
    hh, hw = hm.shape
    px, py = int(coord[0]), int(coord[1])
    if 1 < px < hw - 2 and 1 < py < hh - 2:
        h = hm.astype(np.float64)
        dx = 0.5 * (h[py][px + 1] - h[py][px - 1])
        dy = 0.5 * (h[py + 1][px] - h[py - 1][px])
        dxx = 0.25 * (h[py][px + 2] - 2 * h[py][px] + h[py][px - 2])
        dxy = 0.25 * (h[py + 1][px + 1] - h[py - 1][px + 1] - h[py + 1][px - 1] + h[py - 1][px - 1])
        dyy = 0.25 * (h[py + 2][px] - 2 * h[py][px] + h[py - 2][px])
        if dxx * dyy - dxy ** 2 != 0:
            hess = np.array([[dxx, dxy], [dxy, dyy]])
            coord += -np.linalg.inv(hess) @ np.array([dx, dy])
    return coord


def _ref_dark(hm, center, scale):
    """reference get_final_preds_dark (131-151) with gaussian_blur (113-127) loop by loop; cv2.GaussianBlur is the
    oracle's float64 restatement on the zero-padded map.  Returns (preds, maxvals, log heat-maps)."""
    hm = hm.copy()
    coords, maxvals = oc.get_max_preds(hm)
    n, k, hh, hw = hm.shape
    for i in range(n):
        for j in range(k):
            origin_max = np.max(hm[i, j])
            dr = np.zeros((hh + 10, hw + 10))
            dr[5:-5, 5:-5] = hm[i, j].copy()
            dr = oc.gaussian_blur_reflect101(dr, 11)
            hm[i, j] = dr[5:-5, 5:-5].copy()
            with np.errstate(divide='ignore', invalid='ignore'):
                hm[i, j] *= origin_max / np.max(hm[i, j])
    hm = np.maximum(hm, 1e-10)
    hm = np.log(hm)
    for i in range(n):
        for j in range(k):
            coords[i, j] = _ref_taylor(hm[i][j], coords[i][j])
    preds = coords.copy()
    for i in range(n):
        preds[i] = oc.transform_preds(coords[i], center[i], scale[i], [hw, hh])
    return preds, maxvals, hm


def _hessian(loghm, coords):
    """[M] condition numbers of the restatement's Hessians at the peaks (inf where no step applies)."""
    n, k, hh, hw = loghm.shape
    out = np.full((n, k), np.inf)
    for i in range(n):
        for j in range(k):
            px, py = int(coords[i, j, 0]), int(coords[i, j, 1])
            if 1 < px < hw - 2 and 1 < py < hh - 2:
                h = loghm[i, j].astype(np.float64)
                dxx = 0.25 * (h[py][px + 2] - 2 * h[py][px] + h[py][px - 2])
                dxy = 0.25 * (h[py + 1][px + 1] - h[py - 1][px + 1] - h[py + 1][px - 1] + h[py - 1][px - 1])
                dyy = 0.25 * (h[py + 2][px] - 2 * h[py][px] + h[py - 2][px])
                out[i, j] = np.linalg.cond(np.array([[dxx, dxy], [dxy, dyy]]))
    return out


def _blob_maps(rng, n, k, hh, hw, noise=0.02):
    """Heat-maps like a network's: an anisotropic Gaussian per joint at a random sub-pixel centre, plus noise."""
    yy, xx = np.mgrid[0:hh, 0:hw].astype(np.float64)
    cx = rng.uniform(-2, hw + 1, (n, k, 1, 1))
    cy = rng.uniform(-2, hh + 1, (n, k, 1, 1))
    sx = rng.uniform(1.5, 3.0, (n, k, 1, 1))
    sy = rng.uniform(1.5, 3.0, (n, k, 1, 1))
    amp = rng.uniform(-0.1, 1.0, (n, k, 1, 1))
    hm = amp * np.exp(-((xx - cx) ** 2 / (2 * sx ** 2) + (yy - cy) ** 2 / (2 * sy ** 2)))
    return (hm + noise * rng.standard_normal((n, k, hh, hw))).astype(np.float32)


def _boxes(rng, n):
    return rng.uniform(50, 300, (n, 2)), rng.uniform(0.5, 2.0, (n, 2))


def _decode(hm, use_dark=True, cfg=Cfg):
    """get_final_preds with the identity box: image coordinates = heat-map coordinates."""
    n, hh, hw = hm.shape[0], hm.shape[2], hm.shape[3]
    c, s = np.tile([[hw / 2.0, hh / 2.0]], (n, 1)), np.tile([[hw / 200.0, hh / 200.0]], (n, 1))
    return get_final_preds(cfg, hm, c, s, use_dark=use_dark)


def _ref_decode(hm):
    n, hh, hw = hm.shape[0], hm.shape[2], hm.shape[3]
    return _ref_dark(hm, np.tile([[hw / 2.0, hh / 2.0]], (n, 1)), np.tile([[hw / 200.0, hh / 200.0]], (n, 1)))


def test_taps_are_the_oracle_kernel():
    assert np.array_equal(_dark_taps(), oc.gaussian_kernel_1d(11))


@pytest.mark.parametrize("k", [14, 17])
@pytest.mark.parametrize("hh,hw", [(96, 72), (64, 48), (13, 11)])
def test_numpy_path_matches_the_reference_restatement(k, hh, hw):
    rng = np.random.default_rng(100 * k + hh)
    n = 3
    hm = _blob_maps(rng, n, k, hh, hw)
    hm[0, 0] = 0.0                                       # all-zero map: masked, finite
    center, scale = _boxes(rng, n)
    keep = hm.copy()
    preds, maxvals = get_final_preds(Cfg, hm, center, scale, use_dark=True)
    assert np.array_equal(hm, keep), "the caller's heat-maps were modified"
    rpreds, rmax, loghm = _ref_dark(hm, center, scale)
    assert preds.dtype == np.float32 and preds.shape == (n, k, 2)
    assert np.array_equal(maxvals, rmax)
    assert np.isfinite(preds).all()
    # image px per heat-map px = scale * 200 / (hw, hh); compare in heat-map pixels
    px_per = (scale[:, 0] * 200 / hw)[:, None]          # transform_preds scales both axes by scale[0]
    diff = np.abs(preds - rpreds).max(axis=2) / px_per
    coords, _ = oc.get_max_preds(hm)
    cond = _hessian(loghm, coords)
    stepped = np.isfinite(cond)
    # the log is rounded from float64 here and taken in float32 by np.log there (<= 1 ulp): well-conditioned steps agree
    # to 1e-4 px, unstepped coordinates are the arg-max in both
    assert (diff[~stepped] <= 1e-4).all()
    good = stepped & (cond <= 1e3)
    assert (diff[good] <= 1e-4).all(), diff[good].max()
    if hh > 13:
        assert stepped.sum() >= n * k // 3                # the comparison is not empty


def test_interior_impulse_blurs_to_the_outer_product_of_the_taps():
    hm = np.zeros((1, 1, 31, 27), dtype=np.float32)
    hm[0, 0, 15, 13] = 1.0
    from buctd_amd.core.inference import _dark_blur_host
    b = _dark_blur_host(hm)[0, 0]
    t = _dark_taps()
    want = np.zeros((31, 27))
    want[10:21, 8:19] = np.outer(t, t)
    assert np.array_equal(b, want.astype(np.float32))
    preds, maxvals = _decode(hm)
    assert preds[0, 0].tolist() == [13.0, 15.0] and maxvals[0, 0, 0] == 1.0


@pytest.mark.parametrize("sx,sy", [(2.0, 2.0), (2.0, 3.0), (3.0, 2.5)])
def test_gaussian_blob_centre_is_recovered(sx, sy):
    rng = np.random.default_rng(7)
    hh, hw = 64, 48
    cx = 20 + rng.uniform(0, 1, 16)
    cy = 30 + rng.uniform(0, 1, 16)
    yy, xx = np.mgrid[0:hh, 0:hw].astype(np.float64)
    hm = np.exp(-((xx - cx[:, None, None]) ** 2 / (2 * sx ** 2) + (yy - cy[:, None, None]) ** 2 / (2 * sy ** 2)))
    hm = hm.astype(np.float32)[None]                     # [1, 16, H, W]
    preds, _ = _decode(hm)
    err = np.abs(preds[0] - np.stack([cx, cy], 1)).max()
    assert err <= 0.05, err
    class Plain:
        class TEST:
            POST_PROCESS = False

    plain, _ = _decode(hm, use_dark=False, cfg=Plain)
    miss = np.abs(plain[0] - np.stack([cx, cy], 1))
    assert miss.max() <= 0.5 + 1e-6 and miss.max() >= 0.3     # the arg-max alone is off by up to half a pixel


@pytest.mark.parametrize("x,y", [(1, 10), (2, 1), (9, 10), (8, 12), (0, 0)])
def test_peak_in_the_excluded_border_band_gets_no_offset(x, y):
    hh, hw = 13, 11                                       # eligible: 1 < px < 9, 1 < py < 11
    yy, xx = np.mgrid[0:hh, 0:hw].astype(np.float64)
    hm = np.exp(-((xx - x - 0.3) ** 2 + (yy - y - 0.2) ** 2) / 8.0).astype(np.float32)
    hm[y, x] = 2.0
    preds, _ = _decode(hm[None, None])
    assert preds[0, 0].tolist() == [float(x), float(y)]
    # one step inside the band the same map does get an offset
    if (x, y) == (8, 12):
        hm2 = np.roll(hm, (-4, -1), axis=(0, 1))
        p2, _ = _decode(hm2[None, None])
        assert p2[0, 0].tolist() != [7.0, 8.0]


def test_ties_take_the_first_index():
    hm = np.zeros((1, 1, 20, 20), dtype=np.float32)
    hm[0, 0, 8, 12] = 1.0
    hm[0, 0, 9, 5] = 1.0
    hm[0, 0, 12, 3] = 1.0
    preds, maxvals = _decode(hm)
    rpreds, _, _ = _ref_decode(hm)
    assert maxvals[0, 0, 0] == 1.0
    assert np.abs(preds - rpreds).max() <= 1e-4
    # the step starts at (12, 8), the first of the three in raster order
    assert abs(preds[0, 0, 0] - 12) < 1 and abs(preds[0, 0, 1] - 8) < 1


@pytest.mark.parametrize("peak", [0.0, -0.5])
def test_masked_peak_decodes_to_zero(peak):
    hm = np.full((1, 2, 16, 16), -1.0, dtype=np.float32)
    hm[0, 0, 7, 9] = peak
    hm[0, 1] = 0.0
    preds, maxvals = _decode(hm)
    assert np.array_equal(preds, np.zeros((1, 2, 2), np.float32))
    assert maxvals[0, 0, 0] == peak and maxvals[0, 1, 0] == 0.0


def test_tiny_positive_peak_clamps_to_a_constant_log_and_gets_no_offset():
    """A peak above 0 but below 1e-10: after the renormalisation every sample is clamped to 1e-10, the log neighbourhood is
    constant, det = 0 exactly, no step."""
    hm = np.full((1, 1, 16, 16), -1.0, dtype=np.float32)
    hm[0, 0, 7, 6] = 1e-12
    preds, maxvals = _decode(hm)
    assert preds[0, 0].tolist() == [6.0, 7.0] and maxvals[0, 0, 0] == np.float32(1e-12)
    rpreds, _, _ = _ref_decode(hm)
    assert np.array_equal(preds, rpreds)


def test_negative_blurred_max_follows_the_restatement():
    """Non-finite-prone case: a positive peak in a negative field whose blurred max is negative, so the renormalisation
    flips the sign of the map.  Tested: the result stays finite and equals the restatement."""
    rng = np.random.default_rng(3)
    hm = (-1.0 + 0.05 * rng.standard_normal((1, 1, 24, 20))).astype(np.float32)
    hm[0, 0, 11, 9] = 0.01
    preds, _ = _decode(hm)
    rpreds, _, _ = _ref_decode(hm)
    assert np.isfinite(preds).all()
    assert np.abs(preds - rpreds).max() <= 1e-3


def test_post_process_is_ignored_with_dark():
    rng = np.random.default_rng(11)
    hm = _blob_maps(rng, 2, 14, 64, 48)
    c, s = _boxes(rng, 2)

    class Off:
        class TEST:
            POST_PROCESS = False

    a = get_final_preds(Cfg, hm, c, s, use_dark=True)
    b = get_final_preds(Off, hm, c, s, use_dark=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
