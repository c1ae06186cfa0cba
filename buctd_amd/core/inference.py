"""Heat-map decoding - drop-in for reference lib/core/inference.py:19-151.

get_max_preds keeps the reference's numpy-in / numpy-out contract for callers that already hold host
arrays; device tensors are decoded by the arg-max kernel (first-index tie break, preds zeroed where
maxval <= 0, quarter-pixel refinement included) so that validate() moves K*(2+1+2) floats per person over
PCIe instead of the whole heat-map.  use_dark=True selects the DARK decoder (DarkPose: Taylor step on the
log of the Gaussian-blurred map, reference 90-151): on the device by the DARK kernel, on numpy arrays by a
vectorised restatement (_dark_offsets_host); the device path moves the same K*5 floats per person.
"""
import numpy as np
import torch

from .. import ops
from ..utils.transforms import transform_preds


def _decode_host(heatmaps):
    """numpy [N,K,H,W] -> (coords [N,K,2] float32 zeroed where the peak is <= 0, peak values [N,K,1])."""
    n, k, _, w = heatmaps.shape
    flat = heatmaps.reshape(n, k, -1)
    where = flat.argmax(axis=2)                        # first index on ties, like np.argmax in the reference
    peak = np.take_along_axis(flat, where[..., None], axis=2)
    coords = np.stack([where % w, where // w], axis=2).astype(np.float32)
    coords *= (peak > 0.0).astype(np.float32)
    return coords, peak


def get_max_preds(batch_heatmaps):
    if isinstance(batch_heatmaps, torch.Tensor):
        assert batch_heatmaps.dim() == 4, 'batch_images should be 4-ndim'
        preds, maxvals, _ = ops.argmax_decode(batch_heatmaps.contiguous())
        return preds.cpu().numpy(), maxvals.cpu().numpy()
    assert isinstance(batch_heatmaps, np.ndarray), 'batch_heatmaps should be numpy.ndarray or a device tensor'
    assert batch_heatmaps.ndim == 4, 'batch_images should be 4-ndim'
    return _decode_host(batch_heatmaps)


def _quarter_offsets_host(heatmaps, coords):
    """POST_PROCESS (reference 68-77): +-0.25 px towards the higher neighbour for peaks strictly inside the map."""
    n, k, hh, hw = heatmaps.shape
    px = np.floor(coords[..., 0] + 0.5).astype(np.int64)
    py = np.floor(coords[..., 1] + 0.5).astype(np.int64)
    inside = (px > 1) & (px < hw - 1) & (py > 1) & (py < hh - 1)
    cx, cy = np.clip(px, 1, hw - 2), np.clip(py, 1, hh - 2)
    bi, ji = np.meshgrid(np.arange(n), np.arange(k), indexing='ij')
    dx = heatmaps[bi, ji, cy, cx + 1] - heatmaps[bi, ji, cy, cx - 1]
    dy = heatmaps[bi, ji, cy + 1, cx] - heatmaps[bi, ji, cy - 1, cx]
    return np.stack([np.sign(dx), np.sign(dy)], axis=2) * 0.25 * inside[..., None]


DARK_KSIZE = 11   # reference get_final_preds_dark: gaussian_blur(hm, 11)


def _dark_taps(ksize=DARK_KSIZE):
    """cv2.getGaussianKernel(ksize, 0) in float64: sigma 0.3*((ksize-1)*0.5-1)+0.8 (2.0 for 11 taps)."""
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    k = np.exp(-(x * x) / (2 * sigma * sigma))
    return k / k.sum()


def _dark_blur_host(maps):
    """reference gaussian_blur (106-127) on maps [..., H, W], into a new float32 array: the map zero-padded by 5 px,
    cv2.GaussianBlur(11x11, sigma 0) in float64 (the 5-px zero border keeps cv2's reflect-101 border away from every kept
    pixel, so this is a zero-padded separable convolution), cropped back and stored to float32.  Rows first, tap 0
    first: the order the DARK kernel adds in, so both round to the same float32 values."""
    k = _dark_taps()
    r = DARK_KSIZE // 2
    out = maps.astype(np.float64)
    for axis in (out.ndim - 2, out.ndim - 1):
        pad = [(0, 0)] * out.ndim
        pad[axis] = (r, r)
        p = np.pad(out, pad)
        acc = np.zeros_like(out)
        for t in range(DARK_KSIZE):
            sl = [slice(None)] * out.ndim
            sl[axis] = slice(t, t + out.shape[axis])
            acc += k[t] * p[tuple(sl)]
        out = acc
    return out.astype(np.float32)


def _dark_offsets_host(heatmaps, coords):
    """DARK Taylor offsets [N,K,2] float64 in heat-map pixels (reference taylor 90-110 after gaussian_blur, the float32
    renormalisation to the original peak and log(max(., 1e-10))); (0, 0) where the reference leaves a coordinate as is:
    peaks outside 1 < px < W-2, 1 < py < H-2 (a masked peak sits at (0, 0)) and a zero Hessian determinant.
    The log is evaluated in float64 and rounded to float32, the derivatives and the 2x2 solve in float64 - the DARK
    kernel's arithmetic.  heatmaps is only read."""
    n, k, hh, hw = heatmaps.shape
    off = np.zeros((n, k, 2), dtype=np.float64)
    px = coords[..., 0].astype(np.int64)
    py = coords[..., 1].astype(np.int64)
    go = (px > 1) & (px < hw - 2) & (py > 1) & (py < hh - 2)
    if not go.any():
        return off
    maps = heatmaps[go]                                      # [M, H, W] copy: only the maps that get a step
    px, py = px[go], py[go]
    blurred = _dark_blur_host(maps)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        ratio = maps.max(axis=(1, 2)) / blurred.max(axis=(1, 2))        # float32, as hm *= origin_max / np.max(hm)
    m = np.arange(maps.shape[0])

    def lg(dy, dx):
        with np.errstate(invalid='ignore', over='ignore'):
            v = np.maximum(blurred[m, py + dy, px + dx] * ratio, np.float32(1e-10))
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.log(v.astype(np.float64)).astype(np.float32).astype(np.float64)

    c = lg(0, 0)
    with np.errstate(invalid='ignore', over='ignore'):
        dx = 0.5 * (lg(0, 1) - lg(0, -1))
        dy = 0.5 * (lg(1, 0) - lg(-1, 0))
        dxx = 0.25 * (lg(0, 2) - 2.0 * c + lg(0, -2))
        dxy = 0.25 * (lg(1, 1) - lg(-1, 1) - lg(1, -1) + lg(-1, -1))
        dyy = 0.25 * (lg(2, 0) - 2.0 * c + lg(-2, 0))
        det = dxx * dyy - dxy * dxy
    step = det != 0.0
    safe = np.where(step, det, 1.0)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        ox = np.where(step, -((dyy * dx - dxy * dy) / safe), 0.0)   # -H^-1 [dx, dy]
        oy = np.where(step, -((dxx * dy - dxy * dx) / safe), 0.0)
    off[go] = np.stack([ox, oy], axis=1)
    return off


class DeferredFinalPreds:
    """get_final_preds in two halves for a device tensor: the decode kernel and the copies of its K * 5 floats per person
    into pinned host memory are enqueued here; final_preds(center, scale) waits for them and does the host arithmetic
    (reference inference.py:51-87).  validate() enqueues the next batch's forward between the two halves.
    use_dark: the DARK kernel instead (ops.dark_decode); its offsets travel the way the quarter-pixel ones do, and
    TEST.POST_PROCESS does not apply (the reference returns before it)."""

    def __init__(self, config, batch_heatmaps, use_dark=False):
        self.hh, self.hw = batch_heatmaps.shape[2], batch_heatmaps.shape[3]
        if use_dark:
            self.refine = True
            res = ops.dark_decode(batch_heatmaps.contiguous())
        else:
            self.refine = bool(config.TEST.POST_PROCESS)
            res = ops.argmax_decode(batch_heatmaps.contiguous(), refine=self.refine)
        self.host = []
        for t in (res[0], res[1]) + ((res[3],) if self.refine else ()):
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            self.host.append(h)
        self.event = torch.cuda.Event()
        self.event.record()

    def final_preds(self, center, scale):
        self.event.synchronize()
        coords, maxvals = self.host[0].numpy(), self.host[1].numpy()
        if self.refine:
            coords = coords + self.host[2].numpy()
        preds = np.stack([transform_preds(coords[b], center[b], scale[b], [self.hw, self.hh]) for b in range(coords.shape[0])])
        return preds.astype(coords.dtype), maxvals.copy()


def get_final_preds(config, batch_heatmaps, center, scale, use_dark=False):
    """reference get_final_preds (50-87) and, with use_dark=True, get_final_preds_dark (131-151): coordinates and
    maxvals from the arg-max of the unblurred maps, plus the DARK Taylor offset; TEST.POST_PROCESS is then ignored.
    A device tensor is decoded by the DARK kernel, a numpy array by _dark_offsets_host.  Unlike the reference, which
    blurs its numpy argument in place, the caller's heat-maps are never modified (no BUCTD caller could observe that:
    the reference passes output.clone().cpu().numpy())."""
    hh, hw = batch_heatmaps.shape[2], batch_heatmaps.shape[3]
    refine = bool(config.TEST.POST_PROCESS)
    if isinstance(batch_heatmaps, torch.Tensor):
        return DeferredFinalPreds(config, batch_heatmaps, use_dark=use_dark).final_preds(center, scale)
    else:
        coords, maxvals = get_max_preds(batch_heatmaps)
        if use_dark:
            # reference taylor: coord += offset on the float32 coordinates
            coords = (coords.astype(np.float64) + _dark_offsets_host(batch_heatmaps, coords)).astype(coords.dtype)
        elif refine:
            coords = coords + _quarter_offsets_host(batch_heatmaps, coords).astype(coords.dtype)
    preds = np.stack([transform_preds(coords[b], center[b], scale[b], [hw, hh]) for b in range(coords.shape[0])])
    return preds.astype(coords.dtype), maxvals
