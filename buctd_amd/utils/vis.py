"""Debug pictures (reference lib/utils/vis.py): the heat-map grid and the joint grid of a batch, rendered on the device
by csrc/vis.hip from the tensors of the step and written as PNG files.

  render_batch_heatmaps / render_batch_image_with_joints   the uint8 RGB picture as a device tensor, enqueued on the
                                                            current stream (no host trip: min / max stay on the device)
  save_batch_heatmaps / save_batch_image_with_joints       the reference's signatures: render, one uint8 copy, write
  save_debug_images                                         the reference's DEBUG.* flag logic (utils/vis.py:416-460)
  write_png                                                 8-bit RGB PNG from zlib and struct alone

The pixel definitions are in include/buctd_hip.h; what differs from the reference's cv2 / torchvision pictures is listed
in DESIGN.md.  Only the first three channels of the batch image are drawn (a stacked condition adds channels behind them).
"""
import logging
import os
import struct
import zlib

import numpy as np
import torch

from .. import _C, ops
from .._C import check, lib, ptr, stream_ptr

logger = logging.getLogger(__name__)


def _image(batch_image):
    if not (torch.is_tensor(batch_image) and batch_image.dim() == 4 and batch_image.size(1) >= 3
            and batch_image.dtype == torch.float32):
        raise _C.BuctdHipError("vis: the batch image must be a fp32 [B, 3+, H, W] tensor")
    ptr(batch_image)    # refuses host tensors
    return batch_image.detach()


def _minmax(img):
    lohi = torch.empty(2, dtype=torch.float32, device=img.device)
    B, _, H, W = img.shape
    check(lib().buctd_vis_minmax(ptr(img), B, H, W, *img.stride(), ptr(lohi), stream_ptr()), "vis_minmax")
    return lohi


def _upload(a, device, shape):
    """A host or device array as a contiguous fp32 device tensor of the given shape."""
    t = torch.as_tensor(a).detach().to(device=device, dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise _C.BuctdHipError(f"vis: expected an array of shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _xy(a, device, B, K):
    """Joint positions [B, K, 2+] -> (x, y) fp32 on the device."""
    t = torch.as_tensor(a)
    if t.dim() != 3 or t.size(-1) < 2:
        raise _C.BuctdHipError(f"vis: joints must be [B, K, 2+], got {tuple(t.shape)}")
    return _upload(t[..., :2], device, (B, K, 2))


def _vis_first(a, device, B, K):
    """joint_vis[0] of the reference: the first entry of a [B, K, n] visibility (a [B, K] one as it is)."""
    t = torch.as_tensor(a)
    return _upload(t[..., 0] if t.dim() == 3 else t, device, (B, K))


def _vis_sum(a, device, B, K):
    """sum(cond_joint_vis) of the reference."""
    t = torch.as_tensor(a)
    return _upload(t.to(torch.float32).sum(-1) if t.dim() == 3 else t, device, (B, K))


def render_batch_heatmaps(batch_image, batch_heatmaps, normalize=True, bgr=True):
    """The picture of save_batch_heatmaps: uint8 [B*Hh, (K+1)*Wh, 3] RGB on the device.  bgr: the image's channels are
    B, G, R (DATASET.COLOR_RGB false)."""
    img = _image(batch_image)
    if not (torch.is_tensor(batch_heatmaps) and batch_heatmaps.dim() == 4 and batch_heatmaps.dtype == torch.float32
            and batch_heatmaps.size(0) == img.size(0)):
        raise _C.BuctdHipError("vis: the heat-maps must be a fp32 [B, K, Hh, Wh] tensor with the image's batch size")
    hm = batch_heatmaps.detach().contiguous()
    B, _, H, W = img.shape
    _, K, Hh, Wh = hm.shape
    peaks = ops.argmax_decode(hm)[0]
    lohi = _minmax(img) if normalize else None
    out = torch.empty((B * Hh, (K + 1) * Wh, 3), dtype=torch.uint8, device=img.device)
    check(lib().buctd_vis_heatmap_grid(ptr(img), B, H, W, *img.stride(), ptr(lohi), ptr(hm), K, Hh, Wh, ptr(peaks),
                                       1 if bgr else 0, ptr(out), stream_ptr()), "vis_heatmap_grid")
    return out


def render_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, meta, nrow=8, padding=2, bgr=True):
    """The picture of save_batch_image_with_joints: the normalised make_grid of the batch with the predicted joints
    (batch_joints where batch_joints_vis), meta['joints'] / meta['joints_vis'] and, if present, meta['cond_joints'] /
    meta['cond_joints_vis'] marked.  uint8 [Hg, Wg, 3] RGB on the device; host arrays are uploaded."""
    img = _image(batch_image)
    B, _, H, W = img.shape
    K = torch.as_tensor(batch_joints).shape[1]
    dev = img.device
    pred, pred_vis = _xy(batch_joints, dev, B, K), _vis_first(batch_joints_vis, dev, B, K)
    gt, gt_vis = _xy(meta['joints'], dev, B, K), _vis_first(meta['joints_vis'], dev, B, K)
    cond = cond_vis = None
    if 'cond_joints' in meta:
        cond, cond_vis = _xy(meta['cond_joints'], dev, B, K), _vis_sum(meta['cond_joints_vis'], dev, B, K)
    lohi = _minmax(img)
    xmaps = min(nrow, B)
    ymaps = -(-B // xmaps)
    out = torch.empty((ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3), dtype=torch.uint8, device=dev)
    check(lib().buctd_vis_joint_grid(ptr(img), B, H, W, *img.stride(), ptr(lohi), K, ptr(pred), ptr(pred_vis), ptr(gt),
                                     ptr(gt_vis), ptr(cond), ptr(cond_vis), nrow, padding, 1 if bgr else 0, ptr(out),
                                     stream_ptr()), "vis_joint_grid")
    return out


def _chunk(tag, data):
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, array):
    """array uint8 [H, W, 3] -> an 8-bit RGB PNG: filter type 0 on every row, one IDAT chunk."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: expected a uint8 [H, W, 3] array")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * 3), dtype=np.uint8)      # column 0: the filter byte
    rows[:, 1:] = a.reshape(h, w * 3)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
                _chunk(b'IDAT', zlib.compress(rows.tobytes(), 1)) + _chunk(b'IEND', b''))


def save_batch_heatmaps(batch_image, batch_heatmaps, file_name, normalize=True, bgr=True):
    """reference utils/vis.py:269-332 (bgr is not in the reference: its cv2.imwrite takes B, G, R as they come)."""
    write_png(file_name, render_batch_heatmaps(batch_image, batch_heatmaps, normalize, bgr).cpu().numpy())


def render_batch_attention_maps(batch_image, maps_of_one_layer, bgr=True):
    """Dependency areas of one encoder layer (TransPoseH.attention_maps(...)[1][layer], [B, K, h_tok, w_tok]) as the
    heat-map grid of render_batch_heatmaps: every row of the attention matrix is divided by its own maximum on the device
    (an all-zero row - an undetected joint - stays zero), so each tile uses the whole colour range."""
    img = _image(batch_image)
    m = maps_of_one_layer
    if not (torch.is_tensor(m) and m.dim() == 4 and m.dtype == torch.float32 and m.size(0) == img.size(0)):
        raise _C.BuctdHipError("vis: the attention maps of a layer must be a fp32 [B, K, h_tok, w_tok] tensor with the "
                               "image's batch size")
    ptr(m)              # refuses host tensors
    m = m.detach()
    top = m.amax(dim=(2, 3), keepdim=True)
    m = m / torch.where(top > 0, top, torch.ones_like(top))
    return render_batch_heatmaps(img, m, True, bgr)


def save_batch_attention_maps(batch_image, maps_of_one_layer, file_name, bgr=True):
    write_png(file_name, render_batch_attention_maps(batch_image, maps_of_one_layer, bgr).cpu().numpy())


def save_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, meta, file_name, nrow=8, padding=2,
                                 bgr=True):
    """reference utils/vis.py:75-141."""
    write_png(file_name, render_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, meta, nrow, padding,
                                                        bgr).cpu().numpy())


def save_debug_images(config, input, meta, target, joints_pred, output, prefix, suffix='', output_dir=''):
    """reference utils/vis.py:416-460.  The files are PNG; save_all_image_with_joints (one file per sample, drawn on the
    re-read original image) is not built."""
    if not config.DEBUG.DEBUG:
        return
    bgr = not config.DATASET.COLOR_RGB
    if config.DEBUG.SAVE_BATCH_IMAGES_PRED:
        logger.debug('per-sample pictures (save_all_image_with_joints) are not built (%s)', prefix)
        os.makedirs('{}_pred'.format(prefix), exist_ok=True)
        vis = meta['pred_joints_vis'] if 'pred_joints_vis' in meta else meta['joints_vis']
        save_batch_image_with_joints(input, joints_pred, vis, meta, '{}_pred/batch.png'.format(prefix), bgr=bgr)
    if config.DEBUG.SAVE_HEATMAPS_GT:
        save_batch_heatmaps(input, target, '{}_hm_gt_{}.png'.format(prefix, suffix), bgr=bgr)
    if config.DEBUG.SAVE_HEATMAPS_PRED:
        save_batch_heatmaps(input, output, '{}_hm_pred_{}.png'.format(prefix, suffix), bgr=bgr)
