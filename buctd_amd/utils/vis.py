"""Debug pictures (reference lib/utils/vis.py): the heat-map grid and the joint grid of a batch, rendered on the device
by csrc/vis.hip from the tensors of the step and written as PNG files.

  render_batch_heatmaps / render_batch_image_with_joints   the uint8 RGB picture as a device tensor, enqueued on the
                                                            current stream (no host trip: min / max stay on the device)
  save_batch_heatmaps / save_batch_image_with_joints       the reference's signatures: render, one uint8 copy, write
  save_debug_images                                         the reference's DEBUG.* flag logic (utils/vis.py:416-460)
  write_png                                                 8-bit RGB PNG from zlib and struct alone

Pose overlays (reference tools/vis.py:plot_keypoints, lib/utils/vis.py:vis_keypoints), drawn in place on uint8 [H, W, 3]
device images by csrc/vis_pose.hip, every person of every image in one launch:

  draw_poses                                                skeletons onto one image or a list of images
  render_pose_panels                                        conditions | predictions of tools/inference.py, side by side
  save_pretty_batch_image_with_joints / save_pretty_debug_images   the reference's signatures and flag logic, PNG files
  SKELETONS, rainbow_palette, hsv_wheel                     limb tables and colours

The pixel definitions are in include/buctd_hip.h; what differs from the reference's cv2 / torchvision pictures is listed
in DESIGN.md.  Only the first three channels of the batch image are drawn (a stacked condition adds channels behind them).
"""
import collections
import ctypes
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


# ---------------------------------------------------------------------------------------------------- pose overlays
COCO_KEYPOINTS = ('nose', 'left_eye', 'right_eye', 'left_ear', 'right_ear', 'left_shoulder', 'right_shoulder',
                  'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist', 'left_hip', 'right_hip', 'left_knee',
                  'right_knee', 'left_ankle', 'right_ankle')
CROWDPOSE_KEYPOINTS = ('left_shoulder', 'right_shoulder', 'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist',
                       'left_hip', 'right_hip', 'left_knee', 'right_knee', 'left_ankle', 'right_ankle', 'head', 'neck')

# num_joints: K of the poses it fits.  limbs: rows (a0, a1, b0, b1, colour) of buctd_vis_pose_args.skeleton - end A is the
# floor midpoint of the joints a0 and a1, end B of b0 and b1, colour a palette row or -1 for the person's colour.
# palette: uint8 [n, 3] RGB or None.
Skeleton = collections.namedtuple('Skeleton', ['num_joints', 'limbs', 'palette'])


def rainbow_palette(n):
    """uint8 [n, 3]: matplotlib's `rainbow` at linspace(0, 1, n), each channel * 255 rounded to nearest - the colours
    vis_keypoints hands to cv2.  In closed form: the map is a 256-entry table of r = |2t - 0.5|, g = sin(pi t),
    b = cos(pi t / 2) at t = i / 255, clipped to [0, 1], read at i = min(int(256 x), 255)."""
    t = np.linspace(0, 1, 256)
    table = np.clip(np.stack([np.abs(2 * t - 0.5), np.sin(t * np.pi), np.cos(t * np.pi / 2)], axis=-1), 0, 1)
    at = np.minimum((np.linspace(0, 1, n) * 256).astype(np.int64), 255)
    return np.rint(table[at] * 255.0).astype(np.uint8).reshape(n, 3)


# the break points of matplotlib's `hsv` map: x, then the channel value there (piecewise linear in between)
_HSV_RED = ((0.0, 1.0), (0.158730, 1.0), (0.174603, 0.96875), (0.333333, 0.03125), (0.349206, 0.0), (0.666667, 0.0),
            (0.682540, 0.03125), (0.841270, 0.96875), (0.857143, 1.0), (1.0, 1.0))
_HSV_GREEN = ((0.0, 0.0), (0.158730, 0.9375), (0.174603, 1.0), (0.507937, 1.0), (0.666667, 0.0625), (0.682540, 0.0),
              (1.0, 0.0))
_HSV_BLUE = ((0.0, 0.0), (0.333333, 0.0), (0.349206, 0.0625), (0.507937, 1.0), (0.841270, 1.0), (0.857143, 0.9375),
             (1.0, 0.09375))


def hsv_wheel(n):
    """uint8 [n, 3]: the person colours of tools/inference.py, plt.cm.get_cmap('hsv', n)(i) * 255 rounded to nearest:
    the hsv map sampled at linspace(0, 1, n) (first and last are both red, as there)."""
    x = np.linspace(0, 1, n) if n > 1 else np.zeros(n)
    chans = [np.interp(x, [p[0] for p in tab], [p[1] for p in tab]) for tab in (_HSV_RED, _HSV_GREEN, _HSV_BLUE)]
    return np.rint(np.stack(chans, axis=-1) * 255.0).astype(np.uint8).reshape(n, 3)


def _limbs(names, pairs, colour=None):
    return tuple((names.index(a), names.index(a), names.index(b), names.index(b), -1 if colour is None else colour + i)
                 for i, (a, b) in enumerate(pairs))


def _coco_pretty():
    """vis_keypoints: mid-shoulder - nose and mid-shoulder - mid-hip first (colours 15 and 16 of the 17 rainbow
    colours), then the 15 limbs of kp_connections in colours 0 .. 14."""
    k = COCO_KEYPOINTS.index
    mid = ((k('right_shoulder'), k('left_shoulder'), k('nose'), k('nose'), 15),
           (k('right_shoulder'), k('left_shoulder'), k('right_hip'), k('left_hip'), 16))
    lines = (('left_eye', 'right_eye'), ('left_eye', 'nose'), ('right_eye', 'nose'), ('right_eye', 'right_ear'),
             ('left_eye', 'left_ear'), ('right_shoulder', 'right_elbow'), ('right_elbow', 'right_wrist'),
             ('left_shoulder', 'left_elbow'), ('left_elbow', 'left_wrist'), ('right_hip', 'right_knee'),
             ('right_knee', 'right_ankle'), ('left_hip', 'left_knee'), ('left_knee', 'left_ankle'),
             ('right_shoulder', 'left_shoulder'), ('right_hip', 'left_hip'))
    return Skeleton(17, mid + _limbs(COCO_KEYPOINTS, lines, colour=0), rainbow_palette(17))


SKELETONS = {
    # plot_keypoints' limb lists (tools/vis.py), in its order; everything in the person's colour
    'coco': Skeleton(17, _limbs(COCO_KEYPOINTS, (
        ('nose', 'left_eye'), ('nose', 'right_eye'), ('left_eye', 'left_ear'), ('right_eye', 'right_ear'),
        ('left_ear', 'left_shoulder'), ('right_ear', 'right_shoulder'), ('left_shoulder', 'right_shoulder'),
        ('left_shoulder', 'left_elbow'), ('left_elbow', 'left_wrist'), ('right_shoulder', 'right_elbow'),
        ('right_elbow', 'right_wrist'), ('left_shoulder', 'left_hip'), ('right_shoulder', 'right_hip'),
        ('left_hip', 'right_hip'), ('left_hip', 'left_knee'), ('left_knee', 'left_ankle'), ('right_hip', 'right_knee'),
        ('right_knee', 'right_ankle'))), None),
    'crowdpose': Skeleton(14, _limbs(CROWDPOSE_KEYPOINTS, (
        ('left_shoulder', 'right_shoulder'), ('left_shoulder', 'left_elbow'), ('right_shoulder', 'right_elbow'),
        ('left_elbow', 'left_wrist'), ('right_elbow', 'right_wrist'), ('left_shoulder', 'left_hip'),
        ('right_shoulder', 'right_hip'), ('left_hip', 'right_hip'), ('left_hip', 'left_knee'), ('right_hip', 'right_knee'),
        ('left_knee', 'left_ankle'), ('right_knee', 'right_ankle'), ('left_shoulder', 'head'), ('right_shoulder', 'head'),
        ('head', 'neck'), ('left_elbow', 'neck'), ('right_elbow', 'neck'))), None),
    'coco_pretty': _coco_pretty(),
}

_STYLES = {'plain': _C.VIS_POSE_PLAIN, 'pretty': _C.VIS_POSE_PRETTY}
_CANVAS_ROW = np.dtype([('base', '<u8'), ('row_stride', '<i8'), ('H', '<i4'), ('W', '<i4')])
assert _CANVAS_ROW.itemsize == ctypes.sizeof(_C.VisCanvas)


def _skeleton_tables(skeleton, K):
    """-> (int32 [L, 5] limbs, uint8 [n, 3] palette).  skeleton: a name of SKELETONS, a Skeleton, or an array of limb
    rows (a, b) or (a0, a1, b0, b1, colour).  Every joint index must be < K: checked here, before anything is uploaded."""
    palette = None
    if isinstance(skeleton, str):
        if skeleton not in SKELETONS:
            raise _C.BuctdHipError(f"draw_poses: unknown skeleton '{skeleton}' (known: {sorted(SKELETONS)})")
        skeleton = SKELETONS[skeleton]
    if isinstance(skeleton, Skeleton):
        skeleton, palette = skeleton.limbs, skeleton.palette
    limbs = np.asarray(skeleton, dtype=np.int64)
    if limbs.ndim == 2 and limbs.shape[1] == 2:
        limbs = np.stack([limbs[:, 0], limbs[:, 0], limbs[:, 1], limbs[:, 1], np.full(len(limbs), -1)], axis=1)
    if limbs.ndim != 2 or limbs.shape[1] != 5 or len(limbs) < 1:
        raise _C.BuctdHipError("draw_poses: a skeleton is [L, 2] joint pairs or [L, 5] rows (a0, a1, b0, b1, colour), L >= 1")
    palette = np.zeros((0, 3), dtype=np.uint8) if palette is None else np.ascontiguousarray(palette, dtype=np.uint8)
    if limbs[:, :4].min() < 0 or limbs[:, :4].max() >= K:
        raise _C.BuctdHipError(f"draw_poses (buctd_vis_pose_overlay): a limb names joint {int(limbs[:, :4].max())} "
                               f"(or a negative one) but the poses have K = {K} joints")
    if limbs[:, 4].min() < -1 or limbs[:, 4].max() >= len(palette):
        raise _C.BuctdHipError(f"draw_poses (buctd_vis_pose_overlay): a limb colour is outside the palette of {len(palette)}")
    return limbs.astype(np.int32), palette


def _per_person(value, n, width, what, default):
    """host int32 [n, width] from None (default), one row, or n rows"""
    if value is None:
        return np.tile(np.asarray(default, dtype=np.int32), (n, 1)).reshape(n, width)
    a = torch.as_tensor(value).detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
    if a.ndim == 1 and a.shape[0] == width:
        a = np.tile(a, (n, 1))
    if a.shape != (n, width):
        raise _C.BuctdHipError(f"draw_poses: {what} of an image with {n} persons must be [{n}, {width}], got {a.shape}")
    return np.rint(a.reshape(n, width)).astype(np.int32)


def draw_poses(images, poses, skeleton='coco', colors=None, style='plain', thickness=2, radius=3, score_thresh=-1.0,
               alpha=1.0, offsets=None, clips=None):
    """Draws the skeletons of poses[i] onto images[i], in place, all in one launch on the current stream; returns images.

    images   a list of uint8 [H, W, 3] device tensors (rows may be strided: views of a wider picture work), or one
    poses    per image [P_i, K, 2 or 3] = x, y (, score), host or device, taken as fp32; a missing score counts as 1.  A
             joint is drawn if x, y and score are finite and score > score_thresh (NaN marks an absent joint)
    skeleton a name of SKELETONS, a Skeleton, or limb rows (see _skeleton_tables)
    colors   per image None (hsv_wheel(P_i), as tools/inference.py has it), one RGB colour or [P_i, 3]
    style    'plain' (plot_keypoints: rings, then limbs, in the person's colour) or 'pretty' (vis_keypoints: per limb
             the segment and its two discs in the limb's colour)
    alpha    blend weight of the drawing, taken as round(alpha * 256) / 256
    offsets  per image None or [P_i, 2] integers added to the person's joints; clips: per image None or [P_i, 4] =
             x0, y0, x1, y1, the canvas rectangle the person may touch (default: the whole image)
    With a single image, poses / colors / offsets / clips are that image's entries themselves."""
    single = torch.is_tensor(images)
    imgs = [images] if single else list(images)
    wrap = (lambda v: [v]) if single else (lambda v: [None] * len(imgs) if v is None else list(v))
    pose_list, colors, offsets, clips = wrap(poses), wrap(colors), wrap(offsets), wrap(clips)
    if not imgs or not all(len(v) == len(imgs) for v in (pose_list, colors, offsets, clips)):
        raise _C.BuctdHipError("draw_poses: poses, colors, offsets and clips need one entry per image")
    if style not in _STYLES:
        raise _C.BuctdHipError(f"draw_poses: style must be one of {sorted(_STYLES)}")
    for im in imgs:
        if not (torch.is_tensor(im) and im.dtype == torch.uint8 and im.dim() == 3 and im.size(2) == 3 and im.size(0) >= 1
                and im.size(1) >= 1):
            raise _C.BuctdHipError("draw_poses: an image must be a uint8 [H, W, 3] tensor")
        ptr(im)         # refuses host tensors
        if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.size(1) or im.device != imgs[0].device:
            raise _C.BuctdHipError("draw_poses: an image needs packed RGB pixels, a row stride >= 3 * W and the device of "
                                   "the other images")
    dev = imgs[0].device
    parts = []
    for p in pose_list:
        t = torch.as_tensor(p)
        if t.dim() != 3 or t.size(-1) not in (2, 3):
            raise _C.BuctdHipError(f"draw_poses: the poses of an image must be [P, K, 2 or 3], got {tuple(t.shape)}")
        t = t.detach().to(device=dev, dtype=torch.float32)
        if t.size(-1) == 2:
            t = torch.cat([t, torch.ones_like(t[..., :1])], dim=-1)
        parts.append(t)
    K = parts[0].size(1)
    if any(t.size(1) != K for t in parts):
        raise _C.BuctdHipError("draw_poses: every image's poses need the same number of joints")
    limbs, palette = _skeleton_tables(skeleton, K)
    counts = [t.size(0) for t in parts]
    P = sum(counts)
    if P == 0:
        return images
    joints = torch.cat(parts).contiguous()

    canvases = np.zeros(len(imgs), dtype=_CANVAS_ROW)
    person_offsets = np.zeros(len(imgs) + 1, dtype=np.int32)
    persons, tiles = [], []
    TW, TH = _C.VIS_POSE_TILE_W, _C.VIS_POSE_TILE_H
    for i, (im, n) in enumerate(zip(imgs, counts)):
        H, W = im.size(0), im.size(1)
        canvases[i] = (im.data_ptr(), im.stride(0), H, W)
        person_offsets[i + 1] = person_offsets[i] + n
        if n == 0:
            continue
        off = _per_person(offsets[i], n, 2, 'offsets', (0, 0))
        clip = _per_person(clips[i], n, 4, 'clips', (0, 0, W, H))
        col = hsv_wheel(n).astype(np.int32) if colors[i] is None else _per_person(colors[i], n, 3, 'colors', None)
        if col.min() < 0 or col.max() > 255:
            raise _C.BuctdHipError("draw_poses: colours are RGB bytes")
        persons.append(np.concatenate([off, clip, (col[:, :1] | (col[:, 1:2] << 8) | (col[:, 2:3] << 16))], axis=1))
        # the tiles a clip rectangle reaches; nobody can be drawn on the others
        need = np.zeros((-(-H // TH), -(-W // TW)), dtype=bool)
        for x0, y0, x1, y1 in np.clip(clip, 0, [W, H, W, H]):
            if x0 < x1 and y0 < y1:
                need[y0 // TH:-(-y1 // TH), x0 // TW:-(-x1 // TW)] = True
        rows, cols = np.nonzero(need)
        tiles.append(np.stack([np.full(len(rows), i), cols, rows], axis=1).astype(np.int32))
    tiles = np.concatenate(tiles)
    # one upload for all the small tables, each 16-byte aligned within it
    blobs, at = [], {}
    for name, table in (('canvases', canvases), ('person_offsets', person_offsets),
                        ('persons', np.concatenate(persons).astype(np.int32)), ('skeleton', limbs), ('palette', palette),
                        ('tiles', tiles)):
        raw = np.frombuffer(np.ascontiguousarray(table).tobytes(), dtype=np.uint8)
        at[name] = sum(len(b) for b in blobs)
        blobs += [raw, np.zeros(-len(raw) % 16, dtype=np.uint8)]
    blob = torch.from_numpy(np.concatenate(blobs)).to(dev)
    base = blob.data_ptr()
    args = _C.VisPoseArgs(canvases=base + at['canvases'], person_offsets=base + at['person_offsets'],
                          persons=base + at['persons'], joints=ptr(joints), skeleton=base + at['skeleton'],
                          palette=base + at['palette'] if len(palette) else None, tiles=base + at['tiles'],
                          C=len(imgs), P=P, K=K, L=len(limbs), n_palette=len(palette), n_tiles=len(tiles),
                          canvas_h_max=max(im.size(0) for im in imgs), canvas_w_max=max(im.size(1) for im in imgs),
                          style=_STYLES[style], thickness=int(thickness), radius=int(radius),
                          score_thresh=float(score_thresh), alpha256=int(round(alpha * 256)))
    check(lib().buctd_vis_pose_overlay(ctypes.byref(args), stream_ptr()), "vis_pose_overlay")
    return images


def render_pose_panels(image, conditions, predictions, skeleton='coco', style='plain', thickness=2, radius=3,
                       score_thresh=-1.0, alpha=1.0):
    """The picture of tools/inference.py:295-314 without its text labels: `image` (uint8 [H, W, 3] on the device) twice
    side by side, the conditions [P, K, 2 or 3] drawn on the left copy and the predictions on the right one, each with
    its own hsv_wheel.  uint8 [H, 2 W, 3] on the device; `image` itself is not drawn on."""
    if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.size(2) == 3):
        raise _C.BuctdHipError("render_pose_panels: the image must be a uint8 [H, W, 3] tensor")
    ptr(image)
    H, W = image.size(0), image.size(1)
    out = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device=image.device)
    out[:, :W] = image
    out[:, W:] = image
    draw_poses([out[:, :W], out[:, W:]], [conditions, predictions], skeleton=skeleton, style=style, thickness=thickness,
               radius=radius, score_thresh=score_thresh, alpha=alpha)
    return out


def render_pretty_batch_image_with_joints(batch_image, batch_joints, nrow=8, padding=2, bgr=True, skeleton=None):
    """The picture of save_pretty_batch_image_with_joints: the normalised make_grid of the batch (the joint grid with no
    joint marked) with the skeleton of batch_joints[b] drawn into cell b in the 'pretty' style at alpha 0.7, clipped to
    the cell.  Every joint is drawn (the reference passes score 0 against a threshold of -1) unless a coordinate is not
    finite.  skeleton None: 'coco_pretty', which needs K == 17."""
    img = _image(batch_image)
    B, _, H, W = img.shape
    xy = torch.as_tensor(batch_joints)
    if xy.dim() != 3 or xy.size(0) != B or xy.size(-1) < 2:
        raise _C.BuctdHipError(f"vis: joints must be [B, K, 2+], got {tuple(xy.shape)}")
    K = xy.size(1)
    if skeleton is None:
        if K != 17:
            raise _C.BuctdHipError(f"vis: the default skeleton 'coco_pretty' has 17 joints; pass a skeleton for K = {K}")
        skeleton = 'coco_pretty'
    zeros = np.zeros((B, K, 2), dtype=np.float32)
    hidden = np.zeros((B, K), dtype=np.float32)
    grid = render_batch_image_with_joints(img, zeros, hidden, {'joints': zeros, 'joints_vis': hidden}, nrow, padding, bgr)
    xy = xy[..., :2].detach().to(device=img.device, dtype=torch.float32)
    poses = torch.cat([xy, torch.zeros_like(xy[..., :1])], dim=-1)          # B persons on one canvas, score 0
    xmaps = min(nrow, B)
    left = np.array([(b % xmaps) * (W + padding) + padding for b in range(B)])
    top = np.array([(b // xmaps) * (H + padding) + padding for b in range(B)])
    draw_poses(grid, poses, skeleton=skeleton, style='pretty', thickness=2, radius=3, score_thresh=-1.0,
               alpha=0.7, offsets=np.stack([left, top], axis=1),
               clips=np.stack([left, top, left + W, top + H], axis=1))
    return grid


def save_pretty_batch_image_with_joints(batch_image, batch_joints, batch_joints_vis, file_name, nrow=8, padding=2,
                                        bgr=True, skeleton=None):
    """reference utils/vis.py:42-73 (which does not read batch_joints_vis either).  Any K with a skeleton table."""
    write_png(file_name, render_pretty_batch_image_with_joints(batch_image, batch_joints, nrow, padding, bgr,
                                                               skeleton).cpu().numpy())


def save_pretty_debug_images(config, input, meta, target, joints_pred, output, prefix, suffix=''):
    """reference utils/vis.py:474-496; the files are PNG."""
    if not config.DEBUG.DEBUG:
        return
    bgr = not config.DATASET.COLOR_RGB
    if config.DEBUG.SAVE_BATCH_IMAGES_GT:
        save_pretty_batch_image_with_joints(input, meta['joints'], meta['joints_vis'],
                                            '{}_gt_{}.png'.format(prefix, suffix), bgr=bgr)
    if config.DEBUG.SAVE_BATCH_IMAGES_PRED:
        save_pretty_batch_image_with_joints(input, joints_pred, meta['joints_vis'],
                                            '{}_pred_{}.png'.format(prefix, suffix), bgr=bgr)
    if config.DEBUG.SAVE_HEATMAPS_GT:
        save_batch_heatmaps(input, target, '{}_hm_gt_{}.png'.format(prefix, suffix), bgr=bgr)
    if config.DEBUG.SAVE_HEATMAPS_PRED:
        save_batch_heatmaps(input, output, '{}_hm_pred_{}.png'.format(prefix, suffix), bgr=bgr)
