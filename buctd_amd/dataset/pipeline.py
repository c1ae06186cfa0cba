"""GPU-side sample pipeline and in-process iterative refinement.

DeviceSamplePipeline does what the DataLoader workers of the reference do per sample in
lib/dataset/JointsDataset.py:134-361 - box -> (half-body / scale / rotation / flip augmentation) -> affine crop ->
ToTensor/Normalize -> key points into crop coordinates -> Gaussian target + condition heat-map - for a whole batch:
the scalar geometry (a few dozen float64 operations per person, the same expressions as the reference) stays on the host
(or, with geometry_on_device=True, is one buctd_sample_geometry launch per batch),
every per-pixel step is one batched HIP kernel writing straight into the NCHW network input, the target and the
target weights.  Decoded images are uint8 HWC tensors already resident on the device (JPEG decoding is host I/O).

IterativeRefiner chains conditional top-down passes without touching disk: the reference runs tools/test.py three times
and hands the predictions over through the results json (scripts/test/test_BUCTD_COAM_gen_sample.sh:21,
lib/dataset/dataloader.py:454-508): prediction k -> box from its key points (+ margin, clipped) -> center / scale ->
new crop + re-rendered condition -> prediction k+1, with the rescoring of dataloader.py:596-612.

Generative sampling (DATASET.SYNTHESIS_POSE, JointsDataset.py:165-215): in train mode the condition is a pose synthesized
from the ground truth, fresh for every sample.  DeviceSamplePipeline.__call__ draws it for the whole batch with one
buctd_synthesize_pose launch, takes it through flip and crop affine with buctd_cond_geometry and renders it - the pose
never leaves the device between the synthesis and the network input.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from .. import ops
from .._C import RefineArgs, SampleGeomArgs, TrackArgs, check, lib, ptr, stream_ptr
from ..core.inference import get_final_preds
from ..utils.transforms import (_swap_table, affine_transform, flip_hm, flip_perm, fliplr_joints, get_affine_transform,
                                mirror_condition)
from .pose_synthesis import make_tables, synthesize_pose_batch

_M64 = (1 << 64) - 1
MAX_DEVICE_JOINTS = 32         # buctd_sample_geometry, buctd_refine_step, buctd_cond_geometry, buctd_cond_mirror
GEOM_HAS_BBOX, GEOM_USE_BU_BBOX, GEOM_HALF_BODY, GEOM_FLIP = 1, 2, 4, 8      # BUCTD_GEOM_* of include/buctd_hip.h
NO_BOX = ("sample(s) {bad} of the batch: use_bu_bbox with a condition pose without a non-zero x or y coordinate, or a "
          "box without extent (status {status}): there is no box to crop")
NO_CONDITION = ("Training with empirical sampling is not possible without providing 'cond_kpts'; "
                "please train with generative sampling (DATASET.SYNTHESIS_POSE=True)")


class _WarpItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("flip", C.c_int), ("rx", C.c_int),
                ("ry", C.c_int), ("rw", C.c_int), ("rh", C.c_int), ("m", C.c_double * 6)]


# the same struct for numpy: a whole table is filled column by column
WARP_ITEM = np.dtype({"names": [f[0] for f in _WarpItem._fields_],
                      "formats": [np.uint64] + [np.int32] * 7 + [(np.float64, 6)],
                      "offsets": [getattr(_WarpItem, f[0]).offset for f in _WarpItem._fields_],
                      "itemsize": C.sizeof(_WarpItem)})


def fill_warp_items(items, src, sizes, geos=None):
    """items: zeroed WARP_ITEM array [B], filled column by column.  src: the images' device addresses; sizes: their
    (H, W); geos: geometry() results - flip, keep-rectangle and crop affine - or None where buctd_sample_geometry writes
    those columns itself."""
    items["src"] = src
    items["H"], items["W"] = np.asarray(sizes, dtype=np.int32).reshape(-1, 2).T
    if geos is not None:
        items["flip"] = [int(g["flip"]) for g in geos]
        rects = [g.get("keep_rect") for g in geos]
        items["rx"], items["ry"], items["rw"], items["rh"] = np.array(
            [(0, 0, 0, 0) if r is None else tuple(int(v) for v in r) for r in rects], dtype=np.int32).reshape(-1, 4).T
        items["m"] = [np.asarray(g["trans"], dtype=np.float64).reshape(6) for g in geos]
    return items


def _check_images(images):
    for img in images:
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous() or not img.is_cuda:
            raise ValueError("images must be contiguous uint8 [H, W, 3] device tensors")


def warp_items(images, geos=None, items=None):
    """fill_warp_items for device images, into `items` (a zeroed WARP_ITEM array) or a new table."""
    _check_images(images)
    if items is None:
        items = np.zeros(len(images), dtype=WARP_ITEM)
    return fill_warp_items(items, [img.data_ptr() for img in images], [img.shape[:2] for img in images], geos)


def xywh2cs(x, y, w, h, aspect_ratio, scale_thre, pixel_std=200):
    """Box -> (center, scale) with the network's aspect ratio (reference dataloader.py:305-321)."""
    center = np.array([x + w * 0.5, y + h * 0.5], dtype=np.float32)
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / pixel_std, h * 1.0 / pixel_std], dtype=np.float32)
    if center[0] != -1:
        scale = scale * scale_thre
    return center, scale


def box_from_keypoints(kp, margin, img_w, img_h):
    """Box of the non-zero key-point coordinates +- margin, clipped to the image (JointsDataset.py:217-226)."""
    xs, ys = kp[:, 0][np.nonzero(kp[:, 0])], kp[:, 1][np.nonzero(kp[:, 1])]
    xmin, ymin = np.clip(xs.min() - margin, 0, img_w), np.clip(ys.min() - margin, 0, img_h)
    xmax, ymax = np.clip(xs.max() + margin, 0, img_w), np.clip(ys.max() + margin, 0, img_h)
    return [xmin, ymin, xmax - xmin, ymax - ymin]


def keep_rectangle(bbox, bbox_draws=None):
    """The rectangle of DATASET.NEW_AUGMENTATION (JointsDataset.py:263-279): source pixels outside the person box are
    zeroed before the warp.  bbox: x, y, w, h, truncated like np.array(bbox).astype(int); bbox_draws: the two
    randint(0, 20) of DATASET.BBOX_AUGMENTATION (lines 267-273) or None.  Returns (rx, ry, rw, rh) of buctd_warp_item, cut
    at the origin as oracle.sample.warp_affine_u8 keeps it (rx = max(x, 0), rw = x + w - rx; the reference's negative
    slice indices wrap around instead: out of scope).  buctd_sample_geometry restates these lines."""
    x, y, w, h = (int(v) for v in np.array(bbox).astype(int))
    if bbox_draws is not None:
        x_delta, y_delta = w * int(bbox_draws[0]) // 10, h * int(bbox_draws[1]) // 10
        x = int(x - x_delta) if x - x_delta > 0 else 0
        y = int(y - y_delta) if y - y_delta > 0 else 0
        w, h = int(w + 2 * x_delta), int(h + 2 * y_delta)
    rx, ry = max(x, 0), max(y, 0)
    return rx, ry, x + w - rx, y + h - ry


def synthesis_area(cond):
    """cond [B, K, 3] -> [B]: width * height of the box around the non-zero condition coordinates
    (JointsDataset.py:204-210), every record at once."""
    cond = np.asarray(cond, dtype=np.float64)
    xs, ys = cond[:, :, 0], cond[:, :, 1]
    nx, ny = xs != 0, ys != 0
    if not (nx.any(1) & ny.any(1)).all():
        raise ValueError("pose synthesis: a condition without a non-zero x or y coordinate has no area")
    w = np.where(nx, xs, -np.inf).max(1) - np.where(nx, xs, np.inf).min(1)
    h = np.where(ny, ys, -np.inf).max(1) - np.where(ny, ys, np.inf).min(1)
    return w * h


def pad_near_joints(near, num_joints):
    """near: per record the neighbours' key points in any shape that reshapes to [M_b, K, 3] (JointsDataset.py:212).
    Returns [B, M, K, 3] with M the batch's largest M_b, absent neighbours as zeros (visibility 0: the form
    synthesize_pose_batch takes), or None when no record has a neighbour."""
    per = [np.asarray(n, dtype=np.float64).reshape(-1, num_joints, 3) for n in near]
    m = max((n.shape[0] for n in per), default=0)
    if m == 0:
        return None
    out = np.zeros((len(per), m, num_joints, 3), dtype=np.float64)
    for b, n in enumerate(per):
        out[b, :n.shape[0]] = n
    return out


def target_centres(joints, stride):
    """joints [B, K, >=2] float64 crop coordinates -> float32 [B, K, 3]: per joint a coordinate that the target kernel's
    (int)(v / stride + 0.5f) maps to the reference's heat-map centre mu = int(j / stride + 0.5) (see render())."""
    joints = np.asarray(joints, dtype=np.float64)
    jt = np.zeros(joints.shape[:2] + (3,), dtype=np.float32)
    for a in (0, 1):
        mu = (joints[:, :, a] / stride[a] + 0.5).astype(int)
        jt[:, :, a] = np.where(mu < 0, mu - 1, mu) * stride[a]
    return jt


def trunc_condition(cond):
    """cond [B, K, >=2] float64 -> float32 [B, K, 2]: np.array(kpts).astype(int) of JointsDataset.py:521 as floats."""
    return np.ascontiguousarray(np.trunc(np.asarray(cond, dtype=np.float64)[:, :, :2]).astype(np.float32))


def _layout(sections):
    """[(name, numpy dtype, shape)] -> ({name: (byte offset, dtype, shape)}, total bytes); widest items first, so every
    section is aligned to its item size."""
    at, off = {}, 0
    for name, dt, shape in sorted(sections, key=lambda t: -np.dtype(t[1]).itemsize):
        at[name] = (off, np.dtype(dt), tuple(shape))
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    return at, off


def _views(buf, at):
    """Typed views of the sections of a uint8 tensor (device) or numpy array (host)."""
    out = {}
    for name, (off, dt, shape) in at.items():
        raw = buf[off:off + int(np.prod(shape)) * dt.itemsize]
        if torch.is_tensor(raw):
            out[name] = raw.view(getattr(torch, dt.name)).view(shape)
        else:
            out[name] = raw.view(dt).reshape(shape)
    return out


def history_layout(passes, B, K):
    """The sections of IterativeRefiner's history buffer, what buctd_refine_step writes per pass: for _layout()."""
    f32, f64 = np.float32, np.float64
    return [("score", f64, (passes, B)), ("box_score", f64, (passes, B)), ("keypoint_score", f64, (passes, B)),
            ("preds", f32, (passes, B, K, 3)), ("center", f32, (passes, B, 2)), ("scale", f32, (passes, B, 2)),
            ("status", np.int32, (B,))]


def batch_seed(seed, call):
    """64-bit synthesis seed of call number `call` of a pipeline seeded with `seed` (splitmix64 finaliser: seeds of
    consecutive calls share no counter sequence of the generator in csrc/synth.hip)."""
    z = ((int(seed) & _M64) * 0x9E3779B97F4A7C15 + int(call) + 1) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class DeviceSamplePipeline:
    """Batched sample pipeline.  pipe(records, aug=None, seed=None) -> (input, target, target_weight, meta).

    Generative sampling: with is_train, MODEL.CONDITIONAL_TOPDOWN and DATASET.SYNTHESIS_POSE the condition of every
    record is synthesized on the device (one launch per batch; person index = batch index; num_overlap 0; `seed`, or
    a 64-bit value from the pipeline's seed and a call counter when seed is None: two calls differ, two pipelines with
    the same seed repeat each other).  A record without 'cond_joints' takes joints_3d / joints_3d_vis as its condition
    (JointsDataset.py:165-167); records carry 'near_joints' (anything that reshapes to [M, K, 3]; may be empty).  On
    this path meta['cond_joints'] / meta['cond_joints_vis'] are float64 DEVICE tensors (crop coordinates) and
    meta['synth_joints'] is the synthesized pose in image coordinates, on the device as well; nothing is copied back.
    If any record of the batch has use_bu_bbox=True its crop box depends on the synthesized pose: the batch then takes
    a host fallback - one copy of the synthesized poses to the host, then geometry() and render() as without synthesis
    (same result, slower; meta['cond_joints'] / ['cond_joints_vis'] are host tensors there).  With is_train=False the
    flag changes nothing.  Without the flag a conditional train pipeline refuses records that lack 'cond_joints'.
    The variant of the synthesis is cfg.DATASET.DATASET's: 'coco', 'crowdpose', or the generic one for any other name
    (fish, marmosets, multimouse, a custom data set; pose_synthesis.py:798-816).  synth_ladders: the probability ladders of
    the synthesis (pose_synthesis.make_tables; None = the reference's), e.g. ErrorProfile.ladders() of
    dataset.error_diagnosis: the error mix measured on the bottom-up model whose poses condition the network at test time.

    geometry_on_device=True (train pipelines, NUM_JOINTS <= 32): the scalar geometry leaves the host as well.  __call__
    makes the augmentation draws with the same generators in the same order as the host path (draw(); aug = a list of
    draw() results replays them), uploads the records and the draws as one packed buffer and launches
    buctd_sample_geometry: box (the record's, or under use_bu_bbox the one around the condition pose - the synthesized
    pose never leaves the device, there is no host fallback), half-body override (decided and boxed on the host), scale
    draw, flip, crop affine in closed form (utils.transforms.crop_affine_rot_closed_form), joints and condition in crop
    coordinates, target centres, keep-rectangle.  The crop, target and condition kernels read what it wrote.  On this
    path meta['joints'], ['joints_vis'], ['cond_joints'], ['cond_joints_vis'], ['center'], ['scale'] (float64: see
    apply_draw), ['rotation'] (float64) are DEVICE tensors, meta['table'] is the buctd_warp_item table and
    meta['status'] the kernel's int32 status per sample; nothing is copied back and the call does not wait for the
    device.  A sample without a box (use_bu_bbox with a condition that has no non-zero x or no non-zero y; the host path's
    synthesis_area raises for such a condition) gets status != 0 and an all-zero sample instead of an exception:
    check(meta) reads the status back and raises the ValueError.  Default False: the host path, bit for bit.

    Keep-rectangle (both paths): with is_train and DATASET.NEW_AUGMENTATION a sample that has a box - rec['bbox'], or under
    use_bu_bbox the box around its condition - is cropped from an image zeroed outside that box (JointsDataset.py:263-279),
    widened by the DATASET.BBOX_AUGMENTATION draws; records without 'bbox' are cropped as before.

    joints_weight ([K] or [K, 1], the data set class's self.joints_weight): with cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT
    every target_weight is multiplied by it on the device (JointsDataset.py:450-451); without the flag, or with None,
    it is not looked at."""

    def __init__(self, cfg, flip_pairs=(), upper_body_ids=(), kpt_colors=None, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), is_train=False, seed=0, joints_weight=None, geometry_on_device=False,
                 synth_ladders=None):
        self.cfg = cfg
        self.is_train = is_train
        self.num_joints = cfg.MODEL.NUM_JOINTS
        self.image_size = np.array(cfg.MODEL.IMAGE_SIZE)
        self.heatmap_size = np.array(cfg.MODEL.HEATMAP_SIZE)
        self.sigma = cfg.MODEL.SIGMA
        self.aspect_ratio = self.image_size[0] * 1.0 / self.image_size[1]
        ds = cfg.DATASET
        self.colored = bool(ds.COLORED)
        self.stacked = bool(ds.STACKED_CONDITION)
        self.conditional = bool(cfg.MODEL.CONDITIONAL_TOPDOWN)
        self.scale_factor = getattr(ds, "SCALE_FACTOR", 0.25)
        self.rotation_factor = getattr(ds, "ROT_FACTOR", 30)
        self.flip = bool(getattr(ds, "FLIP", True))
        self.num_joints_half_body = getattr(ds, "NUM_JOINTS_HALF_BODY", 8)
        self.prob_half_body = getattr(ds, "PROB_HALF_BODY", 0.0)
        self.bu_bbox_margin = getattr(ds, "BU_BBOX_MARGIN", 25)
        self.new_augmentation = bool(getattr(ds, "NEW_AUGMENTATION", False))
        self.bbox_augmentation = bool(getattr(ds, "BBOX_AUGMENTATION", False))
        self.scale_thre = getattr(cfg.TEST, "SCALE_THRE", 1.25)
        self.flip_pairs = [list(p) for p in flip_pairs]
        self.upper_body_ids = set(upper_body_ids)
        self.kpt_colors = None if kpt_colors is None else np.asarray(kpt_colors, dtype=np.float32)
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        self.np_rng = np.random.RandomState(seed)
        self.py_rng = random.Random(seed)
        self.synthesis_pose = bool(getattr(ds, "SYNTHESIS_POSE", False))
        self.dataset = getattr(ds, "DATASET", None)
        self.seed = int(seed)
        self.synth_calls = 0
        self.synth_ladders = synth_ladders
        if synth_ladders is not None:
            make_tables(self.dataset, self.num_joints, synth_ladders)      # refuse a malformed value here, not mid-epoch
        self._pair_dev = {}
        self._perm_dev, self._colors_dev = {}, {}                          # the flip test's tables, uploaded once
        self.joints_weight = None
        if joints_weight is not None and bool(getattr(getattr(cfg, "LOSS", None), "USE_DIFFERENT_JOINTS_WEIGHT", False)):
            jw = np.asarray(joints_weight, dtype=np.float32)
            if jw.shape not in ((self.num_joints,), (self.num_joints, 1)):
                raise ValueError(f"joints_weight has shape {jw.shape}, MODEL.NUM_JOINTS is {self.num_joints}")
            self.joints_weight = np.ascontiguousarray(jw.reshape(1, self.num_joints, 1))
        self._weight_dev = {}
        self.geometry_on_device = bool(geometry_on_device)
        if self.geometry_on_device:
            if not is_train:
                raise ValueError("DeviceSamplePipeline(geometry_on_device=True) is the train path (is_train=True): an eval "
                                 "batch has no draws, and IterativeRefiner(on_device=True) keeps its geometry on the device")
            if self.num_joints > MAX_DEVICE_JOINTS:
                raise ValueError(f"DeviceSamplePipeline(geometry_on_device=True) handles at most {MAX_DEVICE_JOINTS} "
                                 f"joints (MODEL.NUM_JOINTS is {self.num_joints})")

    # ---- host-side scalar geometry (reference expressions, float64) -----------------------------------------
    def half_body_transform(self, joints, joints_vis):
        """JointsDataset.py:90-133: box around the visible upper- or lower-body joints."""
        upper = [joints[i] for i in range(self.num_joints) if joints_vis[i][0] > 0 and i in self.upper_body_ids]
        lower = [joints[i] for i in range(self.num_joints) if joints_vis[i][0] > 0 and i not in self.upper_body_ids]
        if self.np_rng.randn() < 0.5 and len(upper) > 2:
            chosen = upper
        else:
            chosen = lower if len(lower) > 2 else upper
        if len(chosen) < 2:
            return None, None
        pts = np.array(chosen, dtype=np.float32)
        center = pts.mean(axis=0)[:2]
        lo, hi = np.amin(pts, axis=0), np.amax(pts, axis=0)
        w, h = hi[0] - lo[0], hi[1] - lo[1]
        if w > self.aspect_ratio * h:
            h = w * 1.0 / self.aspect_ratio
        elif w < self.aspect_ratio * h:
            w = h * self.aspect_ratio
        return center, np.array([w * 1.0 / 200, h * 1.0 / 200], dtype=np.float32) * 1.5

    def draw(self, rec):
        """The random draws of one record, JointsDataset.py:236-269 (same generators, same order): dict(half_body =
        (center, scale) of the half-body box or None, scale_mul = the clipped scale multiplier (None in eval mode: the
        scale keeps its dtype), rot, flip, bbox_aug = the two randint(0, 20) of DATASET.BBOX_AUGMENTATION or None - drawn
        after the flip, whether the record has a box or not).  geometry(rec, aug=<this dict>) replays it."""
        d = dict(half_body=None, scale_mul=None, rot=0, flip=False, bbox_aug=None)
        if not self.is_train:
            return d
        if np.sum(rec["joints_3d_vis"][:, 0]) > self.num_joints_half_body and self.np_rng.rand() < self.prob_half_body:
            c_hb, s_hb = self.half_body_transform(rec["joints_3d"], rec["joints_3d_vis"])
            if c_hb is not None and s_hb is not None:
                d["half_body"] = (c_hb, s_hb)
        sf, rf = self.scale_factor, self.rotation_factor
        d["scale_mul"] = np.clip(self.np_rng.randn() * sf + 1, 1 - sf, 1 + sf)
        d["rot"] = np.clip(self.np_rng.randn() * rf, -rf * 2, rf * 2) if self.py_rng.random() <= 0.6 else 0
        d["flip"] = self.flip and self.py_rng.random() <= 0.5
        if self.new_augmentation and self.bbox_augmentation:
            d["bbox_aug"] = (self.py_rng.randint(0, 20), self.py_rng.randint(0, 20))
        return d

    @staticmethod
    def apply_draw(d, center, scale):
        """center, scale after the half-body override and the scale draw of d = draw(rec).  float32 scale * the float64
        numpy scalar of the draw is a FLOAT64 array (numpy >= 2, NEP 50): in train mode get_affine_transform and
        meta['scale'] see a float64 scale, and buctd_sample_geometry follows that (tests/test_sample_geometry.py pins it)."""
        if d["half_body"] is not None:
            center, scale = d["half_body"]
        if d["scale_mul"] is not None:
            scale = scale * d["scale_mul"]
        return center, scale

    def draw_augmentation(self, rec, center, scale):
        """The random part of JointsDataset.py:233-251 (same draws in the same order): returns center, scale, rot, flip."""
        d = self.draw(rec)
        center, scale = self.apply_draw(d, center, scale)
        return center, scale, d["rot"], d["flip"]

    def condition(self, rec):
        """(cond_joints, cond_joints_vis, has_cond) of a record as float64 copies.  A conditional train pipeline gives a
        record without 'cond_joints' its own joints (JointsDataset.py:165-169) - under DATASET.SYNTHESIS_POSE only."""
        joints, joints_vis = rec["joints_3d"], rec["joints_3d_vis"]
        if "cond_joints" in rec:
            if self.synthesizes and isinstance(rec["cond_joints"], dict):
                raise ValueError("pose synthesis needs one condition per record: 'cond_joints' is a dict of conditions")
            return (np.array(rec["cond_joints"], dtype=np.float64).copy(),
                    np.array(rec["cond_joints_vis"], dtype=np.float64).copy(), True)
        if self.conditional and self.is_train:
            if not self.synthesis_pose:
                raise ValueError(NO_CONDITION)
            return np.array(joints, dtype=np.float64).copy(), np.array(joints_vis, dtype=np.float64).copy(), True
        return np.zeros_like(joints, dtype=np.float64), np.zeros_like(joints_vis, dtype=np.float64), False

    @property
    def synthesizes(self):
        """Whether __call__ replaces the condition by a synthesized pose (JointsDataset.py:202: `and self.is_train`)."""
        return self.synthesis_pose and self.is_train and self.conditional

    def geometry(self, rec, aug=None, cond=None):
        """Everything of a sample that is scalar: returns dict(trans, center, scale, rot, flip, joints, joints_vis,
        cond_joints, cond_joints_vis) with the key points already in crop coordinates.  aug = (center, scale, rot, flip)
        replaces the random draws (parity tests); center is the value BEFORE the flip mirrors it, like in the reference.
        aug = a draw() result replays those draws instead: box, half-body override, scale multiplier, rotation, flip and
        the BBOX_AUGMENTATION integers, as buctd_sample_geometry takes them.
        cond = (cond_joints, cond_joints_vis) replaces the record's condition (a synthesized pose); cond = False leaves
        the condition out (it is transformed on the device): cond_joints / cond_joints_vis come back as zeros.
        keep_rect (only with is_train and DATASET.NEW_AUGMENTATION, for a sample that has a box - the record's 'bbox', or
        under use_bu_bbox the condition's): keep_rectangle() of it, which warp_table() hands to the crop kernel."""
        img = rec["image"]
        ih, iw = int(img.shape[0]), int(img.shape[1])
        joints = np.array(rec["joints_3d"], dtype=np.float64).copy()
        joints_vis = np.array(rec["joints_3d_vis"], dtype=np.float64).copy()
        if cond is None:
            cj, cv, has_cond = self.condition(rec)
        elif cond is False:
            cj, cv, has_cond = np.zeros_like(joints), np.zeros_like(joints_vis), False
        else:
            cj, cv, has_cond = np.array(cond[0], dtype=np.float64).copy(), np.array(cond[1], dtype=np.float64).copy(), True
        if rec.get("use_bu_bbox", False) and has_cond and cj[:, 0].sum() != 0 and cj[0, 1].sum() != 0:
            bbox = box_from_keypoints(cj, self.bu_bbox_margin, iw, ih)
            center, scale = xywh2cs(*bbox, self.aspect_ratio, self.scale_thre)
        else:
            center = np.array(rec["center"], dtype=np.float32).copy()
            scale = np.array(rec["scale"], dtype=np.float32).copy()
            bbox = rec.get("bbox")
        bbox_aug = None
        if aug is None or isinstance(aug, dict):
            d = self.draw(rec) if aug is None else aug
            center, scale = self.apply_draw(d, center, scale)
            center = np.array(center, np.float32).copy()
            rot, flip, bbox_aug = d["rot"], d["flip"], d["bbox_aug"]
        else:
            center, scale, rot, flip = np.array(aug[0], np.float32).copy(), np.array(aug[1], np.float32), aug[2], aug[3]
        keep_rect = None
        if self.is_train and self.new_augmentation and bbox is not None:
            keep_rect = keep_rectangle(bbox, bbox_aug)
        if flip:
            joints, joints_vis = fliplr_joints(joints, joints_vis, iw, self.flip_pairs)
            center[0] = iw - center[0] - 1
            if has_cond:
                cj, cv = fliplr_joints(cj, cv, iw, self.flip_pairs)
        trans = get_affine_transform(center, scale, rot, self.image_size)
        for i in range(self.num_joints):
            if joints_vis[i, 0] > 0.0:
                joints[i, 0:2] = affine_transform(joints[i, 0:2], trans)
            if has_cond and cv[i, 0] > 0.0:
                cj[i, 0:2] = affine_transform(cj[i, 0:2], trans)
        return dict(trans=trans, center=center, scale=scale, rot=rot, flip=bool(flip), joints=joints,
                    joints_vis=joints_vis, cond_joints=cj, cond_joints_vis=cv, keep_rect=keep_rect)

    # ---- batched device work -----------------------------------------------------------------------------------
    def warp_table(self, images, geos):
        """The per-sample table of the device kernels (buctd_warp_item: source image, flip, keep-rectangle, crop affine)
        as a uint8 device tensor."""
        return torch.from_numpy(warp_items(images, geos).view(np.uint8)).to(images[0].device)

    def pair_table(self, dev):
        """int32 [K] on the device: the flip partner of every joint, -1 for a joint without one (uploaded once)."""
        pair = self._pair_dev.get(dev)
        if pair is None:
            K = self.num_joints
            swap = _swap_table(K, self.flip_pairs)
            pair = torch.from_numpy(np.where(swap == np.arange(K), -1, swap).astype(np.int32)).to(dev)
            self._pair_dev[dev] = pair
        return pair

    def flip_perm(self, dev):
        """int32 [K] on the device: the channel permutation of ops.flipback_avg (utils.transforms.flip_perm, uploaded
        once)."""
        perm = self._perm_dev.get(dev)
        if perm is None:
            perm = self._perm_dev[dev] = flip_perm(self.num_joints, self.flip_pairs, dev)
        return perm

    def cond_geometry(self, synth, cond_vis, table):
        """Flip + crop affine of device-resident condition poses (buctd_cond_geometry).  synth, cond_vis: float64 device
        tensors [B, K, 3]; table: warp_table().  Returns cond_joints, cond_joints_vis (float64) and the truncated
        coordinates float32 [B, K, 2] that render(cond_trunc=...) takes - all on the device."""
        dev = synth.device
        B, K = int(synth.shape[0]), int(synth.shape[1])
        pair = self.pair_table(dev)
        cj, cv = torch.empty_like(synth), torch.empty_like(cond_vis)
        cjt = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        check(lib().buctd_cond_geometry(ptr(synth), ptr(cond_vis), ptr(table), ptr(pair), B, K, ptr(cj), ptr(cv), ptr(cjt),
                                        stream_ptr()), "cond_geometry")
        return cj, cv, cjt

    def render(self, images, geos, want_crop=False, table=None, cond_trunc=None, targets=None):
        """images: uint8 HWC device tensors; geos: geometry() results.  Returns input [B, 3(+3), H, W], target
        [B, K, h, w], target_weight [B, K, 1] (+ the uint8 crops) on the device.  table: warp_table(images, geos) if the
        caller built it already; cond_trunc: the condition coordinates as cond_geometry() returns them, instead of
        geos[.]['cond_joints']; targets: (target centres float32 [B, K, 3], visibilities float32 [B, K]) on the device as
        buctd_sample_geometry wrote them, instead of geos[.]['joints'] / ['joints_vis'] (geos is not read then)."""
        dev = images[0].device
        B, K = len(images), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        cc = (K if self.stacked else 3) if self.conditional else 0      # stacked: one condition channel per joint
        x = torch.empty((B, 3 + cc, H, W), dtype=torch.float32, device=dev)
        if table is None:
            table = self.warp_table(images, geos)
        crop = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if want_crop else None
        self._warp(table, B, x, crop)
        # Gaussian targets: the heat-map centre mu = int(j / stride + 0.5) is evaluated here in float64 exactly like the
        # reference (JointsDataset.py:417-418).  The kernel recomputes (int)(v / stride + 0.5f), truncating toward zero as
        # well, so it is handed a v that maps back to the same mu: mu * stride for mu >= 0 and (mu - 1) * stride for mu < 0
        # (v / stride + 0.5 = mu - 0.5 truncates to mu; mu * stride would give mu + 0.5 -> mu + 1 for negative centres:
        # visible joints left of / above the crop would get a shifted Gaussian and a shifted target_weight cut-off)
        if targets is None:
            stride = self.image_size / self.heatmap_size
            jt = target_centres(np.stack([g["joints"] for g in geos]), stride)
            vis = np.stack([g["joints_vis"][:, 0] for g in geos]).astype(np.float32)
            targets = torch.from_numpy(jt).to(dev), torch.from_numpy(vis).to(dev)
        target, weight = ops.gaussian_target(targets[0], targets[1], self.heatmap_size, self.image_size, self.sigma)
        if self.joints_weight is not None:
            # np.multiply(target_weight, self.joints_weight) of JointsDataset.py:450-451, the batch at once
            jw = self._weight_dev.get((dev, B))
            if jw is None:
                jw = self._weight_dev[(dev, B)] = torch.from_numpy(np.repeat(self.joints_weight, B, axis=0)).to(dev)
            weight = ops.mul(weight, jw)
        if cc:
            # np.array(kpts).astype(int) truncates in float64 (JointsDataset.py:521): hand the kernel the integers
            cjt = cond_trunc
            if cjt is None:
                cjt = torch.from_numpy(trunc_condition(np.stack([g["cond_joints"] for g in geos]))).to(dev)
            self.render_condition(x, cjt)
        return (x, target, weight, crop) if want_crop else (x, target, weight)

    def _warp(self, table, B, x, crop=None):
        """The crops of table's first B items into channels [0, 3) of x (+ the uint8 crops): buctd_warp_affine_norm."""
        mean = (C.c_float * 3)(*self.mean.tolist())
        std = (C.c_float * 3)(*self.std.tolist())
        check(lib().buctd_warp_affine_norm(ptr(table), B, int(x.shape[2]), int(x.shape[3]), mean, std, ptr(x), x.stride(0),
                                           ptr(crop), stream_ptr()), "warp_affine_norm")

    def mirror_colors(self, dev):
        """The colour table on the device, uploaded once per device: what the mirrored half of a 3-channel condition is
        rendered with (transforms.flip_hm renders it colored for a mono condition as well)."""
        colors = self._colors_dev.get(dev)
        if colors is None:
            if self.kpt_colors is None:
                raise ValueError("the flip test re-renders a 3-channel condition colored: the pipeline needs kpt_colors")
            colors = torch.from_numpy(np.ascontiguousarray(self.kpt_colors[:self.num_joints])).to(dev)
            self._colors_dev[dev] = colors
        return colors

    def condition_colors(self, dev):
        """mirror_colors() for a colored condition, None for mono / stacked."""
        return self.mirror_colors(dev) if self.colored else None

    def render_condition(self, x, cjt, colors=None, colored=None):
        """Condition heat-map of truncated crop coordinates cjt (float32 [B, K, 2], device) into channels [3, 3 + Cc) of the
        network input x.  colors: condition_colors() if the caller has it already; colored=True renders a mono
        pipeline's 3-channel condition colored as well (the mirrored half of a flip-test input)."""
        dev = x.device
        B, K = int(x.shape[0]), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        colored = self.colored if colored is None else colored
        if colors is None and colored:
            colors = self.mirror_colors(dev)
        ws = ops.workspace(lib().buctd_cond_render_workspace(B * K if self.stacked else B, 3, H, W), dev)
        if self.stacked:
            # get_stacked_condition (JointsDataset.py:471-498): every joint is its own single-impulse image, blurred
            # and peak-normalised on its own - B * K one-joint "images" of one channel for the render kernel
            tmp = torch.empty((B * K, 1, H, W), dtype=torch.float32, device=dev)
            check(lib().buctd_cond_render_into(ptr(cjt), 2, None, B * K, 1, 1, H, W, 0, ptr(tmp), tmp.stride(0), ptr(ws),
                                               ws.numel(), stream_ptr()), "cond_render_into")
            x[:, 3:] = tmp.view(B, K, H, W)
        elif colored:
            check(lib().buctd_cond_render_into(ptr(cjt), 2, ptr(colors), B, K, 3, H, W, 0,
                                               C.c_void_p(x[:, 3:].data_ptr()), x.stride(0), ptr(ws), ws.numel(),
                                               stream_ptr()), "cond_render_into")
        else:
            # mono: the one blurred, int-truncated channel replicated x3 (JointsDataset.py:513-514)
            for c in range(3):
                check(lib().buctd_cond_render_into(ptr(cjt), 2, None, B, K, 1, H, W, 1,
                                                   C.c_void_p(x[:, 3 + c:].data_ptr()), x.stride(0), ptr(ws),
                                                   ws.numel(), stream_ptr()), "cond_render_into")

    def cond_mirror(self, cond_joints, cond_vis=None, out=None):
        """The mirrored, truncated condition coordinates of a batch (buctd_cond_mirror; utils.transforms.mirror_condition
        on the host).  cond_joints: float64 device tensor [B, K, 2 or 3], crop coordinates before any truncation;
        cond_vis: float64 [B, K, 3] or None for all ones.  Returns float32 [B, K, 2] (out, if given)."""
        B, K, js = (int(v) for v in cond_joints.shape)
        dev = cond_joints.device
        if cond_joints.dtype != torch.float64 or js not in (2, 3) or not cond_joints.is_contiguous():
            raise ValueError("cond_mirror: cond_joints must be a contiguous float64 [B, K, 2 or 3] tensor")
        if cond_vis is not None and (cond_vis.dtype != torch.float64 or tuple(cond_vis.shape) != (B, K, 3)
                                     or not cond_vis.is_contiguous() or cond_vis.device != dev):
            raise ValueError("cond_mirror: cond_vis must be a contiguous float64 [B, K, 3] tensor on cond_joints' device")
        if K != self.num_joints:
            raise ValueError(f"cond_mirror: cond_joints has {K} joints, MODEL.NUM_JOINTS is {self.num_joints}")
        if out is None:
            out = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or tuple(out.shape) != (B, K, 2) or not out.is_contiguous() or out.device != dev:
            raise ValueError("cond_mirror: out must be a contiguous float32 [B, K, 2] tensor on cond_joints' device")
        check(lib().buctd_cond_mirror(ptr(cond_joints), js, ptr(cond_vis), ptr(self.pair_table(dev)), B, K,
                                      int(self.image_size[0]), ptr(out), stream_ptr()), "cond_mirror")
        return out

    @staticmethod
    def mirror_rows(src, dst, channel0, count, perm=None):
        """dst[b, channel0 + c, y, x] = src[b, channel0 + perm[c], y, W - 1 - x] for c in [0, count) (buctd_mirror_rows).
        src, dst: float32 NCHW device tensors (or batch slices of one tensor, not overlapping) with dense images; perm:
        int32 [count] on the device, an entry outside [0, count) - the -1 of pair_table() - keeps its channel; None:
        identity."""
        B, _, H, W = (int(v) for v in src.shape)
        for t in (src, dst):
            if t.dtype != torch.float32 or t.dim() != 4 or t.stride()[1:] != (H * W, W, 1):
                raise ValueError("mirror_rows: float32 NCHW tensors with dense channels")
        if tuple(dst.shape[2:]) != (H, W) or int(dst.shape[0]) != B or channel0 < 0 or count < 1 or \
                channel0 + count > min(int(src.shape[1]), int(dst.shape[1])):
            raise ValueError("mirror_rows: src and dst differ in shape, or the channel range leaves them")
        if perm is not None and (perm.dtype != torch.int32 or tuple(perm.shape) != (count,) or not perm.is_contiguous()
                                 or perm.device != src.device):
            raise ValueError("mirror_rows: perm must be a contiguous int32 [count] tensor on src's device")
        if dst.device != src.device or not src.is_cuda:
            raise ValueError("mirror_rows: src and dst must be on one ROCm device")
        check(lib().buctd_mirror_rows(C.c_void_p(src.data_ptr()), src.stride(0), C.c_void_p(dst.data_ptr()), dst.stride(0),
                                      ptr(perm), B, int(channel0), int(count), H, W, stream_ptr()), "mirror_rows")
        return dst

    def warp_and_condition(self, table, cond_trunc, colors=None, mirrored=None):
        """Network input [B, 3 + Cc, H, W] from a device-resident warp_table() and truncated condition coordinates
        (float32 [B, K, 2], device): render() without the Gaussian targets and without any host array - the two kernels an
        inference pass needs.  Nothing is uploaded when colors (condition_colors()) is handed in.

        mirrored = (cond_joints, cond_joints_vis or None): the paired input of the flip test, [2B, 3 + Cc, H, W].  Rows
        [0, B) are the input above, written by the same launches; rows [B, 2B) are what core.function._mirrored_input makes
        of them: the image channels mirrored (buctd_mirror_rows), a stacked condition mirrored with partner channels
        exchanged, a 3-channel condition - colored or mono - rendered colored from the mirrored coordinates
        (buctd_cond_mirror of cond_joints: float64 [B, K, 2 or 3], the crop coordinates before trunc())."""
        if not self.conditional:
            raise ValueError("warp_and_condition renders a condition: MODEL.CONDITIONAL_TOPDOWN is off")
        dev = table.device
        B, K = int(cond_trunc.shape[0]), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        rows = B if mirrored is None else 2 * B
        if mirrored is not None and (mirrored[0].dim() != 3 or int(mirrored[0].shape[0]) != B or mirrored[0].device != dev):
            raise ValueError("warp_and_condition: mirrored[0] must be [B, K, 2 or 3] with the B of cond_trunc, on its device")
        x = torch.empty((rows, 3 + (K if self.stacked else 3), H, W), dtype=torch.float32, device=dev)
        self._warp(table, B, x)
        first, second = x[:B], x[B:]
        self.render_condition(first, cond_trunc, colors)
        if mirrored is not None:
            self.mirror_rows(first, second, 0, 3)
            if self.stacked:
                self.mirror_rows(first, second, 3, K, self.pair_table(dev))
            else:
                cjm = self.cond_mirror(mirrored[0], mirrored[1])
                self.render_condition(second, cjm, self.mirror_colors(dev), colored=True)
        return x

    # ---- scalar geometry on the device (geometry_on_device=True) ------------------------------------------------
    def draw_table(self, records, aug=None):
        """The draws of a batch as the columns buctd_sample_geometry reads: draw() per record, in record order (the same
        generator calls as the host path makes), or aug = a list of draw() results.  Returns numpy arrays: half_body
        float32 [B, 4] (center, scale of the override), draws float64 [B, 4] (scale multiplier, sin and cos of the rotation
        - evaluated here, in float64, by the calls get_dir makes - and the rotation in degrees), bbox_draws int32 [B, 2],
        flags int32 [B] (GEOM_HALF_BODY, GEOM_FLIP)."""
        B = len(records)
        draws = [self.draw(r) for r in records] if aug is None else list(aug)
        if len(draws) != B or not all(isinstance(d, dict) for d in draws):
            raise ValueError("geometry_on_device: aug is a list of draw() results, one per record (center and scale of a "
                             "(center, scale, rot, flip) tuple would replace the box the kernel forms)")
        rot = [d["rot"] for d in draws]
        hb = np.zeros((B, 4), dtype=np.float32)
        has_hb = np.array([d["half_body"] is not None for d in draws], dtype=bool)
        if has_hb.any():
            hb[has_hb] = np.array([np.concatenate(d["half_body"]) for d in draws if d["half_body"] is not None], np.float32)
        dr = np.empty((B, 4), dtype=np.float64)
        dr[:, 0] = [d["scale_mul"] for d in draws]
        dr[:, 1] = [np.sin(np.pi * r / 180) for r in rot]
        dr[:, 2] = [np.cos(np.pi * r / 180) for r in rot]
        dr[:, 3] = rot
        bd = np.array([d["bbox_aug"] if d["bbox_aug"] is not None else (0, 0) for d in draws], dtype=np.int32).reshape(B, 2)
        flags = has_hb * GEOM_HALF_BODY + np.array([bool(d["flip"]) for d in draws], dtype=bool) * GEOM_FLIP
        return dict(half_body=hb, draws=dr, bbox_draws=bd, flags=flags.astype(np.int32))

    def device_geometry(self, records, table, cond=None, cond_vis=None):
        """One upload and one buctd_sample_geometry launch for a batch.  table: draw_table(); cond: the condition poses
        [B, K, 3] in image coordinates - a float64 device tensor (buctd_synthesize_pose's output) or a host array - and
        cond_vis their visibilities (host array), both None without a condition.  Returns device tensors: items (the
        table of buctd_warp_affine_norm), joints, joints_vis, cond_joints, cond_joints_vis (float64 [B, K, 3]), cond_trunc
        (float32 [B, K, 2]), target_xy, target_vis (the inputs of buctd_gaussian_target), center (float32 [B, 2]), scale
        (float64 [B, 2]: see apply_draw), rotation (float64 [B]) and status (int32 [B])."""
        images = [r["image"] for r in records]
        _check_images(images)
        dev = images[0].device
        B, K = len(records), self.num_joints
        f32, f64, i32 = np.float32, np.float64, np.int32
        has_cond = cond is not None
        cond_on_device = has_cond and torch.is_tensor(cond)
        sections = [("joints", f64, (B, K, 3)), ("joints_vis", f64, (B, K, 3)), ("bbox", f64, (B, 4)), ("draws", f64, (B, 4)),
                    ("items", np.uint64, (B, WARP_ITEM.itemsize // 8)), ("center", f32, (B, 2)), ("scale", f32, (B, 2)),
                    ("half_body", f32, (B, 4)), ("flags", i32, (B,)), ("bbox_draws", i32, (B, 2))]
        if has_cond:
            sections.append(("cond_vis", f64, (B, K, 3)))
            if not cond_on_device:
                sections.append(("cond", f64, (B, K, 3)))
        at_in, n_in = _layout(sections)
        host = np.zeros(n_in, dtype=np.uint8)
        hv = _views(host, at_in)
        hv["joints"][:] = np.stack([np.asarray(r["joints_3d"], dtype=f64).reshape(K, 3) for r in records])
        hv["joints_vis"][:] = np.stack([np.asarray(r["joints_3d_vis"], dtype=f64).reshape(K, 3) for r in records])
        hv["center"][:] = np.stack([np.asarray(r["center"], dtype=f32).reshape(2) for r in records])
        hv["scale"][:] = np.stack([np.asarray(r["scale"], dtype=f32).reshape(2) for r in records])
        has_bbox = np.array(["bbox" in r for r in records], dtype=bool)
        if has_bbox.any():
            hv["bbox"][has_bbox] = np.array([r["bbox"] for r in records if "bbox" in r], dtype=f64).reshape(-1, 4)
        use_bu = np.array([bool(r.get("use_bu_bbox", False)) for r in records], dtype=bool)
        hv["flags"][:] = table["flags"] + has_bbox * GEOM_HAS_BBOX + use_bu * GEOM_USE_BU_BBOX
        for key in ("draws", "half_body", "bbox_draws"):
            hv[key][:] = table[key]
        if has_cond:
            hv["cond_vis"][:] = np.asarray(cond_vis, dtype=f64).reshape(B, K, 3)
            if not cond_on_device:
                hv["cond"][:] = np.asarray(cond, dtype=f64).reshape(B, K, 3)
        warp_items(images, items=hv["items"].reshape(-1).view(WARP_ITEM))
        sv = _views(torch.from_numpy(host).to(dev), at_in)
        outs = [("joints", f64, (B, K, 3)), ("joints_vis", f64, (B, K, 3)), ("scale", f64, (B, 2)), ("rotation", f64, (B,)),
                ("target_xy", f32, (B, K, 3)), ("target_vis", f32, (B, K)), ("center", f32, (B, 2)), ("status", i32, (B,))]
        if has_cond:
            outs += [("cond_joints", f64, (B, K, 3)), ("cond_joints_vis", f64, (B, K, 3)), ("cond_trunc", f32, (B, K, 2))]
        at_out, n_out = _layout(outs)
        out = _views(torch.empty(n_out, dtype=torch.uint8, device=dev), at_out)
        a = SampleGeomArgs()
        a.joints, a.joints_vis, a.center, a.scale, a.bbox = (ptr(sv[k]) for k in ("joints", "joints_vis", "center", "scale", "bbox"))
        a.half_body, a.draws, a.bbox_draws, a.flags = (ptr(sv[k]) for k in ("half_body", "draws", "bbox_draws", "flags"))
        a.pair, a.items = ptr(self.pair_table(dev)), ptr(sv["items"])
        if has_cond:
            if cond_on_device and (cond.dtype != torch.float64 or tuple(cond.shape) != (B, K, 3) or not cond.is_contiguous()):
                raise ValueError("device_geometry: cond must be a contiguous float64 [B, K, 3] tensor")
            a.cond, a.cond_vis = ptr(cond if cond_on_device else sv["cond"]), ptr(sv["cond_vis"])
            a.out_cond, a.out_cond_vis, a.cond_trunc = ptr(out["cond_joints"]), ptr(out["cond_joints_vis"]), ptr(out["cond_trunc"])
        a.out_joints, a.out_joints_vis, a.target_xy, a.target_vis = (ptr(out[k]) for k in ("joints", "joints_vis", "target_xy", "target_vis"))
        a.out_center, a.out_scale, a.out_rotation, a.status = (ptr(out[k]) for k in ("center", "scale", "rotation", "status"))
        a.B, a.K, a.crop_w, a.crop_h = B, K, int(self.image_size[0]), int(self.image_size[1])
        a.keep_rect, a.bbox_aug = int(self.is_train and self.new_augmentation), int(self.bbox_augmentation)
        a.margin, a.aspect_ratio, a.scale_thre = float(self.bu_bbox_margin), float(self.aspect_ratio), float(self.scale_thre)
        stride = self.image_size / self.heatmap_size
        a.stride_x, a.stride_y = float(stride[0]), float(stride[1])
        check(lib().buctd_sample_geometry(C.byref(a), stream_ptr()), "sample_geometry")
        out["items"] = sv["items"]
        return out

    def check(self, meta):
        """Reads meta['status'] of a geometry_on_device batch back (one copy, one wait) and raises the host path's
        ValueError for a sample without a box; batches of the host path have no status and pass."""
        status = meta.get("status")
        if status is None:
            return
        st = status.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size:
            raise ValueError("pose synthesis: a condition without a non-zero x or y coordinate has no area - " +
                             NO_BOX.format(bad=bad.tolist(), status=st[bad].tolist()))

    def synthesis_inputs(self, records):
        """Host side of JointsDataset.py:165-167 and 204-212 for a batch: ground-truth joints [B, K, 3], the conditions
        they are perturbed around and their visibilities, the neighbours [B, M, K, 3] (or None) and the areas [B]."""
        K = self.num_joints
        conds = [self.condition(r) for r in records]
        J = np.stack([np.array(r["joints_3d"], dtype=np.float64).reshape(K, 3) for r in records])
        E = np.stack([c[0].reshape(K, 3) for c in conds])
        V = np.stack([c[1].reshape(K, 3) for c in conds])
        near = pad_near_joints([r.get("near_joints", ()) for r in records], K)
        return J, E, V, near, synthesis_area(E)

    def _synthesize(self, records, seed):
        """One buctd_synthesize_pose launch for the batch: the synthesized poses (float64 [B, K, 3] on the device, image
        coordinates) and the conditions' visibilities (host).  seed None: the next of the pipeline's own seeds."""
        if seed is None:
            seed = batch_seed(self.seed, self.synth_calls)
            self.synth_calls += 1
        J, E, V, near, area = self.synthesis_inputs(records)
        synth = synthesize_pose_batch(self.dataset, J, E, near, area, np.zeros(len(records), dtype=np.int32), seed,
                                      device=records[0]["image"].device, ladders=self.synth_ladders)
        return synth, V

    @staticmethod
    def _meta(records, **tensors):
        """meta of a batch: the records' own entries around the geometry's tensors."""
        meta = {"image": [r.get("image_file", "") for r in records]}
        meta.update(tensors)
        meta["score"] = torch.tensor([float(r.get("score", 1)) for r in records])
        meta["annotation_id"] = torch.tensor([int(r.get("annotation_id", -1)) for r in records])
        return meta

    def __call__(self, records, aug=None, seed=None):
        """records: dicts with 'image' (uint8 HWC device tensor), 'joints_3d', 'joints_3d_vis', 'center', 'scale' and,
        for conditional models, 'cond_joints' / 'cond_joints_vis' (+ 'score', 'annotation_id', 'use_bu_bbox'; under
        generative sampling 'near_joints', see the class docstring).  seed: of the pose synthesis of this batch.
        Returns (input, target, target_weight, meta) like a collated DataLoader batch of the reference."""
        images = [r["image"] for r in records]
        extra, synth, V = {}, None, None
        if self.synthesizes:
            synth, V = self._synthesize(records, seed)
            extra["synth_joints"] = synth
        if self.geometry_on_device:                      # the draws on the host, everything after them on the device
            cond, cond_vis = synth, V
            if synth is None:
                conds = [self.condition(r) for r in records]
                if all(c[2] for c in conds):
                    cond, cond_vis = np.stack([c[0] for c in conds]), np.stack([c[1] for c in conds])
                elif any(c[2] for c in conds):
                    raise ValueError("geometry_on_device: either every record of a batch carries 'cond_joints' or none does")
            g = self.device_geometry(records, self.draw_table(records, aug), cond, cond_vis)
            x, target, weight = self.render(images, None, table=g["items"], cond_trunc=g.get("cond_trunc"),
                                            targets=(g["target_xy"], g["target_vis"]))
            zeros = None if cond is not None else torch.zeros_like(g["joints"])
            meta = self._meta(records, joints=g["joints"], joints_vis=g["joints_vis"],
                              cond_joints=g["cond_joints"] if zeros is None else zeros,
                              cond_joints_vis=g["cond_joints_vis"] if zeros is None else zeros,
                              center=g["center"], scale=g["scale"], rotation=g["rotation"])
            meta.update(status=g["status"], table=g["items"], **extra)
            return x, target, weight, meta
        augs = [None] * len(records) if aug is None else aug
        if synth is None:
            geos = [self.geometry(r, a) for r, a in zip(records, augs)]
            x, target, weight = self.render(images, geos)
        elif any(r.get("use_bu_bbox", False) for r in records):
            # the crop box itself comes from the synthesized pose (JointsDataset.py:218-228): host geometry
            host = synth.cpu().numpy()
            geos = [self.geometry(r, a, cond=(host[i], V[i])) for i, (r, a) in enumerate(zip(records, augs))]
            x, target, weight = self.render(images, geos)
        else:
            geos = [self.geometry(r, a, cond=False) for r, a in zip(records, augs)]
            table = self.warp_table(images, geos)
            cj, cv, cjt = self.cond_geometry(synth, torch.from_numpy(V).to(synth.device), table)
            x, target, weight = self.render(images, geos, table=table, cond_trunc=cjt)
            extra["cond_joints"], extra["cond_joints_vis"] = cj, cv
        stack = lambda key: torch.from_numpy(np.stack([g[key] for g in geos]))
        meta = self._meta(records, joints=stack("joints"), joints_vis=stack("joints_vis"), cond_joints=stack("cond_joints"),
                          cond_joints_vis=stack("cond_joints_vis"), center=stack("center"), scale=stack("scale"),
                          rotation=torch.tensor([float(g["rot"]) for g in geos]))
        meta.update(extra)
        return x, target, weight, meta


class IterativeRefiner:
    """BUCTD iterative refinement in one process (README.md:104 '3x iterative refinement'; reference = three CLI runs
    chained through the results json).  use_dark: decode every pass with get_final_preds(..., use_dark=True).

    on_device=True: only pass 0 is set up on the host; from there on the predictions, scores, boxes, crop affines and
    conditions of all passes stay on the device (buctd_refine_step between the decode kernel of one pass and the crop of
    the next) and run() waits for the device once, after the last pass.  Same return value; a person whose predictions
    have no non-zero x or y raises the host path's ValueError, after the last pass instead of in the middle.  Needs an
    eval pipeline (no augmentation draws), a conditional config and NUM_JOINTS <= 32.

    flip_test=True: every pass is the flip test of validate() (reference function.py:213-236, which each of the three CLI
    runs goes through with TEST.FLIP_TEST True): one forward over [crops | mirrored crops], the two heat-maps merged with
    ops.flipback_avg, then decoded.  shift_heatmap: the one-pixel shift of the mirrored half in that merge; None takes
    cfg.TEST.SHIFT_HEATMAP.  The keyword is explicit and off by default - cfg.TEST.FLIP_TEST is NOT read, callers of
    earlier versions keep their results bit for bit; flip_test=cfg.TEST.FLIP_TEST is the setting that equals the
    reference chain.  On the device chain the mirrored half is built on the device as well (buctd_mirror_rows,
    buctd_cond_mirror): still one upload before the loop and one copy back after it, and the model - ForwardGraph and
    Bf16Inference included - sees 2B rows."""

    def __init__(self, cfg, model, pipeline, in_vis_thre=None, use_dark=False, on_device=False, flip_test=False,
                 shift_heatmap=None):
        self.cfg, self.model, self.pipe = cfg, model, pipeline
        self.use_dark = bool(use_dark)
        self.in_vis_thre = cfg.TEST.IN_VIS_THRE if in_vis_thre is None else in_vis_thre
        self.on_device = bool(on_device)
        self.flip_test = bool(flip_test)
        self.shift_heatmap = bool(getattr(cfg.TEST, "SHIFT_HEATMAP", False) if shift_heatmap is None else shift_heatmap)
        if self.on_device:
            if pipeline.is_train:
                raise ValueError("IterativeRefiner(on_device=True) needs a pipeline built with is_train=False: the "
                                 "augmentation draws of a train pipeline are made on the host")
            if not pipeline.conditional:
                raise ValueError("IterativeRefiner(on_device=True) needs a conditional config "
                                 "(MODEL.CONDITIONAL_TOPDOWN): without a condition there is nothing to refine")
            if pipeline.num_joints > MAX_DEVICE_JOINTS:
                raise ValueError(f"IterativeRefiner(on_device=True) handles at most {MAX_DEVICE_JOINTS} joints "
                                 f"(MODEL.NUM_JOINTS is {pipeline.num_joints})")

    @staticmethod
    def rescore(maxvals, box_score, in_vis_thre):
        """dataloader.py:596-612: mean of the key-point scores above in_vis_thre, times the box score."""
        mv = maxvals[:, :, 0]
        counted = mv > in_vis_thre
        n = counted.sum(1)
        kpt_score = np.where(n > 0, (mv * counted).sum(1) / np.maximum(n, 1), 0.0)
        return kpt_score * box_score, kpt_score

    def next_records(self, records, preds, scores):
        """prediction -> condition + box of the next pass (dataloader.py:454-508, _load_coco_pose_results)."""
        out = []
        for r, kp, sc in zip(records, preds, scores):
            ih, iw = int(r["image"].shape[0]), int(r["image"].shape[1])
            cond = np.zeros((kp.shape[0], 3), dtype=np.float64)
            cond[:, :2] = kp[:, :2]
            cond[:, 2] = kp[:, 2] if kp.shape[1] > 2 else 0.0
            x, y, w, h = box_from_keypoints(cond, self.pipe.bu_bbox_margin, iw, ih)
            c, s = xywh2cs(x, y, w, h, self.pipe.aspect_ratio, self.pipe.scale_thre)
            nr = dict(r)
            nr.update(center=c, scale=s, score=float(sc), cond_joints=cond,
                      cond_joints_vis=np.ones((kp.shape[0], 3), dtype=np.float64),
                      joints_3d=np.zeros((kp.shape[0], 3), dtype=np.float64),
                      joints_3d_vis=np.ones((kp.shape[0], 3), dtype=np.float64), use_bu_bbox=False)
            out.append(nr)
        return out

    def mirrored_input(self, x, geos):
        """core.function._mirrored_input for the host chain: the pipeline stands in for the data set (image_size,
        flip_pairs, kpt_colors), the geometry's cond_joints / cond_joints_vis for the batch's meta.  A 3-channel condition
        is rendered from utils.transforms.mirror_condition, which truncates the mirrored coordinates in float64 like the
        reference's .astype(int); transforms.flip_hm rounds them to float32 first, and from the second pass on a person
        whose box has stopped moving has crop coordinates an ulp from an integer (24.999999999999996 is 24 there, 25 in
        float32 - DESIGN.md section 12).  A stacked condition goes through flip_hm: no coordinates."""
        pipe = self.pipe
        if not pipe.conditional:
            return x.flip(3)
        cj = np.stack([g["cond_joints"] for g in geos])
        cv = np.stack([g["cond_joints_vis"] for g in geos])
        if pipe.stacked:
            cond = flip_hm(x[:, 3:], pipe, torch.from_numpy(cj), torch.from_numpy(cv))
        else:
            pts = torch.from_numpy(mirror_condition(cj, cv, int(pipe.image_size[0]), pipe.flip_pairs)).to(x.device)
            cond = ops.cond_render(pts, pipe.mirror_colors(x.device), int(pipe.image_size[1]), int(pipe.image_size[0]))
        return torch.cat((x[:, :3].flip(3), cond), dim=1)

    def _forward(self, x, B):
        """The heat-maps of one pass: the model's last output for B persons.  With flip_test x is validate()'s paired
        input [crops | mirrored crops] and the two halves are merged (buctd_flipback_avg) before the decode."""
        hm = self.model(x)
        hm = (hm[-1] if isinstance(hm, list) else hm).contiguous()
        if self.flip_test:
            hm = ops.flipback_avg(hm[:B], hm[B:], self.pipe.flip_perm(hm.device), self.shift_heatmap)
        return hm

    @torch.no_grad()
    def run(self, records, passes=3):
        """Returns per pass: dict(preds [B, K, 3] image coordinates + max-val, score, box_score, keypoint_score)."""
        if self.on_device:
            return self.run_on_device(records, passes)
        self.model.eval()
        history = []
        for _ in range(passes):
            geos = [self.pipe.geometry(r) for r in records]
            x, _, _ = self.pipe.render([r["image"] for r in records], geos)
            out = self._forward(torch.cat((x, self.mirrored_input(x, geos)), dim=0) if self.flip_test else x, len(records))
            center = np.stack([g["center"] for g in geos])
            scale = np.stack([g["scale"] for g in geos])
            coords, maxvals = get_final_preds(self.cfg, out, center, scale, use_dark=self.use_dark)
            box_score = np.array([float(r.get("score", 1)) for r in records])
            score, kpt_score = self.rescore(maxvals, box_score, self.in_vis_thre)
            preds = np.concatenate([coords, maxvals], axis=2)
            history.append(dict(preds=preds, score=score, box_score=box_score, keypoint_score=kpt_score,
                                center=center, scale=scale))
            records = self.next_records(records, preds, score)
        return history

    def refine_step(self, decoded, state, table, out, p, passes, cond_joints=None):
        """One buctd_refine_step launch: decoded = (coords [B, K, 2], maxvals [B, K, 1], offsets [B, K, 2] or None) of pass
        p; state = (center, scale, box_score, cond_trunc) device tensors, overwritten with those of pass p + 1; table:
        warp_table(), its matrices overwritten; out: the views of history_layout()'s sections."""
        pipe = self.pipe
        coords, maxvals, offset = decoded
        a = RefineArgs()
        a.coords, a.maxvals, a.offset = ptr(coords), ptr(maxvals), ptr(offset)
        a.center, a.scale, a.box_score, a.cond_trunc = (ptr(t) for t in state)
        a.items, a.cond_joints, a.status = ptr(table), ptr(cond_joints), ptr(out["status"])
        a.hist_preds, a.hist_score, a.hist_box_score = ptr(out["preds"]), ptr(out["score"]), ptr(out["box_score"])
        a.hist_keypoint_score, a.hist_center, a.hist_scale = ptr(out["keypoint_score"]), ptr(out["center"]), ptr(out["scale"])
        a.B, a.K, a.pass_, a.passes = int(coords.shape[0]), int(coords.shape[1]), int(p), int(passes)
        a.heatmap_w, a.heatmap_h = int(pipe.heatmap_size[0]), int(pipe.heatmap_size[1])
        a.crop_w, a.crop_h = int(pipe.image_size[0]), int(pipe.image_size[1])
        a.margin, a.aspect_ratio = float(pipe.bu_bbox_margin), float(pipe.aspect_ratio)
        a.in_vis_thre, a.scale_thre = float(self.in_vis_thre), float(pipe.scale_thre)
        check(lib().buctd_refine_step(C.byref(a), stream_ptr()), "refine_step")

    def run_on_device(self, records, passes=3):
        """run() with on_device=True: one upload before the first pass, one copy back after the last."""
        self.model.eval()
        pipe, cfg = self.pipe, self.cfg
        B, K = len(records), pipe.num_joints
        images = [r["image"] for r in records]
        dev = images[0].device
        # pass 0 on the host, as run() does it
        geos = [pipe.geometry(r) for r in records]
        table = pipe.warp_table(images, geos)
        f32, f64 = np.float32, np.float64
        flip = self.flip_test
        sections = [("box_score", f64, (B,)), ("center", f32, (B, 2)), ("scale", f32, (B, 2)), ("cond_trunc", f32, (B, K, 2))]
        if flip:
            # the condition before trunc() - pass 0's from the host geometry, with its visibilities; buctd_refine_step
            # overwrites cond_joints with the next pass's, whose visibilities are all ones
            sections += [("cond_joints", f64, (B, K, 2)), ("cond_vis", f64, (B, K, 3))]
        at_in, n_in = _layout(sections)
        host = np.zeros(n_in, dtype=np.uint8)
        hv = _views(host, at_in)
        hv["box_score"][:] = [float(r.get("score", 1)) for r in records]
        hv["center"][:] = np.stack([g["center"] for g in geos])
        hv["scale"][:] = np.stack([g["scale"] for g in geos])
        hv["cond_trunc"][:] = trunc_condition(np.stack([g["cond_joints"] for g in geos]))
        if flip:
            hv["cond_joints"][:] = np.stack([g["cond_joints"][:, :2] for g in geos])
            hv["cond_vis"][:] = np.stack([g["cond_joints_vis"] for g in geos])
        sv = _views(torch.from_numpy(host).to(dev), at_in)
        state = (sv["center"], sv["scale"], sv["box_score"], sv["cond_trunc"])
        at_out, n_out = _layout(history_layout(passes, B, K))
        result = torch.zeros(n_out, dtype=torch.uint8, device=dev)
        out = _views(result, at_out)
        colors = pipe.condition_colors(dev)
        refine = bool(cfg.TEST.POST_PROCESS)
        for p in range(passes):
            if flip:
                x = pipe.warp_and_condition(table, sv["cond_trunc"], colors,
                                            mirrored=(sv["cond_joints"], sv["cond_vis"] if p == 0 else None))
            else:
                x = pipe.warp_and_condition(table, sv["cond_trunc"], colors)
            hm = self._forward(x, B)
            if self.use_dark:
                res = ops.dark_decode(hm)
            else:
                res = ops.argmax_decode(hm, refine=refine)
            self.refine_step((res[0], res[1], res[3] if (self.use_dark or refine) else None), state, table, out, p, passes,
                             cond_joints=sv["cond_joints"] if flip else None)
        got = _views(result.cpu().numpy(), at_out)
        bad = np.nonzero(got["status"])[0]
        if bad.size:
            raise ValueError(f"iterative refinement: person(s) {bad.tolist()} of the batch have predictions without a "
                             "non-zero x or y coordinate, or a box without extent (status "
                             f"{got['status'][bad].tolist()}): there is no box for the next pass")
        return [dict(preds=got["preds"][p].copy(), score=got["score"][p].copy(), box_score=got["box_score"][p].copy(),
                     keypoint_score=got["keypoint_score"][p].copy(), center=got["center"][p].copy(),
                     scale=got["scale"][p].copy()) for p in range(passes)]


# ---- CTD tracking: the pose of frame t - 1 is the condition of frame t -------------------------------------------------
MAX_TRACK_SLOTS = 64           # buctd_track_step: slots, and detections of one frame


def track_history_layout(T, M, K):
    """The sections of SequenceTracker's history buffer, what buctd_track_step writes per frame: for _layout()."""
    return [("score", np.float64, (T, M)), ("ids", np.int32, (T, M)), ("preds", np.float32, (T, M, K, 3)),
            ("born", np.uint8, (T, M)), ("died", np.uint8, (T, M))]


def mean_keypoint_score(pose):
    """The score a detection is ranked by at birth: its joints' scores summed in joint order, over K (float64)."""
    return np.cumsum(np.asarray(pose, dtype=np.float64)[:, 2])[-1] / pose.shape[0]


class SequenceTracker:
    """CTD tracking of persons (animals) through a frame sequence: max_tracks slots, the slot a person occupies is its
    identity, the pose found in frame t - 1 is the condition of frame t, bottom-up detections only start tracks.

    run(frames, detections): frames = T uint8 [H, W, 3] device tensors of one size; detections = per frame a bottom-up
    pose array [n_t, K, 3] (x, y, score; n_t may be 0).  Returns per frame dict(ids [M] int64 (-1 = empty slot), preds
    [M, K, 3] float32, score [M] float64, born [M] bool, died [M] bool); the rows of empty slots are zeros.  Every frame
    runs the model on exactly M rows - an empty slot carries the whole-image box and an all-zero condition - so an
    engine.ForwardGraph replays.  Per frame:

      birth  the frame's detections by descending mean_keypoint_score, equal ones by index: one whose OKS against every
             live slot's pose - the detections born before it in this frame included - is below birth_oks takes the lowest
             free slot and the next id (ids count up from 0 and are never reused); without a free slot it is dropped.  OKS =
             nms.oks_iou without a visibility threshold, areas = w * h of box_from_keypoints with the pipeline's margin,
             sigmas default nms.COCO_SIGMAS (17 joints; any other K must pass its own).
      pose   the condition of a live slot is its pose - the previous frame's prediction, or the detection it was born
             from; box, crop, condition, forward pass, decode and rescoring (box score 1) are IterativeRefiner's.
      death  a slot whose prediction has no non-zero x or no non-zero y, or a box without extent, dies at once; otherwise a
             keypoint score below death_score is a miss (else the misses reset) and the slot dies at max_misses of them in
             a row.
      merge  the surviving slots in ascending id order: one whose OKS against an older kept slot is >= merge_oks dies.
    A slot freed in frame t can be taken from frame t + 1 on; `died` marks it in frame t, where it still has its id.

    on_device=True: one upload before the first frame (state, all detections with an offsets table, the frame pointers),
    one buctd_track_step launch per frame boundary, one copy back after the last frame; the host never waits inside the
    loop.  M <= 64, K <= 32, at most 64 detections per frame.  Same return value as the host path."""

    def __init__(self, cfg, model, pipeline, max_tracks=16, birth_oks=0.3, merge_oks=0.7, death_score=0.2, max_misses=2,
                 sigmas=None, in_vis_thre=None, use_dark=False, on_device=False):
        from ..nms.nms import COCO_SIGMAS
        self.cfg, self.model, self.pipe = cfg, model, pipeline
        self.max_tracks, self.max_misses = int(max_tracks), int(max_misses)
        self.birth_oks, self.merge_oks, self.death_score = float(birth_oks), float(merge_oks), float(death_score)
        self.use_dark, self.on_device = bool(use_dark), bool(on_device)
        K = pipeline.num_joints
        if sigmas is None:
            if K != COCO_SIGMAS.shape[0]:
                raise ValueError(f"SequenceTracker: the default sigmas are COCO's {COCO_SIGMAS.shape[0]}; a config with "
                                 f"{K} joints must pass its own")
            sigmas = COCO_SIGMAS
        self.sigmas = np.ascontiguousarray(sigmas, dtype=np.float64).reshape(-1)
        if self.sigmas.shape[0] != K:
            raise ValueError(f"SequenceTracker: sigmas has {self.sigmas.shape[0]} entries, MODEL.NUM_JOINTS is {K}")
        if self.max_tracks < 1 or self.max_misses < 1:
            raise ValueError("SequenceTracker: max_tracks and max_misses must be positive")
        if pipeline.is_train or not pipeline.conditional:
            raise ValueError("SequenceTracker needs an eval pipeline (is_train=False) of a conditional config "
                             "(MODEL.CONDITIONAL_TOPDOWN): the previous pose is the condition")
        if self.on_device and (self.max_tracks > MAX_TRACK_SLOTS or K > MAX_DEVICE_JOINTS):
            raise ValueError(f"SequenceTracker(on_device=True) handles at most {MAX_TRACK_SLOTS} tracks and "
                             f"{MAX_DEVICE_JOINTS} joints (max_tracks {self.max_tracks}, MODEL.NUM_JOINTS {K})")
        self.refiner = IterativeRefiner(cfg, model, pipeline, in_vis_thre=in_vis_thre, use_dark=use_dark)
        self.in_vis_thre = self.refiner.in_vis_thre

    # ---- the pieces of the specification ----------------------------------------------------------------------------
    def pose_box(self, pose, iw, ih):
        """(x, y, w, h) of a pose's box, or None where there is none: no non-zero x, no non-zero y, or no extent (the crop
        affine of utils.transforms.crop_affine_closed_form is singular)."""
        from ..utils.transforms import crop_affine_closed_form
        pose = np.asarray(pose, dtype=np.float64)
        if not (pose[:, 0] != 0).any() or not (pose[:, 1] != 0).any():
            return None
        box = box_from_keypoints(pose, self.pipe.bu_bbox_margin, iw, ih)
        c, s = xywh2cs(*box, self.pipe.aspect_ratio, self.pipe.scale_thre)
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = np.isfinite(crop_affine_closed_form(c, s, self.pipe.image_size)).all()
        return box if ok else None

    def oks(self, pose, area, others, areas):
        """OKS of one pose against others [n, K, 3] (nms.oks_iou, every joint counts)."""
        from ..nms.nms import oks_iou
        others = np.asarray(others, dtype=np.float64)
        return oks_iou(np.asarray(pose, dtype=np.float64).reshape(-1), others.reshape(others.shape[0], -1), area,
                       np.asarray(areas, dtype=np.float64), self.sigmas)

    def _check_inputs(self, frames, detections):
        T, K = len(frames), self.pipe.num_joints
        if T == 0 or len(detections) != T:
            raise ValueError(f"SequenceTracker.run: {T} frames, {len(detections)} detection arrays")
        _check_images(frames)
        if any(f.shape != frames[0].shape or f.device != frames[0].device for f in frames):
            raise ValueError("SequenceTracker.run: the frames of a sequence have one size and one device")
        ih, iw = int(frames[0].shape[0]), int(frames[0].shape[1])
        dets = [np.asarray(d, dtype=np.float64).reshape(-1, K, 3) for d in detections]
        for t, d in enumerate(dets):
            if self.on_device and d.shape[0] > MAX_TRACK_SLOTS:
                raise ValueError(f"SequenceTracker(on_device=True): frame {t} has {d.shape[0]} detections, at most "
                                 f"{MAX_TRACK_SLOTS} per frame")
            bad = [i for i in range(d.shape[0]) if self.pose_box(d[i], iw, ih) is None]
            if bad:
                raise ValueError(f"SequenceTracker.run: detection(s) {bad} of frame {t} have no non-zero x or y coordinate, "
                                 "or a box without extent: there is no box to crop")
        return dets, iw, ih

    def _records(self, frame, ids, pose, iw, ih):
        """The M records of one frame: IterativeRefiner.next_records for the live slots, the whole-image box and an
        invisible all-zero condition for the empty ones."""
        K = self.pipe.num_joints
        base = dict(image=frame)
        c, s = xywh2cs(0, 0, iw, ih, self.pipe.aspect_ratio, self.pipe.scale_thre)
        zero = np.zeros((K, 3), dtype=np.float64)
        empty = dict(base, center=c, scale=s, score=1.0, cond_joints=zero, cond_joints_vis=zero, joints_3d=zero,
                     joints_3d_vis=np.ones((K, 3), dtype=np.float64), use_bu_bbox=False)
        live = np.nonzero(ids >= 0)[0]
        recs = [empty] * len(ids)
        for s_, r in zip(live, self.refiner.next_records([base] * len(live), pose[live], np.ones(len(live)))):
            recs[s_] = r
        return recs

    @torch.no_grad()
    def run(self, frames, detections):
        dets, iw, ih = self._check_inputs(frames, detections)
        if self.on_device:
            return self.run_on_device(frames, dets)
        self.model.eval()
        pipe, M, K = self.pipe, self.max_tracks, self.pipe.num_joints
        ids, misses, next_id = np.full(M, -1, dtype=np.int64), np.zeros(M, dtype=np.int64), 0
        pose, area = np.zeros((M, K, 3), dtype=np.float64), np.zeros(M, dtype=np.float64)
        history = []
        for frame, det in zip(frames, dets):
            # birth
            born = np.zeros(M, dtype=bool)
            means = np.array([mean_keypoint_score(d) for d in det], dtype=np.float64)
            for i in sorted(range(det.shape[0]), key=lambda i: (-means[i], i)):
                x, y, w, h = self.pose_box(det[i], iw, ih)
                live, free = np.nonzero(ids >= 0)[0], np.nonzero(ids < 0)[0]
                if live.size and self.oks(det[i], w * h, pose[live], area[live]).max() >= self.birth_oks:
                    continue
                if free.size:
                    s = free[0]
                    ids[s], misses[s], pose[s], area[s], born[s] = next_id, 0, det[i], w * h, True
                    next_id += 1
            # pose
            recs = self._records(frame, ids, pose, iw, ih)
            geos = [pipe.geometry(r) for r in recs]
            x, _, _ = pipe.render([frame] * M, geos)
            hm = self.refiner._forward(x, M)
            center, scale = np.stack([g["center"] for g in geos]), np.stack([g["scale"] for g in geos])
            coords, maxvals = get_final_preds(self.cfg, hm, center, scale, use_dark=self.use_dark)
            score, _ = IterativeRefiner.rescore(maxvals, np.ones(M), self.in_vis_thre)
            preds = np.concatenate([coords, maxvals], axis=2).astype(np.float32)
            was = ids >= 0
            preds[~was], score = 0, np.where(was, score, 0.0).astype(np.float64)
            out = dict(ids=ids.copy(), preds=preds, score=score, born=born, died=np.zeros(M, dtype=bool))
            # death
            for s in np.nonzero(was)[0]:
                pose[s] = preds[s]
                box = self.pose_box(pose[s], iw, ih)
                if box is not None:
                    area[s] = box[2] * box[3]
                    misses[s] = misses[s] + 1 if score[s] < self.death_score else 0
                if box is None or misses[s] >= self.max_misses:
                    out["died"][s] = True
            # merge
            kept = []
            for s in sorted(np.nonzero(was & ~out["died"])[0], key=lambda s: ids[s]):
                if kept and self.oks(pose[s], area[s], pose[kept], area[kept]).max() >= self.merge_oks:
                    out["died"][s] = True
                else:
                    kept.append(s)
            ids[out["died"]], misses[out["died"]] = -1, 0
            history.append(out)
        return history

    # ---- the device loop ----------------------------------------------------------------------------------------------
    def track_step(self, decoded, sv, out, frame, frames, max_dets):
        """One buctd_track_step launch: decoded = (coords [M, K, 2], maxvals [M, K, 1], offsets [M, K, 2] or None) of
        frame `frame`, None for frame = -1; sv: the views of the state upload; out: those of track_history_layout()."""
        pipe = self.pipe
        a = TrackArgs()
        if decoded is not None:
            a.coords, a.maxvals, a.offset = (ptr(t) for t in decoded)
        for k in ("ids", "misses", "next_id", "pose", "center", "scale", "items", "cond_trunc", "dets", "det_offsets",
                  "frame_src", "sigmas"):
            setattr(a, k, ptr(sv[k]))
        a.hist_ids, a.hist_preds, a.hist_score = ptr(out["ids"]), ptr(out["preds"]), ptr(out["score"])
        a.hist_born, a.hist_died = ptr(out["born"]), ptr(out["died"])
        a.M, a.K, a.frame, a.frames = self.max_tracks, pipe.num_joints, int(frame), int(frames)
        a.max_dets, a.max_misses = int(max_dets), self.max_misses
        a.heatmap_w, a.heatmap_h = int(pipe.heatmap_size[0]), int(pipe.heatmap_size[1])
        a.crop_w, a.crop_h = int(pipe.image_size[0]), int(pipe.image_size[1])
        a.margin, a.aspect_ratio = float(pipe.bu_bbox_margin), float(pipe.aspect_ratio)
        a.in_vis_thre, a.scale_thre = float(self.in_vis_thre), float(pipe.scale_thre)
        a.birth_oks, a.merge_oks, a.death_score = self.birth_oks, self.merge_oks, self.death_score
        check(lib().buctd_track_step(C.byref(a), stream_ptr()), "track_step")

    @staticmethod
    def state_layout(T, M, K, n_dets):
        """The sections of the one upload: the slots' state (all empty), the packed detections, the frame pointers."""
        f32, f64, i32 = np.float32, np.float64, np.int32
        return [("pose", f64, (M, K, 3)), ("dets", f64, (max(n_dets, 1), K, 3)), ("sigmas", f64, (K,)),
                ("frame_src", np.uint64, (T,)), ("items", np.uint64, (M, WARP_ITEM.itemsize // 8)), ("center", f32, (M, 2)),
                ("scale", f32, (M, 2)), ("cond_trunc", f32, (M, K, 2)), ("ids", i32, (M,)), ("misses", i32, (M,)),
                ("next_id", i32, (1,)), ("det_offsets", i32, (T + 1,))]

    def run_on_device(self, frames, dets):
        """run() with on_device=True: one upload before the first frame, one copy back after the last."""
        self.model.eval()
        pipe, cfg = self.pipe, self.cfg
        T, M, K = len(frames), self.max_tracks, pipe.num_joints
        dev = frames[0].device
        counts = [d.shape[0] for d in dets]
        at_in, n_in = _layout(self.state_layout(T, M, K, sum(counts)))
        host = np.zeros(n_in, dtype=np.uint8)
        hv = _views(host, at_in)
        hv["ids"][:] = -1
        hv["sigmas"][:] = self.sigmas
        hv["det_offsets"][:] = np.concatenate([[0], np.cumsum(counts)])
        if sum(counts):
            hv["dets"][:sum(counts)] = np.concatenate(dets)
        hv["frame_src"][:] = [f.data_ptr() for f in frames]
        warp_items([frames[0]] * M, items=hv["items"].reshape(-1).view(WARP_ITEM))
        sv = _views(torch.from_numpy(host).to(dev), at_in)
        at_out, n_out = _layout(track_history_layout(T, M, K))
        result = torch.zeros(n_out, dtype=torch.uint8, device=dev)
        out = _views(result, at_out)
        colors = pipe.condition_colors(dev)
        refine = bool(cfg.TEST.POST_PROCESS)
        max_dets = max(counts)
        self.track_step(None, sv, out, -1, T, max_dets)                   # the birth of frame 0
        for t in range(T):
            x = pipe.warp_and_condition(sv["items"], sv["cond_trunc"], colors)
            hm = self.refiner._forward(x, M)
            res = ops.dark_decode(hm) if self.use_dark else ops.argmax_decode(hm, refine=refine)
            self.track_step((res[0], res[1], res[3] if (self.use_dark or refine) else None), sv, out, t, T, max_dets)
        got = _views(result.cpu().numpy(), at_out)
        return [dict(ids=got["ids"][t].astype(np.int64), preds=got["preds"][t].copy(), score=got["score"][t].copy(),
                     born=got["born"][t].astype(bool), died=got["died"][t].astype(bool)) for t in range(T)]
