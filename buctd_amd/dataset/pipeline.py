"""GPU-side sample pipeline and in-process iterative refinement.

DeviceSamplePipeline does what the DataLoader workers of the reference do per sample in
lib/dataset/JointsDataset.py:134-361 - box -> (half-body / scale / rotation / flip augmentation) -> affine crop ->
ToTensor/Normalize -> key points into crop coordinates -> Gaussian target + condition heat-map - for a whole batch:
the scalar geometry (a few dozen float64 operations per person, the same expressions as the reference) stays on the host,
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
from .._C import RefineArgs, check, lib, ptr, stream_ptr
from ..core.inference import get_final_preds
from ..utils.transforms import _swap_table, affine_transform, fliplr_joints, get_affine_transform
from .pose_synthesis import synthesize_pose_batch

_M64 = (1 << 64) - 1
NO_CONDITION = ("Training with empirical sampling is not possible without providing 'cond_kpts'; "
                "please train with generative sampling (DATASET.SYNTHESIS_POSE=True)")


class _WarpItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("flip", C.c_int), ("rx", C.c_int),
                ("ry", C.c_int), ("rw", C.c_int), ("rh", C.c_int), ("m", C.c_double * 6)]


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
    (fish, marmosets, multimouse, a custom data set; pose_synthesis.py:798-816).

    joints_weight ([K] or [K, 1], the data set class's self.joints_weight): with cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT
    every target_weight is multiplied by it on the device (JointsDataset.py:450-451); without the flag, or with None,
    it is not looked at."""

    def __init__(self, cfg, flip_pairs=(), upper_body_ids=(), kpt_colors=None, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), is_train=False, seed=0, joints_weight=None):
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
        self._pair_dev = {}
        self.joints_weight = None
        if joints_weight is not None and bool(getattr(getattr(cfg, "LOSS", None), "USE_DIFFERENT_JOINTS_WEIGHT", False)):
            jw = np.asarray(joints_weight, dtype=np.float32)
            if jw.shape not in ((self.num_joints,), (self.num_joints, 1)):
                raise ValueError(f"joints_weight has shape {jw.shape}, MODEL.NUM_JOINTS is {self.num_joints}")
            self.joints_weight = np.ascontiguousarray(jw.reshape(1, self.num_joints, 1))
        self._weight_dev = {}

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

    def draw_augmentation(self, rec, center, scale):
        """The random part of JointsDataset.py:233-251 (same draws in the same order): returns center, scale, rot, flip."""
        rot, flip = 0, False
        if not self.is_train:
            return center, scale, rot, flip
        if np.sum(rec["joints_3d_vis"][:, 0]) > self.num_joints_half_body and self.np_rng.rand() < self.prob_half_body:
            c_hb, s_hb = self.half_body_transform(rec["joints_3d"], rec["joints_3d_vis"])
            if c_hb is not None and s_hb is not None:
                center, scale = c_hb, s_hb
        sf, rf = self.scale_factor, self.rotation_factor
        scale = scale * np.clip(self.np_rng.randn() * sf + 1, 1 - sf, 1 + sf)
        rot = np.clip(self.np_rng.randn() * rf, -rf * 2, rf * 2) if self.py_rng.random() <= 0.6 else 0
        flip = self.flip and self.py_rng.random() <= 0.5
        return center, scale, rot, flip

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
        cond = (cond_joints, cond_joints_vis) replaces the record's condition (a synthesized pose); cond = False leaves
        the condition out (it is transformed on the device): cond_joints / cond_joints_vis come back as zeros."""
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
            x, y, w, h = box_from_keypoints(cj, self.bu_bbox_margin, iw, ih)
            center, scale = xywh2cs(x, y, w, h, self.aspect_ratio, self.scale_thre)
        else:
            center = np.array(rec["center"], dtype=np.float32).copy()
            scale = np.array(rec["scale"], dtype=np.float32).copy()
        if aug is None:
            center, scale, rot, flip = self.draw_augmentation(rec, center, scale)
        else:
            center, scale, rot, flip = np.array(aug[0], np.float32).copy(), np.array(aug[1], np.float32), aug[2], aug[3]
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
                    joints_vis=joints_vis, cond_joints=cj, cond_joints_vis=cv)

    # ---- batched device work -----------------------------------------------------------------------------------
    def warp_table(self, images, geos):
        """The per-sample table of the device kernels (buctd_warp_item: source image, flip, keep-rectangle, crop affine)
        as a uint8 device tensor."""
        B = len(images)
        items = (_WarpItem * B)()
        for b, (img, g) in enumerate(zip(images, geos)):
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous() or not img.is_cuda:
                raise ValueError("images must be contiguous uint8 [H, W, 3] device tensors")
            items[b].src, items[b].H, items[b].W = img.data_ptr(), int(img.shape[0]), int(img.shape[1])
            items[b].flip = int(g["flip"])
            rect = g.get("keep_rect")
            items[b].rx, items[b].ry, items[b].rw, items[b].rh = (int(v) for v in rect) if rect is not None else (0, 0, 0, 0)
            for k, v in enumerate(np.asarray(g["trans"], dtype=np.float64).reshape(6)):
                items[b].m[k] = float(v)
        return torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(images[0].device)

    def cond_geometry(self, synth, cond_vis, table):
        """Flip + crop affine of device-resident condition poses (buctd_cond_geometry).  synth, cond_vis: float64 device
        tensors [B, K, 3]; table: warp_table().  Returns cond_joints, cond_joints_vis (float64) and the truncated
        coordinates float32 [B, K, 2] that render(cond_trunc=...) takes - all on the device."""
        dev = synth.device
        B, K = int(synth.shape[0]), int(synth.shape[1])
        pair = self._pair_dev.get(dev)
        if pair is None:
            swap = _swap_table(K, self.flip_pairs)
            pair = torch.from_numpy(np.where(swap == np.arange(K), -1, swap).astype(np.int32)).to(dev)
            self._pair_dev[dev] = pair
        cj, cv = torch.empty_like(synth), torch.empty_like(cond_vis)
        cjt = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        check(lib().buctd_cond_geometry(ptr(synth), ptr(cond_vis), ptr(table), ptr(pair), B, K, ptr(cj), ptr(cv), ptr(cjt),
                                        stream_ptr()), "cond_geometry")
        return cj, cv, cjt

    def render(self, images, geos, want_crop=False, table=None, cond_trunc=None):
        """images: uint8 HWC device tensors; geos: geometry() results.  Returns input [B, 3(+3), H, W], target
        [B, K, h, w], target_weight [B, K, 1] (+ the uint8 crops) on the device.  table: warp_table(images, geos) if the
        caller built it already; cond_trunc: the condition coordinates as cond_geometry() returns them, instead of
        geos[.]['cond_joints']."""
        dev = images[0].device
        B, K = len(images), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        cc = (K if self.stacked else 3) if self.conditional else 0      # stacked: one condition channel per joint
        x = torch.empty((B, 3 + cc, H, W), dtype=torch.float32, device=dev)
        if table is None:
            table = self.warp_table(images, geos)
        crop = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if want_crop else None
        mean = (C.c_float * 3)(*self.mean.tolist())
        std = (C.c_float * 3)(*self.std.tolist())
        check(lib().buctd_warp_affine_norm(ptr(table), B, H, W, mean, std, ptr(x), x.stride(0), ptr(crop), stream_ptr()),
              "warp_affine_norm")
        # Gaussian targets: the heat-map centre mu = int(j / stride + 0.5) is evaluated here in float64 exactly like the
        # reference (JointsDataset.py:417-418).  The kernel recomputes (int)(v / stride + 0.5f), truncating toward zero as
        # well, so it is handed a v that maps back to the same mu: mu * stride for mu >= 0 and (mu - 1) * stride for mu < 0
        # (v / stride + 0.5 = mu - 0.5 truncates to mu; mu * stride would give mu + 0.5 -> mu + 1 for negative centres:
        # visible joints left of / above the crop would get a shifted Gaussian and a shifted target_weight cut-off)
        stride = self.image_size / self.heatmap_size
        jt = target_centres(np.stack([g["joints"] for g in geos]), stride)
        vis = np.stack([g["joints_vis"][:, 0] for g in geos]).astype(np.float32)
        target, weight = ops.gaussian_target(torch.from_numpy(jt).to(dev), torch.from_numpy(vis).to(dev),
                                             self.heatmap_size, self.image_size, self.sigma)
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

    def condition_colors(self, dev):
        """The colour table of a colored condition on the device (None for mono / stacked): a fresh upload per call."""
        if not self.colored:
            return None
        return torch.from_numpy(np.ascontiguousarray(self.kpt_colors[:self.num_joints])).to(dev)

    def render_condition(self, x, cjt, colors=None):
        """Condition heat-map of truncated crop coordinates cjt (float32 [B, K, 2], device) into channels [3, 3 + Cc) of the
        network input x.  colors: condition_colors() if the caller uploaded it already."""
        dev = x.device
        B, K = int(x.shape[0]), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        if colors is None:
            colors = self.condition_colors(dev)
        ws = ops.workspace(lib().buctd_cond_render_workspace(B * K if self.stacked else B, 3, H, W), dev)
        if self.stacked:
            # get_stacked_condition (JointsDataset.py:471-498): every joint is its own single-impulse image, blurred
            # and peak-normalised on its own - B * K one-joint "images" of one channel for the render kernel
            tmp = torch.empty((B * K, 1, H, W), dtype=torch.float32, device=dev)
            check(lib().buctd_cond_render_into(ptr(cjt), 2, None, B * K, 1, 1, H, W, 0, ptr(tmp), tmp.stride(0), ptr(ws),
                                               ws.numel(), stream_ptr()), "cond_render_into")
            x[:, 3:] = tmp.view(B, K, H, W)
        elif self.colored:
            check(lib().buctd_cond_render_into(ptr(cjt), 2, ptr(colors), B, K, 3, H, W, 0,
                                               C.c_void_p(x[:, 3:].data_ptr()), x.stride(0), ptr(ws), ws.numel(),
                                               stream_ptr()), "cond_render_into")
        else:
            # mono: the one blurred, int-truncated channel replicated x3 (JointsDataset.py:513-514)
            for c in range(3):
                check(lib().buctd_cond_render_into(ptr(cjt), 2, None, B, K, 1, H, W, 1,
                                                   C.c_void_p(x[:, 3 + c:].data_ptr()), x.stride(0), ptr(ws),
                                                   ws.numel(), stream_ptr()), "cond_render_into")

    def warp_and_condition(self, table, cond_trunc, colors=None):
        """Network input [B, 3 + Cc, H, W] from a device-resident warp_table() and truncated condition coordinates
        (float32 [B, K, 2], device): render() without the Gaussian targets and without any host array - the two kernels an
        inference pass needs.  Nothing is uploaded when colors (condition_colors()) is handed in."""
        if not self.conditional:
            raise ValueError("warp_and_condition renders a condition: MODEL.CONDITIONAL_TOPDOWN is off")
        dev = table.device
        B, K = int(cond_trunc.shape[0]), self.num_joints
        W, H = int(self.image_size[0]), int(self.image_size[1])
        x = torch.empty((B, 3 + (K if self.stacked else 3), H, W), dtype=torch.float32, device=dev)
        mean = (C.c_float * 3)(*self.mean.tolist())
        std = (C.c_float * 3)(*self.std.tolist())
        check(lib().buctd_warp_affine_norm(ptr(table), B, H, W, mean, std, ptr(x), x.stride(0), None, stream_ptr()),
              "warp_affine_norm")
        self.render_condition(x, cond_trunc, colors)
        return x

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

    def __call__(self, records, aug=None, seed=None):
        """records: dicts with 'image' (uint8 HWC device tensor), 'joints_3d', 'joints_3d_vis', 'center', 'scale' and,
        for conditional models, 'cond_joints' / 'cond_joints_vis' (+ 'score', 'annotation_id', 'use_bu_bbox'; under
        generative sampling 'near_joints', see the class docstring).  seed: of the pose synthesis of this batch.
        Returns (input, target, target_weight, meta) like a collated DataLoader batch of the reference."""
        images = [r["image"] for r in records]
        extra = {}
        if self.synthesizes:
            if seed is None:
                seed = batch_seed(self.seed, self.synth_calls)
                self.synth_calls += 1
            J, E, V, near, area = self.synthesis_inputs(records)
            synth = synthesize_pose_batch(self.dataset, J, E, near, area, np.zeros(len(records), dtype=np.int32), seed,
                                          device=images[0].device)
            extra["synth_joints"] = synth
            if any(r.get("use_bu_bbox", False) for r in records):
                # the crop box itself comes from the synthesized pose (JointsDataset.py:218-228): host geometry
                host = synth.cpu().numpy()
                geos = [self.geometry(r, None if aug is None else aug[i], cond=(host[i], V[i]))
                        for i, r in enumerate(records)]
                x, target, weight = self.render(images, geos)
            else:
                geos = [self.geometry(r, None if aug is None else aug[i], cond=False) for i, r in enumerate(records)]
                table = self.warp_table(images, geos)
                cj, cv, cjt = self.cond_geometry(synth, torch.from_numpy(V).to(synth.device), table)
                x, target, weight = self.render(images, geos, table=table, cond_trunc=cjt)
                extra["cond_joints"], extra["cond_joints_vis"] = cj, cv
        else:
            geos = [self.geometry(r, None if aug is None else aug[i]) for i, r in enumerate(records)]
            x, target, weight = self.render(images, geos)
        meta = {
            "image": [r.get("image_file", "") for r in records],
            "joints": torch.from_numpy(np.stack([g["joints"] for g in geos])),
            "joints_vis": torch.from_numpy(np.stack([g["joints_vis"] for g in geos])),
            "cond_joints": torch.from_numpy(np.stack([g["cond_joints"] for g in geos])),
            "cond_joints_vis": torch.from_numpy(np.stack([g["cond_joints_vis"] for g in geos])),
            "center": torch.from_numpy(np.stack([g["center"] for g in geos])),
            "scale": torch.from_numpy(np.stack([g["scale"] for g in geos])),
            "rotation": torch.tensor([float(g["rot"]) for g in geos]),
            "score": torch.tensor([float(r.get("score", 1)) for r in records]),
            "annotation_id": torch.tensor([int(r.get("annotation_id", -1)) for r in records]),
        }
        meta.update(extra)
        return x, target, weight, meta


class IterativeRefiner:
    """BUCTD iterative refinement in one process (README.md:104 '3x iterative refinement'; reference = three CLI runs
    chained through the results json).  use_dark: decode every pass with get_final_preds(..., use_dark=True).

    on_device=True: only pass 0 is set up on the host; from there on the predictions, scores, boxes, crop affines and
    conditions of all passes stay on the device (buctd_refine_step between the decode kernel of one pass and the crop of
    the next) and run() waits for the device once, after the last pass.  Same return value; a person whose predictions
    have no non-zero x or y raises the host path's ValueError, after the last pass instead of in the middle.  Needs an
    eval pipeline (no augmentation draws), a conditional config and NUM_JOINTS <= 32."""

    MAX_DEVICE_JOINTS = 32     # buctd_refine_step: one lane per joint, as buctd_cond_geometry

    def __init__(self, cfg, model, pipeline, in_vis_thre=None, use_dark=False, on_device=False):
        self.cfg, self.model, self.pipe = cfg, model, pipeline
        self.use_dark = bool(use_dark)
        self.in_vis_thre = cfg.TEST.IN_VIS_THRE if in_vis_thre is None else in_vis_thre
        self.on_device = bool(on_device)
        if self.on_device:
            if pipeline.is_train:
                raise ValueError("IterativeRefiner(on_device=True) needs a pipeline built with is_train=False: the "
                                 "augmentation draws of a train pipeline are made on the host")
            if not pipeline.conditional:
                raise ValueError("IterativeRefiner(on_device=True) needs a conditional config "
                                 "(MODEL.CONDITIONAL_TOPDOWN): without a condition there is nothing to refine")
            if pipeline.num_joints > self.MAX_DEVICE_JOINTS:
                raise ValueError(f"IterativeRefiner(on_device=True) handles at most {self.MAX_DEVICE_JOINTS} joints "
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
            out = self.model(x)
            out = out[-1] if isinstance(out, list) else out
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
        warp_table(), its matrices overwritten; out: the history sections of _layout()."""
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

    @staticmethod
    def _layout(sections):
        """[(name, numpy dtype, shape)] -> ({name: (byte offset, dtype, shape)}, total bytes); widest items first, so every
        section is aligned to its item size."""
        at, off = {}, 0
        for name, dt, shape in sorted(sections, key=lambda t: -np.dtype(t[1]).itemsize):
            at[name] = (off, np.dtype(dt), tuple(shape))
            off += int(np.prod(shape)) * np.dtype(dt).itemsize
        return at, off

    @staticmethod
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
        at_in, n_in = self._layout([("box_score", f64, (B,)), ("center", f32, (B, 2)), ("scale", f32, (B, 2)),
                                    ("cond_trunc", f32, (B, K, 2))])
        host = np.zeros(n_in, dtype=np.uint8)
        hv = self._views(host, at_in)
        hv["box_score"][:] = [float(r.get("score", 1)) for r in records]
        hv["center"][:] = np.stack([g["center"] for g in geos])
        hv["scale"][:] = np.stack([g["scale"] for g in geos])
        hv["cond_trunc"][:] = trunc_condition(np.stack([g["cond_joints"] for g in geos]))
        sv = self._views(torch.from_numpy(host).to(dev), at_in)
        state = (sv["center"], sv["scale"], sv["box_score"], sv["cond_trunc"])
        at_out, n_out = self._layout([("score", f64, (passes, B)), ("box_score", f64, (passes, B)),
                                      ("keypoint_score", f64, (passes, B)), ("preds", f32, (passes, B, K, 3)),
                                      ("center", f32, (passes, B, 2)), ("scale", f32, (passes, B, 2)),
                                      ("status", np.int32, (B,))])
        result = torch.zeros(n_out, dtype=torch.uint8, device=dev)
        out = self._views(result, at_out)
        colors = pipe.condition_colors(dev)
        refine = bool(cfg.TEST.POST_PROCESS)
        for p in range(passes):
            x = pipe.warp_and_condition(table, sv["cond_trunc"], colors)
            hm = self.model(x)
            hm = (hm[-1] if isinstance(hm, list) else hm).contiguous()
            if self.use_dark:
                res = ops.dark_decode(hm)
            else:
                res = ops.argmax_decode(hm, refine=refine)
            self.refine_step((res[0], res[1], res[3] if (self.use_dark or refine) else None), state, table, out, p, passes)
        got = self._views(result.cpu().numpy(), at_out)
        bad = np.nonzero(got["status"])[0]
        if bad.size:
            raise ValueError(f"iterative refinement: person(s) {bad.tolist()} of the batch have predictions without a "
                             "non-zero x or y coordinate, or a box without extent (status "
                             f"{got['status'][bad].tolist()}): there is no box for the next pass")
        return [dict(preds=got["preds"][p].copy(), score=got["score"][p].copy(), box_score=got["box_score"][p].copy(),
                     keypoint_score=got["keypoint_score"][p].copy(), center=got["center"][p].copy(),
                     scale=got["scale"][p].copy()) for p in range(passes)]
