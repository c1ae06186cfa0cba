"""Fixtures of the device-side refinement tests (test_refine_closed_form.py on the CPU, test_gpu_refine_step.py and
test_gpu_refine_chain.py on the GPU): seeded decode outputs with the edge cases of buctd_refine_step, what the host
functions make of them, records in the form of tests/test_sample_pipeline.py, and a smooth stand-in network."""
import functools

import numpy as np
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EXTRA_COLORS = [[200, 200, 30], [30, 200, 200], [200, 30, 200]]        # rows 14-16 of a 17-joint colour table
CROP, HEATMAP = (64, 96), (16, 24)                                     # (w, h)
MARGIN, SCALE_THRE, IN_VIS_THRE = 25, 1.25, 0.2
TRUNC_CAP = 0.02              # share of a case's joints that may sit within 1e-6 of an integer (not compared truncated)
KERNEL_SEEDS = {14: 3, 17: 4}  # checked in test_refine_closed_form.py: the host values alone stay inside TRUNC_CAP


def cfg_for(k=14, mode="colored", conditional=True):
    from oracle import cfg as ocfg
    c = ocfg.hrnet_cfg(16, k, CROP, "pose_hrnet_coam" if conditional else "pose_hrnet", use_attention=conditional,
                       colored=mode == "colored", stacked=mode == "stacked", stage_modules=(1, 1, 1))
    c.DATASET.update({"BU_BBOX_MARGIN": MARGIN, "FLIP": False})
    c.TEST.update({"SCALE_THRE": SCALE_THRE, "IN_VIS_THRE": IN_VIS_THRE})
    return c


def pipe_for(k=14, mode="colored", is_train=False, cfg=None):
    from oracle import core as oc
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    colors = oc.CROWDPOSE_KPT_COLORS + EXTRA_COLORS
    pairs = oc.CROWDPOSE_FLIP_PAIRS if k == 14 else []
    return DeviceSamplePipeline(cfg or cfg_for(k, mode), pairs, range(8), colors, MEAN, STD, is_train=is_train)


def records(n, seed, k=14):
    """_records of tests/test_sample_pipeline.py"""
    from oracle import sample as S
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(n):
        h, w = int(rng.randint(90, 200)), int(rng.randint(100, 260))
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        joints = np.zeros((k, 3))
        joints[:, 0], joints[:, 1] = rng.rand(k) * (w - 20) + 10, rng.rand(k) * (h - 20) + 10
        vis = np.repeat((rng.rand(k, 1) > 0.2).astype(float), 3, 1)
        vis[:, 2] = 0
        cond = joints.copy()
        cond[:, :2] += rng.randn(k, 2) * 3
        x, y, bw, bh = S.box_from_keypoints(joints, 10, w, h)
        c, s = S.xywh2cs(x, y, bw, bh, 64 / 96, 1.25)
        recs.append({"image_np": img, "joints_3d": joints, "joints_3d_vis": vis, "cond_joints": cond,
                     "cond_joints_vis": np.ones((k, 3)), "center": c, "scale": s, "score": 0.5 + 0.1 * i,
                     "annotation_id": 100 + i})
    return recs


def on_device(recs, dev):
    return [dict(r, image=torch.from_numpy(r["image_np"]).to(dev)) for r in recs]


def near_integer(xy):
    """[..., 2] -> [...]: a coordinate within 1e-6 of an integer (the convention of tests/test_gpu_synth_pipeline.py)"""
    return (np.abs(xy - np.rint(xy)) <= 1e-6).any(axis=-1)


# ---- the kernel's fixture ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_case(K, B, with_offset):
    """Decode outputs of five persons (B = 1: the last one alone) in a 16 x 24 heat-map:
      0  a wide pose (xywh2cs: w > aspect * h), maxvals straddling IN_VIS_THRE
      1  a tall pose (w < aspect * h)
      2  a crop much larger than its 120 x 90 image: the box is clipped at all four borders
      3  every maxval below IN_VIS_THRE: score 0
      4  center (25, 75), scale 0.5: heat-map x = 4 is image x = 0 and heat-map y = 0 is image y = 0, exactly
         (6.25 * 4 - 25 and 6.25 * 0 + 0 with 6.25 = 50 / 8); joint 2 sits at x = 0 and joint 5 at y = 0, every other
         joint more than the margin to their right / below, so either would move the box's edge to 0 if it were counted
    Returns the inputs, the host's predictions and expected_from(preds): everything after the predictions from the host
    functions, for the float32 predictions it is given."""
    from buctd_amd.dataset.pipeline import box_from_keypoints, xywh2cs
    from buctd_amd.utils.transforms import affine_transform, get_affine_transform, transform_preds
    rng = np.random.RandomState(KERNEL_SEEDS[K])
    n = 5
    sizes = [(230, 180), (200, 190), (120, 90), (250, 170), (200, 150)]                      # image (W, H)
    center = np.array([[110.3, 90.7], [95.1, 99.2], [61.7, 44.9], [130.0, 80.5], [25.0, 75.0]], dtype=np.float32)
    scale = np.array([[0.9, 1.35], [0.8, 1.2], [1.6, 2.4], [0.7, 1.05], [0.5, 0.75]], dtype=np.float32)
    coords = np.zeros((n, K, 2), dtype=np.float32)
    coords[:, :, 0], coords[:, :, 1] = rng.randint(1, 15, (n, K)), rng.randint(1, 23, (n, K))
    coords[0, :, 1] = rng.choice([10, 12, 13], K)            # wide; no joint half-way: that is the crop's centre row, 48
    coords[0, :4] = [[1, 10], [14, 13], [3, 12], [11, 10]]
    coords[1, :, 0] = rng.randint(7, 9, K)                   # tall
    coords[1, :2, 1] = [1, 22]
    coords[2, :4] = [[0, 3], [15, 7], [6, 0], [9, 23]]       # beyond every border of the small image
    coords[4, :, 0], coords[4, :, 1] = rng.randint(9, 15, K), rng.randint(5, 23, K)   # beyond the margin of 25 px
    coords[4, 2, 0] = 4                                      # image x = 0
    coords[4, 5, 1] = 0                                      # image y = 0
    maxvals = (0.25 + 0.7 * rng.rand(n, K, 1)).astype(np.float32)
    thr = np.float32(IN_VIS_THRE)
    maxvals[0, :4, 0] = [np.nextafter(thr, np.float32(0)), thr, np.nextafter(thr, np.float32(1)), 0.05]
    maxvals[3, :, 0] = (0.19 * rng.rand(K)).astype(np.float32)
    maxvals[3, 0, 0] = thr                                   # at the threshold: still not counted
    offset = None
    if with_offset:
        offset = np.where(rng.rand(n, K, 2) < 0.5, rng.choice([-0.25, 0.0, 0.25], (n, K, 2)),
                          rng.randn(n, K, 2) * 0.3).astype(np.float32)      # quarter-pixel steps and DARK-like ones
        offset[4] = np.abs(offset[4])                        # the zero joints stay the extreme ones
        offset[4, 2, 0] = offset[4, 5, 1] = 0.0
    box_score = np.array([0.5, 0.6, 0.7, 0.8, 0.9])
    if B == 1:
        pick = slice(4, 5)
        sizes, center, scale, coords, maxvals, box_score = sizes[4:], center[pick], scale[pick], coords[pick], maxvals[pick], box_score[pick]
        offset = None if offset is None else offset[pick]
    elif B != 5:
        raise ValueError("B is 1 or 5")
    final = coords if offset is None else coords + offset    # float32, DeferredFinalPreds.final_preds
    host64 = np.stack([transform_preds(final[b], center[b], scale[b], list(HEATMAP)) for b in range(B)])[:, :, :2]
    host_preds = host64.astype(np.float32)
    aspect = CROP[0] * 1.0 / CROP[1]

    def expected_from(preds):
        boxes, centers, scales, mats, conds, branch = [], [], [], [], [], []
        for b in range(B):
            cond = np.zeros((K, 3), dtype=np.float64)
            cond[:, :2] = preds[b]
            x, y, w, h = box_from_keypoints(cond, MARGIN, sizes[b][0], sizes[b][1])
            c, s = xywh2cs(x, y, w, h, aspect, SCALE_THRE)
            t = get_affine_transform(c, s, 0, np.array(CROP))
            boxes.append((x, y, w, h)); centers.append(c); scales.append(s); mats.append(t)
            conds.append(np.stack([affine_transform(cond[k, :2], t) for k in range(K)]))
            branch.append("wide" if w > aspect * h else "tall" if w < aspect * h else "equal")
        return dict(box=boxes, center=np.stack(centers), scale=np.stack(scales), mats=np.stack(mats), cond=np.stack(conds),
                    branch=branch)

    return dict(sizes=sizes, center=center, scale=scale, coords=coords, maxvals=maxvals, offset=offset, box_score=box_score,
                host64=host64, host_preds=host_preds, expected_from=expected_from)


def degenerate_case(K):
    """kernel_case(K, 5, False) with person 4's joints all at heat-map x = 4: every image x is exactly 0."""
    case = dict(kernel_case(K, 5, False))
    coords = case["coords"].copy()
    coords[4, :, 0] = 4
    case["coords"] = coords
    return case


# ---- a smooth stand-in network ----------------------------------------------------------------------------------------
class FixedPeaks(torch.nn.Module):
    """Returns, whatever its input, heat-maps with one Gaussian (sigma 2, peak `peak`) per person and joint at a fixed table
    of heat-map positions [B, K, 2]: every pass's predictions are those positions seen through that pass's box."""

    def __init__(self, positions, peak=0.8):
        super().__init__()
        pos = torch.as_tensor(np.asarray(positions), dtype=torch.float64)
        ys = torch.arange(HEATMAP[1], dtype=torch.float64).view(1, 1, -1, 1)
        xs = torch.arange(HEATMAP[0], dtype=torch.float64).view(1, 1, 1, -1)
        d2 = (xs - pos[:, :, 0, None, None]) ** 2 + (ys - pos[:, :, 1, None, None]) ** 2
        self.register_buffer("maps", (peak * torch.exp(-d2 / (2 * 2.0 ** 2))).float())
        self.calls = 0

    def forward(self, x):
        assert x.shape[0] == self.maps.shape[0]
        self.calls += 1
        return self.maps.clone()


def peak_table(B, K, seed):
    rng = np.random.RandomState(seed)
    return np.stack([3 + rng.rand(B, K) * 9, 3 + rng.rand(B, K) * 17], axis=2)
