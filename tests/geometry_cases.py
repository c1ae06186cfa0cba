"""Shared fixtures of tests/test_sample_geometry.py (CPU) and tests/test_gpu_sample_geometry.py: configs, records and
hand-made augmentation draws for DeviceSamplePipeline(geometry_on_device=True), and the tolerance both files use.

Sources are 120 x 160 (H x W), crops 64 x 96 (IMAGE_SIZE [64, 96]), heat-maps 16 x 24, B <= 16."""
import functools

import numpy as np

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMG_H, IMG_W = 120, 160
CROP = (64, 96)

# Largest element error against the exact rational solution of the 3-point system, measured by
# test_rotated_closed_form_against_the_exact_solution over its grid (it asserts that the measurement stays below these):
SOLVE_ERR = 2.7e-10         # get_affine_transform (np.linalg.solve): 2.64e-10
CLOSED_ERR = 1.9e-12        # crop_affine_rot_closed_form: 1.80e-12, at most 2 ulp of any element
# A joint is A x + t: an element error d moves a coordinate of up to 640 px by at most d * (640 + 640 + 1).  Kernel and
# host differ by at most the larger of the two errors through that, times 4 for the one rounding per operation of the
# kernel's own evaluation order: 4 * 2.7e-10 * 1281 = 1.4e-6.
TOL = 4 * max(SOLVE_ERR, CLOSED_ERR) * (2 * 640 + 1)

PAIRS = {1: (), 14: ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)),
         17: ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)), 32: ((0, 1), (2, 3), (30, 31))}


def colors(K):
    return (np.random.RandomState(5).randint(30, 256, (max(K, 3), 3))).astype(np.float32).tolist()


def cfg_for(K=14, mode="colored", conditional=True, synthesis=False, **ds):
    from oracle import cfg as ocfg
    c = ocfg.hrnet_cfg(16, K, CROP, "pose_hrnet_coam" if conditional else "pose_hrnet", use_attention=conditional,
                       colored=mode == "colored", stacked=mode == "stacked", stage_modules=(1, 1, 1))
    c.DATASET.update({"DATASET": "crowdpose", "SYNTHESIS_POSE": synthesis, "SCALE_FACTOR": 0.35, "ROT_FACTOR": 45,
                      "FLIP": True, "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3, "BU_BBOX_MARGIN": 25,
                      "NEW_AUGMENTATION": True, "BBOX_AUGMENTATION": False})
    c.DATASET.update(ds)
    c.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    return c


def pipe_for(K=14, mode="colored", conditional=True, synthesis=False, seed=0, on_device=False, **ds):
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    return DeviceSamplePipeline(cfg_for(K, mode, conditional, synthesis, **ds), PAIRS[K], range(min(K, 8)), colors(K), MEAN,
                                STD, is_train=True, seed=seed, geometry_on_device=on_device)


@functools.lru_cache(maxsize=None)
def records(K=14, n=16, seed=11, with_cond=True):
    """Train records on 120 x 160 images.  Every second record carries 'bbox' (record 2 touches two borders, record 6
    starts left of the image); with_cond: 'cond_joints' = the ground truth moved by a few pixels.  Specials (K > 8):
    ground truth - record 1 joint 3 at (0, 0) visible, record 2 joint 5 at (0, 0) invisible, record 3 joints 2 and K - 1
    invisible with coordinates; condition - record 1 joint 4 at (0, 0), record 4 has y of joint 0 == 0 (the bottom-up box
    is refused), record 5 joint 6 invisible."""
    from oracle import sample as S
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(n):
        img = rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)
        joints = np.ones((K, 3))
        joints[:, 0], joints[:, 1] = rng.rand(K) * (IMG_W - 40) + 20, rng.rand(K) * (IMG_H - 40) + 20
        vis = np.ones((K, 3))
        vis[:, 2] = 0
        cond = joints + np.concatenate([rng.randn(K, 2) * 3, np.zeros((K, 1))], 1)
        cvis = vis.copy()
        if K > 8:
            if i == 1:
                joints[3, :2], cond[4, :2] = 0, 0
            if i == 2:
                joints[5], vis[5] = 0, 0
            if i == 3:
                vis[2], vis[K - 1] = 0, 0
            if i == 4:
                cond[0, 1] = 0
            if i == 5:
                cvis[6] = 0
        x, y, bw, bh = S.box_from_keypoints(np.where(vis > 0, joints, 0) if vis[:, 0].sum() > 1 else joints, 5, IMG_W, IMG_H)
        c, s = S.xywh2cs(x, y, bw, bh, CROP[0] / CROP[1], 1.25)
        rec = {"image_np": img, "joints_3d": joints, "joints_3d_vis": vis, "center": c, "scale": s,
               "score": 0.5 + 0.01 * i, "annotation_id": 100 + i, "near_joints": np.zeros(0)}
        if with_cond:
            rec["cond_joints"], rec["cond_joints_vis"] = cond, cvis
        if i % 2 == 0:
            rec["bbox"] = [x + 0.7, y + 0.4, bw - 1.3, bh - 0.9]
        if i == 2:
            rec["bbox"] = [0.0, 37.6, 80.2, IMG_H - 37.6]
        if i == 6:
            rec["bbox"] = [-7.5, 10.2, 90.0, 70.0]
        recs.append(rec)
    return tuple(recs)


def draws(recs, bbox_aug=False, rotations=(0, 0.01, -90.0, 17.5, 90.0, -0.01, 0, -33.25)):
    """Hand-made draw() results: mixed flips, rotations 0 / small / at the clip ends of ROT_FACTOR 45, a half-body override
    on every fifth record, BBOX_AUGMENTATION integers 0 .. 20."""
    out = []
    for i, r in enumerate(recs):
        hb = None
        if i % 5 == 2:
            hb = (np.array(r["center"], np.float32) + np.float32(3.25), np.array(r["scale"], np.float32) * np.float32(0.8))
        out.append(dict(half_body=hb, scale_mul=np.float64(1 + 0.05 * ((i % 7) - 3) + 1e-3 / 3), rot=rotations[i % len(rotations)],
                        flip=i % 3 == 1, bbox_aug=((i * 5) % 21, 20 - (i * 3) % 21) if bbox_aug else None))
    return out


def on_device(recs, dev, **over):
    import torch
    return [dict(r, image=torch.from_numpy(r["image_np"]).to(dev), **over) for r in recs]


def near_integer(v, tol=TOL):
    return np.abs(v - np.rint(v)) <= tol
