"""Fixtures of the flip-test refinement tests (test_refine_flip.py on the CPU, test_gpu_refine_flip.py on the GPU): condition
poses with the edge cases of buctd_cond_mirror, and a stand-in network for a paired [crops | mirrored crops] forward."""
import numpy as np
import torch

from refine_cases import HEATMAP, FixedPeaks

UNPAIRED = [[0, 3], [5, 6]]                # a pair table that leaves joints without a partner (and is not 2i, 2i + 1)


def pairs_for(K, which):
    from oracle import core as oc
    if K < 12:
        return []
    return oc.CROWDPOSE_FLIP_PAIRS if which == "crowdpose" else UNPAIRED


def mirror_case(K, width, B=2, seed=0):
    """cond_joints float64 [B, K, 3] in crop coordinates of a `width`-pixel crop and visibilities [B, K, 3]:
      joint 0             non-integer x left of the centre (sample 0) / right of it (sample 1)
      joints 1-3 (K > 3)  x = width - 0.6 (> width - 1: the mirror is -0.4, trunc gives 0), x = width + 5.25 (mirror < -1),
                          x = -3.5 (mirror beyond the right border)
      joints 4-5 (K > 5)  integer x and x = (width - 1) / 2, the centre itself
      the rest            random non-integer coordinates on both sides, some outside the crop
    about a fifth of the joints invisible (sample 1's joint 0 among them where K > 1); visibility column 2 is 0 as the
    data sets have it."""
    rng = np.random.RandomState(1000 * K + width + seed)
    cj = np.zeros((B, K, 3))
    cj[:, :, 0] = rng.rand(B, K) * (width + 20) - 10
    cj[:, :, 1] = rng.rand(B, K) * 116 - 10
    cj[0, 0, 0], cj[1 % B, 0, 0] = width * 0.25 + 0.3, width * 0.75 + 0.7
    if K > 3:
        cj[:, 1, 0], cj[:, 2, 0], cj[:, 3, 0] = width - 0.6, width + 5.25, -3.5
        cj[:, 1, 1] = np.resize([-0.4, 95.9], B)
    if K > 5:
        cj[:, 4, 0], cj[:, 5, 0] = 17.0, (width - 1) / 2
    vis = np.repeat((rng.rand(B, K, 1) > 0.2).astype(np.float64), 3, 2)
    vis[0, 0] = 1
    if K > 1:
        vis[1 % B, 0] = 0
        vis[0, K - 1] = 0
    vis[:, :, 2] = 0
    return cj, vis


def oracle_mirror(cj, vis, width, pairs):
    """oracle.core.fliplr_joints per sample, then .astype(int): what the reference's flip_hm hands its renderer"""
    from oracle import core as oc
    if vis is None:
        vis = np.ones_like(cj)
    return np.stack([oc.fliplr_joints(cj[b], vis[b], width, pairs)[0].astype(int)[:, :2] for b in range(cj.shape[0])])


MIRROR_CASES = [(K, width, which) for K in (1, 14, 32) for width in (64, 71) for which in ("crowdpose", "unpaired")
                if K >= 12 or which == "crowdpose"]


def moving_records(n, seed, k=14):
    """refine_cases.records with persons of about 100 x 150 px in the middle of images of about 1000 x 1200 px: the box around
    the predictions +- the margin grows from pass to pass but stays inside the image, so no box settles and no crop
    coordinate is an integer (with refine_cases.records the box is the whole image from pass 1 on)."""
    from oracle import sample as S
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(n):
        h, w = int(rng.randint(1100, 1300)), int(rng.randint(900, 1100))
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        joints = np.zeros((k, 3))
        joints[:, 0] = w * 0.5 + (rng.rand(k) - 0.5) * 90 + 7 * i
        joints[:, 1] = h * 0.5 + (rng.rand(k) - 0.5) * 140 - 5 * i
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


class PairedPeaks(FixedPeaks):
    """FixedPeaks for a paired forward: rows [0, B) as FixedPeaks, rows [B, 2B) the same Gaussians where the mirrored crop
    would show them once the flip test has mirrored them back and shifted them by one pixel - partner joints exchanged,
    x' = W - x.  The merged heat-map is then the one of rows [0, B) again (but for column 0)."""

    def __init__(self, positions, pairs, peak=0.8):
        pos = np.asarray(positions, dtype=np.float64)
        table = np.arange(pos.shape[1])
        for a, b in pairs:
            table[a], table[b] = b, a
        mirrored = pos[:, table].copy()
        mirrored[:, :, 0] = HEATMAP[0] - mirrored[:, :, 0]
        super().__init__(np.concatenate([pos, mirrored]), peak)


class Stub:
    """What transforms.flip_hm reads of a data set"""

    def __init__(self, pipe, colors):
        self.image_size = pipe.image_size
        self.flip_pairs = pipe.flip_pairs
        self.kpt_colors = colors


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
