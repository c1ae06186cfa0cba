"""TEST INFRASTRUCTURE - seeded sets for the hard OKS suppression as nms.oks_nms_grouped takes it (tests/test_soft_nms.py,
tests/test_gpu_soft_nms.py): one multi-image group per set, the persons of an image in descending score order.

  hard17   K = 17, COCO sigmas;
  hard3    K = 3, sigmas [0.05, 0.08, 0.11].

Images of 0, 1, 2, 63, 64, 65 and 129 persons: the empty cases and both sides of the word boundaries of the kernel's
LDS bitmap (64 persons per word).  An image holds clusters of near-duplicates (noise 0.01 to 0.3 of the pose size around
a third as many centres), so the suppression drops some persons and keeps others; joint scores are uniform in [0, 1), so
the joint-score threshold 0.2 counts some joints and not others.  All scores differ.

The expected keep mask is the host nms.oks_nms per image on the float32-rounded key points, widened to fp64 like the
device widens them.  The device's exp and numpy's may differ in the last place, which can flip a decision only where an
OKS sits on the threshold: building a set fails unless every pair's host OKS, with and without the joint-score threshold,
is further than 1e-9 from it.  That is a condition on the inputs, not a tolerance on the result."""
import numpy as np

from buctd_amd.nms import nms

VIS_THRE = 0.2
THRESH = 0.5
COUNTS = (0, 1, 2, 63, 64, 65, 129)
# name -> (K, seed, sigmas)
CONFIGS = {
    'hard17': (17, 41, nms.COCO_SIGMAS),
    'hard3': (3, 42, np.array([0.05, 0.08, 0.11])),
}

_cache = {}


def _image(rng, n, K):
    """n persons in descending score order: kpts float32 [n][K][3], areas [n], scores [n]."""
    centres = [(rng.rand(K, 2) * 120.0 + rng.rand(2) * 1500.0, 80.0 + 60.0 * rng.rand()) for _ in range(max(n // 3, 1))]
    kpts, areas = np.zeros((n, K, 3), dtype=np.float32), np.zeros(n)
    for p in range(n):
        xy, size = centres[p % len(centres)]
        noise = (0.01, 0.04, 0.1, 0.3)[(p // len(centres) + p) % 4]
        kpts[p, :, :2] = xy + rng.randn(K, 2) * noise * size
        kpts[p, :, 2] = rng.rand(K)
        areas[p] = size * size * (0.9 + 0.2 * rng.rand())
    scores = np.sort(rng.permutation(n) + rng.rand(n) * 0.5)[::-1] / max(n, 1)
    return kpts, areas, np.ascontiguousarray(scores)


def case(name):
    """dict(offsets int32 [images + 1], kpts float32 [N][K][3], areas, scores fp64 [N], sigmas fp64 [K], thresh,
    keep: {use_vis: the host's keep mask, int32 [N]}).  The arrays are read-only."""
    if name not in _cache:
        K, seed, sigmas = CONFIGS[name]
        rng = np.random.RandomState(seed)
        parts = [_image(rng, n, K) for n in COUNTS]
        kpts, areas, scores = (np.concatenate(a) for a in zip(*parts))
        offsets = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
        sigmas = np.array(sigmas, dtype=np.float64)
        keep = {}
        for use_vis in (False, True):
            vis = VIS_THRE if use_vis else None
            mask = np.zeros(kpts.shape[0], dtype=np.int32)
            for a, b in zip(offsets[:-1], offsets[1:]):
                flat = kpts[a:b].astype(np.float64).reshape(b - a, K * 3)
                for g in range(b - a - 1):                   # the condition on the inputs: no OKS on the threshold
                    oks = nms.oks_iou(flat[g], flat[g + 1:], areas[a + g], areas[a + g + 1:b], sigmas, vis)
                    assert np.abs(oks - THRESH).min() > 1e-9, (name, use_vis, int(a), g)
                db = [{'keypoints': flat[p], 'score': scores[a + p], 'area': areas[a + p]} for p in range(b - a)]
                kept = nms.oks_nms(db, THRESH, sigmas, vis)
                mask[a + np.asarray(kept, dtype=np.int64)] = 1
                assert b - a < 2 or 0 < len(kept) < b - a, (name, use_vis, int(a))     # some dropped, some kept
            keep[use_vis] = mask
        _cache[name] = dict(offsets=offsets, kpts=kpts, areas=areas, scores=scores, sigmas=sigmas, thresh=THRESH, keep=keep)
        for v in (offsets, kpts, areas, scores, sigmas, keep[False], keep[True]):
            v.setflags(write=False)
    return _cache[name]
