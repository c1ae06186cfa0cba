"""TEST INFRASTRUCTURE - seeded sets for the soft OKS suppression (tests/test_soft_nms.py, tests/test_gpu_soft_nms.py), in
the shape of validate()'s tables (kpt_eval_cases.CaseBuilder) and, derived from them, in the grouped form the kernel takes.

  soft17   K = 17, COCO sigmas, threshold 0.5: images with 0, 1, 20, 21 and 65 persons, the tie image, a reorder image;
  soft5    K = 5, sigmas [0.05] * 5, threshold 0.6: images with 0, 1, 19, 64 and 130 persons, a reorder image.

19 / 20 / 21 straddle the cap of 20 rounds, 64 / 65 one wavefront stride.  Both sets are used with the joint-score
threshold 0.2 inside the suppression's OKS and without it.  A crowd image holds clusters of near-duplicates (closeness
0.01 to 0.25 of the pose size) around a third as many ground truths and persons with no joint score above 0.2.  A reorder
image holds A (0.9), its near-duplicate B (0.8) and a far C (0.5): taken A, C, B.  The tie image holds two persons with
equal scores whose poses lie 1e6 px from each other and from everything else, so every OKS that touches them is exactly
0 and their live scores stay equal: the only tie of the sets.  About 340 persons in all."""
import numpy as np

from tests.helpers import soft_nms_ref as S
from tests.helpers.kpt_eval_cases import COCO_SIGMAS, IMAGE_DIR, SIZES, CaseBuilder

VIS_THRE = 0.2
TIE_IMAGE, REORDER_IMAGE = 70, 80
# name -> (K, seed, sigmas, threshold, {image id: persons})
CONFIGS = {
    'soft17': (17, 31, COCO_SIGMAS, 0.5, {3: 0, 5: 1, 11: 20, 12: 21, 9: 65}),
    'soft5': (5, 32, np.array([0.05] * 5), 0.6, {3: 0, 5: 1, 11: 19, 2: 64, 4: 130}),
}
COUNTS = {name: dict(cfg[4]) for name, cfg in CONFIGS.items()}


def _crowd(b, image_id, n):
    rng = b.rng
    b.image(image_id)
    gts = [b.gt(image_id, rng.rand(2) * 1500 + 250, SIZES[1 + i % 6]) for i in range(max(n // 3, 1))]
    for i in range(n):
        g = gts[i % len(gts)]
        if i % 17 == 5:
            b.det_near(g, 0.02 * (1 + i // len(gts)), joint_scores=rng.rand(b.K) * 0.19)       # no joint above 0.2
        else:
            b.det_near(g, (0.01, 0.04, 0.1, 0.25)[(i // len(gts) + i) % 4])


def _reorder(b, image_id):
    rng, K = b.rng, b.K
    b.image(image_id)
    g = b.gt(image_id, [600.0, 700.0], 90.0)
    xy = np.asarray(g['keypoints']).reshape(K, 3)[:, :2] + rng.randn(K, 2) * 20.0
    b.det(image_id, xy, 90.0, box_score=1.0, joint_scores=np.full(K, 0.9))                     # A
    b.det(image_id, xy + rng.randn(K, 2) * 0.5, 90.0, box_score=1.0, joint_scores=np.full(K, 0.8))     # B, on top of A
    b.det(image_id, xy + 900.0, 90.0, box_score=1.0, joint_scores=np.full(K, 0.5))             # C, far away


def _tie(b, image_id):
    rng, K = b.rng, b.K
    b.image(image_id)
    g = b.gt(image_id, [500.0, 500.0], 60.0)
    for noise, bs in ((0.01, 0.95), (0.04, 0.9), (0.1, 0.85), (0.25, 0.3), (0.04, 0.25), (0.01, 0.2)):
        b.det_near(g, noise, box_score=bs, joint_scores=rng.rand(K) * 0.2 + 0.75)
    js = rng.rand(K) * 0.2 + 0.7
    for far in ((1.0e6, 1.0e6), (2.0e6, 3.0e6)):                      # equal scores; below the cluster's best, above its last
        b.det(image_id, np.asarray(far) + rng.randn(K, 2) * 20.0, 60.0, box_score=0.6, joint_scores=js)


_cache = {}


def case(name):
    """(gt, preds, all_boxes, img_path, settings): settings = dict(K, sigmas, thresh)."""
    if name not in _cache:
        K, seed, sigmas, thresh, counts = CONFIGS[name]
        b = CaseBuilder(K, seed)
        for image_id, n in counts.items():
            _crowd(b, image_id, n)
        _reorder(b, REORDER_IMAGE)
        if name == 'soft17':
            _tie(b, TIE_IMAGE)
        gt, preds, boxes, paths = b.build()
        _cache[name] = (gt, preds, boxes, paths, dict(K=K, sigmas=np.asarray(sigmas, dtype=np.float64), thresh=thresh))
    return _cache[name]


def grouped(name):
    """The persons of a set as the kernel takes them: images by id, within an image by descending rescored score, equal
    scores in input order.  dict(image_ids, offsets int32 [I + 1], rows (input row per grouped position), kpts float32
    [N][K][3], areas, scores fp64 [N], score (per input row)).  The score is the mean joint score (threshold 0, summed in
    joint order in fp64) times the box score."""
    key = ('grouped', name)
    if key not in _cache:
        gt, preds, boxes, paths, kw = case(name)
        N, K = preds.shape[0], kw['K']
        score = np.zeros(N)
        for r in range(N):
            total, count = 0.0, 0
            for j in range(K):
                t = float(preds[r][j][2])
                if t > 0.0:
                    total, count = total + t, count + 1
            score[r] = (total / count if count else 0.0) * float(boxes[r][5])
        image_of = np.array([int(p.split('/')[-1].split('.')[0]) for p in paths], dtype=np.int64).reshape(N)
        image_ids = sorted(im['id'] for im in gt['images'])
        rows, offsets = [], [0]
        for i in image_ids:
            mine = np.flatnonzero(image_of == i)
            rows.extend(mine[np.argsort(-score[mine], kind='stable')].tolist())
            offsets.append(len(rows))
        rows = np.array(rows, dtype=np.int64)
        _cache[key] = dict(image_ids=image_ids, offsets=np.array(offsets, dtype=np.int32), rows=rows, image_of=image_of,
                           kpts=np.ascontiguousarray(preds[rows]), areas=np.ascontiguousarray(boxes[rows, 4]),
                           scores=np.ascontiguousarray(score[rows]), score=score)
    return _cache[key]


def reference(name, decay, use_vis):
    """The restatement on every image of a set, computed once: dict(rank int32 [N], soft_score [N] in grouped order,
    per_image: {image id: the restatement's dict})."""
    key = ('ref', name, decay, use_vis)
    if key not in _cache:
        g, kw = grouped(name), case(name)[4]
        rank, soft, per_image = [], [], {}
        for pos, image_id in enumerate(g['image_ids']):
            a, b = int(g['offsets'][pos]), int(g['offsets'][pos + 1])
            out = S.soft_nms(g['kpts'][a:b], g['areas'][a:b], g['scores'][a:b], kw['sigmas'], kw['thresh'], decay,
                             VIS_THRE if use_vis else None, 20)
            per_image[image_id] = out
            rank.extend(out['rank'])
            soft.extend(out['soft_score'])
        res = dict(rank=np.array(rank, dtype=np.int32).reshape(-1), soft_score=np.array(soft, dtype=np.float64).reshape(-1),
                   per_image=per_image)
        res['rank'].setflags(write=False)
        res['soft_score'].setflags(write=False)
        _cache[key] = res
    return _cache[key]


def tie_positions(name):
    """Grouped positions (within the tie image) of the two persons with equal scores; () for a set without the image."""
    g = grouped(name)
    if TIE_IMAGE not in g['image_ids']:
        return ()
    pos = g['image_ids'].index(TIE_IMAGE)
    s = g['scores'][g['offsets'][pos]:g['offsets'][pos + 1]]
    pair = [p for p in range(len(s)) if np.count_nonzero(s == s[p]) == 2]
    assert len(pair) == 2
    return tuple(pair)
