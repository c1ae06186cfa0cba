"""TEST INFRASTRUCTURE - seeded synthetic sets for buctd_amd/dataset/conditions.py: a COCO-style annotation dict, the
flat results list of a bottom-up model and the same poses in the 'preds' / 'scores' / 'image_paths' form, for K = 17
and K = 5.  Persons stand on a grid whose cells are smaller than the persons, so neighbours overlap.  Per set:

  image 1   two annotations, no prediction
  image 2   three predictions, no annotation
  images 11-15  1, 63, 64, 65 and 130 annotations with one prediction each, in shuffled order (the lane-stride
            boundaries of a 64-lane wavefront); image 11 also holds a prediction of category 2
  image 20  one annotation in a corner and two predictions far from it: every IoU is 0
  image 21  three annotations; the first one's prediction stands twice in the results (bit-identical boxes: an index
            tie); the third has no labelled joint (status 1); the second has joints with v == 0 and non-zero coordinates
  image 22  an annotation at the origin whose prediction has negative coordinates (clipped corner); BU scores 0.05 and
            0.6 with IMAGE_THRE 0.1: the dropped pose is the only neighbour of the kept one
  image 23  two annotations with one box (overlap exactly 1), a third that overlaps them, a zero-area box (bbox width
            1: status 2), and two boxes that touch (intersection 0)

`bad_pose(K)` is a pose whose x are all 0 (status 1 in the non-zero form)."""
import functools
from types import SimpleNamespace

import numpy as np

IMAGE_DIR = "images"
MODEL_KEY = "bu_w32"
IMAGE_THRE, MARGIN, SCALE_THRE = 0.1, 25, 1.25
CROP = (64, 96)
SEEDS = {17: 11, 5: 12}
SMALL_IMAGES = (20, 21, 22, 23)                 # 400 x 300: the ones a test renders


def cfg(K):
    return SimpleNamespace(MODEL=SimpleNamespace(NUM_JOINTS=K, IMAGE_SIZE=list(CROP)),
                           DATASET=SimpleNamespace(BU_BBOX_MARGIN=MARGIN),
                           TEST=SimpleNamespace(IMAGE_THRE=IMAGE_THRE, SCALE_THRE=SCALE_THRE))


class Builder:
    def __init__(self, K, seed):
        self.K, self.rng = K, np.random.RandomState(seed)
        self.images, self.anns, self.results = [], [], []

    def image(self, image_id, width, height):
        self.images.append({'id': image_id, 'width': width, 'height': height, 'file_name': f'{image_id:06d}.jpg'})

    def person(self, image_id, box, v=None, category_id=1, iscrowd=0):
        """An annotation with bbox `box` and integer key points inside it; v: the visibility column, drawn if None."""
        rng, K = self.rng, self.K
        x, y, w, h = box
        kp = np.zeros((K, 3), dtype=np.int64)
        kp[:, 0] = np.floor(x + 1 + rng.rand(K) * max(w - 2, 1))
        kp[:, 1] = np.floor(y + 1 + rng.rand(K) * max(h - 2, 1))
        kp[:, 2] = rng.randint(1, 3, size=K) if v is None else v
        if v is None:
            kp[rng.rand(K) < 0.15] = 0
            kp[0] = (kp[0, 0], kp[0, 1], 2)                                      # at least one labelled joint
        ann = {'id': 1000 + len(self.anns), 'image_id': image_id, 'category_id': category_id,
               'keypoints': [int(t) for t in kp.reshape(-1)], 'num_keypoints': int((kp[:, 2] > 0).sum()),
               'area': float(0.6 * w * h), 'bbox': [float(t) for t in box], 'iscrowd': iscrowd}
        self.anns.append(ann)
        return ann

    def pose(self, image_id, xy, score=None, category_id=1, missing=0.05):
        """A result with key points `xy` [K][2] (two decimals, like a results file), some joints missing (0, 0, 0)."""
        rng, K = self.rng, self.K
        kp = np.zeros((K, 3))
        kp[:, :2] = np.round(np.asarray(xy, dtype=np.float64), 2)
        kp[:, 2] = np.round(0.2 + 0.8 * rng.rand(K), 3)
        gone = rng.rand(K) < missing
        gone[0] = False
        kp[gone] = 0
        res = {'image_id': image_id, 'category_id': category_id, 'keypoints': [float(t) for t in kp.reshape(-1)],
               'score': float(np.round(0.15 + 0.8 * rng.rand(), 3) if score is None else score)}
        self.results.append(res)
        return res

    def pose_of(self, ann, noise=3.0, **kw):
        kp = np.array(ann['keypoints'], dtype=np.float64).reshape(self.K, 3)
        away = kp[:, :2] == 0                                                    # an unlabelled joint is predicted all the same
        xy = np.where(away, ann['bbox'][0] + 0.5 * ann['bbox'][2], kp[:, :2]) + self.rng.randn(self.K, 2) * noise
        return self.pose(ann['image_id'], xy, **kw)

    def crowd(self, image_id, n):
        """n persons on a grid of 70 x 90 cells, 50-90 wide and 70-120 high, and their predictions in shuffled order."""
        rng = self.rng
        anns = []
        for i in range(n):
            c, r = i % 13, i // 13
            box = (40.0 + 70 * c + np.round(rng.rand() * 10, 2), 40.0 + 90 * r + np.round(rng.rand() * 10, 2),
                   np.round(50 + rng.rand() * 40, 2), np.round(70 + rng.rand() * 50, 2))
            anns.append(self.person(image_id, box))
        for i in rng.permutation(n):
            self.pose_of(anns[i])
        return anns


@functools.lru_cache(maxsize=None)
def case(K):
    """-> dict(K, cfg, gt, results, bu_results): gt carries an empty cond_kpts dict per annotation, as the script needs."""
    b = Builder(K, SEEDS[K])
    b.image(1, 400, 300)
    b.person(1, (50.0, 40.0, 80.0, 120.0))
    b.person(1, (90.0, 60.0, 70.0, 110.0))
    b.image(2, 400, 300)
    for _ in range(3):
        b.pose(2, 50 + b.rng.rand(K, 2) * 200)
    for image_id, n in zip((11, 12, 13, 14, 15), (1, 63, 64, 65, 130)):
        b.image(image_id, 1200, 1200)
        b.crowd(image_id, n)
    b.pose(11, 100 + b.rng.rand(K, 2) * 100, category_id=2)
    b.image(20, 400, 300)
    b.person(20, (2.0, 2.0, 40.0, 50.0))
    b.pose(20, np.stack([200 + b.rng.rand(K) * 60, 150 + b.rng.rand(K) * 80], axis=1), missing=0)
    b.pose(20, np.stack([300 + b.rng.rand(K) * 60, 100 + b.rng.rand(K) * 80], axis=1), missing=0)
    b.image(21, 400, 300)
    first = b.person(21, (60.0, 50.0, 90.0, 130.0))
    b.pose(21, 250 + b.rng.rand(K, 2) * 40, missing=0)                           # a decoy before the tied pair
    twin = b.pose_of(first, missing=0)
    b.results.append(dict(twin))                                                 # the same pose again: an index tie
    v = np.full(K, 2)
    v[1::2] = 0                                                                  # v == 0 with coordinates
    b.pose_of(b.person(21, (180.0, 80.0, 100.0, 140.0), v=v))
    blank = b.person(21, (120.0, 60.0, 80.0, 100.0))
    blank['keypoints'] = [0] * (3 * K)                                           # no labelled joint
    blank['num_keypoints'] = 0
    b.image(22, 400, 300)
    origin = b.person(22, (0.0, 0.0, 70.0, 110.0))
    kp = np.array(origin['keypoints'], dtype=np.float64).reshape(K, 3)[:, :2]
    b.pose(22, kp - 12.5, score=0.05, missing=0)                                 # negative coordinates, below IMAGE_THRE
    b.pose(22, kp + 6.25, score=0.6, missing=0)
    b.image(23, 400, 300)
    b.person(23, (40.0, 30.0, 81.0, 121.0))
    b.person(23, (40.0, 30.0, 81.0, 121.0))                                      # one box twice
    b.person(23, (70.0, 60.0, 91.0, 101.0))
    b.person(23, (60.0, 200.0, 1.0, 41.0))                                       # cut box width 0: zero area
    b.person(23, (200.0, 40.0, 51.0, 61.0))                                      # cut box 200 .. 250
    b.person(23, (250.0, 40.0, 51.0, 61.0))                                      # cut box 250 .. 300: they touch
    for ann in b.anns[-6:]:
        b.pose_of(ann)
    for ann in b.anns:
        ann['cond_kpts'] = {}
    gt = {'images': b.images, 'annotations': b.anns, 'categories': [{'id': 1, 'name': 'person'}, {'id': 2, 'name': 'other'}]}
    bu_results = []
    for im in b.images:
        rows = [r for r in b.results if r['image_id'] == im['id'] and r['category_id'] == 1]
        if rows:
            bu_results.append({'preds': [np.array(r['keypoints']).reshape(K, 3).tolist() for r in rows],
                               'scores': [r['score'] for r in rows], 'image_paths': [f"{IMAGE_DIR}/{im['file_name']}"]})
    return dict(K=K, cfg=cfg(K), gt=gt, results=b.results, bu_results=bu_results)


def golden_input():
    """The pair tests/helpers/make_condition_golden.py runs the reference's script on: images 20-23 of case(5) without
    the annotation that has no labelled joint (the script raises on it)."""
    c = case(5)
    gt = {'images': [im for im in c['gt']['images'] if im['id'] in SMALL_IMAGES],
          'annotations': [a for a in c['gt']['annotations'] if a['image_id'] in SMALL_IMAGES and max(a['keypoints']) > 0]}
    return gt, [r for r in c['results'] if r['image_id'] in SMALL_IMAGES]


def bad_pose(K):
    pose = np.zeros((K, 3))
    pose[:, 1] = np.arange(1, K + 1) * 7.5
    pose[:, 2] = 0.5
    return pose


@functools.lru_cache(maxsize=None)
def reference(K):
    """The restatement's outputs for case(K), computed once and shared (treat as read-only)."""
    from tests.helpers import condition_ref as ref
    c = case(K)
    aspect = CROP[0] * 1.0 / CROP[1]
    annotated, rows = ref.match_annotations(c['gt'], c['results'], MODEL_KEY)
    test_db, test_boxes, test_ious = ref.bu_test_records(c['bu_results'], K, MARGIN, IMAGE_THRE, aspect, SCALE_THRE)
    train_db, overlaps = ref.train_records(annotated, K, aspect, SCALE_THRE, image_dir=IMAGE_DIR, model_key=MODEL_KEY)
    return dict(annotated=annotated, rows=rows, test_db=test_db, test_boxes=test_boxes, test_ious=test_ious,
                train_db=train_db, overlaps=overlaps)


def separated(values, points=()):
    """Whether any two of `values`, and any value and any of `points`, are bit-equal or more than 1e-9 apart."""
    v = np.unique(np.concatenate([np.asarray(values, dtype=np.float64).reshape(-1), np.asarray(points, dtype=np.float64)]))
    return v.size < 2 or float(np.diff(v).min()) > 1e-9
