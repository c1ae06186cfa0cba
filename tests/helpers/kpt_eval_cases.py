"""TEST INFRASTRUCTURE - seeded synthetic COCO-style key point sets for the keypoint evaluation tests, in the shape of
validate()'s tables: gt dict, all_preds [N][K][3] float32, all_boxes [N][7] (area in column 4, box score in 5,
annotation id in 6) and img_path."""
import numpy as np

IMAGE_DIR = 'data/synth/images'


def _person(rng, K, center, size, n_vis=None):
    """A ground-truth pose of about `size` pixels around `center`: kpts [K][3] (x, y, v), bbox, area."""
    xy = center + rng.randn(K, 2) * size * 0.3
    v = rng.randint(1, 3, size=K)
    hidden = rng.rand(K) < 0.25
    hidden[rng.randint(K)] = False
    if n_vis == 0:
        hidden[:] = True
    v[hidden] = 0
    xy[hidden] = 0.0
    vis = xy[~hidden] if n_vis != 0 else center + rng.randn(K, 2) * size * 0.3
    x0, y0 = vis.min(0) - 0.05 * size
    x1, y1 = vis.max(0) + 0.05 * size
    bbox = [float(x0), float(y0), float(x1 - x0), float(y1 - y0)]
    return np.concatenate([xy, v[:, None].astype(np.float64)], 1), bbox, float(size * size)


class CaseBuilder:
    def __init__(self, K, seed):
        self.K, self.rng = K, np.random.RandomState(seed)
        self.images, self.anns, self.preds, self.boxes, self.paths = [], [], [], [], []

    def image(self, image_id):
        self.images.append({'id': image_id, 'file_name': f'{image_id:06d}.jpg', 'width': 2000, 'height': 2000})
        return image_id

    def gt(self, image_id, center, size, iscrowd=0, n_vis=None):
        kp, bbox, area = _person(self.rng, self.K, np.asarray(center, dtype=np.float64), size, n_vis)
        ann = {'id': 1000 + len(self.anns), 'image_id': image_id, 'category_id': 1, 'keypoints': [float(x) for x in kp.reshape(-1)],
               'num_keypoints': int((kp[:, 2] > 0).sum()), 'area': area, 'bbox': bbox, 'iscrowd': iscrowd}
        self.anns.append(ann)
        return ann

    def det(self, image_id, xy, size, box_score=None, joint_scores=None, ann_id=0):
        """A detection with key points xy [K][2]."""
        rng, K = self.rng, self.K
        js = rng.rand(K) * 0.9 + 0.1 if joint_scores is None else np.asarray(joint_scores, dtype=np.float64)
        self.preds.append(np.concatenate([xy, js[:, None]], 1))
        c = xy.mean(0)
        bs = float(rng.rand() * 0.9 + 0.1) if box_score is None else box_score
        self.boxes.append([c[0], c[1], size / 200.0, size / 200.0, size * size * (0.8 + 0.4 * rng.rand()), bs, ann_id])
        self.paths.append(f'{IMAGE_DIR}/{image_id:06d}.jpg')

    def det_near(self, ann, noise, **kw):
        """A detection `noise` (in units of the pose size) away from a ground truth; hidden joints get plausible places."""
        kp = np.asarray(ann['keypoints']).reshape(self.K, 3)
        size = np.sqrt(ann['area'])
        xy = kp[:, :2].copy()
        hidden = kp[:, 2] == 0
        b = ann['bbox']
        xy[hidden] = [b[0] + b[2] / 2, b[1] + b[3] / 2] + self.rng.randn(int(hidden.sum()), 2) * size * 0.3
        xy = xy + self.rng.randn(self.K, 2) * noise * size
        self.det(ann['image_id'], xy, size, ann_id=ann['id'], **kw)

    def det_random(self, image_id, center, size, **kw):
        self.det(image_id, np.asarray(center, dtype=np.float64) + self.rng.randn(self.K, 2) * size * 0.3, size, **kw)

    def build(self):
        order = self.rng.permutation(len(self.images))           # `images` is not sorted by id
        gt = {'images': [self.images[i] for i in order], 'annotations': self.anns,
              'categories': [{'id': 1, 'name': 'animal'}]}
        preds = np.asarray(self.preds, dtype=np.float32).reshape(-1, self.K, 3)
        boxes = np.asarray(self.boxes, dtype=np.float64).reshape(-1, 7)
        perm = self.rng.permutation(preds.shape[0])               # persons of an image are not adjacent rows
        return gt, preds[perm], boxes[perm], [self.paths[i] for i in perm]


NOISES = (0.0, 0.01, 0.03, 0.05, 0.08, 0.12, 0.2, 0.4)
SIZES = (20.0, 28.0, 40.0, 60.0, 90.0, 120.0, 200.0)      # areas below 32^2, between 32^2 and 96^2, above 96^2


def matching_set(K, seed):
    """12 images covering the cases of the matching kernel (see tests/test_gpu_keypoint_eval.py)."""
    b = CaseBuilder(K, seed)
    rng = b.rng
    ids = [b.image(7 + 3 * i) for i in range(12)]
    spot = lambda: rng.rand(2) * 1500 + 250
    # 0: ground truths, no detections;  1: detections, no ground truth;  2: neither
    for _ in range(3):
        b.gt(ids[0], spot(), SIZES[rng.randint(len(SIZES))])
    for _ in range(3):
        b.det_random(ids[1], spot(), 80.0)
    # 3: 23 detections (cut to 20) on 4 ground truths
    g3 = [b.gt(ids[3], spot(), SIZES[2 + i]) for i in range(4)]
    for i in range(23):
        if i < 8:
            b.det_near(g3[i % 4], NOISES[i])
        else:
            b.det_random(ids[3], spot(), 70.0)
    # 4: 70 ground truths (more than a wavefront), 10 detections
    g4 = [b.gt(ids[4], spot(), SIZES[i % len(SIZES)]) for i in range(70)]
    for i in range(10):
        b.det_near(g4[7 * i], NOISES[i % len(NOISES)])
    # 5: a ground truth without labelled key points (the bbox-distance form) next to ordinary ones
    g5 = b.gt(ids[5], spot(), 100.0, n_vis=0)
    b.det_near(g5, 0.05)
    b.det_near(g5, 0.6)
    b.det_near(b.gt(ids[5], spot(), 50.0), 0.03)
    # 6: a crowd ground truth overlapped by two detections, and an ordinary one
    g6 = b.gt(ids[6], spot(), 150.0, iscrowd=1)
    b.det_near(g6, 0.02)
    b.det_near(g6, 0.04)
    b.det_near(b.gt(ids[6], spot(), 110.0), 0.05)
    # 7: tied scores: equal box score and equal joint scores, one a hit and one a miss
    g7 = b.gt(ids[7], spot(), 100.0)
    js = rng.rand(K) * 0.5 + 0.4
    b.det_random(ids[7], spot(), 100.0, box_score=0.75, joint_scores=js)
    b.det_near(g7, 0.02, box_score=0.75, joint_scores=js)
    b.det_near(b.gt(ids[7], spot(), 30.0), 0.05, box_score=0.75, joint_scores=js)
    # 8-11: every size class with hits of every quality, misses and duplicates
    for i in range(8, 12):
        for j in range(2 + i % 3):
            g = b.gt(ids[i], spot(), SIZES[(i + 2 * j) % len(SIZES)])
            b.det_near(g, NOISES[(i + j) % len(NOISES)])
            if j == 0:
                b.det_near(g, NOISES[(i + 3) % len(NOISES)])
        b.det_random(ids[i], spot(), 60.0)
    return b.build()


def nms_set(K, seed):
    """Images with 1, 64, 65 and 130 persons: clusters of near-duplicates of every closeness around a third as many
    ground truths, persons whose joint scores all lie below 0.2, and tied scores on poses far apart."""
    b = CaseBuilder(K, seed)
    rng = b.rng
    for image_id, n in ((5, 1), (2, 64), (9, 65), (4, 130)):
        b.image(image_id)
        gts = [b.gt(image_id, rng.rand(2) * 1500 + 250, SIZES[1 + i % 6]) for i in range(max(n // 3, 1))]
        js = rng.rand(K) * 0.5 + 0.4
        for i in range(n):
            g = gts[i % len(gts)]
            if i % 17 == 5:
                b.det_near(g, 0.02 * (1 + i // len(gts)), joint_scores=rng.rand(K) * 0.19)      # no joint above 0.2
            elif i < 2 and n > 1:
                b.det_near(g, 0.03, box_score=0.6, joint_scores=js)                            # a tie, poses far apart
            else:
                b.det_near(g, (0.01, 0.04, 0.1, 0.25)[(i // len(gts) + i) % 4])
    return b.build()


COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
# name -> (set, K, seed, evaluator settings)
CONFIGS = {
    'match17': (matching_set, 17, 11, dict(sigmas=COCO_SIGMAS, use_nms=False)),
    'match5': (matching_set, 5, 12, dict(sigmas=[0.1] * 5, use_nms=False)),
    'match17_nms': (matching_set, 17, 13, dict(sigmas=COCO_SIGMAS, use_nms=True)),
    'nms17': (nms_set, 17, 21, dict(sigmas=COCO_SIGMAS, use_nms=True, in_vis_thre=0.2)),
    'nms5_vis': (nms_set, 5, 22, dict(sigmas=[0.1] * 5, nms_sigmas=[0.05] * 5, use_nms=True, in_vis_thre=0.2,
                                      nms_in_vis_thre=0.2, oks_thre=0.6)),
}
_cache = {}


def case(name):
    """(gt, preds, all_boxes, img_path, settings, reference tables) of a configuration; the reference is computed once."""
    if name not in _cache:
        from tests.helpers import coco_kpt_eval_ref as R
        make, K, seed, kw = CONFIGS[name]
        gt, preds, boxes, paths = make(K, seed)
        image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
        ref = R.evaluate_ref(gt, preds, boxes, image_of, kw['sigmas'], kw.get('nms_sigmas'), kw.get('oks_thre', 0.5),
                             kw.get('in_vis_thre', 0.0), kw['use_nms'], kw.get('nms_in_vis_thre'))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = (gt, preds, boxes, paths, kw, ref)
    return _cache[name]


def threshold_margin(name):
    """The smallest distance of a reference OKS from a threshold it is compared with: the ten matching thresholds for
    the matrices, oks_thre for the suppression."""
    kw, ref = case(name)[4:]
    thrs = np.linspace(.5, 0.95, 10)
    m = [np.abs(np.asarray(o).reshape(-1, 1) - thrs).min() for o in ref['oks'].values() if len(o)]
    if ref['nms_oks'].size:
        m.append(np.abs(ref['nms_oks'] - kw.get('oks_thre', 0.5)).min())
    return min(m)
