"""TEST INFRASTRUCTURE - seeded synthetic sets for the crowding analysis (core/keypoint_analysis.py), in the shape of
validate()'s tables like tests/helpers/kpt_eval_cases.py, whose builder they extend with persons of a given box and a
given number of labelled key points.  Persons stand in clusters of equal boxes shifted by 5 % of their side, so that a
cluster of n gives each member n - 1 overlaps (IoU between 0.38 and 0.90, far from the 0.1 threshold) and clusters do
not meet.  crowding_set holds, per set:

  image 31  no ground truth; a detection that names no annotation (-1) and one that names a person of image 17
  image 12  a single person; two detections with one score, a hit and a miss (tied scores)
  image 17  70 persons (more than a wavefront) in clusters of 1, 2, 3, 4, 5 and 10 (9 overlaps: in no bin), one of them a
            crowd annotation, one without a detection, one with 21 detections
  image 23  annotations that do not count for each of the three reasons - all key point values 0, area == 0, box beyond
            the image's right edge - each overlapping a person that does; two boxes that only touch (IoU exactly 0); two
            persons with one box (IoU 1); two zero-area boxes in one place (denominator 0); a lone person with a stored
            num_overlaps of 4, and the area == 0 annotation with a stored count too
  image 40  three persons of one bin with 23 detections between them and two persons of another bin whose six
            detections score highest, so that a cut to 20 before the bin filter keeps 14 of the 23 and a cut after it 20
  image 8   a person of the bin of image 12's; a detection here that names image 12's person (same bin: it is evaluated
            here, and it is no detection of that person) and one that names a person of a bin this image lacks (dropped)
"""
import numpy as np

from tests.helpers.kpt_eval_cases import COCO_SIGMAS, IMAGE_DIR, NOISES, CaseBuilder

SIDES = (30.0, 60.0, 150.0)          # areas 0.6 * side^2: below 32^2, between 32^2 and 96^2, above 96^2


class CrowdBuilder(CaseBuilder):
    def person(self, image_id, box, n_vis, area=None, iscrowd=0, **extra):
        """A ground truth with bbox `box` (x, y, w, h) and exactly n_vis labelled key points inside it; the others are 0."""
        rng, K = self.rng, self.K
        x, y, w, h = (float(v) for v in box)
        kp = np.zeros((K, 3))
        vis = rng.permutation(K)[:n_vis]
        kp[vis, 0] = x + rng.rand(n_vis) * w
        kp[vis, 1] = y + rng.rand(n_vis) * h
        kp[vis, 2] = rng.randint(1, 3, size=n_vis)
        ann = {'id': 1000 + len(self.anns), 'image_id': image_id, 'category_id': 1,
               'keypoints': [float(v) for v in kp.reshape(-1)], 'num_keypoints': int(n_vis),
               'area': float(0.6 * w * h if area is None else area), 'bbox': [x, y, w, h], 'iscrowd': iscrowd}
        ann.update(extra)
        self.anns.append(ann)
        return ann

    def det_again(self, ann, noise):
        """The last detection once more, every joint `noise` pose sizes away: a duplicate the suppression removes."""
        size = np.sqrt(ann['area'])
        xy = self.preds[-1][:, :2] + self.rng.randn(self.K, 2) * noise * size
        self.det(ann['image_id'], xy, size, ann_id=ann['id'])

    def cluster(self, image_id, origin, n, side, n_vis):
        """n persons with equal boxes, each shifted by 5 % of the side: n - 1 overlaps each."""
        return [self.person(image_id, (origin[0] + 0.05 * side * i, origin[1], side, side), n_vis[i % len(n_vis)])
                for i in range(n)]


def _cells():
    """Origins of a grid of cells no cluster leaves (a cluster of 10 at side 150 is 217.5 wide)."""
    return [(20.0 + 240 * c, 20.0 + 240 * r) for r in range(8) for c in range(8)]


def crowding_set(K, seed, kpt_counts):
    """kpt_counts: the numbers of labelled key points to cycle through, one per num_kpt_group at least."""
    b = CrowdBuilder(K, seed)
    rng = b.rng
    for image_id in (31, 12, 17, 23, 40, 8):
        b.image(image_id)
    js = rng.rand(K) * 0.5 + 0.4
    n0 = kpt_counts[0]
    # image 12: a single person, tied scores
    lone12 = b.person(12, (300, 300, 150, 150), n0)
    b.det_near(lone12, 0.03, box_score=0.7, joint_scores=js)
    b.det_random(12, (1200.0, 1200.0), 150.0, box_score=0.7, joint_scores=js, ann_id=lone12['id'])
    # image 17: 70 persons
    sizes = [1] * 10 + [2] * 8 + [3] * 4 + [4] * 3 + [5] * 2 + [10]
    cells = _cells()
    people = []
    for c, n in enumerate(sizes):
        counts = [kpt_counts[(c + i) % len(kpt_counts)] for i in range(n)]
        people.append(b.cluster(17, cells[2 * c], n, SIDES[c % 3], counts))
    people[10][1]['iscrowd'] = 1                                   # a crowd annotation inside a cluster of 2
    flat = [p for group in people for p in group]
    assert len(flat) == 70
    for i, p in enumerate(flat):
        if i == 3:
            continue                                               # a person with no detection
        if i == 5:
            for j in range(21):                                    # a person with 21 detections
                b.det_near(p, (0.08, 0.12, 0.2, 0.4, 0.05)[j % 5])
            continue
        b.det_near(p, NOISES[i % len(NOISES)])
        if i % 9 == 0:
            b.det_again(p, 0.002)                                  # a near-duplicate for the suppression
    # image 31: no ground truth
    b.det_random(31, (500.0, 500.0), 80.0, ann_id=-1)
    b.det_random(31, (900.0, 900.0), 80.0, ann_id=people[22][0]['id'])
    # image 23: what does not count, and the IoU's corners
    b.det_near(b.person(23, (100, 100, 120, 120), n0), 0.05)
    b.person(23, (110, 110, 120, 120), 0)                                            # all key point values 0
    b.person(23, (120, 100, 120, 120), kpt_counts[1], area=0.0, num_overlaps=1)      # area == 0
    b.det_near(b.person(23, (1950, 100, 90, 90), n0), 0.05)
    b.person(23, (1999.5, 100, 90, 90), kpt_counts[1])                               # beyond the right edge (width 2000)
    for box in ((400, 400, 100, 100), (500, 400, 100, 100),                          # touching
                (700, 400, 100, 100), (700, 400, 100, 100)):                         # identical
        b.det_near(b.person(23, box, kpt_counts[len(b.anns) % len(kpt_counts)]), 0.08)
    for _ in range(2):
        b.det_near(b.person(23, (1000, 400, 0, 0), kpt_counts[2], area=400.0), 0.3)  # zero-area boxes
    b.det_near(b.person(23, (1300, 400, 100, 100), kpt_counts[-1], num_overlaps=4), 0.05)
    # image 40: 23 detections of one bin, outranked by six of another
    first = [b.person(40, (200 + 400 * i, 200, 150, 150), n0) for i in range(3)]
    other = [b.person(40, (200 + 400 * i, 800, 150, 150), kpt_counts[1]) for i in range(2)]
    for i in range(6):
        b.det_near(other[i % 2], 0.05 + 0.05 * (i // 2), box_score=0.99 - 0.01 * i, joint_scores=js)
    for i in range(23):
        if i < 9:
            b.det_near(first[i % 3], NOISES[1 + i % 7], box_score=0.9 - 0.01 * i, joint_scores=js)
        else:
            b.det_random(40, (300.0 + 60 * i, 1500.0), 150.0, box_score=0.9 - 0.01 * i, joint_scores=js,
                         ann_id=first[i % 3]['id'])
    # image 8
    lone8 = b.person(8, (600, 600, 150, 150), n0)
    b.det_near(lone8, 0.05)
    b.det_near(dict(lone12, image_id=8), 0.5)                      # names image 12's person, stands in image 8
    b.det_near(dict(people[22][0], image_id=8), 0.5)               # names a person with 3 overlaps: no such bin here
    return b.build()


def coco_sized_set(K=17, seed=3, images=2300):
    """A COCO-val-sized set for timing: about 2.8 persons an image in clusters of 1-4, one detection per person and a
    duplicate for one in seven."""
    b = CrowdBuilder(K, seed)
    rng = b.rng
    cells = _cells()
    for i in range(images):
        image_id = b.image(1 + i)
        picks = rng.permutation(len(cells))
        for c in range(rng.randint(1, 3)):
            n = int(rng.choice([1, 1, 1, 1, 2, 2, 3, 4]))
            for p in b.cluster(image_id, cells[picks[c]], n, SIDES[rng.randint(3)], [int(v) for v in rng.randint(1, K + 1, size=n)]):
                b.det_near(p, NOISES[rng.randint(len(NOISES))])
                if rng.rand() < 1 / 7:
                    b.det_near(p, 0.1)
    return b.build()


KPT_GROUPS_5 = ((1,), (2,), (3, 4), (5,))
# name -> (K, seed, labelled-key-point counts, evaluator settings, analysis settings)
CONFIGS = {
    'crowd17': (17, 31, (3, 8, 13, 17, 5, 10, 15, 16, 1, 6, 11), dict(sigmas=COCO_SIGMAS, use_nms=False), {}),
    'crowd5_nms': (5, 32, (1, 2, 3, 5, 4), dict(sigmas=[0.1] * 5, use_nms=True, oks_thre=0.95),
                   dict(num_kpt_groups=KPT_GROUPS_5)),
}
_cache = {}


def case(name):
    """(gt, preds, all_boxes, img_path, evaluator settings, analysis settings, reference) of a configuration; the
    reference (tests/helpers/kpt_analysis_ref.AnalysisRef, everything evaluated) is computed once."""
    if name not in _cache:
        from tests.helpers import kpt_analysis_ref as AR
        K, seed, counts, kw, akw = CONFIGS[name]
        gt, preds, boxes, paths = crowding_set(K, seed, counts)
        image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
        ref = AR.AnalysisRef(gt, preds, boxes, image_of, kw['sigmas'], oks_thre=kw.get('oks_thre', 0.5),
                             use_nms=kw['use_nms'], **akw)
        ref.run()
        _cache[name] = (gt, preds, boxes, paths, kw, akw, ref)
    return _cache[name]
