"""CPU suite (no GPU) for the keypoint evaluation: the COCOeval restatement the GPU test compares the kernels with
(tests/helpers/coco_kpt_eval_ref.py) and the product's host accumulation (core/keypoint_eval.accumulate / summarize, fed
with the restatement's match tables) against hand-derived figures; the condition on the seeded sets of
tests/test_gpu_keypoint_eval.py; and the restatement against pycocotools on a machine that has it."""
import numpy as np
import pytest

from tests.helpers import coco_kpt_eval_ref as R
from tests.helpers import kpt_eval_cases as cases

K = 5
SIG = [0.1] * K


def _gt_person(ann_id, image_id, center, size):
    """All joints labelled, on a ring of radius size / 2."""
    ang = np.arange(K) * 2 * np.pi / K
    xy = np.asarray(center, dtype=np.float64) + 0.5 * size * np.stack([np.cos(ang), np.sin(ang)], 1)
    kp = np.concatenate([xy, np.full((K, 1), 2.0)], 1)
    return {'id': ann_id, 'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in kp.reshape(-1)],
            'num_keypoints': K, 'area': float(size * size), 'iscrowd': 0,
            'bbox': [center[0] - size / 2, center[1] - size / 2, float(size), float(size)]}


def _set(persons):
    """persons: (image id, centre, size) -> gt dict."""
    anns = [_gt_person(1 + i, img, c, s) for i, (img, c, s) in enumerate(persons)]
    images = [{'id': i, 'file_name': f'{i}.jpg'} for i in sorted({p[0] for p in persons})]
    return {'images': images, 'annotations': anns, 'categories': [{'id': 1, 'name': 'animal'}]}


def _tables(gt, dets):
    """dets: (annotation to copy, shift in px, box score) -> preds, all_boxes, image ids."""
    by_id = {a['id']: a for a in gt['annotations']}
    preds = np.zeros((len(dets), K, 3), dtype=np.float32)
    boxes = np.zeros((len(dets), 7))
    image_of = []
    for r, (ann_id, shift, score) in enumerate(dets):
        a = by_id[ann_id]
        preds[r] = np.asarray(a['keypoints']).reshape(K, 3)
        preds[r, :, :2] += shift
        preds[r, :, 2] = 1.0                      # joint scores 1: the rescored score is the box score
        boxes[r, 4], boxes[r, 5], boxes[r, 6] = a['area'], score, ann_id
        image_of.append(a['image_id'])
    return preds, boxes, image_of


def _both(gt, dets):
    """The ten figures from the restatement, and from the product's accumulation fed with its match tables."""
    from buctd_amd.core import keypoint_eval as KE
    preds, boxes, image_of = _tables(gt, dets)
    ref = R.evaluate_ref(gt, preds, boxes, image_of, SIG, use_nms=False)
    precision, recall = KE.accumulate(ref['dt_scores'], ref['dt_matched'], ref['dt_ignored'], ref['npig'])
    stats = KE.summarize(precision, recall)
    assert np.array_equal(precision, ref['ev'].eval['precision']) and np.array_equal(recall, ref['ev'].eval['recall'])
    assert stats == ref['stats']
    assert KE.STATS_NAMES == R.STATS_NAMES
    return stats


# two images; sizes 50 (medium: 32^2 <= 2500 <= 96^2) and 150 (large), two of each
PERSONS = [(1, (200.0, 200.0), 50.0), (1, (600.0, 300.0), 150.0), (2, (300.0, 700.0), 50.0), (2, (800.0, 800.0), 150.0)]


def test_perfect_predictions_score_one():
    gt = _set(PERSONS)
    assert _both(gt, [(1, 0.0, 0.9), (2, 0.0, 0.8), (3, 0.0, 0.7), (4, 0.0, 0.6)]) == [1.0] * 10


def test_predictions_far_away_score_zero():
    gt = _set(PERSONS)
    stats = _both(gt, [(1, 1e4, 0.9), (2, 1e4, 0.8), (3, 1e4, 0.7), (4, 1e4, 0.6)])
    assert stats == [0.0] * 10


def test_one_found_one_missed_and_no_medium_ground_truth():
    """One image, two large ground truths, one found exactly: recall 0.5; precision 1 at the 51 recall points <= 0.5 and
    0 above, so AP = 51/101 (the single true positive's precision is 1 / (1 + spacing(1)), within 1e-12).  No medium
    ground truth: AP (M) and AR (M) are -1."""
    gt = _set([(4, (300.0, 300.0), 150.0), (4, (900.0, 900.0), 150.0)])
    stats = dict(zip(R.STATS_NAMES, _both(gt, [(1, 0.0, 0.9)])))
    assert stats['AR'] == 0.5 and stats['AR .5'] == 0.5 and stats['AR (L)'] == 0.5
    for name in ('AP', 'AP .5', 'AP .75', 'AP (L)'):
        assert abs(stats[name] - 51 / 101) <= 1e-12, (name, stats[name])
    assert stats['AP (M)'] == -1 and stats['AR (M)'] == -1


def test_equal_scores_keep_input_order():
    """Two detections with one score on one ground truth, a miss and a hit: miss first gives precision (0, 1/2) -> AP 1/2,
    hit first gives AP 1.  The same across two images: the image with the smaller id comes first."""
    gt = _set([(1, (300.0, 300.0), 150.0)])
    assert abs(_both(gt, [(1, 1e4, 0.5), (1, 0.0, 0.5)])[0] - 0.5) <= 1e-12
    assert abs(_both(gt, [(1, 0.0, 0.5), (1, 1e4, 0.5)])[0] - 1.0) <= 1e-12
    gt = _set([(1, (300.0, 300.0), 150.0), (2, (300.0, 300.0), 150.0)])
    assert abs(_both(gt, [(2, 0.0, 0.5), (1, 1e4, 0.5)])[0] - 0.5 * 51 / 101) <= 1e-12   # image 1's miss first: precision 1/2 up to recall 1/2
    assert abs(_both(gt, [(2, 1e4, 0.5), (1, 0.0, 0.5)])[0] - 51 / 101) <= 1e-12  # image 1's hit first


def test_rescoring_restatement_by_hand():
    preds = np.zeros((2, 3, 3), dtype=np.float32)
    preds[0, :, 2] = [0.5, 0.25, 0.1]
    preds[1, :, 2] = [0.1, 0.05, 0.0]
    boxes = np.zeros((2, 7))
    boxes[:, 4], boxes[:, 5] = 100.0, [0.5, 0.8]
    s, b, k, keep, _ = R.rescore_and_nms(preds, boxes, [1, 1], 0.2, 0.9, [0.1] * 3, False)
    assert list(k) == [0.375, 0.0] and list(s) == [0.1875, 0.0] and list(b) == [0.5, 0.8] and keep.all()


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
def test_seeded_sets_meet_the_condition_on_the_inputs(name):
    """No reference OKS within 1e-9 of a threshold it is compared with, and the sets hold what they claim."""
    gt, preds, boxes, paths, kw, ref = cases.case(name)
    assert cases.threshold_margin(name) > 1e-9
    per_image = {}
    for p in paths:
        per_image[p] = per_image.get(p, 0) + 1
    counts = sorted(per_image.values())
    if name.startswith('match'):
        assert len(gt['images']) == 12 and 23 in counts
        n_gt = {}
        for a in gt['annotations']:
            n_gt[a['image_id']] = n_gt.get(a['image_id'], 0) + 1
        assert 70 in n_gt.values()
        with_dets = {int(p.split('/')[-1].split('.')[0]) for p in paths}
        ids = {im['id'] for im in gt['images']}
        assert (set(n_gt) - with_dets) and (with_dets - set(n_gt)) and (ids - with_dets - set(n_gt))
        assert any(a['num_keypoints'] == 0 for a in gt['annotations']) and any(a['iscrowd'] for a in gt['annotations'])
        areas = np.array([a['area'] for a in gt['annotations']])
        assert (areas < 32 ** 2).any() and ((areas > 32 ** 2) & (areas < 96 ** 2)).any() and (areas > 96 ** 2).any()
        if not kw['use_nms']:
            assert ref['keep'].all() and len(ref['dt_rows']) == len(paths) - 3      # 23 cut to 20
    else:
        assert counts == [1, 64, 65, 130]
        assert not ref['keep'].all() and (ref['keypoint_score'] == 0).any()
    assert len(np.unique(ref['score'])) < len(ref['score'])                           # tied scores
    assert ref['dt_matched'].any() and ref['dt_ignored'].any()


def test_restatement_against_pycocotools():
    """Closes the gap on a machine that has pycocotools: the ten figures of the restatement against COCOeval's."""
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    for name in ('match17', 'match5'):
        gt, preds, boxes, paths, kw, ref = cases.case(name)
        coco = COCO()
        coco.dataset = gt
        coco.createIndex()
        image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
        results = [{'image_id': image_of[r], 'category_id': 1, 'keypoints': [float(v) for v in preds[r].reshape(-1)],
                    'score': float(ref['score'][r])} for r in range(len(paths)) if ref['keep'][r]]
        ev = COCOeval(coco, coco.loadRes(results), 'keypoints')
        ev.params.kpt_oks_sigmas = np.asarray(kw['sigmas'], dtype=np.float64)
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        assert np.abs(np.asarray(ev.stats) - np.asarray(ref['stats'])).max() <= 1e-12
