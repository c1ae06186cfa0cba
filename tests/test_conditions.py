"""Host checks of the condition-record tests' own ground: the seeded sets of tests/helpers/condition_cases.py hold every
situation their docstring lists, the restatement tests/helpers/condition_ref.py gives a few hand-derived values, and its
match equals what the reference's script wrote for the pair under tests/golden/conditions_match.json (recorded by
tests/helpers/make_condition_golden.py).  No GPU; tests/test_gpu_conditions.py compares the package with the
restatement."""
import json
import os

import numpy as np
import pytest

from tests.helpers import condition_cases as cases
from tests.helpers import condition_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conditions_match.json")


@pytest.mark.parametrize("K", [17, 5])
def test_the_sets_hold_every_listed_situation(K):
    c, r = cases.case(K), cases.reference(K)
    anns, results, rows = c['gt']['annotations'], c['results'], r['rows']
    ann_images, res_images = {a['image_id'] for a in anns}, {x['image_id'] for x in results}
    assert ann_images - res_images and res_images - ann_images                 # no predictions / no annotations
    per_image = np.bincount([a['image_id'] for a in anns])
    assert {1, 63, 64, 65, 130} <= set(per_image.tolist())
    assert {1, 63, 64, 65, 130} <= {len(b['preds']) for b in c['bu_results']}
    assert any(w['matched'] >= 0 and max(w['ious']) == 0 and len(w['ious']) > 1 for w in rows)    # best IoU 0
    tie = [w for w in rows if w['ious'] and sorted(w['ious'])[-1] > 0 and w['ious'].count(max(w['ious'])) > 1]
    assert tie and all(w['matched'] == min(i for i, x in enumerate(results) if x['keypoints'] == results[w['matched']]['keypoints'])
                       for w in tie)
    assert [w['status'] for w in rows].count(1) == 1 and all(w['matched'] == -1 for w in rows if w['status'])
    kp = np.array([a['keypoints'] for a in anns], dtype=np.float64).reshape(len(anns), K, 3)
    assert ((kp[:, :, 2] == 0) & (kp[:, :, 0] != 0) & (kp[:, :, 1] != 0)).any()                  # v == 0 with coordinates
    pred = np.array([x['keypoints'] for x in results]).reshape(len(results), K, 3)
    assert (pred[:, :, :2].min(axis=1) < 0).any()                                                # a corner to clip
    assert ref.nonzero_box(cases.bad_pose(K), cases.MARGIN) is None
    overlaps = r['overlaps']
    first = {t['annotation_id']: n for n, t in enumerate(r['train_db'])}
    assert any((o == 1).sum() > 1 for o in overlaps.values())                                   # 1 with another member
    assert [t['overlap_status'] for t in r['train_db']].count(2) >= 1
    touching = [a for a in anns if a['image_id'] == 23][-2:]
    assert overlaps[touching[0]['id']][-1] == 0 and touching[0]['bbox'][0] + touching[0]['bbox'][2] - 1 == touching[1]['bbox'][0]
    assert any(x['category_id'] != 1 for x in results)
    scores = [s for b in c['bu_results'] for s in b['scores']]
    assert min(scores) < cases.IMAGE_THRE < max(scores) and len(r['test_db']) < len(scores)
    lone = [b for b in c['bu_results'] if b['image_paths'][0].endswith('000022.jpg')][0]
    kept = [t for t in r['test_db'] if t['image'] == lone['image_paths'][0]]
    assert len(lone['preds']) == 2 and len(kept) == 1 and kept[0]['cond_max_iou'] > 0            # the dropped pose supplies it
    assert first                                                                                 # train records exist


def test_the_restatement_on_hand_derived_values():
    # two 2 x 2 squares shifted by one in x: intersection 2, union 6
    assert ref.corner_iou([0, 0, 2, 2], [1, 0, 3, 2]) == 1 / 3
    assert ref.xywh_iou([0, 0, 2, 2], [1, 0, 2, 2]) == 1 / 3
    assert ref.xywh_overlap([0, 0, 2, 2], [1, 0, 2, 2]) == (1 / 3, False)
    assert ref.corner_iou([0, 0, 2, 2], [2, 0, 4, 2]) == 0 and ref.xywh_overlap([0, 0, 0, 5], [0, 0, 0, 5]) == (0.0, True)
    # negative corners are set to 0
    assert ref.corner_boxes([[[-3.0, 4.0], [5.0, -1.0]]]).tolist() == [[0.0, 0.0, 5.0, 4.0]]
    # the all-zero argmax quirk: no prediction overlaps, the first of the image is the match
    square = lambda x, y: [x, y, 2, x + 2, y, 2, x, y + 2, 2]
    gt = {'images': [], 'annotations': [{'id': 1, 'image_id': 7, 'category_id': 1, 'keypoints': square(10, 10)}]}
    results = [{'image_id': 8, 'category_id': 1, 'keypoints': square(10, 10)},
               {'image_id': 7, 'category_id': 1, 'keypoints': square(50, 50)},
               {'image_id': 7, 'category_id': 1, 'keypoints': square(80, 80)}]
    out, rows = ref.match_annotations(gt, results, 'm')
    assert rows[0]['matched'] == 1 and rows[0]['best_iou'] == 0 and rows[0]['ious'] == [0, 0]
    assert out['annotations'][0]['cond_kpts']['m'] == square(50, 50)
    # v == 0 zeroes the joint, whatever the prediction says
    gt['annotations'][0]['keypoints'][2] = 0
    assert ref.match_annotations(gt, results, 'm')[0]['annotations'][0]['cond_kpts']['m'][:3] == [0, 0, 0]
    # the != 1 exclusion: two members with one box and a third: the twin's overlap of 1 does not count
    person = lambda i, box: {'id': i, 'image_id': 7, 'category_id': 1, 'bbox': box, 'keypoints': square(12, 12)}
    gt = {'images': [{'id': 7, 'width': 100, 'height': 100, 'file_name': 'a.jpg'}],
          'annotations': [person(1, [10, 10, 3, 3]), person(2, [10, 10, 3, 3]), person(3, [11, 10, 3, 3])]}
    db, overlaps = ref.train_records(gt, 3, 2 / 3, 1.25)
    assert overlaps[1].tolist() == [1.0, 1.0, 1 / 3] and db[0]['cond_max_iou'] == 1 / 3 and len(db[0]['near_joints']) == 3
    db, _ = ref.train_records({'images': gt['images'], 'annotations': gt['annotations'][:2]}, 3, 2 / 3, 1.25)
    assert db[0]['cond_max_iou'] == 0                                      # nothing is left (the reference raises here)


def test_the_restated_match_equals_the_scripts_output():
    d = json.load(open(GOLDEN))
    assert len(d['cond_kpts']) == len(d['gt']['annotations']) >= 8
    out, rows = ref.match_annotations(d['gt'], d['results'], d['model'])
    for ann in out['annotations']:
        assert ann['cond_kpts'][d['model']] == d['cond_kpts'][str(ann['id'])], ann['id']
    assert any(w['best_iou'] == 0 for w in rows) and any(0 in a['keypoints'][2::3] for a in d['gt']['annotations'])
