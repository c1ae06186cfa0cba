"""CPU suite (no GPU) for the crowding analysis (core/keypoint_analysis.py): the conditions on the seeded sets of
tests/helpers/kpt_analysis_cases.py, checked on the values of the restatement tests/helpers/kpt_analysis_ref.py alone;
the restatement's own invariants; that the sets hold what they claim; and the refusals at construction, which come
before any launch and so need no device."""
import numpy as np
import pytest

from tests.helpers import kpt_analysis_cases as cases
from tests.helpers import kpt_analysis_ref as AR

NAMES = sorted(cases.CONFIGS)


@pytest.mark.parametrize("name", NAMES)
def test_seeded_sets_meet_the_conditions_on_the_inputs(name):
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    iou_margin = np.abs(ref.ious - ref.iou_for_overlap).min()
    oks_margin = ref.threshold_margin()
    print(f"{name}: nearest IoU to iou_for_overlap {iou_margin:.3e}, nearest OKS to a threshold {oks_margin:.3e}")
    assert iou_margin > 1e-9
    assert oks_margin > 1e-9
    n = np.array([[ref.bins[(i, j)]['num_instances'] for j in range(len(ref.num_kpt_groups))]
                  for i in range(len(ref.overlap_groups))])
    assert n.shape == (3, 4) and np.count_nonzero(n) >= 9
    assert (n.sum(1) > 0).all() and (n.sum(0) > 0).all()            # every overlap group and every key point group is hit


@pytest.mark.parametrize("name", NAMES)
def test_restatement_invariants(name):
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    seen = set()
    for b in ref.bins.values():
        assert not (seen & set(b['ann_ids']))                       # bins are disjoint
        seen |= set(b['ann_ids'])
        assert b['num_instances'] == len(b['ann_ids'])
    in_some_group = [a for a in ref.anns if ref.valid[a]
                     and any(ref.num_overlaps[a] in g for g in ref.overlap_groups)
                     and any(ref.anns[a]['num_keypoints'] in g for g in ref.num_kpt_groups)]
    assert sum(b['num_instances'] for b in ref.bins.values()) == len(in_some_group) == len(seen)
    assert set(ref.persons) == {a for a in ref.anns if ref.valid[a]}
    rows = np.concatenate([b['dt_rows'] for b in ref.bins.values()])
    assert len(set(rows.tolist())) == rows.shape[0]                 # a detection is evaluated in one bin at the most


@pytest.mark.parametrize("name", NAMES)
def test_seeded_sets_hold_what_they_claim(name):
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    per_image = {}
    for a in gt['annotations']:
        per_image.setdefault(a['image_id'], []).append(a)
    ids = {im['id'] for im in gt['images']}
    assert ids - set(per_image) == {31} and len(per_image[12]) == 1 and len(per_image[17]) == 70
    # the three reasons for not counting, each on an annotation that overlaps a counted one
    why = {'kpts': 0, 'area': 0, 'box': 0}
    for a in per_image[23]:
        if not ref.valid[a['id']]:
            why['kpts' if max(a['keypoints']) == 0 else 'area' if a['area'] == 0 else 'box'] += 1
            assert any(AR.compute_iou(a['bbox'], o['bbox']) > 0.1 for o in per_image[23] if ref.valid[o['id']])
    assert why == {'kpts': 1, 'area': 1, 'box': 1} and sum(not v for v in ref.valid.values()) == 3
    counted = [a for a in per_image[23] if ref.valid[a['id']]]
    ious = {(a['id'], o['id']): AR.compute_iou(a['bbox'], o['bbox']) for a in counted for o in counted if a['id'] < o['id']}
    touching = [k for k, v in ious.items() if v == 0 and ref.anns[k[0]]['bbox'][0] + ref.anns[k[0]]['bbox'][2] == ref.anns[k[1]]['bbox'][0]
                and ref.anns[k[0]]['bbox'][2] > 0]
    assert touching and 1 in ious.values()
    zero = [a for a in counted if a['bbox'][2] * a['bbox'][3] == 0]
    assert len(zero) == 2 and zero[0]['bbox'] == zero[1]['bbox'] and ious[(zero[0]['id'], zero[1]['id'])] == 0
    assert max(ref.num_overlaps.values()) > 8
    stored = [a for a in gt['annotations'] if 'num_overlaps' in a]
    assert {ref.valid[a['id']] for a in stored} == {True, False}
    assert all(ref.num_overlaps[a['id']] == (a['num_overlaps'] if ref.valid[a['id']] else -1) for a in stored)
    assert any(a['iscrowd'] for a in gt['annotations'])
    # detections
    named = boxes[:, 6].astype(np.int64)
    assert (named == -1).any() and not (set(named.tolist()) - {-1} - set(ref.anns))
    image_of = np.array([int(p.split('/')[-1].split('.')[0]) for p in paths])
    abroad = [r for r in range(len(paths)) if named[r] in ref.anns and ref.anns[named[r]]['image_id'] != image_of[r]]
    evaluated = set(np.concatenate([b['dt_rows'] for b in ref.bins.values()]).tolist())
    assert {image_of[r] for r in abroad} == {31, 8}
    assert len([r for r in abroad if image_of[r] == 8 and r in evaluated]) == 1     # same bin as image 8's person
    assert len([r for r in abroad if image_of[r] == 8 and r not in evaluated]) == 1  # a bin image 8 lacks: dropped
    assert not any(r in p['dt_rows'] for r in abroad for p in ref.persons.values())
    # 23 detections of one bin in image 40: the cut to 20 after the bin filter differs from the cut before it
    (b40,) = [b for b in ref.bins.values() if sum(ref.anns[a]['image_id'] == 40 for a in b['ann_ids']) == 3]
    of_bin = [r for r in range(len(paths)) if image_of[r] == 40 and named[r] in b40['ann_ids'] and ref.keep[r]]
    in_image = [r for r in range(len(paths)) if image_of[r] == 40 and ref.keep[r]]
    top20 = sorted(in_image, key=lambda r: -ref.score[r])[:20]
    got = {r for r in b40['dt_rows'] if image_of[r] == 40}
    assert len(of_bin) == 23 and len(got) == 20 and got != {r for r in top20 if r in of_bin}
    # a person without a detection, one with 21 (20 evaluated), tied scores
    n_named = {a: int(((named == a) & ref.keep & (image_of == ref.anns[a]['image_id'])).sum()) for a in ref.persons}
    assert 0 in n_named.values() and 21 in n_named.values()
    assert all(len(p['dt_rows']) == min(n_named[a], 20) for a, p in ref.persons.items())
    assert len(np.unique(ref.score)) < len(ref.score)
    if kw['use_nms']:
        assert not ref.keep.all()


def _evaluator(gt, kw):
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    return KeypointEvaluator(gt, device='cpu', image_dir=cases.IMAGE_DIR, **kw)


def test_construction_refuses_before_any_launch():
    """Host tables only: the evaluator holds them on the CPU, and the refusals come before the first kernel."""
    from buctd_amd.core.keypoint_analysis import NUM_KPT_GROUPS, OVERLAP_GROUPS, CrowdingAnalysis
    assert OVERLAP_GROUPS == AR.OVERLAP_GROUPS and NUM_KPT_GROUPS == AR.NUM_KPT_GROUPS
    gt, preds, boxes, paths, kw, akw, ref = cases.case('crowd5_nms')
    no_size = dict(gt, images=[{k: v for k, v in im.items() if k != 'width'} if im['id'] == 17 else im for im in gt['images']])
    with pytest.raises(ValueError, match="width"):
        CrowdingAnalysis(_evaluator(no_size, kw), **akw)
    ev = _evaluator(gt, kw)
    with pytest.raises(ValueError, match="more than one group"):
        CrowdingAnalysis(ev, overlap_groups=((0, 1), (1, 2)), **akw)
    with pytest.raises(ValueError, match="empty"):
        CrowdingAnalysis(ev, num_kpt_groups=())
    # what the analysis reads from the evaluator, in gt_ids order
    by_id = {a['id']: a for a in gt['annotations']}
    assert [by_id[i]['num_keypoints'] for i in ev.gt_ids] == list(ev.gt_num_keypoints)
    assert ['num_overlaps' in by_id[i] for i in ev.gt_ids] == list(ev.gt_has_num_overlaps)
    assert ev.image_wh.shape == (6, 2) and (ev.image_wh == 2000).all()
