"""GPU suite for the keypoint evaluation (core/keypoint_eval.py over csrc/keypoint_eval.hip) against the fp64 restatement
tests/helpers/coco_kpt_eval_ref.py on the seeded sets of tests/helpers/kpt_eval_cases.py:

  match17 / match5 / match17_nms   12 images at K = 17 (COCO sigmas) and K = 5 ([0.1] * 5): an image with ground truths and
      no detections, one with detections and no ground truth, one with neither, 23 detections cut to 20, 70 ground truths
      (more than a wavefront), a ground truth with num_keypoints == 0 (bbox-distance form), a crowd overlapped by two
      detections, areas in all three ranges, tied scores;
  nms17 / nms5_vis   images with 1, 64, 65 and 130 persons, near-duplicates of every closeness, persons with no joint
      above in_vis_thre, with and without the joint-score threshold inside the suppression's OKS.

Condition on the inputs (checked first, on the restatement's values alone, and on the CPU in test_keypoint_eval.py): no
reference OKS within 1e-9 of a threshold it is compared with.  Under it: OKS matrices and rescored scores within 1e-12
absolute (fp64 values in [0, 1] from a few dozen rounded operations and a <= 1 ulp exp), keep masks, dt_matched and
dt_ignored exactly equal, the ten figures within 1e-12."""
import ctypes as C
import json
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import kpt_eval_cases as cases

pytestmark = pytest.mark.gpu
CFG = SimpleNamespace(OUTPUT_JSON='')
KEYS = {'image_id', 'image_path', 'category_id', 'keypoints', 'score', 'center', 'scale', 'annotation_id', 'box_score',
        'keypoint_score'}


def _evaluator(name, dev, **over):
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, preds, boxes, paths, kw, ref = cases.case(name)
    return KeypointEvaluator(gt, device=dev, image_dir=cases.IMAGE_DIR, **dict(kw, **over))


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
def test_tables_and_figures_equal_the_restatement(dev, name):
    gt, preds, boxes, paths, kw, ref = cases.case(name)
    assert cases.threshold_margin(name) > 1e-9
    ev = _evaluator(name, dev)
    name_value, ap = ev.evaluate(CFG, preds, None, boxes, paths, 0)
    t = ev.tables
    for k in ('score', 'box_score', 'keypoint_score'):
        err = np.abs(t[k] - ref[k]).max()
        print(f"{name}: max |{k} - reference| = {err:.3e}")
        assert err <= 1e-12
    assert np.array_equal(t['keep'], ref['keep'])
    assert np.array_equal(t['dt_rows'], ref['dt_rows'])
    worst = 0.0
    for pos, image_id in enumerate(t['image_ids']):
        want = np.asarray(ref['oks'][int(image_id)])
        got = t['oks'][pos]
        if want.size == 0:
            assert got.size == 0
            continue
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{name}: max |OKS - reference| = {worst:.3e}")
    assert worst <= 1e-12
    matched_ids = np.where(t['dt_matched'] > 0, t['gt_ids'][np.maximum(t['dt_matched'] - 1, 0)], 0)
    assert np.array_equal(matched_ids, ref['dt_matched'])
    assert np.array_equal(t['dt_ignored'] != 0, ref['dt_ignored'])
    assert np.array_equal(ev.npig, ref['npig'])
    err = np.abs(np.asarray(t['stats']) - np.asarray(ref['stats'])).max()
    print(f"{name}: figures {t['stats']}, max |figure - reference| = {err:.3e}")
    assert err <= 1e-12
    assert ap == name_value['AP'] == t['stats'][0]


def test_interface_of_validate(dev, tmp_path):
    """Tables shaped like validate()'s through the signature validate() calls; the results file has the reference's keys;
    use_nms=False keeps every person."""
    gt, preds, boxes, paths, kw, ref = cases.case('match17')
    assert preds.dtype == np.float32 and preds.shape[1:] == (17, 3) and boxes.shape == (preds.shape[0], 7)
    ev = _evaluator('match17', dev)
    name_value, ap = ev.evaluate(CFG, preds, str(tmp_path), boxes, paths, 3, [], [])
    assert isinstance(name_value, OrderedDict)
    assert list(name_value) == ['AP', 'AP .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
    assert ap == name_value['AP'] and all(isinstance(v, float) for v in name_value.values())
    assert ev.tables['keep'].all()
    res = json.load(open(os.path.join(str(tmp_path), 'results', 'keypoints_val_results_epoch3.json')))
    assert len(res) == preds.shape[0] and all(set(r) == KEYS for r in res)
    (first,) = [r for r in res if r['keypoints'] == [float(v) for v in preds[0].reshape(-1)]]
    assert len(first['keypoints']) == 51 and first['annotation_id'] == int(boxes[0, 6]) and first['box_score'] == boxes[0, 5]
    assert first['score'] == ev.tables['score'][0] and first['image_path'] == '/'.join(paths[0].split('/')[-3:])
    assert first['center'] == list(boxes[0, 0:2]) and first['scale'] == list(boxes[0, 2:4]) and first['category_id'] == 1
    # cfg.OUTPUT_JSON names the file; a ready dict and a callable map paths as well
    out = tmp_path / 'named.json'
    by_path = {p: int(p.split('/')[-1].split('.')[0]) for p in paths}
    for image_ids in (by_path, by_path.__getitem__):
        ev2 = _evaluator('match17_nms', dev, image_ids=image_ids)
        g2, p2, b2, paths2 = cases.case('match17_nms')[:4]
        nv2, _ = ev2.evaluate(SimpleNamespace(OUTPUT_JSON=str(out)), p2, str(tmp_path), b2, paths2)
        assert len(json.load(open(out))) == int(ev2.tables['keep'].sum()) < p2.shape[0]
        assert list(nv2.values()) == ev2.tables['stats']
    with pytest.raises(NotImplementedError):
        _evaluator('match17', dev, soft_nms=True)


def test_two_runs_are_bit_identical(dev):
    gt, preds, boxes, paths, kw, ref = cases.case('nms17')
    runs = []
    for _ in range(2):
        ev = _evaluator('nms17', dev)
        ev.evaluate(CFG, preds, None, boxes, paths)
        runs.append(ev.tables)
    for k in ('score', 'box_score', 'keypoint_score', 'keep', 'order', 'dt_rows', 'oks_flat', 'dt_matched', 'dt_ignored',
              'precision', 'recall'):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert runs[0]['stats'] == runs[1]['stats']


def test_refusals_come_before_any_launch(dev):
    from buctd_amd import _C
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, preds, boxes, paths, kw, ref = cases.case('match5')
    with pytest.raises(ValueError):
        KeypointEvaluator(gt, sigmas=[0.1] * 4, device=dev, image_dir=cases.IMAGE_DIR)      # sigmas length != K
    ev = _evaluator('match5', dev)
    with pytest.raises(ValueError):
        ev.evaluate(CFG, preds[:, :4], None, boxes, paths)
    with pytest.raises(KeyError):
        ev.evaluate(CFG, preds, None, boxes, paths[:-1] + ['data/synth/images/999999.jpg'])
    assert ev.tables is None
    # too small a workspace through the C ABI
    lib = _C.lib()
    need = lib.buctd_coco_kpt_match_workspace(4, 10, 3)
    assert need == 4 * 3 * 4 + 4 * 30
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
    dt_off, gt_off, oks_off = i32(0, 2), i32(0, 4), torch.tensor([0, 8], dtype=torch.int64, device=dev)
    dt_kpts, gt_kpts, area, bbox, flags = torch.zeros(2 * 5 * 3, device=dev), f64(4 * 5 * 3), f64(4), f64(16), i32(0, 0, 0, 0)
    sig, thr, rng, oks = f64(5), f64(10), f64(6), f64(8)
    dtm, dti = torch.full((60,), -7, dtype=torch.int32, device=dev), torch.full((60,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    m = _C.KptMatchArgs(images=1, K=5, n_thr=10, n_area=3, dt_total=2, gt_total=4, dt_offsets=_C.ptr(dt_off),
                        gt_offsets=_C.ptr(gt_off), oks_offsets=_C.ptr(oks_off), dt_kpts=_C.ptr(dt_kpts),
                        gt_kpts=_C.ptr(gt_kpts), gt_area=_C.ptr(area), gt_bbox=_C.ptr(bbox), gt_flags=_C.ptr(flags),
                        sigmas=_C.ptr(sig), thresholds=_C.ptr(thr), area_ranges=_C.ptr(rng), oks=_C.ptr(oks),
                        dt_matched=_C.ptr(dtm), dt_ignored=_C.ptr(dti))
    rc = lib.buctd_coco_kpt_match(C.byref(m), _C.ptr(ws), need - 1, _C.stream_ptr())
    assert rc == -3 and b"workspace" in lib.buctd_last_error()                              # BUCTD_EWORKSPACE
    assert lib.buctd_coco_kpt_match(C.byref(m), None, 0, _C.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool((dtm == -7).all()) and bool((dti == -7).all())                               # nothing ran
