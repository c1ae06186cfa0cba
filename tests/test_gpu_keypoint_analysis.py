"""GPU suite for the crowding analysis (core/keypoint_analysis.py over buctd_kpt_crowding / buctd_kpt_segment_ap /
buctd_coco_kpt_match in csrc/keypoint_eval.hip) against the restatement tests/helpers/kpt_analysis_ref.py on the seeded
sets of tests/helpers/kpt_analysis_cases.py (K = 17 on the COCO sigmas without suppression, K = 5 with it; what the
sets hold is listed there and checked in tests/test_keypoint_analysis.py).

Conditions on the inputs (restatement's values alone): no box IoU within 1e-9 of iou_for_overlap, no OKS within 1e-9 of
a threshold it is compared with.  Under them valid, num_overlaps, bin_of_gt, and per bin and per person the evaluated
detection rows, dt_matched (as ground-truth ids) and dt_ignored are exactly equal.  The figures agree within 1e-12
absolute: each is a mean of at most 1010 fp64 values in [0, 1], and re-associating that sum moves it by at most
1010 * 2^-53 = 1.1e-13 (the bar of tests/test_gpu_keypoint_eval.py for the same quantities).
Measured on an MI355X: largest difference of a bin figure 0.0, of a person's figure 4.4e-16."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import kpt_analysis_cases as cases

pytestmark = pytest.mark.gpu
NAMES = sorted(cases.CONFIGS)
CFG = SimpleNamespace(OUTPUT_JSON='')


def _analysis(name, dev):
    from buctd_amd.core.keypoint_analysis import CrowdingAnalysis
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    ev = KeypointEvaluator(gt, device=dev, image_dir=cases.IMAGE_DIR, **kw)
    return ev, CrowdingAnalysis(ev, **akw)


def _conditions(ref):
    assert np.abs(ref.ious - ref.iou_for_overlap).min() > 1e-9
    assert ref.threshold_margin() > 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_overlap_counts_and_bins_of_the_annotations(dev, name):
    ref = cases.case(name)[-1]
    _conditions(ref)
    ev, an = _analysis(name, dev)
    ids = [int(i) for i in ev.gt_ids]
    assert an.valid.dtype == bool and list(an.valid) == [ref.valid[i] for i in ids]
    assert list(an.num_overlaps) == [ref.num_overlaps[i] for i in ids]
    assert list(an.bin_of_gt) == [ref.bin_of[i] for i in ids]


@pytest.mark.parametrize("name", NAMES)
def test_bin_tables_and_figures_equal_the_restatement(dev, name):
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    _conditions(ref)
    ev, an = _analysis(name, dev)
    tables = an.bins(preds, boxes, paths)
    n_kpt = len(an.num_kpt_groups)
    assert list(tables) == ['num_instances'] + ['AP', 'AP .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
    worst = 0.0
    for (i, j), want in ref.bins.items():
        got = an.bin_tables[i * n_kpt + j]
        assert tables['num_instances'][i, j] == want['num_instances']
        assert sorted(got['gt_ids']) == sorted(want['ann_ids'])
        assert np.array_equal(got['dt_rows'], want['dt_rows']), (i, j)
        assert np.array_equal(got['dt_matched'], want['dt_matched']), (i, j)
        assert np.array_equal(got['dt_ignored'], want['dt_ignored']), (i, j)
        assert np.array_equal(got['npig'], want['npig'])
        figures = np.array([tables[k][i, j] for k in list(tables)[1:]])
        worst = max(worst, float(np.abs(figures - np.asarray(want['stats'])).max()))
    print(f"{name}: largest |bin figure - reference| = {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_person_tables_and_figures_equal_the_restatement(dev, name):
    gt, preds, boxes, paths, kw, akw, ref = cases.case(name)
    _conditions(ref)
    ev, an = _analysis(name, dev)
    per = an.instances(preds, boxes, paths)
    t = an.instance_tables
    assert list(per) == [int(i) for i in ev.gt_ids[an.valid]] and set(per) == set(ref.persons)
    worst = 0.0
    for s, ann_id in enumerate(per):
        want = ref.persons[ann_id]
        d0, d1 = t['dt_offsets'][s], t['dt_offsets'][s + 1]
        assert np.array_equal(t['dt_rows'][d0:d1], want['dt_rows']), ann_id
        assert np.array_equal(np.where(t['dt_matched'][:, :, d0:d1] > 0, ann_id, 0), want['dt_matched']), ann_id
        assert np.array_equal(t['dt_ignored'][:, :, d0:d1] != 0, want['dt_ignored']), ann_id
        assert np.array_equal(t['npig'][s], want['npig'])
        assert list(per[ann_id]) == ['AP', 'AP .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
        worst = max(worst, float(np.abs(np.array(list(per[ann_id].values())) - np.asarray(want['stats'])).max()))
    print(f"{name}: largest |person figure - reference| = {worst:.3e} over {len(per)} persons")
    assert worst <= 1e-12


def test_two_runs_are_bit_identical_and_files_are_written(dev, tmp_path):
    gt, preds, boxes, paths = cases.case('crowd17')[:4]
    runs = []
    for _ in range(2):
        ev, an = _analysis('crowd17', dev)
        tables, per = an.bins(preds, boxes, paths), an.instances(preds, boxes, paths)
        runs.append((an, tables, per))
    (a0, t0, p0), (a1, t1, p1) = runs
    for k in ('valid', 'num_overlaps', 'bin_of_gt'):
        assert getattr(a0, k).tobytes() == getattr(a1, k).tobytes(), k
    for k in t0:
        assert t0[k].tobytes() == t1[k].tobytes(), k
    for k in ('dt_rows', 'dt_matched', 'dt_ignored', 'stats', 'recall'):
        assert a0.instance_tables[k].tobytes() == a1.instance_tables[k].tobytes(), k
    assert p0 == p1
    written = a0.write(str(tmp_path))
    assert [os.path.basename(w) for w in written] == ['benchmark_tables.json', 'instance_ap.json']
    on_disk = json.load(open(written[0]))
    assert on_disk['AP'] == t0['AP'].tolist() and on_disk['num_instances'] == t0['num_instances'].tolist()
    assert json.load(open(written[1])) == {str(k): dict(v) for k, v in p0.items()}


def test_the_evaluator_is_left_as_it_was(dev):
    """evaluate() before and after an analysis on the same evaluator: the same tables byte for byte."""
    gt, preds, boxes, paths = cases.case('crowd5_nms')[:4]
    ev, an = _analysis('crowd5_nms', dev)
    before, _ = ev.evaluate(CFG, preds, None, boxes, paths)
    t_before = ev.tables
    an.bins(preds, boxes, paths)
    an.instances(preds, boxes, paths)
    assert ev.tables is t_before
    after, _ = ev.evaluate(CFG, preds, None, boxes, paths)
    assert list(before.items()) == list(after.items())
    for k, v in t_before.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == ev.tables[k].tobytes(), k
    assert t_before['stats'] == ev.tables['stats']


def test_c_abi_refusals_come_before_any_launch(dev):
    from buctd_amd import _C
    lib, st = _C.lib(), _C.stream_ptr()
    EINVAL = -1
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    f64 = lambda n, v=-7.0: torch.full((n,), v, dtype=torch.float64, device=dev)
    seg_off, npig, rec = i32(0, 2), i32(1, 1, 1, 1, 1, 1, 1), f64(101, 0.5)
    dtm, dti = torch.zeros(70 * 65, dtype=torch.int32, device=dev), torch.zeros(70 * 65, dtype=torch.int32, device=dev)
    stats, recall = f64(10), f64(70)
    P = _C.ptr

    def segment_ap(n_area=3, n_thr=10, max_len=2, dt_total=2, n_rec=101, stats_ptr=P(stats)):
        return lib.buctd_kpt_segment_ap(P(seg_off), 1, max_len, dt_total, P(dtm), P(dti), n_area, n_thr, P(npig), P(rec),
                                        n_rec, 0, 5, stats_ptr, P(recall), st)
    assert segment_ap(n_area=7, n_thr=10) == EINVAL and b"64 pairs" in lib.buctd_last_error()
    assert segment_ap(max_len=65, dt_total=65) == EINVAL and b"64 detections" in lib.buctd_last_error()
    assert segment_ap(n_rec=129) == EINVAL and b"128" in lib.buctd_last_error()
    assert segment_ap(stats_ptr=None) == EINVAL and b"null" in lib.buctd_last_error()
    off, bbox, kpts, area, wh = i32(0, 2), f64(8, 1.0), f64(2 * 5 * 3, 1.0), f64(2, 1.0), f64(2, 100.0)
    valid, count = i32(-7, -7), i32(-7, -7)
    for nulled in range(7):
        a = [P(off), P(bbox), P(kpts), P(area), P(wh), P(valid), P(count)]
        a[nulled] = None
        assert lib.buctd_kpt_crowding(a[0], 1, 2, 5, a[1], a[2], a[3], a[4], 0.1, a[5], a[6], st) == EINVAL
        assert b"null" in lib.buctd_last_error()
    torch.cuda.synchronize()
    assert bool((stats == -7).all()) and bool((recall == -7).all())                     # nothing ran
    assert bool((valid == -7).all()) and bool((count == -7).all())
