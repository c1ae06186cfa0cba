"""GPU suite for the soft OKS suppression (buctd_soft_oks_nms_grouped of csrc/keypoint_eval.hip under
nms.soft_oks_nms_grouped / gpu_soft_oks_nms / gpu_oks_nms and KeypointEvaluator(suppression='soft')) against the fp64
restatement tests/helpers/soft_nms_ref.py on the seeded sets of tests/helpers/soft_nms_cases.py.

Condition on the inputs (tests/test_soft_nms.py checks it on the CPU, on the restatement's values alone): outside the
dedicated tie pair no two live scores an arg-max compares lie within 1e-9 relative of each other, and for the linear decay
no OKS lies within 1e-9 of the threshold.  Under it the ranks are exactly equal.  The soft scores are fp64 products of at
most 20 factors, each an OKS of a few dozen rounded operations and <= 1 ulp exps, squared, divided and put through one
more exp: within 1e-12 relative, the bar of tests/test_gpu_keypoint_eval.py."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import oks_nms_cases as hard
from tests.helpers import soft_nms_cases as cases
from tests.helpers import soft_nms_ref as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nms.npz")
VARIANTS = [(d, v) for d in ('gaussian', 'linear') for v in (False, True)]
CFG = SimpleNamespace(OUTPUT_JSON='')


def _device_tables(name, dev):
    g, kw = cases.grouped(name), cases.case(name)[4]
    t = lambda a: torch.as_tensor(a).to(dev)
    return t(g['offsets']), t(g['kpts']), t(g['areas']), t(g['scores']), t(kw['sigmas'])


def _run(name, dev, decay, use_vis):
    from buctd_amd.nms.nms import soft_oks_nms_grouped
    off, kp, ar, sc, sig = _device_tables(name, dev)
    rank, soft = soft_oks_nms_grouped(off, kp, ar, sc, sig, cases.case(name)[4]['thresh'], decay=decay,
                                      in_vis_thre=cases.VIS_THRE if use_vis else None, max_keep=20)
    assert rank.dtype == torch.int32 and soft.dtype == torch.float64 and rank.shape == soft.shape == sc.shape
    return rank.cpu().numpy(), soft.cpu().numpy()


def _rel_err(got, want):
    return float((np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)).max()) if want.size else 0.0


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
@pytest.mark.parametrize("decay,use_vis", VARIANTS)
def test_grouped_equals_the_restatement(dev, name, decay, use_vis):
    ref = cases.reference(name, decay, use_vis)
    rank, soft = _run(name, dev, decay, use_vis)
    assert np.array_equal(rank, ref['rank'])
    err = _rel_err(soft, ref['soft_score'])
    print(f"{name} {decay} vis={use_vis}: max relative |soft_score - reference| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("decay,use_vis", VARIANTS)
def test_equal_scores_keep_grouped_order(dev, decay, use_vis):
    g = cases.grouped('soft17')
    rank, soft = _run('soft17', dev, decay, use_vis)
    a = int(g['offsets'][g['image_ids'].index(cases.TIE_IMAGE)])
    p0, p1 = cases.tie_positions('soft17')
    assert p0 < p1 and g['scores'][a + p0] == g['scores'][a + p1]
    assert rank[a + p0] > 0 and rank[a + p1] == rank[a + p0] + 1          # not first: the tie survived a decay round
    assert soft[a + p0] == soft[a + p1] == g['scores'][a + p0]            # every factor was exactly 1.0


@pytest.mark.parametrize("name", sorted(hard.CONFIGS))
@pytest.mark.parametrize("use_vis", (False, True))
def test_hard_grouped_equals_the_host_oks_nms(dev, name, use_vis):
    """nms.oks_nms_grouped over one multi-image group (0, 1, 2, 63, 64, 65 and 129 persons) against nms.oks_nms per
    image: the kept sets are equal - the sets hold no OKS within 1e-9 of the threshold (tests/test_soft_nms.py)."""
    from buctd_amd.nms.nms import oks_nms_grouped
    c = hard.case(name)
    off, kp, ar, sig = (torch.as_tensor(np.array(c[k])).to(dev) for k in ('offsets', 'kpts', 'areas', 'sigmas'))
    vis = hard.VIS_THRE if use_vis else None
    keep = oks_nms_grouped(off, kp, ar, sig, c['thresh'], in_vis_thre=vis)
    assert keep.dtype == torch.int32 and keep.shape == ar.shape and keep.device == kp.device
    assert np.array_equal(keep.cpu().numpy(), c['keep'][use_vis])
    # the bitmap sized by the caller or read from offsets, and a second run: the same bits
    sized = oks_nms_grouped(off, kp, ar, sig, c['thresh'], in_vis_thre=vis, max_per_image=max(hard.COUNTS))
    again = oks_nms_grouped(off, kp, ar, sig, c['thresh'], in_vis_thre=vis)
    assert keep.cpu().numpy().tobytes() == sized.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    # no person: nothing to keep; no image: every person is kept, nothing ran
    for offsets in (torch.zeros_like(off), off[:1]):
        none = oks_nms_grouped(offsets, kp[:0], ar[:0], sig, c['thresh'], in_vis_thre=vis)
        assert none.dtype == torch.int32 and none.shape == (0,)
    assert bool((oks_nms_grouped(off[:1], kp, ar, sig, c['thresh'], in_vis_thre=vis) == 1).all())


def _db(g, tag):
    k = g[f"kpts_{tag}"]
    return [{"keypoints": k[i].reshape(-1, 3), "score": float(g[f"scores_{tag}"][i]), "area": float(g[f"areas_{tag}"][i])}
            for i in range(k.shape[0])]


def test_entry_points_match_the_reference_golden(dev):
    import buctd_amd.nms.nms as pn
    g = np.load(GOLD)
    for tag in "pq":
        sig = g[f"sigmas_{tag}"] if f"sigmas_{tag}" in g.files else None
        db = _db(g, tag)
        soft = pn.gpu_soft_oks_nms(db, 0.6, sig)
        assert isinstance(soft, np.ndarray) and soft.tolist() == g[f"softnms_{tag}"].tolist() and len(soft) <= 20
        assert pn.gpu_oks_nms(db, 0.6, sig) == g[f"oksnms_{tag}"].tolist()
        assert pn.gpu_oks_nms(db, 0.6, sig, 0.3) == g[f"oksnmsvis_{tag}"].tolist()
        assert pn.gpu_oks_nms(db, 0.6, sig, device_id=dev.index) == g[f"oksnms_{tag}"].tolist()
    with pytest.raises(ValueError, match="sigmas"):
        pn.gpu_soft_oks_nms(_db(g, "p"), 0.6, np.ones(3))


def _soft_evaluator(name, dev, use_vis):
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, preds, boxes, paths, kw = cases.case(name)
    return KeypointEvaluator(gt, sigmas=kw['sigmas'], oks_thre=kw['thresh'], in_vis_thre=0.0, use_nms=True, device=dev,
                             image_dir=cases.IMAGE_DIR, nms_in_vis_thre=cases.VIS_THRE if use_vis else None,
                             suppression='soft')


@pytest.mark.parametrize("name,use_vis", [('soft17', False), ('soft5', True)])
def test_evaluator_with_soft_suppression(dev, tmp_path, name, use_vis):
    from tests.helpers import coco_kpt_eval_ref as R
    gt, preds, boxes, paths, kw = cases.case(name)
    g, ref = cases.grouped(name), cases.reference(name, 'gaussian', use_vis)
    N = preds.shape[0]
    assert max(np.diff(g['offsets'])) > 20
    ev = _soft_evaluator(name, dev, use_vis)
    name_value, ap = ev.evaluate(CFG, preds, str(tmp_path), boxes, paths, 1)
    t = ev.tables
    # the restatement's selection, per input row
    want_keep, want_rank, want_soft = np.zeros(N, dtype=bool), np.full(N, -1, dtype=np.int32), np.zeros(N)
    want_keep[g['rows']], want_rank[g['rows']], want_soft[g['rows']] = ref['rank'] >= 0, ref['rank'], ref['soft_score']
    assert np.array_equal(t['order'], g['rows']) and np.abs(t['score'] - g['score']).max() <= 1e-12
    assert np.array_equal(t['keep'], want_keep) and np.array_equal(t['soft_rank'], want_rank)
    err = _rel_err(t['soft_score'], want_soft)
    print(f"{name}: max relative |soft_score - reference| = {err:.3e}")
    assert err <= 1e-12
    kept_per_image = np.bincount(g['image_of'][t['keep']])
    assert kept_per_image.max() == 20 and np.array_equal(np.sort(t['dt_rows']), np.flatnonzero(want_keep))
    # the results file: exactly those persons, with the rescored scores (the decayed ones only chose them)
    res = json.load(open(os.path.join(str(tmp_path), 'results', 'keypoints_val_results_epoch1.json')))
    row_of = {tuple(float(v) for v in preds[r].reshape(-1)): r for r in range(N)}
    assert len(row_of) == N
    listed = [row_of[tuple(r['keypoints'])] for r in res]
    assert sorted(listed) == np.flatnonzero(want_keep).tolist()
    assert all(r['score'] == t['score'][row] for r, row in zip(res, listed))
    assert any(t['soft_score'][row] < t['score'][row] for row in listed)
    for a, b in zip(res, res[1:]):                                           # within an image by rescored score
        assert a['image_id'] != b['image_id'] or a['score'] >= b['score']
    # the ten figures: the restatement's kept persons through the COCOeval restatement
    results = [{'image_id': int(g['image_of'][r]), 'keypoints': preds[r].astype(np.float64).reshape(-1),
                'score': float(g['score'][r])} for r in range(N) if want_keep[r]]
    want = [float(s) for s in R.KeypointEvalRef(gt, results, kw['sigmas']).run()]
    err = np.abs(np.asarray(t['stats']) - np.asarray(want)).max()
    print(f"{name}: figures {t['stats']}, max |figure - reference| = {err:.3e}")
    assert err <= 1e-12 and ap == name_value['AP'] == t['stats'][0]
    # the hard suppression on the same set keeps other persons: the keyword is what switched
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    hard = KeypointEvaluator(gt, sigmas=kw['sigmas'], oks_thre=kw['thresh'], device=dev, image_dir=cases.IMAGE_DIR)
    hard.evaluate(CFG, preds, None, boxes, paths)
    assert 'soft_rank' not in hard.tables and not np.array_equal(hard.tables['keep'], t['keep'])


def test_crowding_analysis_takes_a_soft_evaluator(dev):
    """CrowdingAnalysis reads the evaluator's suppression through _kept_persons: the persons it evaluates are the soft
    selection."""
    from buctd_amd.core.keypoint_analysis import CrowdingAnalysis
    gt, preds, boxes, paths, kw = cases.case('soft5')
    g, ref = cases.grouped('soft5'), cases.reference('soft5', 'gaussian', True)
    an = CrowdingAnalysis(_soft_evaluator('soft5', dev, True))
    p, pos, rows, img, _ = an._kept(preds, boxes, paths)
    assert np.array_equal(rows, g['rows'][ref['rank'] >= 0])
    tables = an.bins(preds, boxes, paths)
    assert tables['AP'].shape == (3, 4)


def test_two_runs_are_bit_identical(dev):
    for name, decay, use_vis in (('soft17', 'gaussian', False), ('soft5', 'linear', True)):
        a, b = _run(name, dev, decay, use_vis), _run(name, dev, decay, use_vis)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    gt, preds, boxes, paths, kw = cases.case('soft17')
    runs = []
    for _ in range(2):
        ev = _soft_evaluator('soft17', dev, False)
        ev.evaluate(CFG, preds, None, boxes, paths)
        runs.append(ev.tables)
    for k in ('score', 'keep', 'order', 'soft_rank', 'soft_score', 'dt_rows', 'oks_flat', 'dt_matched', 'dt_ignored'):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    assert runs[0]['stats'] == runs[1]['stats']


def test_c_abi_refusals_come_before_any_launch(dev):
    from buctd_amd import _C
    lib = _C.lib()
    off, kp, ar, sc, sig = _device_tables('soft5', dev)
    n, images = int(sc.shape[0]), int(off.shape[0]) - 1
    soft = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    rank = torch.full((n,), -7, dtype=torch.int32, device=dev)
    P = _C.ptr

    def call(off_=P(off), images_=images, kp_=P(kp), ar_=P(ar), sc_=P(sc), sig_=P(sig), K=5, thresh=0.6, decay=0,
             max_keep=20, soft_=P(soft), rank_=P(rank)):
        return lib.buctd_soft_oks_nms_grouped(off_, images_, kp_, ar_, sc_, sig_, K, thresh, decay, 0, 0.0, max_keep, soft_,
                                              rank_, _C.stream_ptr())

    bad = [dict(K=0), dict(K=-1), dict(thresh=0.0), dict(thresh=-0.5), dict(thresh=float('nan')), dict(max_keep=0),
           dict(max_keep=-3), dict(decay=2), dict(decay=-1), dict(images_=-1)]
    bad += [{k: None} for k in ('off_', 'kp_', 'ar_', 'sc_', 'sig_', 'soft_', 'rank_')]
    for kw in bad:
        assert call(**kw) == -1 and lib.buctd_last_error(), kw                       # BUCTD_EINVAL
    torch.cuda.synchronize()
    assert bool((soft == -7.0).all()) and bool((rank == -7).all())                    # nothing ran
    assert call() == 0                                                                # the same call, nothing wrong with it
    torch.cuda.synchronize()
    ref = cases.reference('soft5', 'gaussian', False)
    assert np.array_equal(rank.cpu().numpy(), ref['rank'])
