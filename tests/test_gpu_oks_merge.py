"""GPU suite for the OKS merge (buctd_oks_merge_grouped of csrc/oks_merge.hip under nms.oks_merge_grouped / gpu_oks_merge
and KeypointEvaluator.evaluate_merged) against the host statement nms.oks_merge_levels on the case table of
tests/helpers/oks_merge_cases.py, ten images and three levels in one call per configuration.

Condition on the inputs (tests/test_oks_merge.py checks it on the CPU, on the host values alone): apart from the OKS values
that are exactly 1.0 or exactly 0.0, no max_oks lies within 1e-9 of the threshold.  Under it keep and best are exactly
equal.  max_oks is a sum of at most 17 terms in [0, 1], each from one fp64 exp within a few ulp, and a handful of roundings:
under 1e-14; the bar is 1e-12 absolute, which leaves a hundredfold margin for a different exp.

evaluate_merged is checked against evaluate(): with one set bit for bit; with two and three sets against evaluate() of the
table a host loop builds from nms.oks_nms and nms.oks_merge per image."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import kpt_eval_cases as kcases
from tests.helpers import oks_merge_cases as cases
from tests.helpers.kpt_eval_cases import COCO_SIGMAS, IMAGE_DIR, SIZES, CaseBuilder

pytestmark = pytest.mark.gpu
CFG = SimpleNamespace(OUTPUT_JSON='')
L = cases.L


def _device_table(name, dev):
    t = cases.table(name)
    return [torch.as_tensor(np.array(t[k])).to(dev) for k in ('cells', 'kpts', 'areas', 'sigmas')]


def _run(name, dev):
    from buctd_amd.nms.nms import oks_merge_grouped
    t = cases.table(name)
    cells, kp, ar, sig = _device_table(name, dev)
    keep, max_oks, best = oks_merge_grouped(cells, L, kp, ar, sig, t['thresh'], in_vis_thre=t['in_vis_thre'])
    assert keep.dtype == torch.int32 and max_oks.dtype == torch.float64 and best.dtype == torch.int32
    assert keep.shape == max_oks.shape == best.shape == ar.shape
    return keep.cpu().numpy(), max_oks.cpu().numpy(), best.cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
def test_grouped_equals_the_host_statement(dev, name):
    want_keep, want_max, want_best = cases.reference(name)
    keep, max_oks, best = _run(name, dev)
    err = float(np.abs(max_oks - want_max).max())
    print(f"{name}: max |max_oks - host| = {err:.3e}; kept {int(keep.sum())} of {keep.size}")
    assert np.array_equal(keep, want_keep)
    assert np.array_equal(best, want_best)
    assert err <= 1e-12
    exact = (want_max == -1.0) | (want_max == 0.0) | (want_max == 1.0)
    assert np.array_equal(max_oks[exact], want_max[exact])


def test_two_runs_are_bit_identical(dev):
    for name in ('k17', 'k14_vis'):
        a, b = _run(name, dev), _run(name, dev)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_nan_pose_is_dropped(dev):
    from buctd_amd.nms.nms import oks_merge_grouped, oks_merge_levels
    t = cases.table('k5')
    c = t['cell']['e']
    kpts, areas = t['kpts'][c[0]:c[0] + 5].copy(), t['areas'][c[0]:c[0] + 5]
    kpts[4, 2, 0] = np.nan
    want = oks_merge_levels([0, 3, 5], kpts, areas, t['sigmas'], 0.5)
    tt = lambda a: torch.as_tensor(np.array(a)).to(dev)
    got = [x.cpu().numpy() for x in oks_merge_grouped(torch.tensor([0, 3, 5]), 2, tt(kpts), tt(areas), tt(t['sigmas']), 0.5)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[0][4] == 0
    assert np.isnan(got[1][4]) and np.abs(got[1][:4] - want[1][:4]).max() <= 1e-12


def test_gpu_oks_merge_returns_what_oks_merge_returns(dev):
    import buctd_amd.nms.nms as pn
    t = cases.table('k17')
    lists = cases.pose_lists('k17')
    at = {letter: n for n, letter in enumerate(cases.IMAGES)}
    # (mode 0 = the candidates, mode 1 = the accepted): 70 against 3, the level-1 poses of g against A, and mode 1 empty
    for letter in 'egc':
        mode1, mode0 = lists[at[letter]][0], lists[at[letter]][1]
        host0, host1, dev0, dev1 = list(mode0), list(mode1), list(mode0), list(mode1)
        want = pn.oks_merge(host0, host1, t['thresh'], t['sigmas'])
        got = pn.gpu_oks_merge(dev0, dev1, t['thresh'], t['sigmas'], device_id=dev.index)
        assert want is (host0 if letter == 'c' else host1) and got is (dev0 if letter == 'c' else dev1)
        assert len(got) == len(want) and all(a is b for a, b in zip(got, want)), letter
        assert len(dev0) == len(mode0) and len(got) > len(mode1)             # mode 0 is left as it was
    assert len(lists[at['c']][0]) == 0
    # in_vis_thre reaches the kernel: i is kept with it and dropped without it; COCO sigmas are the default
    tv, lv = cases.table('k14_vis'), cases.pose_lists('k14_vis')[at['i']]
    assert len(pn.gpu_oks_merge(list(lv[1]), list(lv[0]), 0.5, tv['sigmas'], cases.VIS_THRE)) == 2
    assert len(pn.gpu_oks_merge(list(lv[1]), list(lv[0]), 0.5, tv['sigmas'])) == 1
    li = lists[at['e']]
    assert [p['index'] for p in pn.gpu_oks_merge(list(li[1]), list(li[0]))] == \
        [p['index'] for p in pn.oks_merge(list(li[1]), list(li[0]))]
    with pytest.raises(ValueError, match="sigmas"):
        pn.gpu_oks_merge(list(li[1]), list(li[0]), 0.5, np.ones(3))


def test_c_abi_refusals_and_empty_inputs_launch_nothing(dev):
    from buctd_amd import _C
    lib = _C.lib()
    t = cases.table('k5')
    cells, kp, ar, sig = _device_table('k5', dev)
    n, images = int(ar.shape[0]), len(cases.IMAGES)
    keep = torch.full((n,), -7, dtype=torch.int32, device=dev)
    max_oks = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    best = torch.full((n,), -7, dtype=torch.int32, device=dev)
    P = _C.ptr

    def call(cells_=P(cells), images_=images, levels=L, n_=n, kp_=P(kp), ar_=P(ar), sig_=P(sig), K=5, keep_=P(keep),
             max_=P(max_oks), best_=P(best)):
        return lib.buctd_oks_merge_grouped(cells_, images_, levels, n_, kp_, ar_, sig_, K, t['thresh'], 0, 0.0, keep_, max_,
                                           best_, _C.stream_ptr())

    bad = [dict(K=0), dict(K=-1), dict(levels=0), dict(levels=-1), dict(images_=-1), dict(n_=-1),
           dict(images_=1 << 30, levels=2)]
    bad += [{k: None} for k in ('cells_', 'kp_', 'ar_', 'sig_', 'keep_', 'max_', 'best_')]
    for kw in bad:
        assert call(**kw) == -1 and lib.buctd_last_error(), kw                        # BUCTD_EINVAL
    assert call(images_=0) == 0 and call(n_=0) == 0                                   # empty: success, no launch
    torch.cuda.synchronize()
    assert bool((keep == -7).all()) and bool((max_oks == -7.0).all()) and bool((best == -7).all())
    assert call() == 0                                                                # the same call, nothing wrong with it
    torch.cuda.synchronize()
    assert np.array_equal(keep.cpu().numpy(), cases.reference('k5')[0])
    assert np.array_equal(best.cpu().numpy(), cases.reference('k5')[2])


# ---- evaluate_merged
def _results(folder, epoch):
    return json.load(open(os.path.join(str(folder), 'results', f'keypoints_val_results_epoch{epoch}.json')))


@pytest.mark.parametrize("name,over", [('match17_nms', {}), ('match17', {}), ('nms5_vis', {}),
                                       ('nms17', dict(suppression='soft'))])
def test_one_set_equals_evaluate_bit_for_bit(dev, tmp_path, name, over):
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, preds, boxes, paths, kw, ref = kcases.case(name)
    runs = []
    for merged in (False, True):
        ev = KeypointEvaluator(gt, device=dev, image_dir=IMAGE_DIR, **dict(kw, **over))
        out = tmp_path / ('merged' if merged else 'plain')
        if merged:
            res = ev.evaluate_merged(CFG, [(preds, boxes, paths)], str(out), 4)
        else:
            res = ev.evaluate(CFG, preds, str(out), boxes, paths, 4)
        runs.append((res, ev.tables, _results(out, 4)))
    (res0, t0, json0), (res1, t1, json1) = runs
    assert res0 == res1 and list(res0[0].items()) == list(res1[0].items()) and json0 == json1
    assert set(t1) - set(t0) == {'level', 'merge_keep', 'merge_max_oks', 'merge_best'} and 'res_file' in t0
    for k in set(t0) - {'res_file'}:
        if k == 'oks':
            assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(t0[k], t1[k]))
        elif k == 'stats':
            assert t0[k] == t1[k]
        else:
            assert t0[k].dtype == t1[k].dtype and t0[k].shape == t1[k].shape and t0[k].tobytes() == t1[k].tobytes(), k
    assert not t1['level'].any() and np.array_equal(t1['merge_keep'], t0['keep'])
    assert (t1['merge_max_oks'] == -1.0).all() and (t1['merge_best'] == -1).all()


def _ensemble(K, seed, n_sets):
    """A small annotation set and n_sets prediction tables on it.  Image 4: every set, duplicates within a set (for its own
    suppression) and across sets; 9: only the second set; 14: nobody; 19: the first and the last set; 24: a pair of equal
    scores across two sets on poses far apart; 29: 25 ground truths, more accepted persons than max_dets."""
    b = CaseBuilder(K, seed)
    rng = b.rng
    spot = lambda: rng.rand(2) * 1500 + 250
    ids = [b.image(4 + 5 * i) for i in range(6)]
    gts = {i: [b.gt(i, spot(), SIZES[1 + (k + n) % 6]) for k in range(m)] for n, (i, m) in enumerate(zip(ids, (5, 3, 2, 4, 3, 25)))}
    builders = [b] + [CaseBuilder(K, seed + 1 + s) for s in range(n_sets - 1)]
    last = n_sets - 1
    js = rng.rand(K) * 0.5 + 0.4
    for s, sb in enumerate(builders):
        g = gts[ids[0]]
        for k in range(5):
            if (k + s) % 3 != 2:                                   # every set misses other ground truths
                sb.det_near(g[k], 0.01)
                sb.det_near(g[k], (0.02, 0.1, 0.3)[(k + s) % 3])    # its own near-duplicate, of varying closeness
        if s == 1:
            for k in range(3):
                sb.det_near(gts[ids[1]][k], 0.05)
        if s in (0, last):
            for k in range(4):
                if k % 2 == (0 if s == 0 else 1) or k == 3:
                    sb.det_near(gts[ids[3]][k], 0.02 + 0.2 * (s > 0) * (k == 3))
        if s < 2:
            sb.det_near(gts[ids[4]][s], 0.03, box_score=0.7, joint_scores=js)      # equal scores, level decides
            sb.det_near(gts[ids[4]][2], 0.01 + 0.05 * s)
        for k in range(25):
            if k % n_sets == s or k % 7 == 0:
                sb.det_near(gts[ids[5]][k], 0.02 * (1 + s))
    gt, preds, boxes, paths = b.build()
    return gt, [(preds, boxes, paths)] + [sb.build()[1:] for sb in builders[1:]]


def _host_merged_table(sets, K, kw, min_oks_thres, merge_vis):
    """What evaluate_merged states, as a host loop: per set the rescoring and nms.oks_nms per image, then the chain of
    nms.oks_merge per image; the accepted persons by score, then level, then position.  Returns the table of the accepted
    persons (images in order of first appearance) and their rows in the concatenated sets."""
    import buctd_amd.nms.nms as pn
    nms_sig = np.asarray(kw.get('nms_sigmas', kw['sigmas']), dtype=np.float64)
    vis = kw.get('in_vis_thre', 0.0)
    levels, seen, base = {}, [], 0
    for l, (preds, boxes, paths) in enumerate(sets):
        image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
        js = preds[:, :, 2].astype(np.float64)
        score = np.zeros(len(paths))
        for r in range(len(paths)):
            total, count = 0.0, 0
            for j in range(K):
                if js[r, j] > vis:
                    total, count = total + js[r, j], count + 1
            score[r] = (total / count if count else 0.0) * boxes[r, 5]
        for i in image_of:
            if i not in seen:
                seen.append(i)
        for i in sorted(set(image_of)):
            rows = [r for r in range(len(paths)) if image_of[r] == i]
            rows = [rows[k] for k in np.argsort(-score[rows], kind='stable')]
            assert not kw['use_nms'] or len(set(score[rows])) == len(rows)   # oks_nms orders equal scores its own way
            db = [{'keypoints': preds[r].astype(np.float64), 'score': score[r], 'area': boxes[r, 4],
                   'key': (l, pos), 'row': base + r, 'set_row': (l, r)} for pos, r in enumerate(rows)]
            if kw['use_nms']:
                db = [db[k] for k in pn.oks_nms(db, kw.get('oks_thre', 0.5), nms_sig, kw.get('nms_in_vis_thre'))]
            levels.setdefault(i, [[] for _ in sets])[l] = db
        base += len(paths)
    out = []
    for i in seen:
        merged = levels[i][0]
        for level in levels[i][1:]:
            merged = pn.oks_merge(level, merged, min_oks_thres, nms_sig, merge_vis)
        out.extend(sorted(merged, key=lambda p: (-p['score'], p['key'])))
    preds = np.stack([sets[p['set_row'][0]][0][p['set_row'][1]] for p in out])
    boxes = np.stack([sets[p['set_row'][0]][1][p['set_row'][1]] for p in out])
    paths = [sets[p['set_row'][0]][2][p['set_row'][1]] for p in out]
    return preds, boxes, paths, np.array([p['row'] for p in out], dtype=np.int64)


@pytest.mark.parametrize("n_sets,K,kw,min_oks_thres,merge_vis", [
    (2, 17, dict(sigmas=COCO_SIGMAS, use_nms=True), 0.5, None),
    (3, 5, dict(sigmas=[0.1] * 5, nms_sigmas=[0.05] * 5, use_nms=True, in_vis_thre=0.2, oks_thre=0.6), 0.4, 0.2),
    (3, 17, dict(sigmas=COCO_SIGMAS, use_nms=False), 0.5, None),
])
def test_sets_equal_evaluate_of_the_host_merged_table(dev, tmp_path, n_sets, K, kw, min_oks_thres, merge_vis):
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    gt, sets = _ensemble(K, 50 + n_sets + K, n_sets)
    preds_h, boxes_h, paths_h, rows_h = _host_merged_table(sets, K, kw, min_oks_thres, merge_vis)
    ev = KeypointEvaluator(gt, device=dev, image_dir=IMAGE_DIR, **kw)
    name_value, ap = ev.evaluate_merged(CFG, sets, str(tmp_path / 'merged'), 2, min_oks_thres=min_oks_thres,
                                        merge_in_vis_thre=merge_vis)
    t = ev.tables
    host = KeypointEvaluator(gt, device=dev, image_dir=IMAGE_DIR, **dict(kw, use_nms=False))
    want_nv, want_ap = host.evaluate(CFG, preds_h, str(tmp_path / 'host'), boxes_h, paths_h, 2)
    N = sum(s[0].shape[0] for s in sets)
    # the accepted persons are the host loop's, and the merge did reject and accept persons of the later sets
    assert np.array_equal(np.flatnonzero(t['keep']), np.sort(rows_h)) and t['keep'].shape == (N,)
    later = t['level'] > 0
    assert np.array_equal(t['level'], np.repeat(np.arange(n_sets), [s[0].shape[0] for s in sets]))
    assert (t['merge_keep'] & later).any() and (~t['merge_keep'] & later & (t['merge_max_oks'] > min_oks_thres)).any()
    assert np.array_equal(t['keep'], t['merge_keep']) and t['merge_keep'][~later].sum() == t['keep'][~later].sum()
    hit = t['merge_best'] >= 0
    assert np.array_equal(hit, t['merge_max_oks'] >= 0) and t['keep'][t['merge_best'][hit]].all()
    assert (t['level'][t['merge_best'][hit]] < t['level'][hit]).all()
    # figures, matches and the results file
    assert list(name_value.items()) == list(want_nv.items()) and ap == want_ap and t['stats'] == host.tables['stats']
    assert np.array_equal(t['dt_matched'], host.tables['dt_matched'])
    assert np.array_equal(t['dt_ignored'], host.tables['dt_ignored'])
    assert np.array_equal(t['dt_rows'], rows_h[host.tables['dt_rows']])
    assert np.array_equal(t['dt_offsets'], host.tables['dt_offsets']) and np.diff(t['dt_offsets']).max() == 20
    assert _results(tmp_path / 'merged', 2) == _results(tmp_path / 'host', 2)
    assert len(_results(tmp_path / 'merged', 2)) == len(rows_h) > np.diff(t['dt_offsets']).sum()
