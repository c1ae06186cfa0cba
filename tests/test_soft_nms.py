"""Soft OKS suppression, host side (no GPU): the restatement tests/helpers/soft_nms_ref.py against what the REFERENCE's
soft_oks_nms returned (tests/golden/nms.npz) and against the two host implementations on the seeded sets of
tests/helpers/soft_nms_cases.py; the condition on those sets that makes the device comparison of
tests/test_gpu_soft_nms.py well posed; what the sets cover; the refusals that need no device."""
import os

import numpy as np
import pytest

from tests.helpers import soft_nms_cases as cases
from tests.helpers import soft_nms_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nms.npz")
VARIANTS = [(d, v) for d in ('gaussian', 'linear') for v in (False, True)]


def _images(name):
    g = cases.grouped(name)
    for pos, image_id in enumerate(g['image_ids']):
        yield image_id, int(g['offsets'][pos]), int(g['offsets'][pos + 1])


def test_restatement_reproduces_the_reference_golden():
    g = np.load(GOLD)
    for tag in "pq":
        sig = g[f"sigmas_{tag}"] if f"sigmas_{tag}" in g.files else cases.COCO_SIGMAS
        kp = g[f"kpts_{tag}"]
        kp = kp.reshape(kp.shape[0], -1, 3)
        want = g[f"softnms_{tag}"].tolist()
        out = S.soft_nms(kp, g[f"areas_{tag}"], g[f"scores_{tag}"], sig, 0.6)
        assert S.selection(out['rank']) == want and len(want) <= 20
        # the device entry points take float32 key points: the golden selections do not hang on that rounding
        out32 = S.soft_nms(kp.astype(np.float32), g[f"areas_{tag}"], g[f"scores_{tag}"], sig, 0.6)
        assert S.selection(out32['rank']) == want


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
def test_restatement_equals_both_host_implementations(name):
    """float64 key points (the host functions subtract in the dtype they are given), the tie image left out (numpy's
    argsort()[::-1] orders equal scores differently)."""
    import buctd_amd.nms.nms as pn
    from oracle import nms as on
    g, kw = cases.grouped(name), cases.case(name)[4]
    seen = 0
    for image_id, a, b in _images(name):
        if image_id == cases.TIE_IMAGE:
            continue
        kp = g['kpts'][a:b].astype(np.float64)
        db = [{'keypoints': kp[i], 'score': float(g['scores'][a + i]), 'area': float(g['areas'][a + i])} for i in range(b - a)]
        for vis in (None, cases.VIS_THRE):
            want = S.selection(S.soft_nms(kp, g['areas'][a:b], g['scores'][a:b], kw['sigmas'], kw['thresh'], 'gaussian',
                                          vis)['rank'])
            for impl in (pn, on):
                assert [int(i) for i in impl.soft_oks_nms(db, kw['thresh'], kw['sigmas'], vis)] == want, (image_id, vis)
            seen += 1
    assert seen == 2 * (len(g['image_ids']) - (1 if name == 'soft17' else 0))


@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
@pytest.mark.parametrize("decay,use_vis", VARIANTS)
def test_input_condition(name, decay, use_vis):
    """From the restatement alone: outside the tie pair no two live scores an arg-max looked at are within 1e-9
    relative of each other, and for the linear decay no OKS lies within 1e-9 of the threshold."""
    ref, kw = cases.reference(name, decay, use_vis), cases.case(name)[4]
    tie = set(cases.tie_positions(name))
    for image_id, out in ref['per_image'].items():
        for looked_at in out['compared']:
            by_score = sorted(looked_at, key=lambda ps: ps[1])
            for (p0, s0), (p1, s1) in zip(by_score, by_score[1:]):
                if image_id == cases.TIE_IMAGE and {p0, p1} == tie:
                    assert s0 == s1                                   # the tie stays a tie: every factor was exactly 1.0
                    continue
                assert s1 - s0 > 1e-9 * max(abs(s0), abs(s1)), (image_id, p0, p1, s0, s1)
        if decay == 'linear':
            assert all(abs(v - kw['thresh']) > 1e-9 for _, _, _, v, _ in out['formed'])
        if image_id == cases.TIE_IMAGE:
            assert all(v == 0.0 for _, h, c, v, _ in out['formed'] if h in tie or c in tie)


def test_the_sets_cover_every_class():
    counts = {}
    for name in sorted(cases.CONFIGS):
        g, kw = cases.grouped(name), cases.case(name)[4]
        preds = cases.case(name)[1]
        assert preds.dtype == np.float32 and preds.shape[1:] == (kw['K'], 3)
        per_image = {image_id: b - a for image_id, a, b in _images(name)}
        for image_id, n in cases.COUNTS[name].items():
            assert per_image[image_id] == n
        assert per_image[cases.REORDER_IMAGE] == 3
        counts[name] = per_image
        assert (preds[:, :, 2].max(1) < cases.VIS_THRE).sum() >= 3              # persons with no joint above the threshold
        # the reorder image: taken A, C, B under every variant, so a walk in input order fails
        for decay, use_vis in VARIANTS:
            ref = cases.reference(name, decay, use_vis)
            assert ref['per_image'][cases.REORDER_IMAGE]['rank'] == [0, 2, 1]
            for image_id, out in ref['per_image'].items():
                assert sum(r >= 0 for r in out['rank']) == min(per_image[image_id], 20)
        # a crowd image: the 20 taken are not the 20 best by input score
        big = max(cases.COUNTS[name], key=cases.COUNTS[name].get)
        rank = cases.reference(name, 'gaussian', False)['per_image'][big]['rank']
        assert any(r < 0 for r in rank[:20]) and any(r >= 0 for r in rank[20:])
    assert sorted(cases.COUNTS['soft17'].values()) == [0, 1, 20, 21, 65]
    assert sorted(cases.COUNTS['soft5'].values()) == [0, 1, 19, 64, 130]
    assert counts['soft17'][cases.TIE_IMAGE] == 8 and cases.TIE_IMAGE not in counts['soft5']
    assert sum(sum(c.values()) for c in counts.values()) <= 400
    assert [float(s) for s in cases.case('soft5')[4]['sigmas']] == [0.05] * 5 and cases.case('soft5')[4]['thresh'] == 0.6
    assert np.array_equal(cases.case('soft17')[4]['sigmas'], cases.COCO_SIGMAS)
    # the tie pair: equal scores, adjacent in grouped order, taken one right after the other, the earlier one first
    p0, p1 = cases.tie_positions('soft17')
    for decay, use_vis in VARIANTS:
        rank = cases.reference('soft17', decay, use_vis)['per_image'][cases.TIE_IMAGE]['rank']
        assert p0 < p1 and 0 < rank[p0] and rank[p1] == rank[p0] + 1


def test_hard_sets_meet_their_input_condition():
    """Building a set of tests/helpers/oks_nms_cases.py checks that no pair's host OKS lies within 1e-9 of the threshold
    and that every image of two or more persons has some dropped and some kept; the counts are the ones the kernel's
    bitmap words make interesting."""
    from tests.helpers import oks_nms_cases as hard
    assert hard.COUNTS == (0, 1, 2, 63, 64, 65, 129)
    for name, (K, _, sigmas) in hard.CONFIGS.items():
        c = hard.case(name)
        assert c['kpts'].dtype == np.float32 and c['kpts'].shape == (sum(hard.COUNTS), K, 3)
        assert np.array_equal(np.diff(c['offsets']), hard.COUNTS) and len(sigmas) == K
        for a, b in zip(c['offsets'][:-1], c['offsets'][1:]):
            assert (np.diff(c['scores'][a:b]) < 0).all()                            # descending, no two equal
        assert not np.array_equal(c['keep'][False], c['keep'][True])                # the joint-score threshold matters
    assert sorted(K for K, _, _ in hard.CONFIGS.values()) == [3, 17]


def test_oks_nms_grouped_refuses_wrong_shapes_before_any_launch():
    import torch
    from buctd_amd.nms.nms import oks_nms_grouped
    from tests.helpers import oks_nms_cases as hard
    c = hard.case('hard3')
    N = c['kpts'].shape[0]
    off, kp, ar, sig = (torch.as_tensor(np.array(c[k])) for k in ('offsets', 'kpts', 'areas', 'sigmas'))
    good = dict(offsets=off, kpts=kp, areas=ar, sigmas=sig)
    bad = [dict(kpts=kp[:, :, :2]), dict(kpts=kp.reshape(N, -1)), dict(kpts=kp[:-1]), dict(areas=ar[:-1]),
           dict(sigmas=sig[:-1]), dict(sigmas=torch.cat([sig, sig])), dict(offsets=off[:0])]
    for kw in bad:
        a = dict(good, **kw)
        for max_per_image in (None, 129):
            with pytest.raises(ValueError):
                oks_nms_grouped(a['offsets'], a['kpts'], a['areas'], a['sigmas'], 0.5, max_per_image=max_per_image)


def test_refusals_that_need_no_device():
    import buctd_amd.nms.nms as pn
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    assert len(pn.gpu_soft_oks_nms([], 0.5)) == 0 and pn.gpu_oks_nms([], 0.5) == []
    with pytest.raises(ValueError, match="decay"):
        pn.soft_oks_nms_grouped(None, None, None, None, None, 0.5, decay='cubic')
    gt = cases.case('soft5')[0]
    make = lambda **kw: KeypointEvaluator(gt, sigmas=[0.05] * 5, device='cpu', image_dir=cases.IMAGE_DIR, **kw)
    with pytest.raises(ValueError, match="use_nms"):
        make(suppression='soft', use_nms=False)
    with pytest.raises(ValueError, match="suppression"):
        make(suppression='softer')
    with pytest.raises(NotImplementedError, match="suppression='soft'"):
        make(soft_nms=True)
    assert make(suppression='soft').suppression == 'soft' and make().suppression == 'hard'
