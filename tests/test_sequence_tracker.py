"""dataset.pipeline.SequenceTracker, the host path - the specification of CTD tracking - against tests/helpers/track_ref.py
on the scripted sequences of tests/helpers/track_cases.py, and the conditions those fixtures must meet so that the device
tests (tests/test_gpu_sequence_tracker.py) can compare decisions exactly.  No GPU: the crop and the network are replaced by
the script's heat-maps; box, crop affine, decode, rescoring and all book-keeping run as they are."""
import numpy as np
import pytest
import torch

from refine_cases import TRUNC_CAP, cfg_for, near_integer, pipe_for
from tests.helpers import track_cases as TC
from tests.helpers import track_ref


def _host_tracker(K, monkeypatch, case):
    from buctd_amd.dataset import pipeline as P
    pipe = pipe_for(K)
    tracker = P.SequenceTracker(cfg_for(K), torch.nn.Identity(), pipe, max_tracks=TC.M, sigmas=TC.sigmas_for(K), **TC.PARAMS)
    maps = iter(TC.peak_maps(case))
    monkeypatch.setattr(P, "_check_images", lambda images: None)
    monkeypatch.setattr(pipe, "render", lambda images, geos: (None, None, None))
    monkeypatch.setattr(tracker.refiner, "_forward", lambda x, B: next(maps))
    return tracker


@pytest.mark.parametrize("K", [14, 17])
def test_host_path_matches_the_reference(K, monkeypatch):
    case = TC.scripted(K)
    tracker = _host_tracker(K, monkeypatch, case)
    frames = [torch.zeros((TC.IH, TC.IW, 3), dtype=torch.uint8)] * TC.T
    got = tracker.run(frames, case["dets"])
    # both sides decode the same integer peaks through the same box: float32-equal; the score is numpy's float32 mean here
    TC.compare_frames(got, case["expected"], f"K {K}", preds_tol=0.0, score_tol=1e-6)
    for g in got:
        assert g["preds"].dtype == np.float32 and g["preds"].shape == (TC.M, K, 3) and g["score"].dtype == np.float64
        assert not g["preds"][g["ids"] < 0].any() and not g["score"][g["ids"] < 0].any()


@pytest.mark.parametrize("K", [14, 17])
def test_the_script_covers_every_rule(K):
    e = TC.scripted(K)["expected"]
    slot = lambda t, name: e[t]["names"].index(name) if name in e[t]["names"] else None
    # a person that persists keeps id and slot
    assert all(slot(t, "A") == 0 and e[t]["ids"][0] == 0 for t in range(TC.T))
    # births: frame 0, mid-sequence, with ids counting up
    assert e[0]["born"].tolist() == [True, True, False, False] and e[0]["ids"].tolist() == [0, 1, -1, -1]
    assert e[1]["born"].tolist() == [False, False, True, False] and e[1]["ids"][2] == 2      # A's second detection: covered
    # the last slot goes to D, E finds none
    assert e[2]["born"].tolist() == [False, False, False, True] and (e[2]["ids"] >= 0).all() and slot(2, "E") is None
    # B: low in frames 2 and 3, dies in frame 3 and not before; C: low in frame 3 only, lives on
    b = slot(2, "B")
    assert not e[2]["died"][b] and e[3]["died"][b] and e[2]["score"][b] == 0.0
    assert e[3]["score"][slot(3, "C")] == 0.0 and all(slot(t, "C") == 2 and not e[t]["died"][2] for t in range(3, TC.T))
    # D converges on C and is merged away, C (older) stays
    merged = [t for t in range(TC.T) if slot(t, "D") is not None and e[t]["died"][slot(t, "D")]]
    assert len(merged) == 1 and e[merged[0]]["score"][slot(merged[0], "D")] > TC.PARAMS["death_score"]
    # nothing detected in frame 3; the slot B left in frame 3 is taken in frame 4 under a new id
    assert TC.scripted(K)["dets"][3].shape[0] == 0 and not e[3]["born"].any()
    assert slot(4, "F") == b and e[4]["born"][b] and e[4]["ids"][b] == 4 and e[3]["ids"][b] == 1
    # Z: every predicted x is 0 - born and dead in frame 5
    z = slot(5, "Z")
    assert e[5]["born"][z] and e[5]["died"][z] and not e[5]["preds"][z][:, 0].any() and e[5]["preds"][z][:, 1].all()


@pytest.mark.parametrize("K", [14, 17])
def test_no_decision_sits_on_its_threshold(K):
    """Every OKS and score a decision of the scripted sequence compares with a threshold is at least 1e-3 away from it: the
    float32 decode and the float32 / float64 score sums of the two paths cannot flip one."""
    margins = TC.scripted(K)["margins"]
    print({k: (len(v), min(v) if v else None) for k, v in margins.seen.items()})
    assert all(margins.seen[k] for k in ("birth", "merge", "death"))
    assert margins.smallest() >= 1e-3


@pytest.mark.parametrize("Ms,K,D", TC.STEP_SIZES)
def test_step_cases_are_sound(Ms, K, D):
    """The fixtures of the kernel test, from the host's predictions: decisions off their thresholds (both sides are float64
    there: 1e-6 is ample), conditions inside the truncation cap - the truncated condition is compared in that test only; the
    scripted sequences go through a network that ignores its input, and a track that stands still has crop coordinates an
    ulp from an integer by construction - and the events they are meant to hold."""
    case = TC.step_case(Ms, K, D)
    exp = TC.step_expected(case, case["host_preds"], K)
    assert exp["margins"].smallest() >= 1e-6
    live = exp["ids"] >= 0
    if live.any():
        share = near_integer(exp["cond"][live]).mean()
        assert share <= TRUNC_CAP, f"{100 * share:.2f} %"
    if Ms > 3:
        assert exp["died"][1] and not exp["died"][0], "slot 1 is merged into slot 0"
        assert exp["died"].sum() >= 2, "and the low-scoring slot dies of its second miss"
    if D > 2:
        assert exp["born"].any() and exp["born"].sum() < D, "some detections are born, some are covered"
    if D == 64:
        assert live.all(), "more new detections than free slots: every slot is taken"


def test_reference_rules_on_a_hand_case():
    """track_ref itself, on numbers small enough to follow by hand."""
    K = 3
    par = dict(TC.PARAMS, sigmas=np.full(K, 0.1), margin=10, iw=200, ih=200)
    a = np.array([[50, 50, .9], [60, 60, .9], [70, 50, .9]])
    far = a + [100, 100, 0]
    ids, pose, area = np.full(2, -1), np.zeros((2, K, 3)), np.zeros(2)
    born, nxt = track_ref.birth(ids, pose, area, 0, np.stack([a * [1, 1, .5], far, a]), par)
    assert ids.tolist() == [0, 1] and nxt == 2 and born.all()     # far and a (.9 each, by index), the weak copy of a covered
    assert np.array_equal(pose[0], far) and np.array_equal(pose[1], a) and area[1] == 40 * 30
    misses = np.zeros(2, dtype=np.int64)
    died = track_ref.death_and_merge(ids, misses, pose, area, np.stack([a, a]), np.array([.1, .9]), par)
    assert died.tolist() == [False, True] and misses.tolist() == [1, 0] and ids.tolist() == [0, -1]   # the younger merges
    died = track_ref.death_and_merge(ids, misses, pose, area, np.stack([a, a]), np.array([.1, .9]), par)
    assert died.tolist() == [True, False] and ids.tolist() == [-1, -1]                                # the second miss


def test_refusals():
    from buctd_amd.dataset.pipeline import SequenceTracker
    with pytest.raises(ValueError, match="must pass its own"):
        SequenceTracker(cfg_for(14), None, pipe_for(14))
    with pytest.raises(ValueError, match="is_train=False"):
        SequenceTracker(cfg_for(17), None, pipe_for(17, is_train=True))
    with pytest.raises(ValueError, match="at most 64 tracks"):
        SequenceTracker(cfg_for(17), None, pipe_for(17), max_tracks=65, on_device=True)
    SequenceTracker(cfg_for(17), None, pipe_for(17), max_tracks=65)
    tracker = SequenceTracker(cfg_for(17), None, pipe_for(17), on_device=True)
    assert tracker.sigmas.shape == (17,)
