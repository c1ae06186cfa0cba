"""CTD tracking on the device: buctd_track_step alone against tests/helpers/track_ref.py and the host functions, and
SequenceTracker(on_device=True) against the host path - the scripted sequences of tests/helpers/track_cases.py through a
stand-in network, one real small network, and the same under engine.ForwardGraph.  Fixture soundness is checked on the CPU
(tests/test_sequence_tracker.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from refine_cases import TRUNC_CAP, cfg_for, near_integer, pipe_for
from tests.helpers import track_cases as TC

pytestmark = pytest.mark.gpu


def _tracker(K, model, dev, on_device, Ms=TC.M, **kw):
    from buctd_amd.dataset.pipeline import SequenceTracker
    args = dict(TC.PARAMS, max_tracks=Ms, sigmas=TC.sigmas_for(K))
    args.update(kw)
    return SequenceTracker(cfg_for(K), model, pipe_for(K), on_device=on_device, **args)


def _frames(dev, n, seed=5):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 256, (TC.IH, TC.IW, 3)).astype(np.uint8)).to(dev) for _ in range(n)]


# ---- the kernel alone -------------------------------------------------------------------------------------------------------
def _launch(case, dev, Ms, K, D):
    """One buctd_track_step call with frame = 0 of 2: the decode outputs of frame 0, the D detections of frame 1."""
    from buctd_amd.dataset.pipeline import WARP_ITEM, _layout, _views, track_history_layout, warp_items
    tracker = _tracker(K, None, dev, True, Ms=Ms)
    frames = _frames(dev, 2)
    at_in, n_in = _layout(tracker.state_layout(2, Ms, K, D))
    host = np.zeros(n_in, dtype=np.uint8)
    hv = _views(host, at_in)
    hv["ids"][:], hv["misses"][:], hv["next_id"][:] = case["ids"], case["misses"], case["next_id"]
    hv["pose"][:], hv["center"][:], hv["scale"][:] = case["state_pose"], case["center"], case["scale"]
    hv["cond_trunc"][:] = -7.0
    hv["sigmas"][:], hv["det_offsets"][:] = TC.sigmas_for(K), [0, 0, D]
    if D:
        hv["dets"][:] = case["dets"]
    hv["frame_src"][:] = [f.data_ptr() for f in frames]
    warp_items([frames[0]] * Ms, items=hv["items"].reshape(-1).view(WARP_ITEM))
    sv = _views(torch.from_numpy(host).to(dev), at_in)
    at_out, n_out = _layout(track_history_layout(2, Ms, K))
    result = torch.zeros(n_out, dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tracker.track_step((up(case["coords"]), up(case["maxvals"]), up(case["offset"])), sv, _views(result, at_out), 0, 2, D)
    torch.cuda.synchronize()
    state = {k: v.cpu().numpy() for k, v in sv.items()}
    state["items"] = state["items"].reshape(-1).view(WARP_ITEM)
    return state, _views(result.cpu().numpy(), at_out), frames


@pytest.mark.parametrize("Ms,K,D", TC.STEP_SIZES)
def test_track_step_matches_the_reference(dev, Ms, K, D):
    case = TC.step_case(Ms, K, D)
    state, hist, frames = _launch(case, dev, Ms, K, D)
    what = f"M {Ms} K {K} D {D}"
    live = case["live"]
    # predictions: the host's float32, or its float32 neighbour where the float64 value sits on a rounding boundary
    preds, h32 = hist["preds"][0], case["host_preds"]
    off = np.abs(preds[live][:, :, :2].astype(np.float64) - h32[live][:, :, :2]) / np.spacing(np.abs(h32[live][:, :, :2]))
    print(f"{what}: {int((off > 0).sum())} of {off.size} predictions differ from the host's float32, at most {off.max():.1f} ulp")
    assert off.max() <= 1.0 and np.array_equal(preds[live][:, :, 2], h32[live][:, :, 2]) and not preds[~live].any()
    # everything after them from the kernel's own predictions
    exp = TC.step_expected(case, preds, K)
    assert exp["margins"].smallest() >= 1e-6
    assert np.array_equal(hist["died"][0].astype(bool), exp["died"]), f"{what}: died"
    assert np.array_equal(hist["born"][1].astype(bool), exp["born"]), f"{what}: born"
    assert np.array_equal(hist["ids"][1], exp["ids"]) and np.array_equal(state["ids"], exp["ids"]), f"{what}: ids"
    assert np.array_equal(state["misses"], exp["misses"]) and int(state["next_id"][0]) == exp["next_id"]
    assert not hist["born"][0].any() and not hist["died"][1].any() and not hist["ids"][0].any(), "rows of other frames"
    rel = np.abs(hist["score"][0] - exp["score"]) / np.maximum(np.abs(exp["score"]), 1e-300)
    print(f"{what}: score rel {rel.max():.3e}")
    assert rel.max() <= 1e-12
    now = exp["ids"] >= 0
    assert np.array_equal(state["pose"][now], exp["pose"][now]), f"{what}: the slots' poses"
    assert np.array_equal(state["center"], exp["center"]) and np.array_equal(state["scale"], exp["scale"]), f"{what}: box"
    m = state["items"]["m"].reshape(Ms, 2, 3)
    em = np.abs(m - exp["mats"]).max()
    print(f"{what}: |m - get_affine_transform| = {em:.3e}")
    assert em <= 1e-9
    ref = np.trunc(exp["cond"]).astype(np.float32)
    keep = ~near_integer(exp["cond"])
    assert (~keep[now]).mean() <= TRUNC_CAP if now.any() else True
    assert np.array_equal(state["cond_trunc"][keep], ref[keep]) and np.abs(state["cond_trunc"] - ref).max() <= 1.0
    assert not state["cond_trunc"][~now].any(), "an empty slot has an all-zero condition"
    assert (state["items"]["src"] == frames[1].data_ptr()).all()
    assert (state["items"]["H"] == TC.IH).all() and (state["items"]["W"] == TC.IW).all() and not state["items"]["flip"].any()


def test_track_step_refuses_bad_arguments(dev):
    from buctd_amd import _C
    some = torch.zeros(64, dtype=torch.float64, device=dev)

    def args(**kw):
        a = _C.TrackArgs()
        for name, kind in _C.TrackArgs._fields_:
            if kind is C.c_void_p:
                setattr(a, name, some.data_ptr())
        a.M, a.K, a.frame, a.frames, a.max_dets, a.max_misses = 4, 14, -1, 2, 3, 2
        a.heatmap_w, a.heatmap_h, a.crop_w, a.crop_h, a.aspect_ratio = 16, 24, 64, 96, 2 / 3
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, message in ((dict(M=65), "M <= 64"), (dict(max_dets=65), "at most 64 detections"), (dict(K=33), "K <= 32"),
                        (dict(frame=2), r"frame outside"), (dict(ids=None), "NULL argument")):
        with pytest.raises(_C.BuctdHipError, match=message):
            _C.check(_C.lib().buctd_track_step(C.byref(args(**kw)), None), "track_step")
    torch.cuda.synchronize()
    assert not some.any(), "a refused call launches nothing"


# ---- the whole tracker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [14, 17])
def test_scripted_sequence_device_against_host(dev, K):
    case = TC.scripted(K)
    maps = TC.peak_maps(case)
    frames = _frames(dev, TC.T)
    net_d, net_h = TC.ScriptedPeaks(maps).to(dev), TC.ScriptedPeaks(maps).to(dev)
    on = _tracker(K, net_d, dev, True).run(frames, case["dets"])
    host = _tracker(K, net_h, dev, False).run(frames, case["dets"])
    assert net_d.calls == net_h.calls == TC.T
    # the bounds of tests/test_gpu_refine_chain.py between its host and device chains
    TC.compare_frames(on, host, f"K {K} device / host", preds_tol=1e-3, score_tol=1e-5)
    TC.compare_frames(on, case["expected"], f"K {K} device / reference", preds_tol=1e-3, score_tol=1e-5)
    for d, h in zip(on, host):
        assert d.keys() == h.keys()
        for k in d:
            assert d[k].shape == h[k].shape and d[k].dtype == h[k].dtype, k


def _coam(dev):
    from oracle import recipes
    from buctd_amd import models
    cfg, omodel, _, _ = recipes.build("coam_w16_96x64_colored")
    cfg.DATASET.update({"BU_BBOX_MARGIN": 25, "FLIP": False})
    cfg.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    m = models.pose_hrnet_coam.get_pose_net(cfg, is_train=False)
    m.load_state_dict(omodel.state_dict(), strict=True)
    return cfg, m.to(dev).eval(), pipe_for(14, cfg=cfg)


def _real_sequence(dev):
    rng = np.random.RandomState(31)
    pose = lambda c: TC._pose(c, TC._shape(rng, 14), rng.uniform(0.5, 0.9))
    dets = [np.stack([pose((90, 100)), pose((290, 110)), pose((180, 220))]), np.zeros((0, 14, 3)), pose((300, 230))[None],
            np.zeros((0, 14, 3))]
    return _frames(dev, 4, seed=9), dets


def test_real_network_device_against_host(dev):
    from buctd_amd.dataset.pipeline import SequenceTracker
    cfg, m, pipe = _coam(dev)
    frames, dets = _real_sequence(dev)
    kw = dict(max_tracks=4, sigmas=TC.sigmas_for(14))
    on = SequenceTracker(cfg, m, pipe, on_device=True, **kw).run(frames, dets)
    host = SequenceTracker(cfg, m, pipe, **kw).run(frames, dets)
    assert on[0]["born"].tolist() == [True, True, True, False] and (on[0]["ids"][:3] == [0, 1, 2]).all()
    for t, (d, h) in enumerate(zip(on, host)):
        for k in ("ids", "born", "died"):
            assert np.array_equal(d[k], h[k]), f"frame {t}: {k} {d[k]} != {h[k]}"
        same = np.abs(d["preds"][:, :, :2] - h["preds"][:, :, :2]).max(axis=2) <= 1e-3
        dm, ds = np.abs(d["preds"][:, :, 2] - h["preds"][:, :, 2]).max(), np.abs(d["score"] - h["score"]).max()
        print(f"frame {t}: {100 * (1 - same.mean()):.1f} % of the key points moved, maxvals differ by {dm:.3e}, scores by {ds:.3e}")
        assert same.mean() >= 0.95 and dm <= 2e-3 and ds <= 2e-3


def test_on_a_forward_graph(dev):
    from buctd_amd import engine
    from buctd_amd.dataset.pipeline import SequenceTracker
    cfg, m, pipe = _coam(dev)
    frames, dets = _real_sequence(dev)
    kw = dict(max_tracks=4, sigmas=TC.sigmas_for(14), on_device=True)
    eager = SequenceTracker(cfg, m, pipe, **kw).run(frames, dets)
    fg = engine.ForwardGraph(m, warmup=1, autoselect=False)
    graphed = SequenceTracker(cfg, fg, pipe, **kw).run(frames, dets)
    assert fg.replays >= 2
    for a, b in zip(eager, graphed):
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_no_host_wait_inside_the_loop(dev, monkeypatch):
    """The number of host waits and device-to-host copies of a run does not depend on the number of frames."""
    case = TC.scripted(14)
    maps = TC.peak_maps(case)
    frames = _frames(dev, TC.T)
    tracker = _tracker(14, TC.ScriptedPeaks(maps).to(dev), dev, True)
    tracker.run(frames[:1], case["dets"][:1])                      # workspaces and lazy initialisation
    counts = {}

    def counting(owner, name):
        real = getattr(owner, name)

        def wrapper(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, wrapper)

    for owner, name in ((torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "numpy"),
                        (torch.Tensor, "tolist"), (torch.cuda.Event, "synchronize")):
        counting(owner, name)
    seen = []
    for n in (2, TC.T):
        counts.clear()
        tracker.run(frames[:n], case["dets"][:n])
        seen.append(dict(counts))
    print(f"host waits and copies of a run: 2 frames {seen[0]}, {TC.T} frames {seen[1]}")
    assert seen[0] == seen[1] and seen[0].get("cpu", 0) == 1 and "synchronize" not in seen[0]
