"""IterativeRefiner(on_device=True): the passes chained on the device against the host chain.

The seeded test networks amplify one-ulp differences, so two free-running chains are compared only
through a smooth stand-in network (refine_cases.FixedPeaks); on the real network every device pass is compared with ONE
host pass that starts from the device chain's own previous predictions."""
import numpy as np
import pytest
import torch

from refine_cases import FixedPeaks, cfg_for, kernel_case, on_device, peak_table, pipe_for, records

pytestmark = pytest.mark.gpu
KEYS = ("preds", "score", "box_score", "keypoint_score", "center", "scale")


def _coam(dev):
    from oracle import recipes
    from buctd_amd import models
    cfg, omodel, _, _ = recipes.build("coam_w16_96x64_colored")
    cfg.DATASET.update({"BU_BBOX_MARGIN": 25, "FLIP": False})
    cfg.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    m = models.pose_hrnet_coam.get_pose_net(cfg, is_train=False)
    m.load_state_dict(omodel.state_dict(), strict=True)
    return cfg, m.to(dev).eval(), pipe_for(14, cfg=cfg)


def _ulps(a, b):
    """|a - b| in units of the float32 spacing at b"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


def test_teacher_forced_chain_on_a_real_network(dev):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe = _coam(dev)
    recs = on_device(records(3, 21), dev)
    hist = IterativeRefiner(cfg, m, pipe, on_device=True).run(recs, 3)
    host = IterativeRefiner(cfg, m, pipe)
    assert len(hist) == 3 and hist[0]["preds"].shape == (3, 14, 3)
    first = host.run(recs, 1)[0]
    # pass 0 shares the host geometry: the same network input, so the same heat-maps.  The two scores are float64 sums on
    # the device and numpy's float32 sum on the host: within K * 2^-24, like in tests/test_gpu_refine_step.py
    for k in ("preds", "box_score", "center", "scale"):
        assert np.array_equal(hist[0][k], first[k]), f"pass 0: {k} differs from the host path"
    for k in ("score", "keypoint_score"):
        assert np.abs(hist[0][k] - first[k]).max() <= 1e-5, f"pass 0: {k} differs from the host path"
    for p in (1, 2):
        h = host.run(host.next_records(recs, hist[p - 1]["preds"], hist[p - 1]["score"]), 1)[0]
        d = hist[p]
        assert np.array_equal(d["center"], h["center"]) and np.array_equal(d["scale"], h["scale"]), f"pass {p}: box"
        assert np.array_equal(d["box_score"], h["box_score"])
        same = np.abs(d["preds"][:, :, :2] - h["preds"][:, :, :2]).max(axis=2) <= 1e-3
        print(f"pass {p}: {100 * (1 - same.mean()):.1f} % of the key points moved, "
              f"maxvals differ by {np.abs(d['preds'][:, :, 2] - h['preds'][:, :, 2]).max():.3e}")
        assert same.mean() >= 0.95, f"pass {p}: {100 * (1 - same.mean()):.1f}% of the key points moved"
        assert np.abs(d["preds"][:, :, 2] - h["preds"][:, :, 2]).max() <= 2e-3


@pytest.mark.parametrize("mode,use_dark", [("colored", False), ("mono", False), ("stacked", False), ("colored", True)])
def test_free_running_chain_with_a_smooth_network(dev, mode, use_dark):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14, mode), pipe_for(14, mode)
    recs = on_device(records(3, 21), dev)
    net = FixedPeaks(peak_table(3, 14, 8)).to(dev)
    a = IterativeRefiner(cfg, net, pipe, use_dark=use_dark, on_device=True).run(recs, 3)
    b = IterativeRefiner(cfg, net, pipe, use_dark=use_dark).run(recs, 3)
    assert len(a) == len(b) == 3 and net.calls == 6
    for p, (d, h) in enumerate(zip(a, b)):
        assert d.keys() == h.keys()
        for k in KEYS:
            assert d[k].shape == h[k].shape and d[k].dtype == h[k].dtype, f"pass {p}: {k} {d[k].dtype}{d[k].shape}"
        dp = np.abs(d["preds"][:, :, :2] - h["preds"][:, :, :2]).max()
        uc, us = _ulps(d["center"], h["center"]).max(), _ulps(d["scale"], h["scale"]).max()
        ds = max(np.abs(d[k] - h[k]).max() for k in ("score", "box_score", "keypoint_score"))
        print(f"{mode} dark {use_dark} pass {p}: preds {dp:.3e} px, center {uc:.2f} ulp, scale {us:.2f} ulp, scores {ds:.3e}")
        assert dp <= 1e-3 and uc <= 1.0 and us <= 1.0 and ds <= 1e-5
        assert np.array_equal(d["preds"][:, :, 2], h["preds"][:, :, 2])
    assert np.abs(a[2]["center"] - a[0]["center"]).max() > 1.0, "the boxes of the chain are meant to move"


def test_on_a_forward_graph(dev):
    from buctd_amd import engine
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe = _coam(dev)
    recs = on_device(records(3, 21), dev)
    eager = IterativeRefiner(cfg, m, pipe, on_device=True).run(recs, 3)
    fg = engine.ForwardGraph(m, warmup=1, autoselect=False)
    graphed = IterativeRefiner(cfg, fg, pipe, on_device=True).run(recs, 3)
    graphed2 = IterativeRefiner(cfg, fg, pipe, on_device=True).run(recs, 3)
    assert fg.replays >= 4
    for a, b, c in zip(eager, graphed, graphed2):
        for k in KEYS:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_no_host_wait_inside_the_loop(dev, monkeypatch):
    """The number of host waits and device-to-host copies of a run does not depend on the number of passes."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14), pipe_for(14)
    recs = on_device(records(3, 21), dev)
    net = FixedPeaks(peak_table(3, 14, 8)).to(dev)
    refiner = IterativeRefiner(cfg, net, pipe, on_device=True)
    refiner.run(recs, 1)                                        # workspaces and lazy initialisation
    counts = {}

    def counting(owner, name):
        real = getattr(owner, name)

        def wrapper(*args, **kwargs):
            counts[name] = counts.get(name, 0) + 1
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, wrapper)

    counting(torch.cuda, "synchronize")
    counting(torch.Tensor, "cpu")
    counting(torch.Tensor, "item")
    counting(torch.Tensor, "numpy")
    counting(torch.Tensor, "tolist")
    counting(torch.cuda.Event, "synchronize")
    seen = []
    for passes in (1, 3):
        counts.clear()
        refiner.run(recs, passes)
        seen.append(dict(counts))
    print(f"host waits and copies of a run: 1 pass {seen[0]}, 3 passes {seen[1]}")
    assert seen[0] == seen[1] and seen[0].get("cpu", 0) == 1 and "synchronize" not in seen[0]
    # the host path is what the counter is meant to catch
    counts.clear()
    IterativeRefiner(cfg, net, pipe).run(recs, 3)
    assert counts.get("synchronize", 0) >= 3


def test_run_raises_for_a_person_without_a_box(dev):
    """Person 0's peaks all sit at heat-map x = 4, which its box (center x 25, scale 0.5) maps to image x = 0 exactly."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14), pipe_for(14)
    recs = on_device(records(3, 21), dev)
    recs[0] = dict(recs[0], center=np.array([25.0, 75.0], np.float32), scale=np.array([0.5, 0.75], np.float32))
    table = np.rint(peak_table(3, 14, 8))
    table[0, :, 0] = 4
    net = FixedPeaks(table).to(dev)
    with pytest.raises(ValueError):
        IterativeRefiner(cfg, net, pipe).run(recs, 2)                         # the host path: min() of an empty array
    with pytest.raises(ValueError, match=r"person\(s\) \[0\]"):
        IterativeRefiner(cfg, net, pipe, on_device=True).run(recs, 2)
    table[0, :, 0] = 5
    assert len(IterativeRefiner(cfg, FixedPeaks(table).to(dev), pipe, on_device=True).run(recs, 2)) == 2


def test_refusals():
    from buctd_amd.dataset.pipeline import IterativeRefiner
    with pytest.raises(ValueError, match="is_train=False"):
        IterativeRefiner(cfg_for(14), None, pipe_for(14, is_train=True), on_device=True)
    with pytest.raises(ValueError, match="at most 32 joints"):
        IterativeRefiner(cfg_for(33), None, pipe_for(33), on_device=True)
    plain = cfg_for(14, conditional=False)
    with pytest.raises(ValueError, match="conditional config"):
        IterativeRefiner(plain, None, pipe_for(14, cfg=plain), on_device=True)
    IterativeRefiner(cfg_for(14), None, pipe_for(14, is_train=True))          # the host path takes all three
    IterativeRefiner(plain, None, pipe_for(14, cfg=plain))
