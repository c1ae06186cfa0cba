"""The flip test inside IterativeRefiner (flip_test=True) on the host and device chains, and the two kernels that build the
mirrored half of the paired input on the device (buctd_cond_mirror, buctd_mirror_rows).

As in test_gpu_refine_chain.py the seeded real network is compared teacher-forced (every device pass against ONE host pass
that starts from the device chain's previous predictions) and two free-running chains only through a smooth stand-in
network (refine_flip_cases.PairedPeaks)."""
import functools

import numpy as np
import pytest
import torch

from refine_cases import EXTRA_COLORS, MEAN, STD, cfg_for, near_integer, on_device, peak_table, pipe_for, records
from refine_flip_cases import MIRROR_CASES, PairedPeaks, Stub, mirror_case, moving_records, pairs_for, to_dev

pytestmark = pytest.mark.gpu
KEYS = ("preds", "score", "box_score", "keypoint_score", "center", "scale")


def _ulps(a, b):
    """|a - b| in units of the float32 spacing at b"""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


# ---- 1: buctd_cond_mirror ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,width,which", MIRROR_CASES)
def test_cond_mirror_kernel_equals_mirror_condition(dev, K, width, which):
    from buctd_amd._C import check, lib, ptr, stream_ptr
    from buctd_amd.utils.transforms import _swap_table, mirror_condition
    pairs = pairs_for(K, which)
    cj, vis = mirror_case(K, width)
    swap = _swap_table(K, pairs)
    pair = to_dev(np.where(swap == np.arange(K), -1, swap).astype(np.int32), dev)
    for joints, v in ((cj, vis), (cj, None), (cj[:, :, :2], None), (cj[:, :, :2], vis)):
        dj, dv = to_dev(joints, dev), None if v is None else to_dev(v, dev)
        out = torch.full((2, K, 2), np.nan, dtype=torch.float32, device=dev)
        check(lib().buctd_cond_mirror(ptr(dj), joints.shape[2], ptr(dv), ptr(pair), 2, K, width, ptr(out), stream_ptr()),
              "cond_mirror")
        want = mirror_condition(cj, v, width, pairs)
        assert np.array_equal(out.cpu().numpy(), want), f"stride {joints.shape[2]}, vis {'given' if v is not None else 'NULL'}"


def test_cond_mirror_through_the_pipeline(dev):
    from buctd_amd.utils.transforms import mirror_condition
    pipe = pipe_for(14)
    cj, vis = mirror_case(14, 64, B=3)
    got = pipe.cond_mirror(to_dev(cj, dev), to_dev(vis, dev))
    assert np.array_equal(got.cpu().numpy(), mirror_condition(cj, vis, 64, pipe.flip_pairs))
    with pytest.raises(ValueError):
        pipe.cond_mirror(to_dev(cj.astype(np.float32), dev))


# ---- 2: buctd_mirror_rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 7, 64, 71])
@pytest.mark.parametrize("count,perm", [(3, None), (3, "swap"), (14, None), (14, "swap"), (14, "pair")])
def test_mirror_rows_equals_flip_and_index_select(dev, W, count, perm):
    from oracle import core as oc
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    from buctd_amd.utils.transforms import _swap_table
    B, H, c0 = 3, 5, 2
    swap = _swap_table(count, oc.CROWDPOSE_FLIP_PAIRS if count == 14 else [[0, 2]])
    table = None
    if perm == "swap":
        table = to_dev(swap.astype(np.int32), dev)
    elif perm == "pair":
        table = to_dev(np.where(swap == np.arange(count), -1, swap).astype(np.int32), dev)
    select = torch.from_numpy(swap if perm else np.arange(count)).to(dev)
    g = torch.Generator().manual_seed(W * 100 + count)
    # rows [B, 2B) of one tensor from its rows [0, B); the channels outside [c0, c0 + count) are not written
    x = torch.randn((2 * B, c0 + count + 1, H, W), generator=g).to(dev)
    keep = x.clone()
    DeviceSamplePipeline.mirror_rows(x[:B], x[B:], c0, count, table)
    want = keep[:B, c0:c0 + count].flip(3).index_select(1, select)
    assert torch.equal(x[B:, c0:c0 + count], want)
    assert torch.equal(x[:B], keep[:B]) and torch.equal(x[B:, :c0], keep[B:, :c0]) and torch.equal(x[B:, c0 + count:], keep[B:, c0 + count:])
    # two tensors with different batch strides
    dst = torch.full((B, c0 + count, H, W), np.nan, device=dev)
    DeviceSamplePipeline.mirror_rows(keep[:B], dst, c0, count, table)
    assert torch.equal(dst[:, c0:], want) and bool(torch.isnan(dst[:, :c0]).all())


def test_mirror_rows_refuses_overlap_and_a_channel_range_outside(dev):
    from buctd_amd._C import BuctdHipError
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    x = torch.zeros((4, 6, 5, 8), device=dev)
    with pytest.raises(BuctdHipError, match="overlap"):
        DeviceSamplePipeline.mirror_rows(x[:3], x[1:], 0, 3)
    with pytest.raises(ValueError):
        DeviceSamplePipeline.mirror_rows(x[:2], x[2:], 4, 3)


# ---- 3: the paired input -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["colored", "mono", "stacked"])
def test_paired_input(dev, mode):
    from oracle import core as oc
    from buctd_amd.dataset.pipeline import trunc_condition
    from buctd_amd.utils import transforms
    pipe = pipe_for(14, mode)
    recs = records(3, 21)
    for i, r in enumerate(recs):                       # invisible condition joints, a partner pair among them
        r["cond_joints_vis"] = r["cond_joints_vis"].copy()
        r["cond_joints_vis"][[i, 4, 9 + i]] = 0
    recs = on_device(recs, dev)
    geos = [pipe.geometry(r) for r in recs]
    table = pipe.warp_table([r["image"] for r in recs], geos)
    cj, cv = np.stack([g["cond_joints"] for g in geos]), np.stack([g["cond_joints_vis"] for g in geos])
    ct = to_dev(trunc_condition(cj), dev)
    stub = Stub(pipe, oc.CROWDPOSE_KPT_COLORS + EXTRA_COLORS)
    single = pipe.warp_and_condition(table, ct)
    assert single.shape == (3, 3 + (14 if mode == "stacked" else 3), 96, 64)
    for joints, vis in ((cj, cv), (np.ascontiguousarray(cj[:, :, :2]), None)):
        x = pipe.warp_and_condition(table, ct, mirrored=(to_dev(joints, dev), None if vis is None else to_dev(vis, dev)))
        assert x.shape == (6,) + single.shape[1:] and x.is_contiguous()
        assert torch.equal(x[:3], single), "rows [0, B) are the unpaired input"
        v = torch.from_numpy(cv if vis is not None else np.ones_like(cv))
        want = torch.cat((single[:, :3].flip(3), transforms.flip_hm(single[:, 3:], stub, torch.from_numpy(cj), v)), 1)
        assert torch.equal(x[3:], want), f"{mode}: rows [B, 2B) differ from _mirrored_input by " \
                                         f"{float((x[3:] - want).abs().max())}"
    assert float(x[3:, 3:].abs().max()) > 0


# ---- the real network, shared ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coam():
    from oracle import recipes
    from buctd_amd import models
    dev = torch.device("cuda:0")
    cfg, omodel, _, _ = recipes.build("coam_w16_96x64_colored")
    cfg.DATASET.update({"BU_BBOX_MARGIN": 25, "FLIP": False})
    cfg.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    m = models.pose_hrnet_coam.get_pose_net(cfg, is_train=False)
    m.load_state_dict(omodel.state_dict(), strict=True)
    return cfg, m.to(dev).eval(), pipe_for(14, cfg=cfg), omodel


@functools.lru_cache(maxsize=None)
def _host_records(which):
    """'issue': refine_cases.records(3, 21), whose boxes are the whole image from pass 1 on; 'moving': persons in large
    images, whose boxes move in every pass (refine_flip_cases.moving_records)"""
    return records(3, 21) if which == "issue" else moving_records(3, 31)


@functools.lru_cache(maxsize=None)
def _device_flip_chain(which="issue"):
    """3 passes of the device chain with the flip test on the real network: computed once, read by several tests"""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, _ = _coam()
    recs = on_device(_host_records(which), torch.device("cuda:0"))
    return IterativeRefiner(cfg, m, pipe, on_device=True, flip_test=True, shift_heatmap=True).run(recs, 3)


def _settled(pipe, recs):
    """[B] bool: persons with a crop coordinate of their condition within 1e-6 of an integer (host geometry)"""
    return near_integer(np.stack([pipe.geometry(r)["cond_joints"][:, :2] for r in recs])).any(axis=1)


# ---- 4: host chain against the oracle loop -----------------------------------------------------------------------------
def test_host_chain_with_the_flip_test_matches_the_oracle_loop(dev):
    """tests/test_sample_pipeline.py::test_iterative_refinement_matches_oracle_loop with the flip test of reference
    function.py:213-236 in every pass; its bounds."""
    from oracle import core as oc, sample as S
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, omodel = _coam()
    recs = records(3, 21)
    hist = IterativeRefiner(cfg, m, pipe, flip_test=True, shift_heatmap=True).run(on_device(recs, dev), 3)
    assert len(hist) == 3 and hist[0]["preds"].shape == (3, 14, 3)
    colors, pairs = oc.CROWDPOSE_KPT_COLORS[:14], oc.CROWDPOSE_FLIP_PAIRS
    cur = [dict(r) for r in recs]
    for p in range(3):
        xs, xf, cs, ss = [], [], [], []
        for r in cur:
            made = S.make_sample(r["image_np"], r["joints_3d"], r["joints_3d_vis"], r["cond_joints"], r["cond_joints_vis"],
                                 r["center"], r["scale"], 0, False, [64, 96], [16, 24], 2, pairs, MEAN, STD, colors)
            xo, cj_crop = made[0], made[4]
            mirrored = oc.fliplr_joints(cj_crop, r["cond_joints_vis"], 64, pairs)[0]
            cond = oc.get_condition_image_colored(mirrored, (96, 64, 3), colors).transpose(2, 0, 1).astype(np.float32)
            xs.append(xo); xf.append(np.concatenate([xo[:3, :, ::-1], cond], 0)); cs.append(r["center"]); ss.append(r["scale"])
        with torch.no_grad():
            out = omodel(torch.from_numpy(np.stack(xs))).numpy()
            out_flipped = omodel(torch.from_numpy(np.stack(xf))).numpy()
        merged = oc.flip_test_merge(out, out_flipped, pairs, shift=True)
        coords, maxvals = oc.get_final_preds(True, merged, np.stack(cs), np.stack(ss))
        h = hist[p]
        same = np.abs(h["preds"][:, :, :2] - coords).max(axis=2) <= 1e-3
        print(f"pass {p}: {100 * (1 - same.mean()):.1f} % of the key points moved, "
              f"maxvals differ by {np.abs(h['preds'][:, :, 2:] - maxvals).max():.3e}")
        assert same.mean() >= 0.95, f"pass {p}: {100 * (1 - same.mean()):.1f}% of the key points moved"
        assert np.abs(h["preds"][:, :, 2:] - maxvals).max() <= 2e-3
        nxt = []
        for r, kp, sc in zip(cur, h["preds"], h["score"]):      # continue from the product's predictions
            cond = np.zeros((14, 3)); cond[:, :2] = kp[:, :2]; cond[:, 2] = kp[:, 2]
            x, y, w, hh = S.box_from_keypoints(cond, 25, r["image_np"].shape[1], r["image_np"].shape[0])
            c, s = S.xywh2cs(x, y, w, hh, 64 / 96, 1.25)
            nxt.append(dict(r, center=c, scale=s, score=float(sc), cond_joints=cond, cond_joints_vis=np.ones((14, 3)),
                            joints_3d=np.zeros((14, 3)), joints_3d_vis=np.ones((14, 3))))
        cur = nxt


# ---- 5: device chain against host chain --------------------------------------------------------------------------------
class _Capture(torch.nn.Module):
    """The network, keeping a copy of every input it is given"""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x):
        self.seen.append(x.clone())
        return self.net(x)

    def take(self):
        seen, self.seen = self.seen, []
        return seen


@pytest.mark.parametrize("which", ["issue", "moving"])
def test_teacher_forced_flip_chain_on_a_real_network(dev, which):
    """Every device pass against ONE host pass that starts from the device chain's previous predictions - the network
    inputs of the two (captured) stage by stage, then the predictions.

    The device chain forms the crop affine in closed form, the host chain solves for it; the two differ by <= 2.5e-11
    (tests/test_refine_closed_form.py).  Two discrete steps can turn that into another network input, neither of them part
    of the flip test:
      - trunc() of a condition coordinate.  A person whose box has stopped moving has the previous pass's heat-map grid as
        crop coordinates, integers to 2e-15.  'issue' records (refine_cases.records(3, 21)): the box is the whole image from
        pass 1 on, in pass 2 all 28 coordinates of all three persons are such; compared anyway, 14.3 % of the key points are
        more than 1e-3 px and max-vals up to 7.2e-2 apart.  'moving' records: no such person in any pass - asserted.
      - the fixed-point rounding of buctd_warp_affine_norm (source coordinates in 1/1024 px, half to even).  'moving'
        records, pass 2, person 0: 397 of its 18432 crop values differ between the chains (up to 0.12), the conditions of
        both halves are equal; compared anyway, heat-maps 4.3e-2 and max-vals 1.2e-2 apart, 1 of 42 key points moved.
    So: the condition channels of both halves are compared exactly for every person without an integer coordinate, the
    mirrored image half exactly against the plain one, and the predictions under the bounds of the same comparison without
    the flip (95 % of the key points within 1e-3 px, max-vals within 2e-3) for every person whose network input is the
    same in both chains.  On the 'moving' records that must be at least two of the three persons in every pass."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, _ = _coam()
    recs = on_device(_host_records(which), dev)
    cap = _Capture(m).eval()
    kw = dict(flip_test=True, shift_heatmap=True)
    hist = IterativeRefiner(cfg, cap, pipe, on_device=True, **kw).run(recs, 3)
    dev_x = cap.take()
    for a, b in zip(hist, _device_flip_chain(which)):
        assert all(np.array_equal(a[k], b[k]) for k in KEYS), "capturing the inputs changes nothing"
    host = IterativeRefiner(cfg, cap, pipe, **kw)
    assert len(hist) == 3 and hist[0]["preds"].shape == (3, 14, 3) and len(dev_x) == 3
    first = host.run(recs, 1)[0]
    assert torch.equal(cap.take()[0], dev_x[0]), "pass 0: the same network input"
    for k in ("preds", "box_score", "center", "scale"):
        assert np.array_equal(hist[0][k], first[k]), f"pass 0: {k} differs from the host path"
    for k in ("score", "keypoint_score"):
        assert np.abs(hist[0][k] - first[k]).max() <= 1e-5, f"pass 0: {k} differs from the host path"
    nxt, B = recs, 3
    for p in (1, 2):
        nxt = host.next_records(nxt, hist[p - 1]["preds"], hist[p - 1]["score"])
        h = host.run(nxt, 1)[0]
        d, xd, xh = hist[p], dev_x[p], cap.take()[0]
        assert np.array_equal(d["center"], h["center"]) and np.array_equal(d["scale"], h["scale"]), f"pass {p}: box"
        assert np.array_equal(d["box_score"], h["box_score"])
        settled = _settled(pipe, nxt)
        if which == "moving" or p == 1:
            assert not settled.any(), f"pass {p}: person(s) {np.nonzero(settled)[0].tolist()} on integer crop coordinates"
        # the network input: [crops | mirrored crops] x [image | condition]
        assert xd.shape == xh.shape == (2 * B, 6, 96, 64)
        assert torch.equal(xd[B:, :3], xd[:B, :3].flip(3)), f"pass {p}: the mirrored image half"
        same_input = np.zeros(B, dtype=bool)
        for b in np.nonzero(~settled)[0]:
            assert torch.equal(xd[b, 3:], xh[b, 3:]), f"pass {p}, person {b}: condition"
            assert torch.equal(xd[B + b, 3:], xh[B + b, 3:]), f"pass {p}, person {b}: mirrored condition"
            assert float(xd[B + b, 3:].abs().max()) > 0 and not torch.equal(xd[B + b, 3:], xd[b, 3:])
            same_input[b] = torch.equal(xd[b], xh[b]) and torch.equal(xd[B + b], xh[B + b])
        every = np.abs(d["preds"][:, :, :2] - h["preds"][:, :, :2]).max(axis=2) <= 1e-3
        print(f"{which} pass {p}: {int(settled.sum())} of 3 persons on integer crop coordinates, {int(same_input.sum())} with the "
              f"same network input; {100 * (1 - every.mean()):.1f} % of all key points moved, maxvals differ by "
              f"{np.abs(d['preds'][:, :, 2] - h['preds'][:, :, 2]).max():.3e}; crop values that differ per person "
              f"{(xd[:B, :3] != xh[:B, :3]).flatten(1).sum(1).tolist()}")
        if which == "moving":
            assert same_input.sum() >= 2, f"pass {p}: only {int(same_input.sum())} person(s) left to compare"
        if same_input.any():
            same = every[same_input]
            assert same.mean() >= 0.95, f"pass {p}: {100 * (1 - same.mean()):.1f}% of the key points moved"
            assert np.abs(d["preds"][same_input][:, :, 2] - h["preds"][same_input][:, :, 2]).max() <= 2e-3
    if which == "moving":
        assert np.abs(hist[2]["center"] - hist[1]["center"]).max() > 1.0, "the boxes are meant to move"


def test_the_no_flip_chain_on_the_issue_records_has_no_settled_person(dev):
    """tests/test_gpu_refine_chain.py compares the same two chains without the flip on records(3, 21) and holds every
    person to its bounds: there the boxes keep moving, no person of passes 1 and 2 has an integer crop coordinate."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, _ = _coam()
    recs = on_device(records(3, 21), dev)
    refiner = IterativeRefiner(cfg, m, pipe, on_device=True)
    hist = refiner.run(recs, 3)
    nxt = recs
    for p in (1, 2):
        nxt = refiner.next_records(nxt, hist[p - 1]["preds"], hist[p - 1]["score"])
        assert not _settled(pipe, nxt).any(), f"pass {p}"
        assert np.abs(hist[p]["center"] - hist[p - 1]["center"]).max() > 0 or np.abs(hist[p]["scale"] - hist[p - 1]["scale"]).max() > 0


@pytest.mark.parametrize("mode,use_dark", [("colored", False), ("mono", False), ("stacked", False), ("colored", True)])
def test_free_running_flip_chain_with_a_smooth_network(dev, mode, use_dark):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14, mode), pipe_for(14, mode)
    recs = on_device(records(3, 21), dev)
    net = PairedPeaks(peak_table(3, 14, 8), pipe.flip_pairs).to(dev)
    kw = dict(use_dark=use_dark, flip_test=True, shift_heatmap=True)
    a = IterativeRefiner(cfg, net, pipe, on_device=True, **kw).run(recs, 3)
    b = IterativeRefiner(cfg, net, pipe, **kw).run(recs, 3)
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


# ---- 6, 7: the keyword ---------------------------------------------------------------------------------------------------
def test_the_flip_is_applied_and_off_is_the_refiner_without_the_keyword(dev):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, _ = _coam()
    recs = on_device(records(3, 21), dev)
    flipped = {True: _device_flip_chain(),
               False: IterativeRefiner(cfg, m, pipe, flip_test=True, shift_heatmap=True).run(recs, 1)}
    for on_dev in (True, False):
        plain = IterativeRefiner(cfg, m, pipe, on_device=on_dev).run(recs, 2)
        off = IterativeRefiner(cfg, m, pipe, on_device=on_dev, flip_test=False, shift_heatmap=True).run(recs, 2)
        for a, b in zip(plain, off):
            for k in KEYS:
                assert np.array_equal(a[k], b[k]), f"on_device={on_dev}: flip_test=False changes {k}"
        moved = np.abs(flipped[on_dev][0]["preds"] - plain[0]["preds"]).max()
        print(f"on_device={on_dev}: the flip test moves pass 0's predictions by up to {moved:.3f}")
        assert moved > 0, f"on_device={on_dev}: flip_test=True returns the predictions of flip_test=False"
    # the config's own TEST.FLIP_TEST is not read
    was = cfg.TEST.FLIP_TEST
    try:
        cfg.TEST.FLIP_TEST = True
        again = IterativeRefiner(cfg, m, pipe, on_device=True).run(recs, 1)
    finally:
        cfg.TEST.FLIP_TEST = was
    plain_dev = IterativeRefiner(cfg, m, pipe, on_device=True).run(recs, 1)
    assert np.array_equal(again[0]["preds"], plain_dev[0]["preds"])


def test_shift_heatmap_defaults_to_the_config(dev):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14), pipe_for(14)
    was = cfg.TEST.SHIFT_HEATMAP
    try:
        for value in (True, False):
            cfg.TEST.SHIFT_HEATMAP = value
            assert IterativeRefiner(cfg, None, pipe, flip_test=True).shift_heatmap is value
            assert IterativeRefiner(cfg, None, pipe, flip_test=True, shift_heatmap=not value).shift_heatmap is (not value)
    finally:
        cfg.TEST.SHIFT_HEATMAP = was
    assert IterativeRefiner(cfg, None, pipe).flip_test is False


# ---- 8: ForwardGraph ---------------------------------------------------------------------------------------------------
def test_flip_chain_on_a_forward_graph(dev):
    from buctd_amd import engine
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, m, pipe, _ = _coam()
    recs = on_device(records(3, 21), dev)
    eager = _device_flip_chain()
    fg = engine.ForwardGraph(m, warmup=1, autoselect=False)
    kw = dict(on_device=True, flip_test=True, shift_heatmap=True)
    graphed = IterativeRefiner(cfg, fg, pipe, **kw).run(recs, 3)
    graphed2 = IterativeRefiner(cfg, fg, pipe, **kw).run(recs, 3)
    assert fg.replays >= 4
    for a, b, c in zip(eager, graphed, graphed2):
        for k in KEYS:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


# ---- 9: no host wait ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["colored", "stacked"])
def test_no_host_wait_inside_the_loop_with_the_flip(dev, monkeypatch, mode):
    """The number of host waits and device-to-host copies of a run does not depend on the number of passes."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14, mode), pipe_for(14, mode)
    recs = on_device(records(3, 21), dev)
    net = PairedPeaks(peak_table(3, 14, 8), pipe.flip_pairs).to(dev)
    refiner = IterativeRefiner(cfg, net, pipe, on_device=True, flip_test=True, shift_heatmap=True)
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
    IterativeRefiner(cfg, net, pipe, flip_test=True, shift_heatmap=True).run(recs, 3)
    assert counts.get("synchronize", 0) >= 3


# ---- 10, 11 ------------------------------------------------------------------------------------------------------------
def test_refusals_with_the_flip():
    from buctd_amd.dataset.pipeline import IterativeRefiner
    kw = dict(on_device=True, flip_test=True)
    with pytest.raises(ValueError, match="is_train=False"):
        IterativeRefiner(cfg_for(14), None, pipe_for(14, is_train=True), **kw)
    with pytest.raises(ValueError, match="at most 32 joints"):
        IterativeRefiner(cfg_for(33), None, pipe_for(33), **kw)
    plain = cfg_for(14, conditional=False)
    with pytest.raises(ValueError, match="conditional config"):
        IterativeRefiner(plain, None, pipe_for(14, cfg=plain), **kw)
    IterativeRefiner(cfg_for(14), None, pipe_for(14, is_train=True), flip_test=True)      # the host path takes all three
    IterativeRefiner(plain, None, pipe_for(14, cfg=plain), flip_test=True)


def test_flip_chain_raises_for_a_person_without_a_box(dev):
    """Person 0's merged peaks all sit at heat-map x = 4, which its box (center x 25, scale 0.5) maps to image x = 0."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    cfg, pipe = cfg_for(14), pipe_for(14)
    recs = on_device(records(3, 21), dev)
    recs[0] = dict(recs[0], center=np.array([25.0, 75.0], np.float32), scale=np.array([0.5, 0.75], np.float32))
    table = np.rint(peak_table(3, 14, 8))
    table[0, :, 0] = 4
    net = PairedPeaks(table, pipe.flip_pairs).to(dev)
    kw = dict(flip_test=True, shift_heatmap=True)
    with pytest.raises(ValueError):
        IterativeRefiner(cfg, net, pipe, **kw).run(recs, 2)                    # the host path: min() of an empty array
    with pytest.raises(ValueError, match=r"person\(s\) \[0\]"):
        IterativeRefiner(cfg, net, pipe, on_device=True, **kw).run(recs, 2)
    table[0, :, 0] = 5
    assert len(IterativeRefiner(cfg, PairedPeaks(table, pipe.flip_pairs).to(dev), pipe, on_device=True, **kw).run(recs, 2)) == 2
