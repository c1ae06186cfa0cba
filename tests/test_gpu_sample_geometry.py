"""DeviceSamplePipeline(geometry_on_device=True): buctd_sample_geometry against geometry() record by record, the whole
pipeline with the flag against without it, a generative-sampling batch with use_bu_bbox records against the oracle, the
status bits and one core.function.train pass.

Tolerance of the float64 outputs (the matrix, the joints, the condition joints): geometry_cases.TOL = 1.4e-6.  It is the
larger of the two errors tests/test_sample_geometry.py measures against the exact solution of the 3-point system (the
solve's, 2.64e-10 -> 2.7e-10), carried through |A| |x| + |t| for a coordinate of 640 px (x 1281) and multiplied by 4 for
the kernel's own one rounding per operation."""
import numpy as np
import pytest
import torch

import geometry_cases as G
from test_sample_geometry import pipeline_batch

pytestmark = pytest.mark.gpu


def _table(items):
    from buctd_amd.dataset.pipeline import WARP_ITEM
    return items.cpu().numpy().reshape(-1).view(WARP_ITEM)


def _host(pipe, recs, ds, cond=None, vis=None):
    blank = np.zeros((G.IMG_H, G.IMG_W, 3), np.uint8)
    return [pipe.geometry(dict(r, image=blank), aug=d, cond=None if cond is None else (cond[i], vis[i]))
            for i, (r, d) in enumerate(zip(recs, ds))]


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [14, 17, 1, 32])
def test_kernel_matches_geometry_record_by_record(dev, K):
    from buctd_amd.dataset.pipeline import target_centres, trunc_condition
    B = 16
    base = G.records(K, B, seed=11 + K)
    recs = [dict(r, use_bu_bbox=i % 2 == 0) for i, r in enumerate(base)]
    ds = G.draws(recs, bbox_aug=True)
    pipe = G.pipe_for(K, BBOX_AUGMENTATION=True)
    cond = np.stack([r["cond_joints"] for r in recs])
    vis = np.stack([r["cond_joints_vis"] for r in recs])
    if K == 1:
        # a single joint is the centre of its own bottom-up box and lands on the crop's centre, an integer, on the host
        # path alone: put it within the margin of two borders, where the clipped box is not centred on it
        cond[:, 0, 0], cond[:, 0, 1] = 3.3 + 1.1 * np.arange(B), G.IMG_H - 4.7 - 0.9 * np.arange(B)
    host = _host(pipe, recs, ds, cond, vis)
    g = pipe.device_geometry(G.on_device(recs, dev), pipe.draw_table(recs, ds), torch.from_numpy(cond).to(dev), vis)
    got = {k: v.cpu().numpy() for k, v in g.items() if k != "items"}
    items = _table(g["items"])
    assert not got["status"].any()
    assert np.array_equal(items["flip"], [int(d["flip"]) for d in ds]) and 0 < items["flip"].sum() < B
    rect = np.array([h["keep_rect"] if h["keep_rect"] is not None else (0, 0, 0, 0) for h in host])
    assert np.array_equal(np.stack([items[k] for k in ("rx", "ry", "rw", "rh")], 1), rect)
    assert (rect[:, 2] > 0).sum() >= B // 2 and (rect[1::2, 2] == 0).all()          # odd records: no 'bbox', no bottom-up box
    for key, ref in (("joints", "joints"), ("cond_joints", "cond_joints")):
        err = np.abs(got[key] - np.stack([h[ref] for h in host])).max()
        print(f"K = {K}: max |{key} - host| = {err:.3e}")
        assert err <= G.TOL, (key, err)
    err = np.abs(items["m"].reshape(B, 2, 3) - np.stack([h["trans"] for h in host])).max()
    print(f"K = {K}: max |m - host| = {err:.3e}")
    assert err <= G.TOL
    assert np.array_equal(got["joints_vis"], np.stack([h["joints_vis"] for h in host]))
    assert np.array_equal(got["cond_joints_vis"], np.stack([h["cond_joints_vis"] for h in host]))
    assert np.array_equal(got["target_vis"], np.stack([h["joints_vis"][:, 0] for h in host]).astype(np.float32))
    assert np.array_equal(got["center"], np.stack([h["center"] for h in host]))
    assert np.array_equal(got["scale"], np.stack([h["scale"] for h in host])) and got["scale"].dtype == np.float64
    assert np.array_equal(got["rotation"], [float(d["rot"]) for d in ds])
    # integer steps: equal wherever the host value is clear of one by the tolerance.  Only coordinates that went through
    # the affine can be near one on one side alone; the others are bit-identical inputs
    hj, hc = np.stack([h["joints"] for h in host]), np.stack([h["cond_joints"] for h in host])
    moved_j = np.stack([h["joints_vis"][:, 0] > 0 for h in host])[:, :, None]
    moved_c = np.stack([h["cond_joints_vis"][:, 0] > 0 for h in host])[:, :, None]
    stride = np.array([4.0, 4.0])
    skip_t = G.near_integer(hj[:, :, :2] / stride + 0.5) & moved_j
    skip_c = G.near_integer(hc[:, :, :2]) & moved_c
    left_out = (skip_t.any(2) | skip_c.any(2)).mean()
    print(f"K = {K}: {100 * left_out:.2f} % of the joints within {G.TOL:.1e} of an integer step")
    assert left_out <= 0.02
    ref_t, ref_c = target_centres(hj, stride), trunc_condition(hc)
    assert np.array_equal(got["target_xy"][:, :, :2][~skip_t], ref_t[:, :, :2][~skip_t])
    assert np.array_equal(got["cond_trunc"][~skip_c], ref_c[~skip_c])
    assert np.abs(got["cond_trunc"] - ref_c).max() <= 1 and np.abs(got["target_xy"][:, :, :2] - ref_t[:, :, :2]).max() <= 4
    # the cases the fixture is there for
    took_box = [i for i, (r, h) in enumerate(zip(recs, host)) if r["use_bu_bbox"] and not np.array_equal(h["center"][1], r["center"][1])
                and ds[i]["half_body"] is None]
    assert len(took_box) >= 4
    if K > 8:
        assert np.array_equal(got["center"][4, 1], recs[4]["center"][1]), "y of joint 0 is 0: the record's box"
        assert np.array_equal(got["joints"][2, 5], [0, 0, 0]) and got["joints_vis"][3, 2, 0] == 0
    assert sum(d["half_body"] is not None for d in ds) >= 3


# ---- 2. the pipeline with the flag against without it -----------------------------------------------------------------
def _levels(x):
    mean, std = np.asarray(G.MEAN, np.float32)[None, :, None, None], np.asarray(G.STD, np.float32)[None, :, None, None]
    return np.rint((x[:, :3] * std + mean) * 255).astype(int)


@pytest.mark.parametrize("mode,conditional,synthesis", [("colored", True, True), ("mono", True, True), ("stacked", True, True),
                                                        ("colored", True, False), ("mono", True, False),
                                                        ("stacked", True, False), ("colored", False, False)])
def test_pipeline_with_the_flag_equals_the_host_path(dev, mode, conditional, synthesis):
    from oracle import sample as S
    recs, ds = pipeline_batch()
    if synthesis or not conditional:
        recs = [{k: v for k, v in r.items() if not k.startswith("cond_")} for r in recs]
    dev_recs = G.on_device(recs, dev)
    on = G.pipe_for(14, mode, conditional, synthesis, seed=3, on_device=True)(dev_recs, ds, seed=77)
    off = G.pipe_for(14, mode, conditional, synthesis, seed=3)(dev_recs, ds, seed=77)
    assert on[0].shape == off[0].shape and on[0].shape[0] == len(recs)
    meta = on[3]
    for key in ("joints", "joints_vis", "cond_joints", "cond_joints_vis", "center", "scale", "rotation"):
        assert meta[key].is_cuda, key
        ref = off[3][key].cpu().numpy()
        # the host path keeps the rotation as float32 (torch.tensor of Python floats): 0.01 is rounded there
        tol = G.TOL if key in ("joints", "cond_joints") else 1e-5 if key == "rotation" else 0
        assert np.abs(meta[key].cpu().numpy() - ref).max() <= tol, key
    items = _table(meta["table"])
    x_on, x_off = on[0].cpu().numpy(), off[0].cpu().numpy()
    rects = 0
    for i, (r, d) in enumerate(zip(recs, ds)):
        it = items[i]
        rect = (it["rx"], it["ry"], it["rw"], it["rh"]) if it["rw"] > 0 else None
        rects += rect is not None
        crop = S.warp_affine_u8(r["image_np"], it["m"].reshape(2, 3), G.CROP, flip_src=bool(it["flip"]), keep_rect=rect)
        assert np.array_equal(x_on[i, :3], S.to_tensor_normalize(crop, G.MEAN, G.STD)), f"sample {i}: crop differs from the oracle"
    assert rects >= 3
    la, lb = _levels(x_on), _levels(x_off)
    assert np.abs(la - lb).max() <= 1 and (la != lb).mean() <= 1e-3
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2]), "target / target_weight"
    if conditional:
        dc = np.abs(x_on[:, 3:] - x_off[:, 3:])
        assert float(np.abs(x_on[:, 3:]).max()) > 0.5
        assert dc.max() <= (1.0 if mode == "mono" else 2e-3) and (dc > 2e-3).mean() <= 1e-3
    if synthesis:
        assert torch.equal(meta["synth_joints"], off[3]["synth_joints"])


# ---- 3. generative sampling with use_bu_bbox records -------------------------------------------------------------------
def test_bu_bbox_records_stay_on_the_device_and_match_the_oracle(dev, monkeypatch):
    """The bounds of test_bu_bbox_records_take_the_host_fallback_and_match_the_oracle; augmentation and the keep-rectangle
    switched off (oracle.sample.make_sample knows neither half body nor rectangle)."""
    from oracle import sample as S
    off = {"SCALE_FACTOR": 0.0, "ROT_FACTOR": 0.0, "FLIP": False, "PROB_HALF_BODY": 0.0, "NEW_AUGMENTATION": False}
    base = [{k: v for k, v in r.items() if not k.startswith("cond_")} for r in G.records(14, 16)[:5]]
    recs = [dict(r, use_bu_bbox=i != 2) for i, r in enumerate(base)]
    dev_recs = G.on_device(recs, dev)
    pipe = G.pipe_for(14, synthesis=True, on_device=True, **off)
    pipe(dev_recs, seed=98)                                       # workspaces, the pair table
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
    x, target, weight, meta = pipe(dev_recs, seed=99)
    assert counts == {}, f"device-to-host copies or waits inside __call__: {counts}"
    monkeypatch.undo()
    assert meta["cond_joints"].is_cuda and meta["synth_joints"].is_cuda
    pipe.check(meta)
    synth, center, scale = meta["synth_joints"].cpu().numpy(), meta["center"].cpu().numpy(), meta["scale"].cpu().numpy()
    cj = meta["cond_joints"].cpu().numpy()
    colors = np.asarray(G.colors(14))[:14]
    boxed = 0
    for i, r in enumerate(recs):
        pose = synth[i]
        if i != 2 and pose[:, 0].sum() != 0 and pose[0, 1] != 0:          # JointsDataset.py:218
            c, s = S.xywh2cs(*S.box_from_keypoints(pose, 25, G.IMG_W, G.IMG_H), G.CROP[0] / G.CROP[1], 1.25)
            boxed += 1
        else:
            c, s = r["center"], r["scale"]
        assert np.array_equal(center[i], c) and np.array_equal(scale[i], s.astype(np.float64)), f"sample {i}: box"
        xo, to, wo, jo, cjo, _ = S.make_sample(r["image_np"], r["joints_3d"], r["joints_3d_vis"], pose, r["joints_3d_vis"], c,
                                               scale[i], 0, False, list(G.CROP), [16, 24], 2, G.PAIRS[14], G.MEAN, G.STD, colors)
        assert np.array_equal(x[i, :3].cpu().numpy(), xo[:3]), f"sample {i}: normalised crop differs"
        assert np.abs(target[i].cpu().numpy() - to).max() <= 2e-7 and np.array_equal(weight[i].cpu().numpy(), wo)
        assert np.abs(cj[i] - cjo).max() <= 1e-9
        dc = np.abs(x[i, 3:].cpu().numpy() - xo[3:])
        assert dc.max() <= 2e-3, f"sample {i}: condition differs by {dc.max()}"
    assert boxed >= 3


# ---- 4. status -----------------------------------------------------------------------------------------------------------
def test_a_pose_without_a_non_zero_x_sets_its_status_bit(dev):
    recs = [dict(r, use_bu_bbox=True) for r in G.records(14, 16)[:6]]
    cond = np.stack([r["cond_joints"] for r in recs])
    cond[1, :, 0] = 0                                           # sample 1 (flipped by its draw): no non-zero x
    cond[4, :, 1] = 0                                           # sample 4: no non-zero y
    recs = [dict(r, cond_joints=cond[i]) for i, r in enumerate(recs)]
    ds = G.draws(recs)
    pipe = G.pipe_for(14, on_device=True)
    g = pipe.device_geometry(G.on_device(recs, dev), pipe.draw_table(recs, ds), cond, np.stack([r["cond_joints_vis"] for r in recs]))
    assert g["status"].cpu().tolist() == [0, 1, 0, 0, 1, 0]
    items = _table(g["items"])
    for b in (1, 4):
        assert not items["m"][b].any() and items["flip"][b] == 0 and items["rw"][b] == 0, "the table entry is untouched"
        assert items["H"][b] == G.IMG_H and items["W"][b] == G.IMG_W
        assert not g["joints"][b].any() and not g["target_vis"][b].any() and not g["cond_trunc"][b].any()
    assert items["m"][0].any() and items["flip"][1] == 0 and ds[1]["flip"]
    x, target, weight, meta = pipe(G.on_device(recs, dev), ds)               # the call itself does not raise
    with pytest.raises(ValueError, match="without a non-zero x or y"):
        pipe.check(meta)
    ok = pipe(G.on_device(G.records(14, 16)[:6], dev), ds)
    pipe.check(ok[3])
    assert torch.isfinite(x).all() and torch.isfinite(target).all()


def test_refusals(dev):
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    with pytest.raises(ValueError, match="is_train"):
        DeviceSamplePipeline(G.cfg_for(14), G.PAIRS[14], range(8), G.colors(14), is_train=False, geometry_on_device=True)
    recs = G.on_device(G.records(14, 16)[:2], dev)
    pipe = G.pipe_for(14, on_device=True)
    with pytest.raises(ValueError, match="draw"):
        pipe(recs, [(r["center"], r["scale"], 0, False) for r in recs])


# ---- 5. the train entry point ------------------------------------------------------------------------------------------
def test_train_pass_on_flag_on_batches(dev, tmp_path):
    from oracle import core as oc
    from buctd_amd import engine, models
    from buctd_amd.config import cfg as base, hrnet_extra
    from buctd_amd.core.function import train
    from buctd_amd.core.loss import JointsMSELoss
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    c = base.clone()
    c.defrost()
    c.MODEL.NAME, c.MODEL.NUM_JOINTS, c.MODEL.IMAGE_SIZE, c.MODEL.HEATMAP_SIZE, c.MODEL.SIGMA = "pose_hrnet_coam", 14, [64, 96], [16, 24], 2
    c.MODEL.ATT_MODULES, c.MODEL.CONDITIONAL_TOPDOWN = [False, True, False, False], True
    c.MODEL.EXTRA = hrnet_extra(16, use_attention=True, modules=(1, 1, 1))
    c.DATASET.DATASET, c.DATASET.SYNTHESIS_POSE, c.DATASET.COLORED = "crowdpose", True, True
    c.PRINT_FREQ = 1
    c.freeze()
    assert c.DATASET.NEW_AUGMENTATION is True
    pipe = DeviceSamplePipeline(c, oc.CROWDPOSE_FLIP_PAIRS, range(8), oc.CROWDPOSE_KPT_COLORS, G.MEAN, G.STD, is_train=True,
                                seed=3, geometry_on_device=True)
    recs = [{k: v for k, v in r.items() if not k.startswith("cond_")} for r in G.records(14, 16)[:5]]
    recs = G.on_device([dict(r, use_bu_bbox=i % 2 == 0) for i, r in enumerate(recs)], dev)
    loader = [pipe(recs[:3]), pipe(recs[2:])]
    for x, _, _, meta in loader:
        assert x.is_cuda and meta["cond_joints"].is_cuda and meta["scale"].is_cuda
        pipe.check(meta)
    torch.manual_seed(5)
    model = engine.DataParallel(models.pose_hrnet_coam.get_pose_net(c, is_train=False)).cuda()
    opt = engine.get_optimizer(c, model)

    class Writer:
        losses = []

        def add_scalar(self, key, v, s):
            if key == "train_loss":
                self.losses.append(float(v))

    wd = {"writer": Writer(), "train_global_steps": 0}
    train(c, loader, model, JointsMSELoss(True).cuda(), opt, 0, str(tmp_path), str(tmp_path), wd)
    assert len(Writer.losses) == 2 and all(np.isfinite(v) and v > 0 for v in Writer.losses), Writer.losses
