"""Generic pose synthesis on the device (every DATASET.DATASET but coco / crowdpose: reference synthesize_pose_fish).
buctd_synthesize_pose with the generic tables against the table-driven CPU twin (tests/helpers/synth_generic_ref.py)
sample by sample, its class frequencies over 4000 persons per scene against what the imported reference produced
(tests/golden/pose_synthesis_generic.npz), DeviceSamplePipeline for a marmoset recipe (device path and use_bu_bbox
fallback) against the twin + oracle.sample, and the joints_weight argument.

Distribution tolerance: the GPU one of tests/test_pose_synthesis.py per joint and class - 4.5 sigma of the difference of
two binomial frequencies (4000 and 1500 samples), variance floor 1e-3, plus 0.004 - and the same formula on the frequencies
pooled over the scene's joints (see tests/test_synth_generic.py): per joint sigma is ~ 0.011 against ladder steps of 0.05 to
0.07, pooled over 7 joints ~ 0.004, which is what tells a wrong row or threshold from the right one."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import synth_generic_ref as G

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MARMOSET_K = 15
MARMOSET_FLIP_PAIRS = [[1, 3], [4, 6], [5, 7], [8, 9], [10, 11]]          # reference lib/dataset/marmosets.py:39
MARMOSET_UPPER_BODY = (0, 1, 2, 3, 4, 6, 10, 11, 12)                      # marmosets.py:41


# ---- 1. the kernel against the twin, sample by sample -----------------------------------------------------------------
def _persons(K, spec):
    """spec: (annotated joints, num_overlap, with neighbours) per person -> J, E [B, K, 3], N [B, 2, K, 3], ov [B]."""
    J, E, N = [], [], []
    for b, (n_ann, _, with_near) in enumerate(spec):
        joints, est, near, area = G.make_scene(K, n_ann, 2, 20 + b)
        if not with_near:
            near[:, :, 2] = 0
        J.append(joints), E.append(est), N.append(near)
    return np.stack(J), np.stack(E), np.stack(N), np.array([s[1] for s in spec]), area


def _check_batch(dataset, K, spec, seed):
    from buctd_amd.dataset import pose_synthesis as D
    J, E, N, ov, area = _persons(K, spec)
    B, T = len(spec), G.generic_tables(K)
    out = D.synthesize_pose_batch(dataset, J, E, N, [area] * B, ov, seed=seed)
    assert out.shape == (B, K, 3) and out.dtype == torch.float64
    out = out.cpu().numpy()
    alone = D.synthesize_pose_batch(dataset, J, E, None, [area] * B, ov, seed=seed).cpu().numpy()      # M = 0
    assert not out[:, :, 2].any() and not alone[:, :, 2].any()
    moved = 0
    for b in range(B):
        ref = G.synthesize_pose(T, J[b], E[b], N[b], area, int(ov[b]), seed=seed, person=b)
        err = np.abs(out[b] - ref).max()
        assert err <= 1e-6, f"K {K}, person {b} {spec[b]}: HIP differs from the twin by {err}"
        ref0 = G.synthesize_pose(T, J[b], E[b], np.zeros((0, K, 3)), area, int(ov[b]), seed=seed, person=b)
        err = np.abs(alone[b] - ref0).max()
        assert err <= 1e-6, f"K {K}, person {b} {spec[b]} without neighbours (M = 0): HIP differs from the twin by {err}"
        if not spec[b][2]:
            assert np.array_equal(out[b], alone[b]), "invisible neighbours are no neighbours"
        moved += int((np.abs(out[b, :, :2] - np.where(J[b][:, 2:3] != 0, J[b], E[b])[:, :2]).max(1) > 1e-3).sum())
    assert moved >= B * K * 0.9, "the output is the input pose"


def test_hip_generic_synthesis_matches_the_twin(dev):
    # annotated counts 7...2, num_overlap 0 and 1 where the crowded rule looks at it (nv <= 5), one person whose
    # neighbours are all invisible; the whole batch once more with near=None
    spec = [(7, 0, True), (6, 0, True), (5, 0, True), (5, 1, True), (4, 0, True), (4, 1, True), (3, 1, True), (2, 0, True),
            (2, 1, True), (7, 0, False)]
    assert len(spec) == 10
    _check_batch("fish", 7, spec, seed=4242)


@pytest.mark.parametrize("K,spec", [(1, [(1, 0, True), (1, 1, True), (0, 1, True)]),
                                    (32, [(32, 0, True), (5, 1, True), (2, 0, False)])])
def test_hip_generic_synthesis_at_the_smallest_and_largest_joint_count(dev, K, spec):
    _check_batch("anything", K, spec, seed=99)


def test_reference_signature_for_a_fish_config(dev):
    from buctd_amd.dataset import pose_synthesis as D
    joints, est, near, area = G.make_scene(7, 6, 2, 31)

    class Cfg:
        class MODEL:
            NUM_JOINTS = 7

        class DATASET:
            DATASET = "fish"
    one = D.synthesize_pose(Cfg, joints, est, near, area, 1, seed=77)
    assert isinstance(one, np.ndarray) and one.shape == (7, 3)
    assert np.abs(one - G.synthesize_pose(G.generic_tables(7), joints, est, near, area, 1, seed=77)).max() <= 1e-6
    none = D.synthesize_pose(Cfg, joints, est, np.zeros((0, 7, 3)), area, 1, seed=78)
    assert np.abs(none - G.synthesize_pose(G.generic_tables(7), joints, est, np.zeros((0, 7, 3)), area, 1, seed=78)).max() <= 1e-6


# ---- 2. the distribution against the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("scene", range(len(G.SCENES)))
def test_hip_generic_distribution_matches_reference_golden(dev, scene):
    from buctd_amd.dataset import pose_synthesis as D
    K, n_ann, ov, n_near, seed = G.SCENES[scene]
    joints, est, near, area = G.make_scene(K, n_ann, n_near, seed)
    n = 4000
    big = D.synthesize_pose_batch("marmosets" if K == 15 else "fish", np.stack([joints] * n), np.stack([est] * n),
                                  np.stack([near] * n) if n_near else None, [area] * n, [ov] * n, seed=9 + scene).cpu().numpy()
    assert not big[:, :, 2].any()
    G.check_against_golden(G.class_counts(big, joints, est, near, area), n, scene, 1e-3, 0.004)


# ---- 3. DeviceSamplePipeline for a marmoset recipe ---------------------------------------------------------------------
def _colors():
    from oracle import core as oc
    return oc.CROWDPOSE_KPT_COLORS + [[200, 200, 30]]


def _cfg(different_weight=False, **ds):
    from oracle import cfg as ocfg
    c = ocfg.hrnet_cfg(16, MARMOSET_K, (64, 96), "pose_hrnet_coam", use_attention=True, colored=True, stage_modules=(1, 1, 1))
    c.DATASET.update({"DATASET": "marmosets", "SYNTHESIS_POSE": True, "SCALE_FACTOR": 0.35, "ROT_FACTOR": 45, "FLIP": True,
                      "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3, "BU_BBOX_MARGIN": 25})
    c.DATASET.update(ds)
    c.LOSS.update({"USE_DIFFERENT_JOINTS_WEIGHT": different_weight})
    c.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    return c


def _pipe(different_weight=False, seed=0, ds=None, **kw):
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    return DeviceSamplePipeline(_cfg(different_weight, **(ds or {})), MARMOSET_FLIP_PAIRS, MARMOSET_UPPER_BODY, _colors(),
                                MEAN, STD, is_train=True, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def _records(n=5, seed=12):
    """Train records without cond_joints, as in tests/test_gpu_synth_pipeline.py: two un-annotated joints per person,
    2 / 0 / 1 / 2 / 1 neighbours."""
    from oracle import sample as S
    k = MARMOSET_K
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(n):
        h, w = int(rng.randint(90, 200)), int(rng.randint(100, 260))
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        joints = np.ones((k, 3))
        joints[:, 0], joints[:, 1] = rng.rand(k) * (w - 20) + 10, rng.rand(k) * (h - 20) + 10
        vis = np.ones((k, 3))
        vis[:, 2] = 0
        for j in rng.choice(np.arange(1, k), 2, replace=False):
            joints[j], vis[j] = 0, 0
        m = [2, 0, 1, 2, 1][i % 5]
        near = np.ones((m, k, 3))
        near[:, :, 0], near[:, :, 1] = rng.rand(m, k) * w, rng.rand(m, k) * h
        if m:
            near[0, 5, 2] = 0
        x, y, bw, bh = S.box_from_keypoints(joints, 10, w, h)
        c, s = S.xywh2cs(x, y, bw, bh, 64 / 96, 1.25)
        recs.append({"image_np": img, "joints_3d": joints, "joints_3d_vis": vis, "near_joints": near.reshape(-1),
                     "center": c, "scale": s, "score": 0.5 + 0.1 * i, "annotation_id": 100 + i})
    return tuple(recs)


def _augs(recs):
    return [(r["center"] + np.float32(i), r["scale"] * np.float32(1 + 0.07 * i), [0, 17.5, -33, 0, 45][i % 5], bool(i % 2))
            for i, r in enumerate(recs)]


def _on_device(recs, dev, **over):
    return [dict(r, image=torch.from_numpy(r["image_np"]).to(dev), **over) for r in recs]


@functools.lru_cache(maxsize=None)
def _twin_poses(seed):
    """The twin's pose of every record of _records() as person i of a batch with seed `seed` (computed once, read only)."""
    k, T, out = MARMOSET_K, G.generic_tables(MARMOSET_K), []
    for i, r in enumerate(_records()):
        J = r["joints_3d"]
        xs, ys = J[:, 0][np.nonzero(J[:, 0])], J[:, 1][np.nonzero(J[:, 1])]           # JointsDataset.py:204-210
        area = (np.max(xs) - np.min(xs)) * (np.max(ys) - np.min(ys))
        near = np.asarray(r["near_joints"], dtype=np.float64).reshape(-1, k, 3)
        pose = G.synthesize_pose(T, J, J, near, area, 0, seed, person=i)
        pose.setflags(write=False)
        out.append(pose)
    return tuple(out)


def _oracle_sample(r, pose, c, s, rot, flip):
    from oracle import sample as S
    return S.make_sample(r["image_np"], r["joints_3d"], r["joints_3d_vis"], pose, r["joints_3d_vis"], c, s, rot, flip,
                         [64, 96], [16, 24], 2, MARMOSET_FLIP_PAIRS, MEAN, STD, _colors()[:MARMOSET_K], mono=False, stacked=False)


def _check_condition(got, ref, what):
    """the bound of tests/test_gpu_synth_pipeline.py for a colored condition"""
    dc = np.abs(got - ref)
    assert dc.max() <= 2e-3, f"{what}: condition differs by {dc.max()}"


def test_marmoset_pipeline_matches_the_twin_and_the_oracle_render(dev):
    k, seed = MARMOSET_K, 4242
    recs = _records()
    augs = _augs(recs)
    x, target, weight, meta = _pipe()(_on_device(recs, dev), augs, seed=seed)
    assert x.shape == (5, 6, 96, 64)
    for key in ("synth_joints", "cond_joints", "cond_joints_vis"):
        assert meta[key].is_cuda and meta[key].dtype == torch.float64 and meta[key].shape == (5, k, 3), key
    synth, cj_dev = meta["synth_joints"].cpu().numpy(), meta["cond_joints"].cpu().numpy()
    xh, th, wh = x.cpu().numpy(), target.cpu().numpy(), weight.cpu().numpy()
    assert any(a[3] for a in augs) and not all(a[3] for a in augs)
    for i, (r, a, pose) in enumerate(zip(recs, augs, _twin_poses(seed))):
        err = np.abs(synth[i] - pose).max()
        assert err <= 1e-6, f"sample {i}: meta['synth_joints'] differs from the twin by {err}"
        xo, to, wo, jo, cjo, _ = _oracle_sample(r, pose, *a)
        assert np.array_equal(xh[i, :3], xo[:3]), f"sample {i}: normalised crop differs"
        assert np.abs(th[i] - to).max() <= 2e-7 and np.array_equal(wh[i], wo)
        assert np.abs(cj_dev[i] - cjo).max() <= 1e-5, f"sample {i}: meta['cond_joints'] differs"
        _check_condition(xh[i, 3:], xo[3:], f"sample {i}")
        gt = _oracle_sample(r, r["joints_3d"], *a)[0][3:]
        assert np.abs(xh[i, 3:]).max() > 0.5, f"sample {i}: the condition channels are empty"
        assert np.abs(xh[i, 3:] - gt).max() > 0.5, f"sample {i}: the condition is the un-perturbed ground truth"


def test_marmoset_bu_bbox_records_take_the_host_fallback(dev):
    """Augmentation switched off: centre and scale are those of the box around the synthesized pose."""
    from oracle import sample as S
    off = {"SCALE_FACTOR": 0.0, "ROT_FACTOR": 0.0, "FLIP": False, "PROB_HALF_BODY": 0.0}
    recs, seed = _records(), 4242
    dev_recs = [dict(r, use_bu_bbox=i != 2) for i, r in enumerate(_on_device(recs, dev))]
    x, target, weight, meta = _pipe(ds=off)(dev_recs, seed=seed)
    assert meta["synth_joints"].is_cuda and not meta["cond_joints"].is_cuda
    synth = meta["synth_joints"].cpu().numpy()
    boxed = 0
    for i, (r, pose) in enumerate(zip(recs, _twin_poses(seed))):
        err = np.abs(synth[i] - pose).max()
        assert err <= 1e-6, f"sample {i}: meta['synth_joints'] differs from the twin by {err}"
        h, w = r["image_np"].shape[:2]
        if i != 2 and pose[:, 0].sum() != 0 and pose[0, 1] != 0:          # JointsDataset.py:218
            c, s = S.xywh2cs(*S.box_from_keypoints(pose, 25, w, h), 64 / 96, 1.25)
            boxed += 1
        else:
            c, s = r["center"], r["scale"]
        # the twin's pose is within 1e-6 of the kernel's: its box may round to a neighbouring float32
        mc, ms = meta["center"][i].numpy(), meta["scale"][i].numpy()
        assert np.abs(mc - c).max() <= 1e-4 and np.abs(ms - s).max() <= 1e-6, f"sample {i}: box"
        xo, to, wo, jo, cjo, _ = _oracle_sample(r, pose, mc, ms, 0, False)
        assert np.array_equal(x[i, :3].cpu().numpy(), xo[:3]), f"sample {i}: normalised crop differs"
        assert np.abs(target[i].cpu().numpy() - to).max() <= 2e-7 and np.array_equal(weight[i].cpu().numpy(), wo)
        assert np.abs(meta["cond_joints"][i].numpy() - cjo).max() <= 1e-5
        _check_condition(x[i, 3:].cpu().numpy(), xo[3:], f"sample {i}")
    assert boxed >= 3


# ---- 4. joints_weight ---------------------------------------------------------------------------------------------------
JOINTS_WEIGHT = np.array([1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5, 0.5, 2., 1.3], dtype=np.float32)


@pytest.mark.parametrize("bu_bbox", [False, True])
def test_joints_weight_scales_the_target_weight(dev, bu_bbox):
    recs = _on_device(_records(), dev, use_bu_bbox=bu_bbox)
    augs = _augs(recs)
    plain = _pipe()(recs, augs, seed=5)
    for jw in (JOINTS_WEIGHT, JOINTS_WEIGHT.reshape(MARMOSET_K, 1)):
        got = _pipe(True, joints_weight=jw)(recs, augs, seed=5)
        assert got[2].shape == (5, MARMOSET_K, 1) and got[2].dtype == torch.float32
        assert torch.equal(got[2].cpu(), plain[2].cpu() * torch.from_numpy(JOINTS_WEIGHT).view(1, MARMOSET_K, 1))
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    w = plain[2].cpu().numpy()
    assert (w == 0).any() and (w == 1).any() and not torch.equal(got[2], plain[2])
    # flag off: the argument is not looked at; flag on without the argument: nothing to multiply by
    for other in (_pipe(False, joints_weight=JOINTS_WEIGHT), _pipe(True)):
        out = other(recs, augs, seed=5)
        assert all(torch.equal(a, b) for a, b in zip(out[:3], plain[:3]))
        assert out[3].keys() == plain[3].keys()
        for key, v in plain[3].items():
            assert torch.equal(out[3][key], v) if torch.is_tensor(v) else out[3][key] == v, key
    with pytest.raises(ValueError):
        _pipe(True, joints_weight=JOINTS_WEIGHT[:14])
