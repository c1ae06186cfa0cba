"""Pose error diagnosis on the device (buctd_pose_error_types in csrc/synth_diag.hip, buctd_amd/dataset/error_diagnosis.py)
against the plain-loop restatement tests/helpers/error_types_ref.py on the seeded sets of
tests/helpers/error_types_cases.py, the closed loop synthesiser -> diagnosis -> ladders on the device, and the path
ConditionSource.train_records -> diagnose_records -> ladders -> DeviceSamplePipeline(synth_ladders=...).

Condition on the seeded inputs, asserted on the restatement's values alone: no comparison of the definition lies within
1e-9 (relative) of its threshold, so no joint is left out and code, hist and per_joint are equal to the restatement; ks is
within 1e-12 relative (exp and log of the device and of libm may differ in the last bits)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests.helpers import condition_cases as ccases
from tests.helpers import error_types_cases as cases
from tests.helpers import error_types_ref as ref

pytestmark = pytest.mark.gpu
EINVAL = -1
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _tables(dataset, K):
    """The product's tables; for the generic 32-joint case a copy with the supplied pair table."""
    from buctd_amd.dataset.pose_synthesis import _Tables, make_tables
    t = make_tables(dataset, K)
    pairs = cases.pairs_of(dataset, K)
    if pairs:
        t = _Tables.from_buffer_copy(bytes(t))
        for a, b in pairs:
            t.pair[a], t.pair[b] = b, a
    return t


def _diagnose(dev, c, sl=slice(None), profile=None):
    from buctd_amd.dataset.error_diagnosis import diagnose
    K = c["joints"].shape[1]
    near = None if c["near"] is None else c["near"][sl]
    return diagnose(c["dataset"], c["joints"][sl], c["estimated"][sl], near, c["area"][sl], c["num_overlap"][sl],
                    tables=_tables(c["dataset"], K), profile=profile, device=dev)


@pytest.mark.parametrize("dataset,B,K,M", cases.SHAPES)
def test_kernel_equals_the_restatement(dev, dataset, B, K, M):
    c, want = cases.seeded(dataset, B, K, M), cases.seeded_reference(dataset, B, K, M)
    left_out = want["margin"] <= 1e-9
    assert not left_out.any()
    runs = [_diagnose(dev, c) for _ in range(2)]
    p = runs[0]
    code, ks = p.code.cpu().numpy(), p.ks.cpu().numpy()
    assert code.dtype == np.int32 and code.shape == (B, K) and ks.dtype == np.float64
    assert np.array_equal(code, want["code"])
    assert np.array_equal(p.hist.cpu().numpy(), want["hist"]) and p.hist.dtype == torch.int64
    assert np.array_equal(p.per_joint.cpu().numpy(), want["per_joint"])
    err = np.abs(ks - want["ks"])
    print(f"{dataset} B {B} K {K} M {M}: max relative ks error {float((err / np.maximum(want['ks'], 1e-300)).max()):.3e}")
    assert (err <= 1e-12 * want["ks"]).all()
    assert (ks[want["code"] < 0] == 0).all() and (ks[want["code"] == 5] == 0).all()
    for name in ("code", "ks", "hist", "per_joint"):                       # two runs are bit-identical
        assert getattr(runs[0], name).cpu().numpy().tobytes() == getattr(runs[1], name).cpu().numpy().tobytes(), name


def test_exact_ties_resolve_own_then_inversion_then_swap(dev):
    from buctd_amd.dataset.error_diagnosis import diagnose
    K = 14
    J, near = np.ones((1, K, 3)), np.ones((1, 1, K, 3))
    J[0, :, 0] = near[0, 0, :, 0] = 100.0 + 60.0 * np.arange(K)
    J[0, :, 1], near[0, 0, :, 1] = 100.0, 400.0
    near[0, 0, 0, :2] = J[0, 0, :2]                        # r0 == rS: own
    near[0, 0, 3, :2] = J[0, 3, :2]                        # joint 2 at its partner 3: rI == rS: inversion
    J[0, 5, :2] = J[0, 4, :2]                              # r0 == rI: own
    E = J.copy()
    E[0, 0, :2] += (1.5, -2.25)
    E[0, 2, :2] = J[0, 3, :2] + (0.75, 1.0)
    E[0, 4, :2] += (-2.0, 0.5)
    E[0, 1, :2] = J[0, 0, :2] + (0.5, 0.5)                 # joint 1 at its partner 0 = the neighbour's joint 0: inversion
    want = ref.error_types(ref.tables("crowdpose", K), J, E, near, [10000.0], [0])
    assert want["code"][0, :6].tolist() == [0, 2, 2, 0, 0, 0] and (want["margin"][0, [0, 1, 2, 4]] == 0).all()
    p = diagnose("crowdpose", J, E, near, [10000.0], device=dev)
    assert np.array_equal(p.code.cpu().numpy(), want["code"])
    assert np.array_equal(p.hist.cpu().numpy(), want["hist"])


def test_counters_accumulate_over_batches(dev):
    c, want = cases.seeded("crowdpose", 65, 14, 1), cases.seeded_reference("crowdpose", 65, 14, 1)
    p = _diagnose(dev, c, slice(0, 32))
    assert p.code.shape == (32, 14) and not np.array_equal(p.hist.cpu().numpy(), want["hist"])
    q = _diagnose(dev, c, slice(32, 65), profile=p)
    assert q is p and p.code.shape == (65, 14) and p.ks.shape == (65, 14)
    assert np.array_equal(p.code.cpu().numpy(), want["code"])
    assert np.array_equal(p.hist.cpu().numpy(), want["hist"])
    assert np.array_equal(p.per_joint.cpu().numpy(), want["per_joint"])


def test_c_abi_refusals_come_before_any_launch(dev):
    from buctd_amd import _C
    from buctd_amd.dataset.pose_synthesis import _Tables, make_tables
    lib, st, P = _C.lib(), _C.stream_ptr(), _C.ptr
    f64 = lambda n: torch.ones(n, dtype=torch.float64, device=dev)
    J, E, near, area = f64(2 * 33 * 3), f64(2 * 33 * 3), f64(2 * 32 * 33 * 3), f64(2)
    ov = torch.zeros(2, dtype=torch.int32, device=dev)
    code = torch.full((2 * 33,), -7, dtype=torch.int32, device=dev)
    ks = torch.full((2 * 33,), -7.0, dtype=torch.float64, device=dev)
    hist = torch.full((72,), -7, dtype=torch.int64, device=dev)
    pj = torch.full((33 * 6,), -7, dtype=torch.int64, device=dev)
    t = make_tables("fish", 5)

    def call(tables=t, B=2, K=5, M=1, **nulled):
        a = dict(J=P(J), E=P(E), near=P(near), area=P(area), ov=P(ov), code=P(code), ks=P(ks), hist=P(hist), pj=P(pj))
        a.update(nulled)
        tp = None if tables is None else C.byref(tables)
        return lib.buctd_pose_error_types(tp, a["J"], a["E"], a["near"], a["area"], a["ov"], B, K, M, a["code"], a["ks"],
                                          a["hist"], a["pj"], st)
    for kw in (dict(K=33), dict(M=32), dict(near=None), dict(K=0), dict(B=0), dict(M=-1), dict(tables=None),
               dict(J=None), dict(E=None), dict(area=None), dict(ov=None), dict(code=None), dict(ks=None), dict(hist=None),
               dict(pj=None)):
        assert call(**kw) == EINVAL, kw
        assert b"buctd_pose_error_types: bad argument (K <= 32, M <= 31)" in lib.buctd_last_error(), kw
    assert call(near=None, M=0) == 0                                        # no neighbours: a null table is fine
    torch.cuda.synchronize()
    assert bool((code[:10] != -7).all()) and bool((code[10:] == -7).all())
    code[:10], ks[:10], hist[:], pj[:30] = -7, -7.0, -7, -7
    bad = _Tables.from_buffer_copy(bytes(t))
    bad.swap_cls[4] = 3
    assert call(tables=bad) == EINVAL and b"class outside [0, 3)" in lib.buctd_last_error()
    bad = _Tables.from_buffer_copy(bytes(t))
    bad.pair[0] = 5
    assert call(tables=bad) == EINVAL and b"pair outside the pose" in lib.buctd_last_error()
    torch.cuda.synchronize()
    for out in (code, ks, hist, pj):
        assert bool((out == -7).all())                                      # nothing ran


# ---- closed loop: synthesise under a ladder, diagnose, read the ladder back ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _closed_loop(dev, ladder_key):
    from buctd_amd.dataset.error_diagnosis import diagnose
    from buctd_amd.dataset.pose_synthesis import synthesize_pose_batch
    c = cases.spread()
    lad = None if ladder_key is None else cases.LADDER
    synth = synthesize_pose_batch("crowdpose", c["joints"].copy(), c["estimated"].copy(), c["near"].copy(), c["area"].copy(),
                                  c["num_overlap"].copy(), seed=2024, device=dev, ladders=lad)
    return diagnose("crowdpose", c["joints"], synth, c["near"], c["area"], c["num_overlap"], device=dev)


def test_spread_layout_keeps_all_sources_two_d10_apart():
    c = cases.spread()
    d10 = max(math.sqrt(-2.0 * (2 * s) ** 2 * math.log(0.10)) for s in c["T"]["sigmas"])
    pts = np.concatenate([c["joints"][0, :, :2], c["near"][0, 0, :, :2], c["estimated"][0, :, :2]])
    gaps = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(2)) + np.eye(len(pts)) * 1e9
    assert c["joints"].shape == (2048, 14, 3) and gaps.min() >= 2 * d10
    assert (c["joints"][:, :, :2] == c["joints"][0, :, :2]).all() and (c["area"] == 1).all()


def test_closed_loop_recovers_a_non_default_ladder(dev):
    from buctd_amd.dataset.pose_synthesis import default_ladders
    p = _closed_loop(dev, "LADDER")
    hist = p.hist.cpu().numpy()
    assert all(default_ladders("crowdpose")[k] == cases.DEFAULT[k] != cases.LADDER[k] for k in cases.TYPES)
    # every populated cell: >= 1000 eligible joints, frequency within 5 sigma of the generating ladder
    assert cases.check_cells(hist, cases.LADDER, 1000) == 6 + 9 + 2 + 6
    # ... and the jitter cells farther than that from the default ladder
    assert cases.check_cells(hist, cases.DEFAULT, 1000, want_close=False, types=(0,)) == 6
    lad = p.ladders(default_ladders("crowdpose"), min_count=1000)
    for t, name in enumerate(cases.TYPES):
        for r in range(3):
            for k in range(3):
                if hist[t, r, k, 1]:
                    assert cases.cell(lad, t, r, k) == hist[t, r, k, 0] / hist[t, r, k, 1]
    assert lad["inv_p"][0] == 0.01 and lad["jitter_nv"] == 10             # never eligible: the base's value
    assert not (p.code.cpu().numpy() == 5).any()


def test_closed_loop_without_ladders_recovers_the_default(dev):
    hist = _closed_loop(dev, None).hist.cpu().numpy()
    assert cases.check_cells(hist, cases.DEFAULT, 1000) == 6 + 9 + 2 + 6
    assert cases.check_cells(hist, cases.LADDER, 1000, want_close=False, types=(0,)) == 6


# ---- end to end: condition records -> profile -> calibrated train batch ------------------------------------------------------
def _train_pipe(**kw):
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    from oracle import cfg as ocfg
    from oracle import core as oc
    c = ocfg.hrnet_cfg(16, 17, (64, 96), "pose_hrnet_coam", use_attention=True, colored=True, stage_modules=(1, 1, 1))
    c.DATASET.update({"DATASET": "coco", "SYNTHESIS_POSE": True, "SCALE_FACTOR": 0.35, "ROT_FACTOR": 45, "FLIP": True,
                      "NUM_JOINTS_HALF_BODY": 8, "PROB_HALF_BODY": 0.3, "BU_BBOX_MARGIN": 25})
    c.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    colors = oc.CROWDPOSE_KPT_COLORS + [[200, 200, 30], [30, 200, 200], [200, 30, 200]]
    return DeviceSamplePipeline(c, oc.COCO_FLIP_PAIRS, range(8), colors, MEAN, STD, is_train=True, seed=3, **kw)


def test_condition_records_to_a_calibrated_train_batch(dev):
    from buctd_amd.dataset.conditions import ConditionSource
    from buctd_amd.dataset.error_diagnosis import diagnose_records
    from buctd_amd.dataset.pose_synthesis import default_ladders
    K = 17
    r = ccases.reference(K)
    records = ConditionSource(ccases.cfg(K), r["annotated"], device=dev).train_records(image_dir=ccases.IMAGE_DIR,
                                                                                      model_key=ccases.MODEL_KEY)
    records = [t for t in records if "cond_joints" in t and t["cond_joints"][:, 0].any() and t["cond_joints"][:, 1].any()]
    assert len(records) > 300
    profile = diagnose_records(_train_pipe(), records, batch=128)            # three batches, one of them partial
    n = len(records)
    assert profile.code.shape == (n, K) and profile.ks.shape == (n, K) and profile.code.device.type == "cuda"
    per_joint = profile.per_joint.cpu().numpy()
    labelled = sum(int((np.asarray(t["joints_3d_vis"])[:, 0] > 0).sum()) for t in records)
    assert per_joint.sum() == labelled == int((profile.code >= 0).sum()) and labelled > 4000
    tab = profile.table()
    assert np.allclose(sum(tab.values())[per_joint.sum(1) > 0], 1.0) and 0.2 < tab["good"].mean() < 0.9
    lad = profile.ladders(default_ladders("coco"))
    assert lad != default_ladders("coco")
    # one train batch with the calibrated ladders: the default pipeline's shapes, another synthesized pose at the same seed
    sizes = {f"{ccases.IMAGE_DIR}/{im['file_name']}": (im["height"], im["width"]) for im in r["annotated"]["images"]}
    batch = [t for t in records if len(t["near_joints"]) > 0 and sizes[t["image"]] == (300, 400)][:8]
    assert len(batch) >= 3
    rng = np.random.RandomState(5)
    images = {p: torch.from_numpy(rng.randint(0, 256, (300, 400, 3)).astype(np.uint8)).to(dev) for p in {t["image"] for t in batch}}
    batch = [dict(t, image=images[t["image"]]) for t in batch]
    x0, y0, w0, m0 = _train_pipe()(batch, seed=99)
    x1, y1, w1, m1 = _train_pipe(synth_ladders=lad)(batch, seed=99)
    assert x1.shape == x0.shape and y1.shape == y0.shape and w1.shape == w0.shape and x1.dtype == x0.dtype
    assert m1["synth_joints"].shape == m0["synth_joints"].shape == (len(batch), K, 3)
    assert not torch.equal(m1["synth_joints"], m0["synth_joints"])
    x2, _, _, m2 = _train_pipe(synth_ladders=default_ladders("coco"))(batch, seed=99)
    assert torch.equal(m2["synth_joints"], m0["synth_joints"]) and torch.equal(x2, x0)
