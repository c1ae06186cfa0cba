"""Generative-sampling train batches (DATASET.SYNTHESIS_POSE), host side of DeviceSamplePipeline: the area and the
neighbour table handed to the synthesis kernel against hand-written vectors of reference lib/dataset/JointsDataset.py:
204-212, the error paths (a conditional train pipeline without a condition source, a dict of conditions), the batch
seeds, and the whole-batch numpy expressions of render() against the per-sample loops they replace."""
import numpy as np
import pytest
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _pipe(synthesis, is_train=True, conditional=True, seed=0):
    from oracle import cfg as ocfg, core as oc
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    c = ocfg.hrnet_cfg(16, 14, (64, 96), "pose_hrnet_coam", use_attention=conditional, colored=True, stage_modules=(1, 1, 1))
    c.DATASET.update({"DATASET": "crowdpose", "SYNTHESIS_POSE": synthesis})
    return DeviceSamplePipeline(c, oc.CROWDPOSE_FLIP_PAIRS, range(8), oc.CROWDPOSE_KPT_COLORS, MEAN, STD,
                                is_train=is_train, seed=seed)


def _record(with_cond=False):
    joints = np.zeros((14, 3))
    joints[:, 0], joints[:, 1] = np.arange(14) * 7.0 + 20, np.arange(14) * 5.0 + 30
    rec = {"image": torch.zeros((100, 150, 3), dtype=torch.uint8), "joints_3d": joints, "joints_3d_vis": np.ones((14, 3)),
           "center": np.array([75.0, 50.0], np.float32), "scale": np.array([0.5, 0.75], np.float32)}
    if with_cond:
        rec.update(cond_joints=joints + 1.0, cond_joints_vis=np.ones((14, 3)))
    return rec


def test_area_matches_hand_written_vectors():
    from buctd_amd.dataset.pipeline import synthesis_area
    cond = np.zeros((3, 4, 3))
    # record 0: x in {10, 40, 25}, one x exactly 0 (left out); y in {5, 65}, two y exactly 0: (40 - 10) * (65 - 5)
    cond[0, :, 0], cond[0, :, 1] = [10, 0, 40, 25], [0, 5, 65, 0]
    # record 1: negative coordinates count, zeros do not: x in {-8, 12}, y in {-3.5, 0.5} -> 20 * 4
    cond[1, :, 0], cond[1, :, 1] = [-8, 12, 0, 0], [0.5, 0, -3.5, 0]
    # record 2: one non-zero x -> width 0 -> area 0
    cond[2, :, 0], cond[2, :, 1] = [0, 0, 7, 0], [1, 2, 3, 4]
    assert np.array_equal(synthesis_area(cond), [1800.0, 80.0, 0.0])
    # the reference's expression, record by record, on random poses with dropped joints
    rng = np.random.RandomState(5)
    cond = rng.rand(6, 14, 3) * 200 - 20
    cond[rng.rand(6, 14) < 0.3] = 0
    ref = []
    for cj in cond:
        xs, ys = cj[:, 0][np.nonzero(cj[:, 0])], cj[:, 1][np.nonzero(cj[:, 1])]
        ref.append((np.max(xs) - np.min(xs)) * (np.max(ys) - np.min(ys)))
    assert np.array_equal(synthesis_area(cond), np.array(ref))
    cond[2] = 0                               # np.min of nothing raises in the reference as well
    with pytest.raises(ValueError):
        synthesis_area(cond)


def test_near_joints_are_reshaped_and_padded_with_visibility_zero():
    from buctd_amd.dataset.pipeline import pad_near_joints
    K = 4
    two = np.arange(2 * K * 3, dtype=np.float64) + 1          # flat, like a record stores it: reshapes to [2, K, 3]
    one = (np.arange(K * 3, dtype=np.float64) + 100).reshape(K, 3)
    out = pad_near_joints([two, [], one], K)
    assert out.shape == (3, 2, K, 3) and out.dtype == np.float64
    assert np.array_equal(out[0], two.reshape(2, K, 3))
    assert not out[1].any()
    assert np.array_equal(out[2, 0], one) and not out[2, 1].any()
    assert np.array_equal(out[2, 1, :, 2], np.zeros(K))       # the padding's visibility column: absent for the kernel
    assert pad_near_joints([[], np.zeros((0, K, 3))], K) is None


def test_synthesis_inputs_default_the_condition_to_the_ground_truth():
    """JointsDataset.py:165-167: a record without cond_joints is perturbed around its own joints; one with a stored
    condition around that condition."""
    pipe = _pipe(True)
    a, b = _record(), _record(with_cond=True)
    b["near_joints"] = np.ones(14 * 3)
    J, E, V, near, area = pipe.synthesis_inputs([a, b])
    assert np.array_equal(J[0], a["joints_3d"]) and np.array_equal(E[0], a["joints_3d"]) and np.array_equal(V[0], a["joints_3d_vis"])
    assert np.array_equal(E[1], b["cond_joints"]) and np.array_equal(J[1], b["joints_3d"])
    assert near.shape == (2, 1, 14, 3) and not near[0].any() and near[1].all()
    assert np.array_equal(area, [(13 * 7.0) * (13 * 5.0)] * 2)
    assert E[0] is not a["joints_3d"]
    E[0][:] = -1                                              # copies: the record is left alone
    assert a["joints_3d"][0, 0] == 20.0


def test_conditional_train_pipeline_without_a_condition_source_raises():
    from buctd_amd.dataset.pipeline import NO_CONDITION
    pipe = _pipe(False)
    with pytest.raises(ValueError, match="generative sampling"):
        pipe.geometry(_record())
    with pytest.raises(ValueError) as e:
        pipe([_record()])
    assert str(e.value) == NO_CONDITION
    # a stored condition, an eval pipeline and an unconditional one are as before
    assert np.array_equal(pipe.geometry(_record(with_cond=True), (np.array([75.0, 50.0]), np.array([0.5, 0.75]), 0, False))
                          ["cond_joints_vis"], np.ones((14, 3)))
    for p in (_pipe(False, is_train=False), _pipe(False, conditional=False), _pipe(True, is_train=False)):
        g = p.geometry(_record(), (np.array([75.0, 50.0]), np.array([0.5, 0.75]), 0, False))
        assert not g["cond_joints"].any() and not g["cond_joints_vis"].any()
        assert not p.synthesizes
    assert _pipe(True).synthesizes


def test_a_dict_of_conditions_raises_under_synthesis():
    pipe = _pipe(True)
    rec = _record()
    rec["cond_joints"] = {"dekr": rec["joints_3d"] + 1}
    rec["cond_joints_vis"] = {"dekr": np.ones((14, 3))}
    with pytest.raises(ValueError, match="dict"):
        pipe([rec])


def test_batch_seeds():
    from buctd_amd.dataset.pipeline import batch_seed
    seeds = [batch_seed(0, n) for n in range(200)] + [batch_seed(1, n) for n in range(200)]
    assert len(set(seeds)) == 400 and all(0 <= s < 1 << 64 for s in seeds)
    assert batch_seed(7, 3) == batch_seed(7, 3)
    # the generator of the synthesis kernel adds seed to a multiple of the golden-ratio constant: seeds that differ by
    # such a multiple would replay each other's sequence at shifted indices
    g = 0x9E3779B97F4A7C15
    near = {(seeds[0] + k * g) & ((1 << 64) - 1) for k in range(-64, 65)}
    assert not near & set(seeds[1:])


def test_make_tables_is_cached_per_dataset_and_joint_count():
    from buctd_amd.dataset.pose_synthesis import make_tables
    assert make_tables("crowdpose", 14) is make_tables("crowdpose", 14)
    assert make_tables("coco", 17) is not make_tables("crowdpose", 14)
    assert [make_tables("coco", 17).pair[j] for j in range(5)] == [-1, 2, 1, 4, 3]


def test_vectorised_centres_and_truncation_equal_the_per_sample_loops():
    from buctd_amd.dataset.pipeline import target_centres, trunc_condition
    rng = np.random.RandomState(9)
    B, K = 6, 17
    joints = rng.rand(B, K, 3) * 160 - 40                      # negative centres included
    joints[0, :4, :2] = [[-2.0, -6.0], [-0.5, 1.999999], [2.0, 6.0], [-7.999999, 94.0]]   # on and next to the .5 boundaries
    stride = np.array([64, 96]) / np.array([16, 24])
    jt = np.zeros((B, K, 3), dtype=np.float32)
    for b in range(B):
        mu_x = (joints[b][:, 0] / stride[0] + 0.5).astype(int)
        mu_y = (joints[b][:, 1] / stride[1] + 0.5).astype(int)
        jt[b, :, 0] = np.where(mu_x < 0, mu_x - 1, mu_x) * stride[0]
        jt[b, :, 1] = np.where(mu_y < 0, mu_y - 1, mu_y) * stride[1]
    got = target_centres(joints, stride)
    assert got.dtype == np.float32 and got.tobytes() == jt.tobytes()
    assert (jt[:, :, :2] < 0).any()
    cond = rng.randn(B, K, 3) * 50
    cond[1, :3, :2] = [[-0.5, 0.5], [-1.0, 63.999999999], [1e-12, -1e-12]]
    cj = np.stack([np.trunc(cond[b][:, :2]) for b in range(B)]).astype(np.float32)
    got = trunc_condition(cond)
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and got.tobytes() == np.ascontiguousarray(cj).tobytes()
