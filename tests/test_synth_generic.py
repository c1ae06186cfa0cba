"""Generic pose synthesis (every DATASET.DATASET but coco / crowdpose: reference synthesize_pose_fish), host side.
The kernel's tables for such data sets; today's thresholds in the coco / crowdpose tables; the table-driven CPU twin
(tests/helpers/synth_generic_ref.py) against oracle.pose_synthesis sample by sample when it is handed the coco / crowdpose
constants; and the twin's class frequencies against what the imported reference produced on the scenes of
tests/golden/pose_synthesis_generic.npz (tests/helpers/make_synth_generic_golden.py, 1500 runs per scene).

Tolerance of the distribution check: the one of tests/test_pose_synthesis.py per joint and class - 4.5 sigma of the
difference of two binomial frequencies (250 and 1500 samples), variance floor 2e-3, plus 0.01.  At 250 samples that cannot
tell a ladder's rows apart per joint (sigma ~ 0.027 against steps of 0.05), so the same formula is also applied to the
frequencies pooled over a scene's K joints: K times the samples on both sides, and the pooled count's variance is at most
the binomial one of the pooled frequency (p (1 - p) is concave), so the bound is no tighter than 4.5 sigma."""
import numpy as np
import pytest

from tests.helpers import synth_generic_ref as G


def _mat(field, rows, cols=3):
    return [[field[r][c] for c in range(cols)] for r in range(rows)]


@pytest.mark.parametrize("dataset,K", [("fish", 7), ("marmosets", 15), ("multimouse", 12), ("anything", 1)])
def test_generic_tables(dataset, K):
    from buctd_amd.dataset.pose_synthesis import make_tables
    t = make_tables(dataset, K)
    assert make_tables(dataset, K) is t and make_tables(dataset, K + 1) is not t and make_tables("other", K) is not t
    assert list(t.pair) == [-1] * 32
    assert list(t.sigmas) == [0.1] * K + [0.0] * (32 - K)
    assert t.out_vis == 0.0
    for cls in (t.jitter_cls, t.miss_cls, t.inv_cls, t.swap_cls):
        assert list(cls) == [0] * 32
    assert _mat(t.jitter_p, 2, 1) == [[0.20], [0.15]]
    assert _mat(t.miss_p, 3, 1) == [[0.20], [0.13], [0.05]]
    assert t.inv_p[0] == 0.03
    assert _mat(t.swap_p, 2, 1) == [[0.10], [0.04]]
    assert t.jitter_nv == 4 and list(t.miss_nv) == [2, 4]
    assert list(t.crowd_nv) == [4, 5] and list(t.crowd_ov) == [1, 1]
    # the same constants as the twin's, which restates the reference on its own
    T = G.generic_tables(K)
    assert (t.jitter_nv, tuple(t.miss_nv), tuple(zip(t.crowd_nv, t.crowd_ov))) == (T["jitter_nv"], T["miss_nv"], T["crowd"])
    assert np.array_equal(np.array(t.sigmas)[:K], T["sigmas"])


def test_generic_tables_take_1_to_32_joints():
    from buctd_amd.dataset.pose_synthesis import make_tables
    assert make_tables("fish", 32).sigmas[31] == 0.1
    for k in (0, 33):
        with pytest.raises(ValueError):
            make_tables("fish", k)
    for dataset, k in (("coco", 14), ("crowdpose", 17), ("coco", 33)):
        with pytest.raises(ValueError):
            make_tables(dataset, k)


@pytest.mark.parametrize("dataset,K", [("coco", 17), ("crowdpose", 14)])
def test_coco_and_crowdpose_tables_carry_todays_thresholds(dataset, K):
    from oracle import pose_synthesis as P
    from buctd_amd.dataset.pose_synthesis import make_tables
    t = make_tables(dataset, K)
    assert t.jitter_nv == 10 and list(t.miss_nv) == [5, 10]
    assert list(t.crowd_nv) == [10, 15] and list(t.crowd_ov) == [1, 3]
    assert _mat(t.jitter_p, 2) == P.JITTER_P and _mat(t.miss_p, 3) == P.MISS_P
    assert list(t.inv_p) == P.INV_P and _mat(t.swap_p, 2) == P.SWAP_P
    assert t.out_vis == P.tables(dataset)["out_vis"]
    assert list(t.jitter_cls)[:K] == P.tables(dataset)["jitter_cls"] and list(t.swap_cls)[:K] == P.tables(dataset)["swap_cls"]


@pytest.mark.parametrize("dataset", ["coco", "crowdpose"])
def test_twin_with_coco_or_crowdpose_tables_equals_the_oracle(dataset):
    """20 seeds on the oracle's scene, 6 each on a variant with few annotated joints (5: the first row of every ladder,
    crowded by num_overlap 1) and on a crowded one with all joints (num_overlap 3: the second clause of the rule)."""
    from oracle import pose_synthesis as P
    T = G.human_tables(dataset)
    joints, est, near, area = P.make_scene(dataset, 7)
    few = joints.copy()
    few[6:, 2] = 0                                        # joint 3 is un-annotated in the scene already
    assert int((few[:, 2] > 0).sum()) == 5
    cases = [(joints, 0, s) for s in range(20)] + [(few, 1, s) for s in range(20, 26)] + [(joints, 3, s) for s in range(26, 32)]
    differs = 0
    for J, ov, seed in cases:
        ref = P.synthesize_pose(dataset, J, est, near, area, ov, seed=seed, person=seed % 3)
        got = G.synthesize_pose(T, J, est, near, area, ov, seed=seed, person=seed % 3)
        assert np.array_equal(got, ref), f"seed {seed}, num_overlap {ov}"
        differs += not np.array_equal(ref, P.synthesize_pose(dataset, J, est, near, area, 0, seed=seed, person=seed % 3))
    assert differs > 0, "num_overlap changed nothing: the crowded rows are not exercised"


@pytest.mark.parametrize("scene", range(len(G.SCENES)))
def test_twin_distribution_matches_reference_golden(scene):
    K, n_ann, ov, n_near, seed = G.SCENES[scene]
    joints, est, near, area = G.make_scene(K, n_ann, n_near, seed)
    assert int((joints[:, 2] > 0).sum()) == n_ann and near.shape == (n_near, K, 3)
    assert not joints[joints[:, 2] == 0].any() and est[:, :2].all()
    T, n = G.generic_tables(K), 250
    out = np.stack([G.synthesize_pose(T, joints, est, near, area, ov, seed=50_000 + 1000 * scene + it) for it in range(n)])
    assert not out[:, :, 2].any()
    G.check_against_golden(G.class_counts(out, joints, est, near, area), n, scene, 2e-3, 0.01)


def test_vectorised_classification_labels_hand_placed_points():
    joints, est, near, area = G.make_scene(7, 6, 2, 3)
    d50, d85 = (np.sqrt(-2 * area * 0.04 * np.log(ks)) for ks in (0.50, 0.85))
    un = int(np.nonzero(joints[:, 2] == 0)[0][0])
    pts = np.zeros((5, 7, 3))
    gt = np.where(joints[:, 2:3] != 0, joints[:, :2], est[:, :2])
    pts[0, :, :2] = gt + [0.5 * d85, 0]                       # good (the un-annotated joint: around the estimate)
    pts[1, :, :2] = gt + [0, 0.5 * (d85 + d50)]               # jitter
    pts[2, :, :2] = near[1, :, :2] + [0.1, 0]                 # on a neighbour's joint: swap, unless that is near the truth
    pts[3, :, :2] = gt + [3000.0, 0]                          # far from everything: miss
    cls = G.classify(pts, joints, est, near, area)            # pts[4]: dropped
    far = np.hypot(*(near[1, :, :2] + [0.1, 0] - gt).T) > d50
    assert cls.shape == (5, 7) and far.sum() >= 4
    assert (cls[0] == 0).all() and (cls[1] == 1).all() and (cls[2][far] == 3).all() and (cls[3] == 4).all() and (cls[4] == 5).all()
    assert joints[un, 0] == 0 and cls[0, un] == 0
    assert np.array_equal(G.class_counts(pts, joints, est, near, area).sum(1), [5] * 7)
    # an invisible neighbour joint is no swap source
    j0 = 7 // 2
    lone = np.zeros((1, 7, 3))
    lone[0, :, :2] = near[0, :, :2]
    near1 = near[:1]
    assert near1[0, j0, 2] == 0 and np.hypot(*(near1[0, j0, :2] - gt[j0])) > d50
    assert G.classify(lone, joints, est, near1, area)[0, j0] == 4
