"""Pose error diagnosis, the parts that need no device: the restatement tests/helpers/error_types_ref.py on hand-placed
points and on the outputs of the synthesiser's CPU twin, ErrorProfile.ladders / table, and the `ladders` argument of
make_tables (None: byte-identical to the tables before the argument existed)."""
import hashlib
import math

import numpy as np
import pytest
import torch

from tests.helpers import error_types_cases as cases
from tests.helpers import error_types_ref as ref

# sha256 of bytes(make_tables(dataset, K)) of the commit before make_tables took ladders
PARENT_TABLES = {("coco", 17): "965d0964ddfdc15d1a0814fb8ae4772a3dae8a4ddbcc85b42b7c7bf2095429ac",
                 ("crowdpose", 14): "d697eabac05909873c3b7d003ae3265e7acc52841a6c23391f36230cd16e8ac4",
                 ("fish", 5): "6e287057ddb29d66c6fc2f34305552ff61ddbefa2049bf76cd4d88dbd6c0adc5"}


def _scene():
    """crowdpose, area 10000: joint 0 (sigma 0.079) has d85 = 9.008, d50 = 18.60.  Person at y = 100, x = 100 + 60 j;
    one neighbour at y = 400."""
    K = 14
    J, near = np.ones((1, K, 3)), np.ones((1, 1, K, 3))
    J[0, :, 0] = near[0, 0, :, 0] = 100.0 + 60.0 * np.arange(K)
    J[0, :, 1], near[0, 0, :, 1] = 100.0, 400.0
    return ref.tables("crowdpose", K), J, near, np.array([10000.0]), np.array([0])


def _run(T, J, E, near, area, ov):
    return ref.error_types(T, J, E, near, area, ov)


def test_restatement_one_point_per_code():
    T, J, near, area, ov = _scene()
    J[0, 5, 2] = 0                                         # unlabelled: not scored; joint 4 loses its inversion source
    E = J.copy()
    E[0, 0, :2] = (100.0 + 3.0, 100.0)                     # good: 3 < d85
    E[0, 1, :2] = (160.0, 100.0 + 12.0)                    # jitter: d85 <= 12 < d50
    E[0, 2, :2] = (280.0 + 2.0, 100.0)                     # inversion: at joint 3, the partner of 2
    E[0, 3, :2] = (280.0, 400.0 - 5.0)                     # swap: at the neighbour's joint 3
    E[0, 6, :2] = (460.0, 250.0)                           # miss: 150 from everything
    E[0, 7, :2] = 0.0                                      # absent
    E[0, 8, :2] = (640.0, 400.0 + 1.0)                     # swap through the neighbour's PAIRED joint (9 of 8)
    out = _run(T, J, E, near, area, ov)
    assert out["code"][0].tolist() == [0, 1, 2, 3, 0, -1, 4, 5, 3, 0, 0, 0, 0, 0]
    d = 2.0 * 10000.0 * (2 * 0.079) ** 2
    assert out["ks"][0, 0] == math.exp(-(3.0 * 3.0) / d) and out["ks"][0, 5] == 0 and out["ks"][0, 7] == 0
    assert out["per_joint"].sum() == 13 and out["per_joint"][7].tolist() == [0, 0, 0, 0, 0, 1]
    # nv = 13: jitter row 1, miss row 2, swap row 1 (not crowded).  12 scored and present joints
    h = out["hist"]
    assert h[0, 1, :, 1].sum() == 12 and h[0, 1, :, 0].sum() == 1 and h[0, 0].sum() == 0
    assert h[1, 2, :, 1].sum() == 12 and h[1, 2, T["miss_cls"][6], 0] == 1
    assert h[2, 0, :, 1].sum() == 9                       # 12 minus joints 12, 13 (no partner) and 4 (partner unlabelled)
    assert h[2, 0, T["inv_cls"][2], 0] == 1 and h[3, 1, :, 1].sum() == 12 and h[3, 1, :, 0].sum() == 2
    assert np.isinf(out["margin"][0, 5]) and np.isinf(out["margin"][0, 7]) and out["margin"][0, 0] > 1e-3


def test_restatement_beyond_d10_of_everything_is_a_miss_and_rows_follow_nv():
    T, J, near, area, _ = _scene()
    J[0, 4:, 2] = 0                                        # nv = 4: jitter row 0, miss row 0; ov = 1: crowded, swap row 0
    E = J.copy()
    E[0, 0, :2] = (5000.0, 5000.0)
    out = _run(T, J, E, near, area, np.array([1]))
    assert out["code"][0, :4].tolist() == [4, 0, 0, 0] and (out["code"][0, 4:] == -1).all()
    assert out["hist"][0, 0, :, 1].sum() == 4 and out["hist"][1, 0, :, 1].sum() == 4 and out["hist"][3, 0, :, 1].sum() == 4
    assert out["hist"][1, 0, T["miss_cls"][0], 0] == 1 and out["hist"][3, 1].sum() == 0


def test_restatement_tie_order_own_then_inversion_then_swap():
    """Sources at exactly equal coordinates: the distances are bit-equal however they are rounded."""
    T, J, near, area, ov = _scene()
    near[0, 0, 0, :2] = J[0, 0, :2]                        # the neighbour's joint 0 on the own joint 0: r0 == rS
    near[0, 0, 3, :2] = J[0, 3, :2]                        # the neighbour's joint 3 on joint 3 = the partner of 2: rI == rS
    J[0, 5, :2] = J[0, 4, :2]                              # the partner of 4 on joint 4: r0 == rI
    E = J.copy()
    E[0, 0, :2] += (1.5, -2.25)
    E[0, 2, :2] = J[0, 3, :2] + (0.75, 1.0)
    E[0, 4, :2] += (-2.0, 0.5)
    out = _run(T, J, E, near, area, ov)
    assert out["code"][0, 0] == 0 and out["code"][0, 2] == 2 and out["code"][0, 4] == 0 and out["code"][0, 5] == 0
    assert out["margin"][0, 0] == 0 and out["margin"][0, 2] == 0 and out["margin"][0, 4] == 0


def test_seeded_cases_hold_what_they_promise():
    for dataset, B, K, M in cases.SHAPES:
        c, r = cases.seeded(dataset, B, K, M), cases.seeded_reference(dataset, B, K, M)
        assert float(r["margin"].min()) > 1e-9, (dataset, B, K, M)         # no comparison near its threshold: none left out
        assert (c["joints"][:, :, 2] == 0).any()
    r = cases.seeded_reference("crowdpose", 65, 14, 1)
    c = cases.seeded("crowdpose", 65, 14, 1)
    assert set(np.unique(r["code"])) == {-1, 0, 1, 2, 3, 4, 5}
    nv = (c["joints"][:, :, 2] > 0).sum(1)
    assert {5, 6, 10, 11, 14} <= set(nv.tolist()) and set(c["num_overlap"].tolist()) == {0, 3}
    assert (r["hist"][:, :, :, 1] > 0).sum() >= 20                          # every row of every ladder is reached
    T = c["T"]
    lone = [(b, j) for b in range(65) for j in range(12) if c["joints"][b, j, 2] > 0 and c["joints"][b, T["pair"][j], 2] == 0]
    assert lone and c["near"][:, :, :, 2].min() == 0
    g = cases.seeded("fish", 4, 32, 3)
    assert g["T"]["pair"][30] == 31 and g["T"]["pair"][12] == -1


def _profile(hist, dataset="crowdpose", K=14):
    from buctd_amd.dataset.error_diagnosis import ErrorProfile
    from buctd_amd.dataset.pose_synthesis import make_tables
    return ErrorProfile(dataset, None, None, torch.as_tensor(hist), torch.zeros((K, 6), dtype=torch.int64),
                        make_tables(dataset, K))


def test_ladders_counts_to_probabilities_and_min_count_fallback():
    from buctd_amd.dataset.pose_synthesis import default_ladders, make_tables
    hist = np.zeros((4, 3, 3, 2), dtype=np.int64)
    hist[0, 0, 1] = (30, 100)                              # jitter row 0 class 1: 0.30
    hist[0, 1, 2] = (9, 99)                                # below min_count: keeps the base
    hist[1, 2, 0] = (0, 500)                               # miss row 2 class 0: 0
    hist[2, 0, 2] = (25, 1000)                             # inversion class 2: 0.025
    hist[2, 1, 2] = (1000, 1000)                           # not a row of the inversion ladder: ignored
    hist[3, 1, 1] = (7, 200)
    base = default_ladders("crowdpose")
    lad = _profile(hist).ladders(base)
    want = default_ladders("crowdpose")
    want["jitter_p"][0][1], want["miss_p"][2][0], want["inv_p"][2], want["swap_p"][1][1] = 0.30, 0.0, 0.025, 0.035
    assert lad == want and base == default_ladders("crowdpose")              # the base is left as it was
    assert _profile(hist).ladders(base, min_count=99)["jitter_p"][1][2] == 9 / 99
    assert _profile(hist).ladders(None, min_count=501)["miss_p"][2][0] == base["miss_p"][2][0]
    only_p = {k: v for k, v in base.items() if k.endswith("_p")}
    assert _profile(hist).ladders(only_p) == want                            # probabilities only: thresholds from the default
    t = make_tables("crowdpose", 14, lad)
    assert t.jitter_p[0][1] == 0.30 and t.inv_p[2] == 0.025 and t.jitter_nv == 10 and t.miss_p[0][0] == 0.15
    assert make_tables("crowdpose", 14, lad) is t and make_tables("crowdpose", 14, want) is t


def test_ladders_refuse_a_negative_p_good():
    hist = np.zeros((4, 3, 3, 2), dtype=np.int64)
    hist[0, 0, 1] = (600, 1000)                            # jitter 0.6 (class 1: joints 0-5)
    hist[1, 0, 2] = (300, 1000)                            # miss 0.3 (class 2 holds joints 2-5)
    with pytest.raises(ValueError, match=r"jitter 1, miss 2, inversion 1, swap 1.*rows \(jitter 0, miss 0, swap 0\).*> 1"):
        _profile(hist).ladders()                           # 0.6 + 0.3 + 0.03 + 0.15
    hist[0, 0, 1] = (500, 1000)
    assert _profile(hist).ladders()["jitter_p"][0][1] == 0.5      # 0.5 + 0.3 + 0.03 + 0.15 = 0.98


def test_table_is_the_fraction_of_each_code_per_joint():
    from buctd_amd.dataset.error_diagnosis import CODES
    p = _profile(np.zeros((4, 3, 3, 2), dtype=np.int64))
    p.per_joint[0] = torch.tensor([6, 2, 0, 0, 1, 1])
    tab = p.table()
    assert list(tab) == list(CODES) == ["good", "jitter", "inversion", "swap", "miss", "absent"]
    assert tab["good"][0] == 0.6 and tab["absent"][0] == 0.1 and not np.stack(list(tab.values()), 1)[1:].any()


@pytest.mark.parametrize("dataset,K", list(PARENT_TABLES))
def test_tables_without_ladders_are_byte_identical_to_before(dataset, K):
    from buctd_amd.dataset.pose_synthesis import default_ladders, make_tables
    t = make_tables(dataset, K)
    assert hashlib.sha256(bytes(t)).hexdigest() == PARENT_TABLES[(dataset, K)]
    assert make_tables(dataset, K, None) is t
    assert bytes(make_tables(dataset, K, default_ladders(dataset))) == bytes(t)
    changed = default_ladders(dataset)
    changed["jitter_p"][0][0] = 0.5
    assert bytes(make_tables(dataset, K, changed)) != bytes(t)
    for bad in ({"jitter": [[0.1] * 3] * 2}, {"jitter_p": [0.1] * 3}, {"inv_p": [0.1, 0.2, 1.5]}):
        with pytest.raises(ValueError, match="ladders"):
            make_tables(dataset, K, bad)


def test_restatement_recovers_the_ladder_from_the_cpu_twin():
    """oracle.pose_synthesis.synthesize_pose on the spread-out layout (all sources more than 2 d10 apart: every type is
    feasible), fully labelled persons without overlap: the restatement's code frequencies per cell are within
    5 sqrt(p (1 - p) / n) of the default ladder."""
    from oracle import pose_synthesis as twin
    n = 200
    c = cases.spread(groups=((14, 0, n),))
    T = c["T"]
    d10 = max(math.sqrt(-2.0 * (2 * s) ** 2 * math.log(0.10)) for s in T["sigmas"])
    pts = np.concatenate([c["joints"][0, :, :2], c["near"][0, 0, :, :2]])
    gaps = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(2)) + np.eye(len(pts)) * 1e9
    assert gaps.min() >= 2 * d10
    E = np.stack([twin.synthesize_pose("crowdpose", c["joints"][b], c["estimated"][b], c["near"][b], 1.0, 0, seed=77, person=b)
                  for b in range(n)])
    out = ref.error_types(T, c["joints"], E, c["near"], c["area"], c["num_overlap"])
    assert not (out["code"] == 5).any() and (out["code"] >= 0).all()
    assert cases.check_cells(out["hist"], cases.DEFAULT, 2 * n) == 3 + 3 + 2 + 3
    assert set(np.unique(out["code"])) == {0, 1, 2, 3, 4}
