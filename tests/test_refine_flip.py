"""utils.transforms.mirror_condition - the numpy statement of buctd_cond_mirror, the condition coordinates of the mirrored
half of a flip-test input - against the oracle's fliplr_joints followed by the renderer's .astype(int)."""
import numpy as np
import pytest

from refine_flip_cases import MIRROR_CASES, mirror_case, oracle_mirror, pairs_for


@pytest.mark.parametrize("K,width,which", MIRROR_CASES)
def test_mirror_condition_matches_the_oracle(K, width, which):
    from buctd_amd.utils.transforms import mirror_condition
    pairs = pairs_for(K, which)
    cj, vis = mirror_case(K, width)
    keep = cj.copy(), vis.copy()
    got = mirror_condition(cj, vis, width, pairs)
    assert got.dtype == np.float32 and got.shape == (2, K, 2)
    assert np.array_equal(cj, keep[0]) and np.array_equal(vis, keep[1]), "the arguments are not written"
    assert np.array_equal(got, oracle_mirror(cj, vis, width, pairs))
    # every pass after the first: all visible, the [B, K, 2] coordinates buctd_refine_step leaves
    got = mirror_condition(cj[:, :, :2], None, width, pairs)
    assert np.array_equal(got, oracle_mirror(cj, None, width, pairs))


def test_the_cases_hold_what_they_are_meant_to():
    cj, vis = mirror_case(14, 64)
    m = oracle_mirror(cj, np.ones_like(vis), 64, [])
    assert m[0, 1, 0] == 0 and 64 - 1 - cj[0, 1, 0] < 0, "trunc(-0.4) is 0"
    assert m[0, 2, 0] < -1 and m[0, 3, 0] > 64
    assert (cj[:, 0, 0] < 31.5).any() and (cj[:, 0, 0] > 31.5).any()
    assert (vis[:, :, 0] == 0).any() and (vis[:, :, 0] == 1).any()
    # the mirror of the truncated coordinate is another number
    x = cj[0, 0, 0]
    assert np.trunc(64 - 1 - x) != 64 - 1 - np.trunc(x)
    # an invisible joint lands on (0, 0), and its partner's coordinates come with the partner's visibility
    from oracle import core as oc
    from buctd_amd.utils.transforms import mirror_condition
    got = mirror_condition(cj, vis, 64, oc.CROWDPOSE_FLIP_PAIRS)
    assert vis[1, 0, 0] == 0 and np.array_equal(got[1, 1], [0, 0])


def test_truncation_toward_zero_and_the_partner_exchange_by_hand():
    from buctd_amd.utils.transforms import mirror_condition
    cj = np.array([[[10.25, 5.75, 0], [63.6, -0.5, 0], [70.0, 20.0, 0]]])
    vis = np.array([[[1, 1, 0], [1, 1, 0], [0, 0, 0]]], dtype=np.float64)
    # width 64: x' = 52.75, -0.6, -7 -> rows 0 and 1 exchanged, row 2 invisible
    assert np.array_equal(mirror_condition(cj, vis, 64, [[0, 1]]), [[[0, 0], [52, 5], [0, 0]]])
    assert np.array_equal(mirror_condition(cj, None, 64, [[0, 1]]), [[[0, 0], [52, 5], [-7, 20]]])
    assert np.array_equal(mirror_condition(cj, None, 65, []), [[[53, 5], [0, 0], [-6, 20]]])
