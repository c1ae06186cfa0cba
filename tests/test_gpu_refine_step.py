"""buctd_refine_step alone against the host functions it replaces between two refinement passes - transform_preds,
IterativeRefiner.rescore, box_from_keypoints, xywh2cs, get_affine_transform, affine_transform, trunc_condition - on
identical inputs, stage by stage: the predictions from the same decode outputs, everything after them from the
kernel's own float32 predictions.  Fixtures and their CPU checks: tests/refine_cases.py, tests/test_refine_closed_form.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from refine_cases import IN_VIS_THRE, TRUNC_CAP, cfg_for, degenerate_case, kernel_case, near_integer, pipe_for

pytestmark = pytest.mark.gpu
PASSES, PASS = 2, 1          # the call writes row 1 of two history rows; row 0 must stay as it was


def _launch(case, dev, K):
    """One buctd_refine_step call on the case's inputs.  Returns the kernel's outputs as numpy arrays and the warp table
    before and after (as _WarpItem arrays)."""
    from buctd_amd.dataset.pipeline import IterativeRefiner, _WarpItem, _layout, _views, history_layout
    from buctd_amd.utils.transforms import get_affine_transform
    pipe = pipe_for(K)
    refiner = IterativeRefiner(cfg_for(K), None, pipe, on_device=True)
    B = case["coords"].shape[0]
    images = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for w, h in case["sizes"]]
    geos = [dict(flip=False, trans=get_affine_transform(c, s, 0, pipe.image_size)) for c, s in zip(case["center"], case["scale"])]
    table = pipe.warp_table(images, geos)
    before = (_WarpItem * B).from_buffer_copy(table.cpu().numpy().tobytes())
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    state = (up(case["center"]), up(case["scale"]), up(case["box_score"]), torch.full((B, K, 2), -7.0, device=dev))
    at, n = _layout(history_layout(PASSES, B, K))
    result = torch.zeros(n, dtype=torch.uint8, device=dev)
    cond64 = torch.full((B, K, 2), -7.0, dtype=torch.float64, device=dev)
    refiner.refine_step((up(case["coords"]), up(case["maxvals"]), up(case["offset"])), state, table,
                        _views(result, at), PASS, PASSES, cond_joints=cond64)
    torch.cuda.synchronize()
    got = _views(result.cpu().numpy(), at)
    got.update(new_center=state[0].cpu().numpy(), new_scale=state[1].cpu().numpy(), new_box_score=state[2].cpu().numpy(),
               cond_trunc=state[3].cpu().numpy(), cond=cond64.cpu().numpy())
    after = (_WarpItem * B).from_buffer_copy(table.cpu().numpy().tobytes())
    return got, before, after


def _check_predictions(got, case, what):
    """Equal to the host's float32 wherever the host's float64 value is not within 1e-9 (relative) of a float32 rounding
    boundary - the midpoint of two neighbouring float32 values - and within one float32 ulp elsewhere."""
    h64, h32 = case["host64"], case["host_preds"]
    dev = got["preds"][PASS][:, :, :2]
    lo, hi = np.nextafter(h32, np.float32(-np.inf)).astype(np.float64), np.nextafter(h32, np.float32(np.inf)).astype(np.float64)
    mid_lo, mid_hi = (lo + h32) / 2, (hi + h32) / 2
    near = np.minimum(np.abs(h64 - mid_lo), np.abs(h64 - mid_hi)) <= 1e-9 * np.abs(h64)
    print(f"{what}: {int(near.sum())} of {near.size} host predictions within 1e-9 of a float32 rounding boundary; "
          f"{int((dev != h32).sum())} device predictions differ from the host's float32")
    assert np.array_equal(dev[~near], h32[~near]), f"{what}: predictions differ from transform_preds(...).astype(float32)"
    assert ((dev == h32) | (dev == lo.astype(np.float32)) | (dev == hi.astype(np.float32))).all()
    assert np.array_equal(got["preds"][PASS][:, :, 2], case["maxvals"][:, :, 0])


def _check_person(got, before, after, case, exp, b, what):
    """Everything after the predictions, for person b, against the host functions fed with the kernel's predictions."""
    assert np.array_equal(got["new_center"][b], exp["center"][b]), f"{what}: center {got['new_center'][b]} != {exp['center'][b]}"
    assert np.array_equal(got["new_scale"][b], exp["scale"][b]), f"{what}: scale {got['new_scale'][b]} != {exp['scale'][b]}"
    m = np.array(after[b].m[:]).reshape(2, 3)
    em, ec = np.abs(m - exp["mats"][b]).max(), np.abs(got["cond"][b] - exp["cond"][b]).max()
    print(f"{what}: |m - get_affine_transform| = {em:.3e}, |cond - affine_transform| = {ec:.3e}")
    assert em <= 1e-9 and ec <= 1e-9
    keep = ~near_integer(exp["cond"][b])
    ref = np.trunc(exp["cond"][b]).astype(np.float32)
    assert np.array_equal(got["cond_trunc"][b][keep], ref[keep]), f"{what}: truncated condition differs"
    assert np.abs(got["cond_trunc"][b] - ref).max() <= 1.0
    for f in ("src", "H", "W", "flip", "rx", "ry", "rw", "rh"):
        assert getattr(after[b], f) == getattr(before[b], f), f"{what}: the table's {f} changed"


@pytest.mark.parametrize("with_offset", [False, True])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [14, 17])
def test_refine_step_matches_the_host_functions(dev, K, B, with_offset):
    from buctd_amd.dataset.pipeline import IterativeRefiner
    case = kernel_case(K, B, with_offset)
    got, before, after = _launch(case, dev, K)
    what = f"K {K} B {B} offset {with_offset}"
    assert not got["status"].any()
    _check_predictions(got, case, what)
    dev_preds = got["preds"][PASS][:, :, :2]
    zero = B - 1                                                     # the person with a joint at x = 0 and one at y = 0
    assert dev_preds[zero, 2, 0] == 0.0 and dev_preds[zero, 5, 1] == 0.0
    exp = case["expected_from"](dev_preds)
    share = near_integer(exp["cond"]).mean()
    assert share <= TRUNC_CAP, f"{100 * share:.2f} % of the joints are left out of the truncation comparison"
    assert exp["box"][zero][0] > 0.0 and exp["box"][zero][1] > 0.0     # the zeros are not part of the box
    for b in range(B):
        _check_person(got, before, after, case, exp, b, f"{what} person {b}")
    score, kpt = IterativeRefiner.rescore(case["maxvals"], case["box_score"], IN_VIS_THRE)
    print(f"{what}: |score - rescore| = {np.abs(got['score'][PASS] - score).max():.3e}")
    assert np.abs(got["score"][PASS] - score).max() <= 1e-5 and np.abs(got["keypoint_score"][PASS] - kpt).max() <= 1e-5
    assert np.array_equal(got["new_box_score"], got["score"][PASS])         # the next pass's box score
    if B == 5:
        assert got["score"][PASS][3] == 0.0 and got["keypoint_score"][PASS][3] == 0.0
        assert exp["branch"][:2] == ["wide", "tall"]
    # the history row of this pass holds its inputs, the other row is untouched
    assert np.array_equal(got["box_score"][PASS], case["box_score"])
    assert np.array_equal(got["center"][PASS], case["center"]) and np.array_equal(got["scale"][PASS], case["scale"])
    for k in ("preds", "score", "box_score", "keypoint_score", "center", "scale"):
        assert not got[k][0].any(), f"history row 0 of {k} was written"


@pytest.mark.parametrize("K", [14, 17])
def test_refine_step_flags_a_person_without_a_box(dev, K):
    """Person 4's image x are all exactly 0: its status is set, its center, scale, matrix and condition stay; the other
    persons come out as in test_refine_step_matches_the_host_functions."""
    case = degenerate_case(K)
    good = kernel_case(K, 5, False)
    got, before, after = _launch(case, dev, K)
    ref, _, ref_after = _launch(good, dev, K)
    assert (got["preds"][PASS][4, :, 0] == 0.0).all() and (got["preds"][PASS][4, :, 1] != 0.0).sum() == K - 1
    assert got["status"].tolist() == [0, 0, 0, 0, 1]
    assert np.array_equal(got["new_center"][4], case["center"][4]) and np.array_equal(got["new_scale"][4], case["scale"][4])
    assert after[4].m[:] == before[4].m[:]
    assert (got["cond_trunc"][4] == -7.0).all() and (got["cond"][4] == -7.0).all()
    for k in ("new_center", "new_scale", "new_box_score", "cond_trunc", "cond"):
        assert np.array_equal(got[k][:4], ref[k][:4]), k
    for k in ("preds", "score", "box_score", "keypoint_score", "center", "scale"):
        assert np.array_equal(got[k][PASS][:4], ref[k][PASS][:4]), k
    for b in range(4):
        assert after[b].m[:] == ref_after[b].m[:]
    exp = good["expected_from"](ref["preds"][PASS][:, :, :2])
    for b in range(4):
        _check_person(got, before, after, good, exp, b, f"K {K} person {b} beside the degenerate one")


def test_refine_step_refuses_bad_arguments(dev):
    from buctd_amd import _C
    a = _C.RefineArgs()
    with pytest.raises(_C.BuctdHipError, match="NULL argument"):
        _C.check(_C.lib().buctd_refine_step(C.byref(a), None), "refine_step")
