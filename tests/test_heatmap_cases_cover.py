"""The case tables of tests/helpers/heatmap_cases.py against the code paths of csrc/loss_decode.hip and csrc/nms.hip (no
GPU): every path name of every kernel is taken by a case, the long cases reach the loop trip they exist for, the dispatch
thresholds sit between neighbouring cases, no case needs more than 200 MB - and the fp64 references reproduce the
reference's own outputs in tests/golden/core.npz and target.npz (and the oracle's restatements), which is what keeps them
honest."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import heatmap_cases as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("kernel", sorted(S.PATHS))
def test_every_path_is_taken_by_a_case(kernel):
    taken = {}
    for case in S.TABLES[kernel]:
        for name in S.path_of(kernel, case):
            assert name in S.PATHS[kernel], f"{kernel}: case {case} takes a path that PATHS does not list: {name}"
            taken.setdefault(name, case)
    print(f"\n{kernel}: {len(S.TABLES[kernel])} cases")
    for name in S.PATHS[kernel]:
        print(f"  {name:32s} {taken.get(name, '-')}")
    missing = [n for n in S.PATHS[kernel] if n not in taken]
    assert not missing, f"{kernel}: no case takes {missing}"


def test_tables_and_paths_name_the_same_kernels():
    assert sorted(S.TABLES) == sorted(S.PATHS)


@pytest.mark.parametrize("i", range(len(S.SECOND_TRIPS)))
def test_long_cases_reach_their_trip(i):
    kernel, pick, name = S.SECOND_TRIPS[i]
    cases = [c for c in S.TABLES[kernel] if pick(c)]
    assert cases, f"{kernel}: the table has no case for {name}"
    for c in cases:
        assert name in S.path_of(kernel, c), f"{kernel} {c} does not reach {name}"


def test_the_dispatch_thresholds_sit_between_neighbouring_cases():
    nk = sorted({c[0] * c[1] for c in S.MSE})
    assert 256 in nk and 257 in nk                                       # 256 / 257 partials
    assert "final:one-trip" in S.path_of("joints_mse", (16, 16, 5, "w", 1, 0.125))
    assert "final:second-trip" in S.path_of("joints_mse", (257, 1, 3, "null", 1, 1.0))
    assert S.grid_trips(4096 * 256, S.ADAM_GRID_CAP) == 1 and S.grid_trips(4096 * 256 + 1, S.ADAM_GRID_CAP) == 2
    assert S.ADAM_LONG > 4096 * 256 * 4 > 1027                            # float4 items of the Adam body
    assert "body:second-trip" not in S.path_of("adam_step", (4096 * 256 * 4, 1, 1.0, "one"))
    assert "body:second-trip" in S.path_of("adam_step", (4096 * 256 * 4 + 4, 1, 1.0, "one"))
    assert S.grid_trips(8192 * 256, S.SGD_GRID_CAP) == 1 and S.grid_trips(8192 * 256 + 1, S.SGD_GRID_CAP) == 2
    assert S.SGD_LONG > 8192 * 256 > 257
    total = S.FLIP_LONG_N * 14 * 24 * 18
    assert total > 4096 * 256 >= total - 14 * 24 * 18                     # one sample fewer would fit in one trip
    assert S.grid_trips(4096 * 256, S.FLIP_GRID_CAP) == 1 and S.grid_trips(total, S.FLIP_GRID_CAP) == 2
    assert {64, 65} <= {c[0] for c in S.NMS}                              # 64 / 65 boxes
    assert "blocks:1" in S.path_of("nms", (64, 5, "random", 0.5)) and "blocks:2-ragged" in S.path_of("nms", (65, 5, "random", 0.7))
    assert {c[0] * c[1] for c in S.ARGMAX} >= {1, 40, 100, 256, 257, 432}


def test_no_case_is_larger_than_200_mb():
    for kernel, table in S.TABLES.items():
        for case in table:
            assert S.case_bytes(kernel, case) < 200e6, f"{kernel} {case}: {S.case_bytes(kernel, case) / 1e6:.0f} MB"


def test_tie_rows_hold_their_maximum_twice_and_the_first_wins():
    for case in S.ARGMAX:
        hm, names = S.argmax_operand(case)
        idx, preds, mx, quarter = S.argmax_ref(hm, case[0], case[1])
        for r, name in enumerate(names):
            if name.startswith("tie:"):
                at = (hm[r] == hm[r].max()).nonzero().view(-1).tolist()
                assert len(at) == 2 and idx[r].item() == at[0], f"{case} row {r} ({name})"
        if case[2] == "quarter":
            elig = [S.quarter_eligible(case[0], case[1], py, px) for py, px, _, _ in S.quarter_rows(*case[:2])]
            moved = (quarter[:len(elig)] != 0).any(1).tolist()
            assert not any(m and not e for m, e in zip(moved, elig)), f"{case}: an ineligible peak was moved"
            assert (case[0] < 4 or case[1] < 4) == (not any(elig))
            assert not quarter[-1].any() and not preds[-1].any(), "the masked peak decodes to (0, 0)"


def test_condition_inputs_leave_at_most_a_thousandth_of_the_pixels_near_a_whole_number():
    frac = S.cond_band_fraction()
    print(f"\npixels of the truncate cases within the bar of a whole number: {100 * frac:.4f} %")
    assert frac <= 1e-3


def test_condition_reference_matches_the_oracle_restatement():
    """the dense-matrix blur against oracle.core's padded one (pinned to the reference by oracle/make_golden.py)"""
    from oracle import core as oc
    for case in ((33, 31, 3, 64, 3, 0, 1), (3, 9, 1, 17, 2, 1, 0), (64, 48, 1, 64, 3, 1, 1), (15, 16, 3, 17, 2, 0, 0)):
        H, W, Cc = case[:3]
        j = S.cond_operand(case)
        colors = S.cond_colors(Cc, case[3])
        ref, cnt = S.cond_ref(j, colors, case)
        for b in range(S.COND_B):
            if Cc == 3:
                want = oc.get_condition_image_colored(j[b, :, :2].numpy(), (H, W, 3), colors.numpy().tolist()).transpose(2, 0, 1)
            else:
                z = np.zeros((H, W))
                for kp in j[b, :, :2].numpy().astype(int):
                    if 0 < kp[0] < W and 0 < kp[1] < H:
                        z[kp[1] - 1][kp[0] - 1] = 255
                want = oc.generate_heatmap(z)[None]
            assert np.abs(ref[b].numpy() - want).max() <= 1e-10, f"{case} member {b}"
        assert cnt[1] == 0 and not ref[1].any()


def test_gaussian_reference_matches_the_oracle_and_the_golden():
    from oracle import core as oc
    for case in S.GAUSS:
        Hh, Wh, sx, sy, sigma = case
        joints, vis = S.gauss_operand(case)
        t, w = S.gauss_ref(joints, vis, case)
        for b in range(2):
            v3 = vis[b].view(-1, 1).repeat(1, 3).numpy()
            sg = int(sigma) if sigma == int(sigma) else sigma
            to, wo = oc.generate_target(joints[b].numpy(), v3, vis.shape[1], (Wh, Hh), (Wh * sx, Hh * sy), sg)
            assert np.array_equal(w[b].numpy(), wo[:, 0]), f"{case}: weights"
            assert np.abs(t[b].numpy() - to).max() <= 1e-7, f"{case}: target (the oracle's is fp32)"
    g = np.load(os.path.join(GOLD, "target.npz"))
    for tag in ("crowdpose", "coco256"):
        hw0, hw1, iw0, iw1, sig, k = (int(v) for v in g[f"{tag}_meta"])
        joints = torch.from_numpy(g[f"{tag}_joints"]).float()[None]
        vis = torch.from_numpy(g[f"{tag}_vis"][:, 0].copy())[None]
        t, w = S.gauss_ref(joints, vis, (hw1, hw0, iw0 / hw0, iw1 / hw1, float(sig)))
        assert np.array_equal(w[0].numpy()[:, None], g[f"{tag}_weight"])
        assert np.abs(t[0].numpy() - g[f"{tag}_target"]).max() <= 6e-8      # the golden is fp32: one rounding of values <= 1


def test_references_reproduce_the_core_golden():
    core = np.load(os.path.join(GOLD, "core.npz"))
    pred, gt, wt = (torch.from_numpy(core[k]) for k in ("pred", "gt", "wt"))
    N, K = pred.shape[:2]
    loss, grad = S.mse_ref(pred.view(N, K, -1), gt.view(N, K, -1), wt.view(N, K), 1.0)
    assert abs(loss.item() - float(core["loss"])) <= 2e-7 * float(core["loss"])       # the golden is an fp32 sum
    assert np.abs(grad.view(pred.shape).numpy() - core["loss_grad"]).max() <= 1e-9
    hm = torch.from_numpy(core["hm"])
    H, W = hm.shape[2:]
    idx, preds, mx, quarter = S.argmax_ref(hm.view(N * K, -1), H, W)
    assert np.array_equal(preds.view(N, K, 2).numpy(), core["preds"]) and np.array_equal(mx.view(N, K, 1).numpy(), core["maxvals"])
    # the quarter offsets: get_final_preds(POST_PROCESS) = transform_preds(coords + quarter)
    from oracle import core as oc
    coords = (preds + quarter).view(N, K, 2).numpy()
    final = np.stack([oc.transform_preds(coords[i], core["center"][i], core["scale"][i], [W, H]) for i in range(N)])
    assert quarter.abs().max().item() == 0.25 and np.abs(final - core["final_preds"]).max() <= 1e-4
    perm = S.flip_perm(K, "swapped")
    fb = S.flip_ref(torch.zeros_like(hm), hm, perm, 0) * 2.0
    assert np.array_equal(fb.numpy(), core["flip_back"])
    merged = S.flip_ref(hm, torch.from_numpy(core["hm"][::-1].copy()), perm, 1)
    assert np.abs(merged.numpy() - core["merged"]).max() <= 1e-7


def test_nms_reference_cases():
    from oracle import nms as on
    for case in S.NMS:
        n, dim, kind, thresh = case
        boxes = S.nms_boxes(case)
        keep = S.nms_ref(boxes, thresh)
        if kind == "disjoint":
            assert keep == list(range(n))
        if kind == "identical":
            assert keep == [0]
        if kind == "chain":
            for A, B, C in S.nms_chains(n):
                assert A in keep and B not in keep and C in keep, f"{case}: chain {A, B, C}"
                assert S.nms_ref(boxes[[B, C]], thresh) == [0], "B alone would have killed C"
        if kind == "threshold":
            assert 2 in keep and 4 in keep and 6 not in keep and (n < 65 or 64 in keep)      # IoU exactly 1/2 survives, 6/10 does not
        if dim == 5:
            assert [int(i) for i in on.nms(boxes.numpy(), S.f32(thresh))] == keep, f"{case}: the oracle's float64 nms"


def test_adam_and_sgd_references_follow_torch_optim():
    p, m, v, grads = S.adam_operand((1023, 1, 1.0, "three"))
    q = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=S.f32(1e-3), betas=(S.f32(0.9), S.f32(0.999)), eps=S.f32(1e-8))
    for k, g in enumerate(grads):
        q.grad = g.double()
        opt.step()
        p, m, v = S.adam_ref(p, g, m, v, 1 + k, 1.0, torch.float64)
    assert (p - q.detach()).abs().max().item() <= 1e-12
    for form in S.SGD_FORMS[1:]:
        mu, nesterov, wd, first, gscale = form
        p, g, buf = S.sgd_operand((257,) + form + (0,))
        q = p.double().clone().requires_grad_(True)
        opt = torch.optim.SGD([q], lr=S.f32(S.SGD_LR), momentum=S.f32(mu), weight_decay=S.f32(wd), nesterov=bool(nesterov))
        if not first:
            opt.state[q]["momentum_buffer"] = buf.double().clone()
        q.grad = g.double() * S.f32(gscale)
        opt.step()
        p2, b2 = S.sgd_ref(p, g, buf, (257,) + form + (0,), torch.float64)
        assert (p2 - q.detach()).abs().max().item() <= 1e-12 and (b2 - opt.state[q]["momentum_buffer"]).abs().max().item() <= 1e-12
