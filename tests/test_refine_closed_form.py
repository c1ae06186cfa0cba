"""utils.transforms.crop_affine_closed_form - the specification of the crop affine inside buctd_refine_step - against
get_affine_transform's 3-point solve, and the seeded fixtures of tests/test_gpu_refine_step.py checked where no GPU is
needed: the joints left out of the truncation comparison and the joints that sit at exactly 0."""
import numpy as np
import pytest

from refine_cases import TRUNC_CAP, kernel_case, near_integer


def _boxes(n=200, seed=5):
    """center, scale (float32) of n boxes in a 640 x 480 image: scales 0.1 .. 5, centres inside the image and - every
    fourth - on its border; the scale pair comes from xywh2cs, half the boxes from either aspect branch."""
    from buctd_amd.dataset.pipeline import xywh2cs
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        s0 = np.float32(0.1 * 50.0 ** rng.rand())                     # log-uniform in [0.1, 5]
        w = float(s0) * 200.0 / 1.25
        h = w / (64 / 96) * (0.3 + 0.6 * rng.rand()) if i % 2 else w / (64 / 96)     # w > a * h: the scale follows w
        if i % 2 == 0:
            w *= 0.3 + 0.6 * rng.rand()                               # w < a * h: the scale follows h
        _, s = xywh2cs(0.0, 0.0, w, h, 64 / 96, 1.25)
        c = np.array([rng.rand() * 640, rng.rand() * 480], dtype=np.float32)
        if i % 4 == 0:
            c[i // 4 % 4 // 2] = [0.0, 640.0, 0.0, 480.0][i // 4 % 4]
        out.append((c, s))
    return out


def test_boxes_cover_what_they_should():
    boxes = _boxes()
    s0 = np.array([s[0] for _, s in boxes])
    assert len(boxes) == 200 and s0.min() < 0.15 and s0.max() > 4.0 and s0.min() >= 0.099 and s0.max() <= 5.01
    ratio = np.array([s[0] / s[1] for _, s in boxes])
    assert np.allclose(ratio, 64 / 96, rtol=1e-6)                      # xywh2cs: both branches end at the aspect ratio
    assert sum(c[0] in (0.0, 640.0) or c[1] in (0.0, 480.0) for c, _ in boxes) == 50


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("size", [(64, 96), (16, 24), (192, 256), (48, 64)])
def test_closed_form_matches_the_solve(size, inv):
    from buctd_amd.utils.transforms import crop_affine_closed_form, get_affine_transform
    worst = 0.0
    for c, s in _boxes():
        ref = get_affine_transform(c, s, 0, list(size), inv=inv)
        got = crop_affine_closed_form(c, s, list(size), inv=inv)
        assert got.shape == (2, 3) and got.dtype == np.float64
        worst = max(worst, float(np.abs(got - ref).max()))
    print(f"size {size} inv {inv}: max |closed form - solve| = {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("K", [14, 17])
@pytest.mark.parametrize("with_offset", [False, True])
def test_kernel_fixture_on_the_host(K, with_offset):
    """What tests/test_gpu_refine_step.py relies on, from the host functions alone: the joints at exactly 0, the share of
    joints left out of the truncation comparison, both aspect branches, every border clipped, a person without score."""
    from buctd_amd.dataset.pipeline import IterativeRefiner
    case = kernel_case(K, 5, with_offset)
    exp = case["expected_from"](case["host_preds"])
    p = case["host_preds"]
    assert p[4, 2, 0] == 0.0 and p[4, 5, 1] == 0.0, "the fixture's zero joints are not exactly 0 on the host"
    assert p[4, :, 0].min() == 0.0 and p[4, :, 1].min() == 0.0
    assert exp["box"][4][0] > 0.0 and exp["box"][4][1] > 0.0, "a counted 0 would put the box's edge at 0"
    share = near_integer(exp["cond"]).mean()
    print(f"K {K} offset {with_offset}: {100 * share:.2f} % of the joints within 1e-6 of an integer")
    assert share <= TRUNC_CAP
    assert exp["branch"][0] == "wide" and exp["branch"][1] == "tall"
    x, y, w, h = exp["box"][2]
    W, H = case["sizes"][2]
    assert x == 0 and y == 0 and x + w == W and y + h == H, "person 2 is clipped at all four borders"
    score, kpt = IterativeRefiner.rescore(case["maxvals"], case["box_score"], 0.2)
    assert kpt[3] == 0.0 and score[3] == 0.0 and (kpt[[0, 1, 2, 4]] > 0).all()
    thr = np.float32(0.2)
    assert {np.nextafter(thr, np.float32(0)), thr, np.nextafter(thr, np.float32(1))} <= set(case["maxvals"][0, :, 0].tolist())
