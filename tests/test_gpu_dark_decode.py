"""The DARK decoder on the device (buctd_argmax_decode_dark, ops.dark_decode, get_final_preds(use_dark=True) on a tensor)
against the numpy path of core/inference.py, and its opt-in through validate() and IterativeRefiner."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class Cfg:
    class TEST:
        POST_PROCESS = True       # ignored by the DARK decoder


def _blob_maps(rng, n, k, hh, hw, noise=0.02):
    yy, xx = np.mgrid[0:hh, 0:hw].astype(np.float64)
    cx = rng.uniform(-2, hw + 1, (n, k, 1, 1))
    cy = rng.uniform(-2, hh + 1, (n, k, 1, 1))
    sx = rng.uniform(1.5, 3.0, (n, k, 1, 1))
    sy = rng.uniform(1.5, 3.0, (n, k, 1, 1))
    amp = rng.uniform(-0.1, 1.0, (n, k, 1, 1))
    hm = amp * np.exp(-((xx - cx) ** 2 / (2 * sx ** 2) + (yy - cy) ** 2 / (2 * sy ** 2)))
    return (hm + noise * rng.standard_normal((n, k, hh, hw))).astype(np.float32)


def _cond(hm):
    """[N,K] condition numbers of the numpy path's Hessians at the peaks; inf where no step applies."""
    from buctd_amd.core.inference import _dark_blur_host, get_max_preds
    coords, _ = get_max_preds(hm)
    n, k, hh, hw = hm.shape
    with np.errstate(all='ignore'):
        b = _dark_blur_host(hm)
        r = hm.max(axis=(2, 3)) / b.max(axis=(2, 3))
        lg = np.log(np.maximum(b * r[..., None, None], np.float32(1e-10)).astype(np.float64)).astype(np.float32)
    out = np.full((n, k), np.inf)
    for i in range(n):
        for j in range(k):
            px, py = int(coords[i, j, 0]), int(coords[i, j, 1])
            if 1 < px < hw - 2 and 1 < py < hh - 2:
                h = lg[i, j].astype(np.float64)
                dxx = 0.25 * (h[py][px + 2] - 2 * h[py][px] + h[py][px - 2])
                dxy = 0.25 * (h[py + 1][px + 1] - h[py - 1][px + 1] - h[py + 1][px - 1] + h[py - 1][px - 1])
                dyy = 0.25 * (h[py + 2][px] - 2 * h[py][px] + h[py - 2][px])
                out[i, j] = np.linalg.cond(np.array([[dxx, dxy], [dxy, dyy]]))
    return out


def _compare(dev, hm, min_share=0.0):
    """Device vs numpy on the same maps: the arg-max outputs bit-equal to buctd_argmax_decode, the offsets and the final
    coordinates within 1e-3 px wherever the numpy Hessian is well conditioned.  Returns the share of rows compared."""
    from buctd_amd import ops
    from buctd_amd.core.inference import _dark_offsets_host, get_final_preds, get_max_preds
    n, k, hh, hw = hm.shape
    x = torch.from_numpy(hm).to(dev)
    keep = x.clone()
    preds, maxvals, idx, off = ops.dark_decode(x)
    p0, m0, i0 = ops.argmax_decode(x)
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "dark_decode modified its input"
    assert torch.equal(preds, p0) and torch.equal(maxvals, m0) and torch.equal(idx, i0)
    off = off.cpu().numpy()
    coords, _ = get_max_preds(hm)
    want = _dark_offsets_host(hm, coords)
    cond = _cond(hm)
    stepped = np.isfinite(cond)
    assert np.array_equal(off[~stepped], np.zeros_like(off[~stepped]))
    good = stepped & (cond <= 1e3)
    assert np.abs(off[good] - want[good]).max(initial=0.0) <= 1e-3
    # the public entry point: a device tensor and the numpy array through get_final_preds
    rng = np.random.default_rng(n * k)
    center = rng.uniform(50, 300, (n, 2))
    scale = rng.uniform(0.5, 2.0, (n, 2))
    dp, dm = get_final_preds(Cfg, x, center, scale, use_dark=True)
    hp, hmv = get_final_preds(Cfg, hm, center, scale, use_dark=True)
    assert np.array_equal(dm, hmv)
    diff = np.abs(dp - hp).max(axis=2) / (scale[:, 0] * 200 / hw)[:, None]     # in heat-map pixels
    compared = ~stepped | good
    assert diff[compared].max() <= 1e-3, diff[compared].max()
    share = compared.mean()
    assert share >= min_share, share
    return share


@pytest.mark.parametrize("n", [1, 7, 64])
@pytest.mark.parametrize("k", [14, 17])
@pytest.mark.parametrize("hh,hw", [(96, 72), (64, 48), (13, 11), (17, 9)])
def test_device_matches_numpy_on_blob_maps(dev, n, k, hh, hw):
    rng = np.random.default_rng(1000 * n + 10 * k + hh)
    hm = _blob_maps(rng, n, k, hh, hw)
    hm[0, 0] = 0.0                                       # all-zero map
    if n > 1:
        hm[1, 0] = -0.25                                 # masked peak
        hm[1, 1, hh // 2, :] = 1.0                       # ties along a row: first index
    _compare(dev, hm)


@pytest.mark.parametrize("shape", [(8, 17, 64, 48), (8, 14, 96, 72), (16, 17, 13, 11)])
def test_device_matches_numpy_on_pure_noise(dev, shape):
    hm = np.random.default_rng(sum(shape)).uniform(0, 1, shape).astype(np.float32)
    _compare(dev, hm, min_share=0.9)


def test_device_tiny_peak_and_negative_blur(dev):
    """The hand-derived edge cases of tests/test_dark_decode.py on the device: a positive peak below 1e-10 (constant log
    neighbourhood, det = 0, no step) and a positive peak whose blurred max is negative."""
    from buctd_amd import ops
    hm = np.full((1, 2, 24, 20), -1.0, dtype=np.float32)
    hm[0, 0, 7, 6] = 1e-12
    hm[0, 1] += 0.05 * np.random.default_rng(3).standard_normal((24, 20)).astype(np.float32)
    hm[0, 1, 11, 9] = 0.01
    _, _, _, off = ops.dark_decode(torch.from_numpy(hm).to(dev))
    off = off.cpu().numpy()
    assert off[0, 0].tolist() == [0.0, 0.0]
    assert np.isfinite(off).all()
    _compare(dev, hm)


def test_oversized_map_is_refused(dev):
    from buctd_amd import _C, ops
    assert ops.DARK_MAX_PIXELS == 8000
    ok = torch.rand(1, 2, 100, 80, device=dev)           # 8000 px: the limit itself
    ops.dark_decode(ok)
    with pytest.raises(_C.BuctdHipError, match="limit"):
        ops.dark_decode(torch.rand(1, 2, 100, 81, device=dev))
    torch.cuda.synchronize()


def _hrnet(dev):
    from oracle import recipes
    from buctd_amd import models
    from buctd_amd.config import cfg as base, hrnet_extra
    c = base.clone()
    c.defrost()
    c.MODEL.NAME = "pose_hrnet"
    c.MODEL.NUM_JOINTS = 17
    c.MODEL.IMAGE_SIZE = [64, 96]
    c.MODEL.HEATMAP_SIZE = [16, 24]
    c.MODEL.SIGMA = 2
    c.MODEL.PRETRAINED = ""
    c.MODEL.CONDITIONAL_TOPDOWN = True
    c.MODEL.EXTRA = hrnet_extra(16, use_pre_net=True, modules=(1, 2, 2))
    c.DATASET.DATASET = "coco"
    c.DATASET.COLORED = True
    c.TEST.SHIFT_HEATMAP = True
    c.PRINT_FREQ = 100
    c.freeze()
    _, omodel, x, _ = recipes.build("prenet_w16_96x64")
    net = models.pose_hrnet.get_pose_net(c, is_train=False)
    net.load_state_dict(omodel.state_dict(), strict=True)
    return c, net.to(dev).eval(), x


@pytest.mark.parametrize("flip", [False, True])
def test_validate_use_dark_equals_host_decode_of_the_same_forward(dev, flip):
    from buctd_amd.core.function import validate
    from buctd_amd.core.inference import get_final_preds
    from buctd_amd.core.loss import JointsMSELoss
    from buctd_amd.utils.transforms import flip_merge_device
    c, net, x = _hrnet(dev)
    c.defrost()
    c.TEST.FLIP_TEST = flip
    c.TEST.POST_PROCESS = True
    c.freeze()

    class Dataset:
        flip_pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
        image_size = c.MODEL.IMAGE_SIZE
        kpt_colors = [[(37 * k) % 256, (91 * k) % 256, (53 * k) % 256] for k in range(17)]

        def __init__(self, n):
            self.n, self.captured = n, None

        def __len__(self):
            return self.n

        def evaluate(self, cfg, preds, output_dir, all_boxes, img_path, *a, **k):
            self.captured = preds.copy()
            return {"AP": 0.0}, 0.0

    n = x.shape[0]
    batches = []
    for i in range(2):
        g = torch.Generator().manual_seed(960 + i)
        xi = x + 0.02 * i * torch.randn(x.shape, generator=g)
        meta = {"center": torch.rand(n, 2, generator=g) * 100 + 50, "scale": torch.ones(n, 2) * 0.5,
                "score": torch.rand(n, generator=g), "annotation_id": torch.arange(n) + n * i,
                "image": [f"im_{i}_{j}.jpg" for j in range(n)],
                "cond_joints": torch.cat([torch.rand(n, 17, 2, generator=g) * 60, torch.zeros(n, 17, 1)], 2),
                "cond_joints_vis": torch.ones(n, 17, 3)}
        batches.append((xi, torch.zeros(n, 17, 24, 16), torch.ones(n, 17, 1), meta))
    outs = []
    hook = net.register_forward_hook(lambda m, a, o: outs.append((o[-1] if isinstance(o, list) else o).clone()))
    tables = {}
    try:
        for dark in (False, True):
            outs.clear()
            ds = Dataset(2 * n)
            validate(c, batches, ds, net, JointsMSELoss(True), "/tmp", "/tmp", None, use_dark=dark)
            tables[dark] = ds.captured
    finally:
        hook.remove()
    # the heat-maps validate() decoded: the hooked forwards, flip-merged as validate() merges them
    merged = []
    if flip and len(outs) == 2:              # one forward over [crops | mirrored crops] per batch
        merged = [flip_merge_device(o[:n].contiguous(), o[n:].contiguous(), Dataset.flip_pairs, True) for o in outs]
    elif flip:                               # two forwards per batch
        merged = [flip_merge_device(outs[2 * i].contiguous(), outs[2 * i + 1].contiguous(), Dataset.flip_pairs, True)
                  for i in range(2)]
    else:
        merged = outs
    assert len(merged) == 2
    rows = 0
    for i, hm in enumerate(merged):
        meta = batches[i][3]
        center, scale = meta["center"].numpy(), meta["scale"].numpy()
        got = tables[True][i * n:(i + 1) * n]
        dp, dm = get_final_preds(c, hm, center, scale, use_dark=True)             # device path, same heat-maps
        assert np.array_equal(got[:, :, :2], dp) and np.array_equal(got[:, :, 2:], dm)
        hm_np = hm.cpu().numpy()
        hp, hmv = get_final_preds(c, hm_np, center, scale, use_dark=True)        # numpy path
        assert np.array_equal(got[:, :, 2:], hmv)
        cond = _cond(hm_np)
        ok = ~np.isfinite(cond) | (cond <= 1e3)
        diff = np.abs(got[:, :, :2] - hp).max(axis=2) / (scale[:, 0] * 200 / hm_np.shape[3])[:, None]
        assert diff[ok].max() <= 1e-3
        rows += ok.sum()
    assert rows >= 0.9 * 2 * n * 17
    # DARK changed the coordinates and nothing else
    assert np.array_equal(tables[True][:, :, 2], tables[False][:, :, 2])
    assert not np.array_equal(tables[True][:, :, :2], tables[False][:, :, :2])


def test_iterative_refiner_use_dark_equals_host_decode_pass_by_pass(dev):
    from oracle import core as oc, recipes
    from buctd_amd import models
    from buctd_amd.core.inference import get_final_preds
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline, IterativeRefiner
    from oracle import sample as S
    cfg, omodel, _, _ = recipes.build("coam_w16_96x64_colored")
    cfg.DATASET.update({"BU_BBOX_MARGIN": 25, "FLIP": False})
    cfg.TEST.update({"SCALE_THRE": 1.25, "IN_VIS_THRE": 0.2})
    m = models.pose_hrnet_coam.get_pose_net(cfg, is_train=False)
    m.load_state_dict(omodel.state_dict(), strict=True)
    m = m.to(dev).eval()
    outs = []
    m.register_forward_hook(lambda mod, a, o: outs.append((o[-1] if isinstance(o, list) else o).clone()))
    pipe = DeviceSamplePipeline(cfg, oc.CROWDPOSE_FLIP_PAIRS, range(8), oc.CROWDPOSE_KPT_COLORS, MEAN, STD, is_train=False)
    rng = np.random.RandomState(21)
    recs = []
    for i in range(3):
        h, w = int(rng.randint(90, 200)), int(rng.randint(100, 260))
        joints = np.zeros((14, 3))
        joints[:, 0], joints[:, 1] = rng.rand(14) * (w - 20) + 10, rng.rand(14) * (h - 20) + 10
        x, y, bw, bh = S.box_from_keypoints(joints, 10, w, h)
        c, s = S.xywh2cs(x, y, bw, bh, 64 / 96, 1.25)
        img = torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev)
        recs.append({"image": img, "joints_3d": joints, "joints_3d_vis": np.ones((14, 3)), "cond_joints": joints.copy(),
                     "cond_joints_vis": np.ones((14, 3)), "center": c, "scale": s, "score": 0.5 + 0.1 * i,
                     "annotation_id": 100 + i})
    hist = IterativeRefiner(cfg, m, pipe, use_dark=True).run(recs, 3)
    assert len(hist) == 3 and len(outs) == 3
    moved = False
    for h, out in zip(hist, outs):
        dp, dm = get_final_preds(cfg, out, h["center"], h["scale"], use_dark=True)
        assert np.array_equal(h["preds"][:, :, :2], dp) and np.array_equal(h["preds"][:, :, 2:], dm)
        hm = out.cpu().numpy()
        hp, hmv = get_final_preds(cfg, hm, h["center"], h["scale"], use_dark=True)
        assert np.array_equal(h["preds"][:, :, 2:], hmv)
        cond = _cond(hm)
        ok = ~np.isfinite(cond) | (cond <= 1e3)
        assert ok.mean() >= 0.9
        diff = np.abs(h["preds"][:, :, :2] - hp).max(axis=2) / (h["scale"][:, 0] * 200 / hm.shape[3])[:, None]
        assert diff[ok].max() <= 1e-3
        plain, _ = get_final_preds(cfg, out, h["center"], h["scale"])
        moved |= not np.array_equal(plain, dp)
    assert moved


@pytest.mark.slow
def test_dark_decode_speed_report(dev):
    """Time per launch of the DARK kernel at 64 x 14 x 96 x 72 against the plain arg-max decode (printed; no bar)."""
    from buctd_amd import ops
    hm = torch.from_numpy(_blob_maps(np.random.default_rng(5), 64, 14, 96, 72)).to(dev)
    for f in (ops.dark_decode, ops.argmax_decode):
        for _ in range(5):
            f(hm)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(200):
            f(hm)
        b.record()
        b.synchronize()
        print(f"\n{f.__name__}: {1000 * a.elapsed_time(b) / 200:.1f} us per launch at 64x14x96x72")
