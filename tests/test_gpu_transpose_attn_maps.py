"""Attention maps of the TransPose-H encoder on the small TransPose net (oracle recipe transpose_w16_96x64: T = 384 tokens on
a 24 x 16 grid, d = 48, one head, 2 layers): TransPoseH.attention_maps, the encoder's return_atten_map flag and the picture.

Bars.  The kernel stage (a layer's map against the fp64 soft-max of that layer's own projected q | k) has the project's
attention bar, 2e-5 relative L2.  End to end against the oracle in fp64 the maps carry the fp32 trunk in front of them;
measured on the MI355X the per-layer relative L2 is 4.3e-5 (layer 0) and 9.1e-6 (layer 1), within the 1e-3 bar
test_gpu_models.py applies to this network's heat-maps, so that bar is used."""
import copy
import math

import numpy as np
import pytest
import torch

from tests.helpers.png_read import decode_png
from tests.test_gpu_attention_heads import BAR, _e
from tests.test_gpu_models import BAR as MODEL_BAR, product_model

pytestmark = pytest.mark.gpu

NAME = "transpose_w16_96x64"


class _Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    from oracle import recipes
    c = _Case()
    c.cfg, c.omodel, x, _ = recipes.build(NAME)
    c.x = x
    c.net = product_model(c.cfg, c.omodel, dev).eval()
    c.xd = x.to(dev)
    with torch.no_grad():
        c.y_before = c.net(c.xd).clone()
    c.heatmaps, c.full, c.full_rows = c.net.attention_maps(c.xd, None)
    with torch.no_grad():
        c.y_after = c.net(c.xd).clone()
    return c


def _soft64(qk, h):
    B, T, two_d = qk.shape
    d = two_d // 2
    dh = d // h
    q = qk[..., :d].double().reshape(B, T, h, dh).permute(0, 2, 1, 3)
    k = qk[..., d:].double().reshape(B, T, h, dh).permute(0, 2, 3, 1)
    return torch.softmax(torch.matmul(q, k) / math.sqrt(dh), -1).mean(1)


def test_default_forward_is_unchanged(case):
    assert torch.equal(case.y_before, case.y_after)
    assert torch.equal(case.heatmaps, case.y_before)
    B, K, H, W = case.heatmaps.shape
    layers = case.cfg.MODEL.ENCODER_LAYERS
    assert case.full_rows is None and case.full.shape == (layers, B, H * W, H * W) and (H, W) == (24, 16)
    assert not case.net.training and all(l.self_attn.qk_sink is None for l in case.net.global_encoder.layers)
    # the mode of the network is put back
    case.net.train()
    try:
        case.net.attention_maps(case.xd, np.zeros((B, 1, 2)))
        assert case.net.training and case.net.global_encoder.layers[0].self_attn.training
    finally:
        case.net.eval()


def test_each_layer_against_fp64_of_its_own_projection(case, monkeypatch):
    from buctd_amd import ops
    seen = []
    raw = ops.attention_rows

    def spy(qk, *a, **kw):
        seen.append(qk)
        return raw(qk, *a, **kw)

    monkeypatch.setattr(ops, "attention_rows", spy)
    _, maps, _ = case.net.attention_maps(case.xd, None)
    assert len(seen) == maps.shape[0] == 2
    assert torch.equal(maps, case.full)
    for layer, qk in enumerate(seen):
        assert qk.shape == (case.xd.shape[0], 384, 96)
        err = _e(maps[layer], _soft64(qk, case.cfg.MODEL.N_HEAD))
        print("layer", layer, "kernel stage", err)
        assert err <= BAR, (layer, err)


def test_row_query_equals_rows_of_the_full_map(case, dev):
    from buctd_amd import ops
    B, K, H, W = case.heatmaps.shape
    hm, maps, rows = case.net.attention_maps(case.xd, "pred")
    assert torch.equal(hm, case.heatmaps) and maps.shape == (2, B, K, H, W) and rows.shape == (B, K) and rows.dtype == torch.int32
    preds, maxvals, _ = ops.argmax_decode(case.heatmaps)
    found = maxvals.view(B, K) > 0
    assert int(found.sum()) >= K                                       # the recipe's heat-maps have positive peaks
    want_rows = torch.where(found, (preds[..., 1] * W + preds[..., 0]).to(torch.int32), torch.full_like(rows, -1))
    assert torch.equal(rows, want_rows)
    idx = rows.clamp_min(0).long()[None, :, :, None].expand(2, -1, -1, H * W)
    assert torch.equal(maps.view(2, B, K, H * W), case.full.gather(2, idx) * found[None, :, :, None])
    # points given by hand, on the host: the same rows
    pts = preds.cpu().numpy() + 0.4
    _, maps_pts, rows_pts = case.net.attention_maps(case.xd, pts)
    assert torch.equal(rows_pts[found], rows[found]) and torch.equal(maps_pts[:, found], maps[:, found])
    # a joint whose heat-map is <= 0 everywhere: index -1, an all-zero map
    net = product_model(case.cfg, case.omodel, dev).eval()             # the same weights in a second network
    with torch.no_grad():
        net.final_layer.weight[3].zero_()
        net.final_layer.bias[3].fill_(-1.0)
    hm2, maps2, rows2 = net.attention_maps(case.xd, "pred")
    assert bool((hm2[:, 3] <= 0).all()) and rows2[:, 3].tolist() == [-1] * B
    assert bool((maps2[:, :, 3] == 0).all())
    keep = [j for j in range(K) if j != 3]
    assert torch.equal(maps2[:, :, keep], maps[:, :, keep]) and torch.equal(rows2[:, keep], rows[:, keep])


def test_encoder_flag_returns_the_stacked_maps(dev):
    from buctd_amd.models import transpose_h as T
    torch.manual_seed(3)
    layer = T.TransformerEncoderLayer(48, 2, dim_feedforward=64, dropout=0.1, return_atten_map=True)
    enc = T.TransformerEncoder(layer, 2, return_atten_map=True).to(dev).eval()
    src = torch.randn(2, 96, 48, device=dev)
    pos = torch.randn(96, 48, device=dev)
    with torch.no_grad():
        out, maps = enc(src, pos=pos)
        plain = T.TransformerEncoder(T.TransformerEncoderLayer(48, 2, dim_feedforward=64, dropout=0.1), 2).to(dev).eval()
        plain.load_state_dict(enc.state_dict())
        assert torch.equal(plain(src, pos=pos), out)
        rows = torch.tensor([[0, 95, -1], [7, 7, 96]], dtype=torch.int32, device=dev)
        out_r, maps_r = enc(src, pos=pos, rows=rows)
    assert out.shape == (2, 96, 48) and maps.shape == (2, 2, 96, 96) and maps_r.shape == (2, 2, 3, 96)
    sums = maps.double().sum(-1)
    assert _e(sums, torch.ones_like(sums)) <= BAR
    assert torch.equal(out_r, out) and torch.equal(maps_r[:, 0, 1], maps[:, 0, 95]) and bool((maps_r[:, 1, 2] == 0).all())
    enc.train()
    with pytest.raises(NotImplementedError, match="dropout"):
        enc(src, pos=pos)


def test_full_maps_against_the_oracle_in_fp64(case):
    omodel = copy.deepcopy(case.omodel).double().eval()
    got = []
    hooks = [l.self_attn.register_forward_hook(lambda mod, inp, out: got.append(out[1]))
             for l in omodel.global_encoder.layers]
    with torch.no_grad():
        y64 = omodel(case.x.double())
    for hk in hooks:
        hk.remove()
    assert len(got) == 2 and all(g is not None and g.shape == (case.x.shape[0], 384, 384) for g in got)
    assert float((case.heatmaps.cpu().double() - y64).abs().max()) <= MODEL_BAR
    for layer, ref in enumerate(got):
        err = _e(case.full[layer].cpu(), ref)
        print("layer", layer, "against the fp64 oracle", err)
        assert err <= MODEL_BAR, (layer, err)


def test_attention_picture(case, dev, tmp_path):
    from buctd_amd.utils import vis
    g = torch.Generator().manual_seed(1)
    B, K, h, w = 2, 5, 6, 4
    maps = torch.rand(B, K, h, w, generator=g) * 0.01
    maps[1, 2] = 0.0                                                   # an undetected joint
    img = torch.randn(B, 3, 4 * h, 4 * w, generator=g)
    top = maps.amax(dim=(2, 3), keepdim=True)
    normalised = maps / torch.where(top > 0, top, torch.ones_like(top))
    pic = vis.render_batch_attention_maps(img.to(dev), maps.to(dev))
    want = vis.render_batch_heatmaps(img.to(dev), normalised.to(dev))
    assert pic.dtype == torch.uint8 and pic.shape == (B * h, (K + 1) * w, 3) and torch.equal(pic, want)
    with pytest.raises(Exception, match="attention maps"):
        vis.render_batch_attention_maps(img.to(dev), maps[0].to(dev))
    path = str(tmp_path / "att.png")
    _, m, _ = case.net.attention_maps(case.xd, "pred")
    vis.save_batch_attention_maps(case.xd, m[-1], path)
    got = decode_png(path)
    Bn, Kn, H, W = case.heatmaps.shape
    assert got.shape == (Bn * H, (Kn + 1) * W, 3)
    assert np.array_equal(got, vis.render_batch_attention_maps(case.xd, m[-1]).cpu().numpy())
