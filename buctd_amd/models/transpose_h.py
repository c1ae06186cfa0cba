"""BUCTD-TransPose-H on the MI355X engine - drop-in for reference lib/models/transpose_h.py
(TransformerEncoder 110-150, TransformerEncoderLayer 168-243, TransPoseH 419-714): HRNet stages 1-3 -> 1x1 reduce
-> (+16 condition channels) -> post-norm Transformer encoder with a sine, learnable or no position embedding -> 1x1 head.
Same constructor, state_dict keys (incl. self_attn.in_proj_weight / out_proj) and init; tokens are kept
batch-major [B, T, d] (the flattened NHWC tensor) instead of the reference's [T, B, d] - same math, no transposes.
Attention maps (return_atten_map, and TransPoseH.attention_maps for the dependency areas of chosen tokens) come from
ops.attention_rows: rows of the soft-max matrix computed from the projected q | k, beside the unchanged attention output.
"""
import copy
import math

import torch

from .. import nn
from .. import ops
from .. import ops_seq
from .hrnet_common import HRNetTrunk, init_weights_hrnet, to_device_input


class MultiheadAttention(nn.Module):
    """Parameter container with nn.MultiheadAttention's names (in_proj_weight, in_proj_bias, out_proj.*)."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        torch.nn.init.xavier_uniform_(self.in_proj_weight)
        torch.nn.init.constant_(self.in_proj_bias, 0.0)
        torch.nn.init.constant_(self.out_proj.bias, 0.0)

    # a list while TransPoseH.attention_maps runs: every forward leaves its projected q | k [B, T, 2d] there
    qk_sink = None

    def check_map_mode(self):
        if self.training and float(self.dropout) > 0.0:
            raise NotImplementedError("attention maps are the eval-mode soft-max weights: a training-mode layer with "
                                      f"attention dropout p = {self.dropout} would return dropped-out weights; call "
                                      ".eval() or build the layer with dropout 0")

    def forward(self, qin, src, rows=None, need_map=False):
        """q = k = qin (src + pos), v = src; returns the attention output [B, T, d].  need_map: also the head-averaged
        soft-max weights of the query tokens `rows` (int32 [B, R] on the device; None: all, [B, T, T]), from the same
        projected q | k - the output itself takes the route it takes without the map."""
        if need_map:
            self.check_map_mode()
        qk, v = ops_seq.InProjection.apply(qin, src, self.in_proj_weight, self.in_proj_bias)
        if self.qk_sink is not None:
            self.qk_sink.append(qk.detach())
        p_eff = float(self.dropout) if self.training else 0.0
        needs_grad = torch.is_grad_enabled() and (qk.requires_grad or v.requires_grad)
        if p_eff == 0.0 and not needs_grad and ops.mha_fused_ok(qk.shape[1], self.embed_dim, self.num_heads):
            # inference (BASELINE config C5): flash-style fused attention, no T x T matrix in HBM
            out = ops.mha_fwd(qk, v) if self.num_heads == 1 else ops.mha_fwd(qk, v, h=self.num_heads)
        elif ops.mha_train_ok(qk.shape[1], self.embed_dim, self.num_heads):
            # training: fused in both directions - forward with in-kernel attention dropout, flash-style backward
            out = ops.FusedMHA.apply(qk, v, float(self.dropout), self.training, self.num_heads)
        else:
            # shapes the fused kernels do not take (T not a multiple of 64, head width not a multiple of 16):
            # materialised soft-max with the same counter-hash dropout
            out = ops.PositionAttention.apply(qk, None, v, self.num_heads, float(self.dropout), self.training)
        if need_map:
            return self.out_proj(out), ops.attention_rows(qk.detach(), rows, self.num_heads)
        return self.out_proj(out)


class TransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu", normalize_before=False,
                 return_atten_map=False):
        super().__init__()
        if activation != "relu" or normalize_before:
            raise NotImplementedError("TransPoseH builds post-norm ReLU layers")
        self.return_atten_map = return_atten_map
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = torch.nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = torch.nn.LayerNorm(d_model)
        self.norm2 = torch.nn.LayerNorm(d_model)
        self.dropout1 = torch.nn.Dropout(dropout)
        self.dropout2 = torch.nn.Dropout(dropout)

    def forward(self, src, pos=None, rows=None):
        """return_atten_map: -> (src, att_map [B, R, T]) with the rows of the query tokens `rows` (None: [B, T, T])"""
        qin = src if pos is None else ops_seq.add_pos(src, pos)
        att_map = None
        if self.return_atten_map:
            src2, att_map = self.self_attn(qin, src, rows=rows, need_map=True)
        else:
            src2 = self.self_attn(qin, src)
        src2 = ops_seq.Dropout.apply(src2, float(self.dropout1.p), self.training)
        src = ops_seq.AddLayerNorm.apply(src, src2, self.norm1, ops.grad_anchor(self.norm1.parameters()))
        ff = self.linear1(src, relu=True)
        ff = ops_seq.Dropout.apply(ff, float(self.dropout.p), self.training)
        ff = self.linear2(ff)
        ff = ops_seq.Dropout.apply(ff, float(self.dropout2.p), self.training)
        src = ops_seq.AddLayerNorm.apply(src, ff, self.norm2, ops.grad_anchor(self.norm2.parameters()))
        return (src, att_map) if self.return_atten_map else src


class TransformerEncoder(nn.Module):
    def __init__(self, encoder_layer, num_layers, norm=None, pe_only_at_begin=False, return_atten_map=False):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm
        self.pe_only_at_begin = pe_only_at_begin
        self.return_atten_map = return_atten_map
        for p in self.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)

    def forward(self, src, pos=None, rows=None):
        """return_atten_map: -> (out, maps [layers, B, R, T]); rows=None is the reference's [layers, B, T, T]"""
        maps = []
        ops_seq.AddPos.begin(pos)       # a learnable embedding counts its uses per forward pass (once-per-backward gradient)
        for layer in self.layers:
            if self.return_atten_map:
                # as in the reference, the layers are built with the flag too and return (src, att_map)
                src, att_map = layer(src, pos=pos, rows=rows)
                maps.append(att_map)
            else:
                src = layer(src, pos=pos)
            pos = None if self.pe_only_at_begin else pos
        if self.norm is not None:
            raise NotImplementedError("TransPoseH never sets a final encoder norm")
        return (src, torch.stack(maps)) if self.return_atten_map else src


def query_rows(query, batch, h_tok, w_tok, device):
    """(x, y) points in heat-map pixels [B, Q, 2], host or device -> int32 [B, Q] token indices y * w_tok + x on `device`;
    coordinates are truncated towards zero (the reference's .astype(int)), a point outside the grid becomes -1."""
    pts = torch.as_tensor(query)
    if pts.dim() != 3 or pts.shape[0] != batch or pts.shape[2] != 2 or pts.shape[1] < 1:
        raise ValueError(f"attention_maps: query points must be [B = {batch}, Q >= 1, 2] (x, y), got {tuple(pts.shape)}")
    if pts.dtype == torch.bool or pts.is_complex():
        raise ValueError(f"attention_maps: query points must be numbers, got {pts.dtype}")
    pts = pts.detach().to(device)
    if pts.is_floating_point():
        # NaN compares false everywhere below; the clamp keeps huge values inside int64 (and outside every grid)
        xy = pts.double().clamp(-2.0 ** 40, 2.0 ** 40).trunc()
        x, y = xy[..., 0], xy[..., 1]
    else:
        x, y = pts[..., 0].to(torch.int64), pts[..., 1].to(torch.int64)
    inside = (x >= 0) & (x < w_tok) & (y >= 0) & (y < h_tok)
    x, y = (torch.where(inside, v, torch.zeros_like(v)).to(torch.int64) for v in (x, y))
    return torch.where(inside, y * w_tok + x, torch.full_like(x, -1)).to(torch.int32).contiguous()


class TransPoseH(HRNetTrunk):
    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.inplanes = 64
        self.cfg = cfg
        extra = cfg["MODEL"]["EXTRA"]
        pre = self.build_trunk(extra, last_stage=3)
        d_model = cfg.MODEL.DIM_MODEL
        w, h = cfg.MODEL.IMAGE_SIZE
        self.reduce = nn.Conv2d(pre[0], d_model, 1, bias=False)
        if self.cfg.MODEL.EXTRA.USE_ATTENTION:
            self.trans_cond = nn.Conv2d(3, 16, 1, bias=False)
            d_model += 16
        self._make_position_embedding(w, h, d_model, cfg.MODEL.POS_EMBEDDING)
        layer = TransformerEncoderLayer(d_model=d_model, nhead=cfg.MODEL.N_HEAD,
                                        dim_feedforward=cfg.MODEL.DIM_FEEDFORWARD, activation="relu")
        self.global_encoder = TransformerEncoder(layer, cfg.MODEL.ENCODER_LAYERS)
        k = extra["FINAL_CONV_KERNEL"]
        self.final_layer = nn.Conv2d(in_channels=d_model, out_channels=cfg["MODEL"]["NUM_JOINTS"], kernel_size=k,
                                     stride=1, padding=1 if k == 3 else 0)
        self.pretrained_layers = extra["PRETRAINED_LAYERS"]

    def _make_position_embedding(self, w, h, d_model, pe_type="sine"):
        assert pe_type in ["none", "learnable", "sine"]
        if pe_type == "none":
            self.pos_embedding = None
            return
        self.pe_h, self.pe_w = h // 4, w // 4
        length = self.pe_h * self.pe_w
        if pe_type == "learnable":
            self.pos_embedding = nn.Parameter(torch.randn(length, 1, d_model))
        else:
            self.pos_embedding = nn.Parameter(self._make_sine_position_embedding(d_model), requires_grad=False)

    def _make_sine_position_embedding(self, d_model, temperature=10000, scale=2 * math.pi):
        """2-D sine embedding: first half of the channels encodes y, second half x; sin / cos interleaved."""
        h, w = self.pe_h, self.pe_w
        half = d_model // 2
        ys = torch.arange(1, h + 1, dtype=torch.float32).view(h, 1).expand(h, w)
        xs = torch.arange(1, w + 1, dtype=torch.float32).view(1, w).expand(h, w)
        eps = 1e-6
        ys = ys / (float(h) + eps) * scale
        xs = xs / (float(w) + eps) * scale
        idx = torch.arange(half, dtype=torch.float32)
        dim_t = temperature ** (2 * (idx // 2) / half)

        def enc(v):
            p = v[:, :, None] / dim_t
            return torch.stack((p[:, :, 0::2].sin(), p[:, :, 1::2].cos()), dim=3).flatten(2)

        pos = torch.cat((enc(ys), enc(xs)), dim=2)  # [h, w, d]
        return pos.reshape(h * w, 1, -1).contiguous()  # [T, 1, d] like the reference parameter

    def forward(self, x):
        x = to_device_input(x)
        use_att = self.cfg.MODEL.EXTRA.USE_ATTENTION
        if use_att and x.shape[1] - 3 <= 0:
            raise Exception("condition is empty, please check your dataloader")
        feat = self.stem(ops.nchw_to_nhwc(x, 0, 3 if use_att else x.shape[1]))
        y = self.stage2(self.enter_stage(2, feat, first=True))
        y = self.stage3(self.enter_stage(3, y))
        t = self.reduce(y[0])
        b, h, w, c = t.shape
        if use_att:
            cond = ops.resize_bilinear_from_nchw(x, 3, 3, h, w)
            t = ops_seq.ConcatChannels.apply(t, self.trans_cond(cond))
            c = t.shape[3]
        tokens = t.view(b, h * w, c)
        pos = None if self.pos_embedding is None else self.pos_embedding.view(h * w, c)
        tokens = self.global_encoder(tokens, pos=pos)
        return ops.ToNCHW.apply(self.final_layer(tokens.view(b, h, w, c)))

    def attention_maps(self, x, query="pred"):
        """Dependency areas: which tokens the query tokens attend to, per encoder layer -> (heatmaps, maps, rows).
        query  "pred": one row per joint, at the arg-max of that joint's output heat-map (a joint whose maximum is <= 0
                       gets index -1 and an all-zero map);
               [B, Q, 2] (x, y) in heat-map pixels, host or device, truncated like the reference's .astype(int) (a point
                       outside the grid: -1);
               None:   every token - the full map.
        heatmaps is forward(x) in eval mode; maps is [layers, B, Q, h_tok, w_tok] (the token grid is the heat-map grid), or
        [layers, B, T, T] for the full map; rows the int32 [B, Q] token indices y * w_tok + x used (None for the full map).
        Runs in eval mode under no_grad: the forward keeps each layer's projected q | k ([B, T, 2d]) and the rows kernel
        runs per layer afterwards, since "pred" knows its rows only once the heat-maps exist."""
        attns = [layer.self_attn for layer in self.global_encoder.layers]
        modes = [(m, m.training) for m in self.modules()]
        sink = []
        self.eval()
        try:
            for a in attns:
                a.qk_sink = sink
            with torch.no_grad():
                heatmaps = self.forward(x)
                b, _, h, w = heatmaps.shape
                if len(sink) != len(attns) or any(qk.shape[1] != h * w for qk in sink):
                    raise RuntimeError("attention_maps: the encoder's token grid is not the heat-map grid")
                if query is None:
                    rows = None
                elif isinstance(query, str):
                    if query != "pred":
                        raise ValueError(f"attention_maps: query is 'pred', a [B, Q, 2] array or None, not {query!r}")
                    _, maxvals, idx = ops.argmax_decode(heatmaps.contiguous())
                    rows = torch.where(maxvals.view(idx.shape) > 0, idx, torch.full_like(idx, -1))
                else:
                    rows = query_rows(query, b, h, w, heatmaps.device)
                maps = torch.stack([ops.attention_rows(qk, rows, a.num_heads) for qk, a in zip(sink, attns)])
                if rows is not None:
                    maps = maps.view(len(attns), b, rows.shape[1], h, w)
        finally:
            for a in attns:
                a.qk_sink = None
            for m, was in modes:
                m.training = was
        return heatmaps, maps, rows

    def init_weights(self, pretrained="", print_load_info=False):
        init_weights_hrnet(self, pretrained)


def get_pose_net(cfg, is_train, **kwargs):
    model = TransPoseH(cfg, **kwargs)
    if is_train and cfg["MODEL"]["INIT_WEIGHTS"]:
        model.init_weights(cfg["MODEL"]["PRETRAINED"])
    return model
