"""Attention maps of the TransPose-H encoder, the parts that need no GPU: the C ABI of the rows kernel, the layer
constructors, the query -> token-row logic of TransPoseH.attention_maps and the picture function's argument checks."""
import ctypes

import numpy as np
import pytest
import torch


def test_rows_kernel_is_declared_and_resolves():
    from buctd_amd import _C
    assert "buctd_attn_rows" in _C.SIGNATURES and "buctd_attn_rows_supported" in _C.SIGNATURES
    lib = _C.lib()
    assert lib.buctd_attn_rows_supported(3072, 1, 112) == 1
    assert lib.buctd_attn_rows_supported(1, 7, 4) == 1 and lib.buctd_attn_rows_supported(70, 4, 12) == 1
    for T, h, dh in [(0, 1, 16), (64, 0, 16), (64, 1, 6), (64, 1, 132), (64, 1, 0)]:
        assert lib.buctd_attn_rows_supported(T, h, dh) == 0, (T, h, dh)
    # the Python mirror has the C struct's layout: 5 ints, 2 pointers, 2 ints, pointer, float, 2 pointers
    a = _C.AttnRowsArgs
    assert [n for n, _ in a._fields_] == ["B", "T", "h", "dh", "R", "q", "k", "ldq", "ldk", "rows", "scale", "out", "out_heads"]
    assert (a.q.offset, a.ldq.offset, a.rows.offset, a.scale.offset, a.out.offset, ctypes.sizeof(a)) == (24, 40, 48, 56, 64, 80)


def test_argument_errors_are_refused_before_any_launch():
    """null descriptor / null operands: refused with a message on a machine without a GPU - no launch is reached"""
    from buctd_amd import _C
    lib = _C.lib()
    assert lib.buctd_attn_rows(None, None) != 0 and b"null descriptor" in lib.buctd_last_error()
    a = _C.AttnRowsArgs()
    a.B, a.T, a.h, a.dh, a.R = 1, 64, 1, 16, 64
    assert lib.buctd_attn_rows(ctypes.byref(a), None) != 0 and b"null q, k or out" in lib.buctd_last_error()


def test_layer_with_attention_map_output_builds():
    from buctd_amd.models import transpose_h as T
    layer = T.TransformerEncoderLayer(32, 1, return_atten_map=True)
    assert layer.return_atten_map is True
    enc = T.TransformerEncoder(layer, 2, return_atten_map=True)
    assert enc.return_atten_map is True and all(l.return_atten_map for l in enc.layers)
    assert T.TransformerEncoderLayer(32, 1).return_atten_map is False
    assert "without attention-map output" not in (T.__doc__ or "")


@pytest.mark.parametrize("kwargs", [{"activation": "gelu"}, {"normalize_before": True},
                                    {"activation": "gelu", "return_atten_map": True}])
def test_other_layer_variants_still_raise(kwargs):
    from buctd_amd.models import transpose_h as T
    with pytest.raises(NotImplementedError, match="post-norm ReLU"):
        T.TransformerEncoderLayer(32, 1, **kwargs)


def test_maps_refuse_train_mode_with_attention_dropout():
    """refused before anything is computed (host tensors never reach a kernel here)"""
    from buctd_amd.models import transpose_h as T
    layer = T.TransformerEncoderLayer(32, 1, dropout=0.1, return_atten_map=True).train()
    x = torch.zeros(1, 4, 32)
    with pytest.raises(NotImplementedError, match="dropout"):
        layer(x)
    enc = T.TransformerEncoder(layer, 2, return_atten_map=True).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        enc(x)
    with pytest.raises(NotImplementedError, match="dropout"):
        layer.self_attn(x, x, need_map=True)


def test_query_points_become_token_rows():
    from buctd_amd.models.transpose_h import query_rows
    h, w = 24, 16
    pts = np.array([[[0.0, 0.0], [15.9, 23.9], [3.7, 2.2], [-0.5, 0.5],      # truncation towards zero, like .astype(int)
                     [16.0, 0.0], [0.0, 24.0], [-1.0, 5.0], [5.0, -1.2], [float("nan"), 1.0], [1e30, 1.0]]])
    rows = query_rows(pts, 1, h, w, torch.device("cpu"))
    assert rows.dtype == torch.int32 and rows.shape == (1, 10) and rows.is_contiguous()
    want = [0, 23 * w + 15, 2 * w + 3, 0, -1, -1, -1, -1, -1, -1]
    assert rows[0].tolist() == want
    finite = pts[:, :8]
    xy = finite.astype(int)                                                    # the reference's conversion
    inside = (xy[..., 0] >= 0) & (xy[..., 0] < w) & (xy[..., 1] >= 0) & (xy[..., 1] < h)
    assert rows[0, :8].tolist() == np.where(inside, xy[..., 1] * w + xy[..., 0], -1)[0].tolist()
    # integer points and torch tensors are taken as they are
    assert query_rows(torch.tensor([[[3, 2]], [[16, 2]]]), 2, h, w, torch.device("cpu")).tolist() == [[2 * w + 3], [-1]]
    assert query_rows(torch.tensor([[[3.9, 2.9]]], dtype=torch.float64), 1, h, w, torch.device("cpu")).tolist() == [[2 * w + 3]]


@pytest.mark.parametrize("bad", [np.zeros((2, 3)), np.zeros((1, 3, 2)), np.zeros((2, 3, 3)), np.zeros((2, 0, 2)),
                                 np.zeros((2, 3, 2), dtype=bool)])
def test_query_points_of_the_wrong_shape_are_refused(bad):
    from buctd_amd.models.transpose_h import query_rows
    with pytest.raises(ValueError, match="query points"):
        query_rows(bad, 2, 24, 16, torch.device("cpu"))


def test_attention_rows_refuses_operands_that_require_grad():
    from buctd_amd import _C, ops
    qk = torch.zeros(1, 4, 32, requires_grad=True)
    with pytest.raises(_C.BuctdHipError, match="no backward"):
        ops.attention_rows(qk)
    # operand errors name this op
    with pytest.raises(_C.BuctdHipError, match="attention_rows q: fp32 expected"):
        ops.attention_rows(torch.zeros(1, 4, 32, dtype=torch.float16))
    with pytest.raises(_C.BuctdHipError, match="attention_rows: q and k must have the same"):
        ops.attention_rows(torch.zeros(1, 4, 32), k=torch.zeros(1, 5, 32))


def test_attention_picture_refuses_host_tensors():
    from buctd_amd import _C
    from buctd_amd.utils import vis
    img = torch.zeros(2, 3, 16, 16)
    maps = torch.zeros(2, 5, 4, 4)
    with pytest.raises(_C.BuctdHipError, match="ROCm device"):
        vis.render_batch_attention_maps(img, maps)
    with pytest.raises(_C.BuctdHipError, match="batch image"):
        vis.render_batch_attention_maps(img.numpy(), maps)
