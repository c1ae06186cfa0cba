"""buctd_attn_rows (attn_rows.hip) and ops.attention_rows: chosen rows of the attention matrix against the fp64 formula
softmax(scale q k^T) per head, averaged over the heads, evaluated by torch in fp64 on the device (as
test_gpu_attention_heads.py::_ref64).  Bar: the project's attention bar, 2e-5 relative L2 over each case's output.

Shapes: the smallest at which the kernel can go wrong - one key (T = 1), whole 16-key blocks with every wavefront busy (64),
a masked tail (70, 200), fewer blocks than the key split wants (96), the TransPose test net's 384; head widths that are a
multiple of 16 (48, 112, 16, 128: the exact tile), that are not (24, 12, 4: zero-padded contraction), several heads (the
read-modify-write head mean); R = 1 and 17 (two row tiles, the second nearly empty, keys split over workgroups), R = T.
Up to there a call has fewer than 128 row tiles (B ceil(R / 16) <= 72), the launcher's regime with the keys split over
grid.x where T allows; test_many_row_tiles runs the other one (132 tiles: one key chunk per workgroup) with the same checks.
There is one kernel per head width and the launcher varies the grid alone."""
import ctypes
import math

import pytest
import torch

from tests.helpers.guard_bands import Bands
from tests.test_gpu_attention_heads import BAR, _e, _operands

pytestmark = pytest.mark.gpu

TS = (1, 64, 70, 96, 200, 384)
HEADS = ((1, 48), (1, 112), (2, 24), (7, 16), (4, 12), (1, 128), (1, 4))
BATCHES = (1, 3)
ROWS = (1, 17, "full")


def _ref64(q, k, h, scale=None):
    """-> (mean over heads [B, T, T], per head [B, h, T, T]) of softmax(scale q k^T) in fp64"""
    q, k = q.detach().double(), k.detach().double()
    B, T, hd = q.shape
    dh = hd // h
    qh = q.reshape(B, T, h, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, T, h, dh).permute(0, 2, 3, 1)
    att = torch.softmax(torch.matmul(qh, kh) * (1.0 / math.sqrt(dh) if scale is None else scale), -1)
    return att.mean(1), att


def _gather(full, rows):
    """rows [B, R] of full [B, (h,) T, T]; an index outside [0, T) gives zeros"""
    T = full.shape[-1]
    valid = (rows >= 0) & (rows < T)
    idx = rows.clamp(0, T - 1).long()
    if full.dim() == 3:
        return full.gather(1, idx[:, :, None].expand(-1, -1, T)) * valid[:, :, None]
    h = full.shape[1]
    return full.gather(2, idx[:, None, :, None].expand(-1, h, -1, T)) * valid[:, None, :, None]


def _q_k(qk, k, hd):
    return (qk[..., :hd], qk[..., hd:]) if k is None else (qk, k)


def _rows(B, T, R, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, T, (B, R), generator=g, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("layout", ["packed", "views"])
@pytest.mark.parametrize("T", TS)
def test_rows_against_fp64(dev, T, layout):
    from buctd_amd import ops
    errs = []
    for h, dh in HEADS:
        for B in BATCHES:
            qk, k, _ = _operands(B, T, h, dh, layout, dev, 100 + T + 7 * h + dh + B)
            q_, k_ = _q_k(qk, k, h * dh)
            full, full_h = _ref64(q_, k_, h)
            for R in ROWS:
                rows = None if R == "full" else _rows(B, T, R, dev, T + R)
                out, heads = ops.attention_rows(qk, rows, h, k=k, per_head=True)
                want, want_h = (full, full_h) if rows is None else (_gather(full, rows), _gather(full_h, rows))
                assert out.shape == want.shape and heads.shape == want_h.shape and out.dtype == torch.float32
                assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(heads).all())
                errs.append((h, dh, B, R, _e(out, want), _e(heads, want_h)))
    assert len(errs) == len(HEADS) * len(BATCHES) * len(ROWS)          # no case is left out
    print(f"T{T} {layout}: worst", max(max(e[4], e[5]) for e in errs))
    over = [e for e in errs if not (e[4] <= BAR and e[5] <= BAR)]
    assert not over, f"T{T} {layout}: over {BAR}: {over[:8]}"


def test_large_logits_stay_finite(dev):
    """q scaled by 30: logits of a few hundred, the soft-max must subtract the row maximum"""
    from buctd_amd import ops
    B, T, h, dh = 1, 200, 2, 24
    qk, _, _ = _operands(B, T, h, dh, "packed", dev, 9)
    qk[..., :h * dh] *= 30.0
    full, full_h = _ref64(qk[..., :h * dh], qk[..., h * dh:], h)
    assert float((torch.matmul(qk[..., :dh], qk[..., h * dh:h * dh + dh].transpose(1, 2)) / math.sqrt(dh)).abs().max()) > 150
    rows = _rows(B, T, 17, dev, 3)
    for r in (rows, None):
        out, heads = ops.attention_rows(qk, r, h, per_head=True)
        want, want_h = (full, full_h) if r is None else (_gather(full, r), _gather(full_h, r))
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(heads).all())
        e, eh = _e(out, want), _e(heads, want_h)
        print("q x 30:", e, eh)
        assert e <= BAR and eh <= BAR, (e, eh)


def test_invalid_rows_are_zero_and_duplicates_identical(dev):
    from buctd_amd import ops
    B, T, h, dh = 2, 70, 2, 24
    qk, _, _ = _operands(B, T, h, dh, "packed", dev, 11)
    # 0, T-1, a duplicate pair 16 rows apart (two row tiles), -1 and T; padded to 19 rows
    base = [0, T - 1, 33, -1, T, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 33]
    rows = torch.tensor([base, base[::-1]], dtype=torch.int32, device=dev)
    out, heads = ops.attention_rows(qk, rows, h, per_head=True)
    full, full_h = _ref64(qk[..., :h * dh], qk[..., h * dh:], h)
    assert _e(out, _gather(full, rows)) <= BAR and _e(heads, _gather(full_h, rows)) <= BAR
    for b in range(B):
        r = rows[b].tolist()
        for i, tok in enumerate(r):
            if tok < 0 or tok >= T:
                assert bool((out[b, i] == 0).all()) and bool((heads[b, :, i] == 0).all()), (b, i)
            else:
                assert float(out[b, i].sum()) > 0.99
        i, j = [n for n, tok in enumerate(r) if tok == 33]
        assert torch.equal(out[b, i], out[b, j]) and torch.equal(heads[b, :, i], heads[b, :, j])
    # a row of a row query is the full map's row, bit for bit
    full_out, full_heads = ops.attention_rows(qk, None, h, per_head=True)
    assert torch.equal(out[0, 2], full_out[0, 33]) and torch.equal(heads[0, :, 1], full_heads[0, :, T - 1])


def test_head_mean_and_determinism(dev):
    from buctd_amd import ops
    B, T, h, dh = 3, 96, 7, 16
    q, k, _ = _operands(B, T, h, dh, "views", dev, 13)
    rows = _rows(B, T, 17, dev, 5)
    for r in (rows, None):
        out, heads = ops.attention_rows(q, r, h, k=k, per_head=True)
        assert _e(out, heads.double().mean(1)) <= BAR
        out2, heads2 = ops.attention_rows(q, r, h, k=k, per_head=True)
        assert torch.equal(out, out2) and torch.equal(heads, heads2)
        assert torch.equal(out, ops.attention_rows(q, r, h, k=k))      # without the per-head output


def _call(B, T, h, dh, R, q, k, ldq, ldk, rows, out, heads, scale=None):
    from buctd_amd import _C
    a = _C.AttnRowsArgs()
    a.B, a.T, a.h, a.dh, a.R = B, T, h, dh, R
    a.q, a.k, a.ldq, a.ldk = q, k, ldq, ldk
    a.rows = rows if isinstance(rows, int) else (rows.data_ptr() if rows is not None else None)
    a.scale = 1.0 / math.sqrt(max(dh, 1)) if scale is None else scale
    a.out, a.out_heads = out.data_ptr(), (heads.data_ptr() if heads is not None else None)
    rc = _C.lib().buctd_attn_rows(ctypes.byref(a), _C.stream_ptr())
    torch.cuda.synchronize()
    return rc, (_C.lib().buctd_last_error() or b"").decode()


@pytest.mark.parametrize("B,T,h,dh,R", [(2, 70, 2, 24, 17), (1, 200, 1, 112, 200), (3, 1, 4, 12, 1), (1, 96, 7, 16, 3)])
def test_outputs_stay_inside_guard_bands(dev, B, T, h, dh, R):
    qk, _, _ = _operands(B, T, h, dh, "packed", torch.device("cpu"), 17)
    bands = Bands(dev, True)
    qk_d = bands.ro(qk)                                                # NaN bands: a load next to q | k shows in the result
    rows = None if R == T else bands.ro(torch.randint(0, T, (B, R), dtype=torch.int32))
    out, heads = bands.new((B, R, T), "out"), bands.new((B, h, R, T), "out_heads")
    hd = h * dh
    rc, msg = _call(B, T, h, dh, R, qk_d.data_ptr(), qk_d.data_ptr() + 4 * hd, 2 * hd, 2 * hd, rows, out, heads)
    assert rc == 0, msg
    bands.check(f"attn_rows B{B} T{T} h{h} dh{dh} R{R}")
    full, full_h = _ref64(qk_d[..., :hd], qk_d[..., hd:], h)
    want, want_h = (full, full_h) if rows is None else (_gather(full, rows), _gather(full_h, rows))
    assert _e(out, want) <= BAR and _e(heads, want_h) <= BAR


def test_many_row_tiles(dev):
    """B ceil(R / 16) = 3 * 44 = 132 >= 128: grid.x is 1 and the row tiles fill the machine (the regime of a full map at
    T = 3072); T = 700 has a masked key tail.  fp64 parity, guard bands, and the rows of a row query (4 tiles, keys split
    over grid.x) are the full map's rows bit for bit."""
    from buctd_amd import ops
    B, T, h, dh = 3, 700, 2, 24
    hd = h * dh
    qk, _, _ = _operands(B, T, h, dh, "packed", torch.device("cpu"), 23)
    bands = Bands(dev, True)
    qk_d = bands.ro(qk)
    out, heads = bands.new((B, T, T), "out"), bands.new((B, h, T, T), "out_heads")
    rc, msg = _call(B, T, h, dh, T, qk_d.data_ptr(), qk_d.data_ptr() + 4 * hd, 2 * hd, 2 * hd, None, out, heads)
    assert rc == 0, msg
    bands.check("attn_rows full map, 132 row tiles")
    full, full_h = _ref64(qk_d[..., :hd], qk_d[..., hd:], h)
    e, eh = _e(out, full), _e(heads, full_h)
    print("132 row tiles:", e, eh)
    assert e <= BAR and eh <= BAR, (e, eh)
    assert torch.equal(out, ops.attention_rows(qk_d, None, h))         # the host op takes the same route
    rows = _rows(B, T, 17, dev, 29)
    rows[:, 0], rows[:, 1] = 0, T - 1
    out_r, heads_r = ops.attention_rows(qk_d, rows, h, per_head=True)
    idx = rows.long()
    assert torch.equal(out_r, out.gather(1, idx[:, :, None].expand(-1, -1, T)))
    assert torch.equal(heads_r, heads.gather(2, idx[:, None, :, None].expand(-1, h, -1, T)))


def test_bad_arguments_are_refused_without_a_launch(dev):
    B, T, h, dh = 1, 64, 1, 16
    big = torch.randn(B, T, 2 * 136 + 8, device=dev)
    rows = torch.zeros(B, 5, dtype=torch.int32, device=dev)
    out = torch.full((B, T, T), -7.0, device=dev)
    p = big.data_ptr()
    cases = [("rows == NULL", dict(dh=16, R=5, rows=None, q=p)),
             ("dh6", dict(dh=6, R=5, rows=rows, q=p)),
             ("dh132", dict(dh=132, R=5, rows=rows, q=p)),
             ("aligned", dict(dh=16, R=5, rows=rows, q=p + 4)),
             ("rows must be 4-byte aligned", dict(dh=16, R=5, rows=rows.data_ptr() + 2, q=p)),
             ("multiples of 4", dict(dh=16, R=5, rows=rows, q=p, ld=big.shape[2] - 2))]
    for word, c in cases:
        ld = c.get("ld", big.shape[2])
        rc, msg = _call(B, T, h, c["dh"], c["R"], c["q"], p + 4 * 136, ld, ld, c["rows"], out, None)
        assert rc != 0 and word in msg and msg.startswith("buctd_attn_rows:"), (word, rc, msg)
        assert bool((out == -7.0).all()), f"{word}: the refused call wrote to out"
