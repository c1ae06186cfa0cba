"""Device-seed (_dseed) entries of the dropout kernels: the seed is read from device memory when the kernel runs, so a
replayed step graph can draw fresh masks (engine.StepGraph, fresh_dropout_masks=True).  With *seed == s every _dseed entry
must give what its value entry gives with seed s, bit for bit, forward and backward; buctd_dropout_seed_fill must write
exactly the seeds ops.next_seed() hands out."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567ABC          # both 32-bit halves matter (the smallqk kernels key rows and columns by one each)
U64 = (1 << 64) - 1


def _table(dev, *seeds):
    """uint64 seeds in an int64 device tensor (same bits)"""
    return torch.tensor([s - (1 << 64) if s >> 63 else s for s in seeds], dtype=torch.int64, device=dev)


def _u64(t):
    return [int(v) & U64 for v in t.cpu().tolist()]


def _stream():
    from buctd_amd._C import stream_ptr
    return stream_ptr()


@pytest.mark.parametrize("L", [96, 1000])          # one wave per row / one workgroup per row
def test_softmax_dropout_dseed_equals_value_seed(dev, L):
    from buctd_amd import ops
    g = torch.Generator().manual_seed(L)
    s = torch.randn(3, 37, L, generator=g).to(dev)
    dpd = torch.randn(3, 37, L, generator=g).to(dev)
    table = _table(dev, 5, SEED)
    seed = ops.DeviceSeed(table, 1)
    p_v, pd_v = ops.softmax_dropout_fwd(s, L, 0.7, 0.25, SEED, inplace=False)
    p_d, pd_d = ops.softmax_dropout_fwd(s, L, 0.7, 0.25, seed, inplace=False)
    assert torch.equal(p_v, p_d) and torch.equal(pd_v, pd_d)
    assert (pd_v == 0).any() and not torch.equal(pd_v, p_v)        # the mask is live
    ds_v = ops.softmax_dropout_bwd(dpd, p_v, L, 0.7, 0.25, SEED, inplace=False)
    ds_d = ops.softmax_dropout_bwd(dpd, p_v, L, 0.7, 0.25, seed, inplace=False)
    assert torch.equal(ds_v, ds_d)
    _, pd_other = ops.softmax_dropout_fwd(s, L, 0.7, 0.25, ops.DeviceSeed(table, 0), inplace=False)
    assert not torch.equal(pd_other, pd_v)                         # the slot is what is read


def test_elementwise_dropout_dseed_equals_value_seed(dev):
    from buctd_amd import ops
    x = torch.randn(5, 1234, generator=torch.Generator().manual_seed(2)).to(dev)
    table = _table(dev, SEED)
    y_v = ops.dropout(x, 0.1, SEED)
    y_d = ops.dropout(x, 0.1, ops.DeviceSeed(table, 0))
    assert torch.equal(y_v, y_d) and (y_v == 0).any()


def test_fused_mha_dseed_equals_value_seed(dev):
    import ctypes as C
    from buctd_amd import ops
    from buctd_amd._C import MhaArgs, lib, check
    B, T, d = 2, 256, 32
    g = torch.Generator().manual_seed(3)
    qk = torch.randn(B, T, 2 * d, generator=g).to(dev)
    v = torch.randn(B, T, d, generator=g).to(dev)
    dout = torch.randn(B, T, d, generator=g).to(dev)
    table = _table(dev, SEED)
    scale, p = 1.0 / math.sqrt(d), 0.1
    res = []
    for dseed in (False, True):
        fwd = lib().buctd_mha_heads_fwd_train_dseed if dseed else lib().buctd_mha_heads_fwd_train
        bwd = lib().buctd_mha_heads_bwd_dseed if dseed else lib().buctd_mha_heads_bwd
        s = table.data_ptr() if dseed else SEED
        out = torch.empty(B, T, d, device=dev)
        lse = torch.empty(B, T, device=dev)
        a = MhaArgs()                      # one head, packed: k = q + d
        a.B, a.T, a.h, a.dh = B, T, 1, d
        a.q, a.k, a.v, a.ldq, a.ldk, a.ldv = qk.data_ptr(), qk.data_ptr() + 4 * d, v.data_ptr(), 2 * d, 2 * d, d
        a.out, a.ldo, a.lse, a.scale, a.p_drop = out.data_ptr(), d, lse.data_ptr(), scale, p
        check(fwd(C.byref(a), s, _stream()), "mha_fwd_train")
        dqk = torch.empty_like(qk)
        dv = torch.empty_like(v)
        ws = ops.workspace(lib().buctd_mha_heads_bwd_workspace(B, 1, T), dev)
        a.dout, a.lddo = dout.data_ptr(), d
        a.dq, a.dk, a.dv, a.lddq, a.lddk, a.lddv = dqk.data_ptr(), dqk.data_ptr() + 4 * d, dv.data_ptr(), 2 * d, 2 * d, d
        check(bwd(C.byref(a), s, ws.data_ptr(), ws.numel(), _stream()), "mha_bwd")
        res.append((out, lse, dqk, dv))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("b3", [0, 1, 2])          # fp32 MFMA, bf16x3, bf16x6
def test_smallqk_dseed_equals_value_seed(dev, b3):
    from buctd_amd._C import lib, check
    B, T, R4, Cn = 2, 1728, 4, 48                  # the CoAM-W48 position attention (d_cond 3 -> R4 4)
    g = torch.Generator().manual_seed(4 + b3)
    q = torch.randn(B, T, R4, generator=g).to(dev)
    q[:, :, 3] = 0.0
    k = torch.randn(B, T, R4, generator=g).to(dev)
    v = torch.randn(B, T, Cn, generator=g).to(dev)
    dout = torch.randn(B, T, Cn, generator=g).to(dev)
    table = _table(dev, SEED)
    scale, p = 1.0 / math.sqrt(Cn), 0.1
    res = []
    for dseed in (False, True):
        fwd = lib().buctd_attn_smallqk_fwd_dseed if dseed else lib().buctd_attn_smallqk_fwd
        bwd = lib().buctd_attn_smallqk_bwd_dseed if dseed else lib().buctd_attn_smallqk_bwd
        s = table.data_ptr() if dseed else SEED
        out = torch.empty(B, T, Cn, device=dev)
        m = torch.empty(B, T, device=dev)
        linv = torch.empty(B, T, device=dev)
        check(fwd(B, T, R4, Cn, q.data_ptr(), k.data_ptr(), v.data_ptr(), scale, p, s, b3, out.data_ptr(), m.data_ptr(),
                  linv.data_ptr(), _stream()), "attn_smallqk_fwd")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dvec = torch.empty(B, T, device=dev)
        check(bwd(B, T, R4, Cn, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), m.data_ptr(),
                  linv.data_ptr(), scale, p, s, b3, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dvec.data_ptr(),
                  _stream()), "attn_smallqk_bwd")
        res.append((out, m, linv, dq, dk, dv))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("base,counter0", [(0x243F6A8885A308D3, 0), (U64, U64 - 2), (12345, (1 << 64) - 1)])
def test_seed_fill_equals_next_seed(dev, base, counter0):
    """table[i] is the seed of the (i + 1)-th draw after draw number counter0 - including across the 2^64 wrap of the
    counter"""
    from buctd_amd import ops
    from buctd_amd._C import lib, check
    saved = dict(ops._seed_state)
    try:
        n = 300
        table = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        check(lib().buctd_dropout_seed_fill(table.data_ptr(), n, base, counter0, _stream()), "dropout_seed_fill")
        ops.manual_seed(base)
        ops._seed_state["counter"] = counter0
        want = [ops.next_seed() for _ in range(n)]
        got = _u64(table)
        assert got[:n] == want and got[n] == 0
        # ops.fill_seed_table: the same seeds, and the host counter moves on by n
        ops.manual_seed(base)
        ops._seed_state["counter"] = counter0
        table.zero_()
        ops.fill_seed_table(table, n)
        assert ops.seeds_drawn() == counter0 + n
        assert _u64(table)[:n] == want
    finally:
        ops._seed_state.update(saved)
