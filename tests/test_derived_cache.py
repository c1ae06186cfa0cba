"""The one cache of tensors derived from a parameter (ops._Derived: prepared 3x3 / gathered / Linear images), its batched
refresh, the rebuild counter it shares with the eval BatchNorm fold, and the BatchNorm-partials helper.  The host tests run
ops._Derived.get on CPU tensors with builders of their own; what needs a device (events, the batched kernels) is marked gpu."""
import pytest
import torch

from buctd_amd import ops


class _Builder:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.full((4,), float(self.calls))


def test_get_builds_once_per_key_and_slot():
    w, build = torch.zeros(8, 8, 3, 3), _Builder()
    a = ops._Derived.get(w, "c3", 0, build)
    assert ops._Derived.get(w, "c3", 0, build) is a and build.calls == 1
    b = ops._Derived.get(w, "c3", 1, build)
    assert b is not a and build.calls == 2
    g = ops._Derived.get(w, "gc", (2, 0), build)
    assert ops._Derived.get(w, "gc", (2, 0), build) is g and build.calls == 3
    assert ops._Derived.get(w, "gc", (2, 1), build) is not g and build.calls == 4
    assert ops._Derived.get(w, "c3", 0, build) is a and ops._Derived.get(w, "c3", 1, build) is b and build.calls == 4


def test_get_rebuilds_after_a_version_bump_and_a_mode_change():
    w, build = torch.zeros(8, 8, 3, 3), _Builder()
    a = ops._Derived.get(w, "c3", 0, build)
    w.add_(1.0)
    b = ops._Derived.get(w, "c3", 0, build)
    assert b is not a and build.calls == 2 and ops._Derived.get(w, "c3", 0, build) is b
    ops.set_conv_math("bf16x3")
    try:
        c = ops._Derived.get(w, "c3", 0, build)
    finally:
        ops.set_conv_math("bf16x6")
    assert c is not b and build.calls == 3


def test_same_storage_new_epoch_goes_to_the_batched_refresh(monkeypatch):
    """weights_updated() alone (same pointer, same version): get asks _prep_all for the refresh; a refresh that brings the key up
    to date (here: a stand-in, the real one wants device tensors) leaves the image object in place - no lazy rebuild.  A version
    bump is no case for the batched refresh."""
    w, build, refreshed = torch.zeros(8, 8, 3, 3), _Builder(), []

    def refresh(device):
        refreshed.append(device)
        w._buctd_derived.key = (w.data_ptr(), w._version, ops.weights_epoch(), ops.get_conv_math())
    monkeypatch.setattr(ops, "_prep_all", refresh)
    a = ops._Derived.get(w, "c3", 0, build)
    ops.weights_updated()
    assert ops._Derived.get(w, "c3", 0, build) is a and build.calls == 1 and refreshed == [w.device]
    w.add_(1.0)
    assert ops._Derived.get(w, "c3", 0, build) is not a and build.calls == 2 and len(refreshed) == 1
    # the real refresh skips a host tensor: its key stays stale and the image is rebuilt lazily
    monkeypatch.undo()
    ops.weights_updated()
    ops._Derived.get(w, "c3", 0, build)
    assert build.calls == 3
    # a Linear image has no batched refresh: rebuilt on its next use, _prep_all not asked (checked on the device below)


def test_predicate_same_storage_other_epoch():
    assert ops._rewritten_in_place((10, 3, 1, "bf16x6"), (10, 3, 2, "bf16x6"))
    assert not ops._rewritten_in_place((10, 3, 1, "bf16x6"), (10, 3, 1, "bf16x6"))
    assert not ops._rewritten_in_place((10, 3, 1, "bf16x6"), (10, 4, 2, "bf16x6"))
    assert not ops._rewritten_in_place((10, 3, 1, "bf16x6"), (11, 3, 2, "bf16x6"))
    assert not ops._rewritten_in_place((10, 3, 1, "bf16x6"), (10, 3, 2, "bf16x3"))


def test_get_registers_a_weight_once():
    w, build = torch.zeros(8, 8, 3, 3), _Builder()

    def entries():
        return sum(1 for r in ops._prep_registry["weights"] if r() is w)
    assert entries() == 0
    for _ in range(3):
        ops._Derived.get(w, "c3", 0, build)
        ops._Derived.get(w, "gc", (1, 1), build)
        w.add_(1.0)
        ops.weights_updated()
    assert entries() == 1 and build.calls == 6


class _NoAttributes(torch.Tensor):
    def __setattr__(self, name, value):
        raise AttributeError(name)


def test_get_tolerates_a_tensor_that_refuses_attributes():
    w, build = torch.zeros(8, 8, 3, 3).as_subclass(_NoAttributes), _Builder()
    with pytest.raises(AttributeError):
        w._buctd_derived = None
    n = len(ops._prep_registry["weights"])
    a = ops._Derived.get(w, "c3", 0, build)
    b = ops._Derived.get(w, "c3", 0, build)
    assert build.calls == 2 and float(a[0]) == 1.0 and float(b[0]) == 2.0        # correct, uncached
    assert len(ops._prep_registry["weights"]) == n and not hasattr(w, "_buctd_derived")


def test_rebuild_counter_on_the_host_families():
    w, build = torch.zeros(8, 8, 3, 3), _Builder()
    for family, slot in (("c3", 0), ("c3", 1), ("gc", (1, 0))):
        n = ops.derived_rebuilds()
        ops._Derived.get(w, family, slot, build)
        assert ops.derived_rebuilds() == n + 1
        ops._Derived.get(w, family, slot, build)
        assert ops.derived_rebuilds() == n + 1
    w.add_(1.0)
    n = ops.derived_rebuilds()
    ops._Derived.get(w, "c3", 0, build)
    ops._Derived.get(w, "c3", 0, build)
    assert ops.derived_rebuilds() == n + 1


def test_stats_buffers_memoises_ints_and_allocates_counts_on_request():
    asked = []

    def query(ng, rpg):          # a *_stats_groups entry point: two int* results, status 0
        asked.append(1)
        ng._obj.value, rpg._obj.value = 5, 7
        return 0
    cpu = torch.device("cpu")
    part, info = ops._stats_buffers(("test_derived_cache", 1), query, 12, cpu)
    assert part.shape == (5, 12, 2) and part.dtype == torch.float32 and info == (5, 7)
    assert all(type(v) is int for v in info)
    part2, info2 = ops._stats_buffers(("test_derived_cache", 1), query, 12, cpu, True)
    assert len(asked) == 1 and part2 is not part and info2[:2] == (5, 7) and type(info2[0]) is int and type(info2[1]) is int
    assert info2[2].shape == (5,) and info2[2].dtype == torch.int32
    ops._stats_buffers(("test_derived_cache", 2), query, 12, cpu)
    assert len(asked) == 2


# ---- on the device -----------------------------------------------------------------------------------------------------


class _Counted:
    """Counts the calls of some entry points of the loaded library while the test runs."""

    def __init__(self, monkeypatch, names):
        self.n = dict.fromkeys(names, 0)
        lib = ops.lib()
        for name in names:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def counted(*args):
            self.n[name] += 1
            return fn(*args)
        return counted

    def take(self):
        n, self.n = self.n, dict.fromkeys(self.n, 0)
        return n


BATCHED = ("buctd_conv3x3_bf16x3_prep_batched", "buctd_gconv_x6_prep_batched")
LAZY = ("buctd_conv3x3_bf16x6_prep", "buctd_gconv_x6_prep", "buctd_x6_image")


@pytest.mark.gpu
def test_refresh_is_one_launch_per_family_and_linear_images_rebuild_lazily(dev, monkeypatch):
    """The inputs of test_gpu_gconv.test_prepared_images_follow_in_place_weight_updates plus a 192 x 192 Linear weight in both
    orientations: after weights_updated() + refresh_prepared() every convolution image is current from exactly one batched launch
    per family and no lazy prep; the Linear images rebuild on their next use; a second refresh launches nothing."""
    assert ops.get_conv_math() == "bf16x6"
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 12, 8, 48, generator=g).to(dev)
    ws = [(torch.randn(96, 48, 3, 3, generator=g) / 20).contiguous(memory_format=torch.channels_last).to(dev),
          (torch.randn(48, 48, 1, 1, generator=g) / 7).contiguous(memory_format=torch.channels_last).to(dev),
          (torch.randn(48, 48, 3, 3, generator=g) / 20).contiguous(memory_format=torch.channels_last).to(dev)]
    cfgs = [(2, 1), (1, 0), (1, 1)]
    lin = (torch.randn(192, 192, generator=g) / 14).to(dev)

    def run():
        outs = []
        for w, (st, pad) in zip(ws, cfgs):
            y = ops.conv_fwd(x, w, None, st, pad)
            outs += [y, ops.conv_dgrad(torch.ones_like(y), w, tuple(x.shape), st, pad)]
        return outs + [ops._x6_weight_image(lin, 192, 192, False), ops._x6_weight_image(lin, 192, 192, True)]
    ops.refresh_prepared(dev)                 # whatever earlier tests left registered is current from here on
    counted = _Counted(monkeypatch, BATCHED + LAZY)
    rebuilds = ops.derived_rebuilds()
    before = run()
    first = counted.take()                    # 3x3 stride 1: two images; 1x1 and 3x3 stride 2: two each; Linear: two
    assert first == {BATCHED[0]: 0, BATCHED[1]: 0, LAZY[0]: 2, LAZY[1]: 4, LAZY[2]: 2}
    assert ops.derived_rebuilds() == rebuilds + 8
    again = run()
    assert not any(counted.take().values()) and ops.derived_rebuilds() == rebuilds + 8
    assert again[6] is before[6] and again[7] is before[7]
    for w in ws + [lin]:
        w.data.mul_(1.5).add_(0.01)           # in place like the fused optimizer kernel: no version bump
    ops.weights_updated()
    ops.refresh_prepared(dev)
    assert counted.take() == {BATCHED[0]: 1, BATCHED[1]: 1, LAZY[0]: 0, LAZY[1]: 0, LAZY[2]: 0}
    ops.refresh_prepared(dev)                 # nothing changed since
    assert not any(counted.take().values())
    fresh = run()
    assert counted.take() == {BATCHED[0]: 0, BATCHED[1]: 0, LAZY[0]: 0, LAZY[1]: 0, LAZY[2]: 2}
    assert ops.derived_rebuilds() == rebuilds + 10
    ref = []
    for w, (st, pad) in zip(ws, cfgs):
        w2 = w.detach().clone().contiguous(memory_format=torch.channels_last)
        y = ops.conv_fwd(x, w2, None, st, pad)
        ref += [y, ops.conv_dgrad(torch.ones_like(y), w2, tuple(x.shape), st, pad)]
    lin2 = lin.clone()
    ref += [ops._x6_weight_image(lin2, 192, 192, False), ops._x6_weight_image(lin2, 192, 192, True)]
    assert all(torch.equal(a, b) for a, b in zip(fresh, ref))
    assert not any(torch.equal(a, b) for a, b in zip(fresh, before))


@pytest.mark.gpu
def test_rebuild_counter_on_the_linear_image_and_the_bn_fold(dev):
    lin = torch.randn(192, 192, generator=torch.Generator().manual_seed(3)).to(dev)
    n = ops.derived_rebuilds()
    a = ops._x6_weight_image(lin, 192, 192, False)
    assert ops.derived_rebuilds() == n + 1
    assert ops._x6_weight_image(lin, 192, 192, False) is a and ops.derived_rebuilds() == n + 1
    ops._x6_weight_image(lin, 192, 192, True)
    assert ops.derived_rebuilds() == n + 2
    lin.mul_(2.0)
    assert ops._x6_weight_image(lin, 192, 192, False) is not a and ops.derived_rebuilds() == n + 3
    bn = torch.nn.BatchNorm2d(16).to(dev).eval()
    n = ops.derived_rebuilds()
    s1 = ops.bn_fold_cached(bn, bn.weight, bn.bias, bn.eps)
    assert ops.derived_rebuilds() == n + 1
    s2 = ops.bn_fold_cached(bn, bn.weight, bn.bias, bn.eps)
    assert s2[0] is s1[0] and s2[1] is s1[1] and ops.derived_rebuilds() == n + 1
    with torch.no_grad():
        bn.running_var.mul_(4.0)
    s3 = ops.bn_fold_cached(bn, bn.weight, bn.bias, bn.eps)
    assert ops.derived_rebuilds() == n + 2
    assert torch.allclose(s3[0], s1[0] / 2, rtol=1e-4)
