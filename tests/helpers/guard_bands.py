"""Guard bands around device tensors, shared by the per-plan and per-path suites: an output is a view into a larger
allocation pre-filled with a sentinel (a store next to the output lands there and is seen), a read-only operand sits
between NaN bands (a load next to the operand shows up as NaN in the result).  Ordinary in-bounds allocations only."""
import torch

SENTINEL = -12345.678


def banded(t, dev, shape, fill=float("nan")):
    """a copy of t (device) in the middle of a larger allocation filled with `fill`: >= 2 * SW + 3 rows of it on either side"""
    W, Cn = shape[2], t.shape[-1]
    pad = (2 * (W + 1) + 3 + 5) * Cn
    big = torch.full((2 * pad + t.numel(),), fill, dtype=torch.float32, device=dev)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, big, pad


def untouched(big, pad, n, fill=SENTINEL):
    fill = torch.tensor(fill, dtype=big.dtype).item()       # the sentinel as the buffer's type stores it
    return bool((big[:pad] == fill).all()) and bool((big[pad + n:] == fill).all())


BAND16 = 256        # elements of 4 bytes on either side: a multiple of 16 bytes, so the view keeps the allocation's alignment


def banded16(t, dev, fill=float("nan"), pad=BAND16):
    """banded() for the streaming kernels: bands of whole 16-byte pieces (the kernels see the alignment they are written
    for), any 4-byte element type"""
    assert pad % 4 == 0 and t.element_size() == 4
    big = torch.full((2 * pad + t.numel(),), fill, dtype=t.dtype, device=dev)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view, big, pad


BAND16_2B = 512     # elements of 2 bytes on either side: the same 1024 bytes as BAND16


def banded16_2b(t, dev, fill=float("nan"), pad=BAND16_2B):
    """banded16() for 2-byte element types (torch.bfloat16 activations and filter images)"""
    assert pad % 8 == 0 and t.element_size() == 2
    big = torch.full((2 * pad + t.numel(),), fill, dtype=t.dtype, device=dev)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view, big, pad


class Bands:
    """Places the operands of one call.  on=True: read-only operands between NaN bands, outputs between sentinel bands
    (check() asserts the bands are intact); on=False: plain tensors, the unbanded call the banded one must equal."""

    def __init__(self, dev, on):
        self.dev, self.on, self.keep, self.outs = dev, on, [], []

    def ro(self, t):
        if t is None:
            return None
        if not self.on:
            plain = t.to(self.dev).contiguous()
            self.keep.append(plain)         # the caller may pass only the address on: the allocation lives as long as this object
            return plain
        # NaN around a floating operand; around an integer one (row counts) a value that would wreck any sum it enters
        view, big, _ = banded16(t, self.dev, float("nan") if t.dtype.is_floating_point else -(1 << 30))
        self.keep.append(big)
        return view

    def out(self, init, name="output"):
        """an output (or in/out) tensor that starts as `init`; pass torch.empty-like garbage as a NaN-filled tensor"""
        if not self.on:
            return init.to(self.dev).clone().contiguous()
        fill = SENTINEL if init.dtype.is_floating_point else -12345
        view, big, pad = banded16(init, self.dev, fill)
        self.outs.append((big, pad, init.numel(), fill, name))
        return view

    def new(self, shape, name="output", dtype=torch.float32):
        init = torch.full(tuple(shape), float("nan") if dtype.is_floating_point else -7, dtype=dtype)
        return self.out(init, name)

    def check(self, what=""):
        for big, pad, n, fill, name in self.outs:
            assert untouched(big, pad, n, fill), f"{what}: the launch wrote outside {name}"


class BandsAny(Bands):
    """Bands for calls whose operands mix 4-byte and 2-byte element types (the bf16 inference kernels): bands of 1024 bytes
    on either side whatever the type.  A bf16 output's sentinel is SENTINEL as bf16 stores it."""

    @staticmethod
    def _banded(t, dev, fill):
        return banded16_2b(t, dev, fill) if t.element_size() == 2 else banded16(t, dev, fill)

    def ro(self, t):
        if t is None or not self.on:
            return super().ro(t)
        view, big, _ = self._banded(t, self.dev, float("nan") if t.dtype.is_floating_point else -(1 << 30))
        self.keep.append(big)
        return view

    def out(self, init, name="output"):
        if not self.on:
            return super().out(init, name)
        fill = SENTINEL if init.dtype.is_floating_point else -12345
        view, big, pad = self._banded(init, self.dev, fill)
        self.outs.append((big, pad, init.numel(), fill, name))
        return view
