"""Gradient-norm clipping restated for the tests: torch.nn.utils.clip_grad_norm_'s norm and coefficient in fp64 (numpy and
math.fsum, no torch arithmetic), and the optimizer steps of csrc/loss_decode.hip in fp32 in the kernels' order with
hyper-parameters that fp32 holds exactly - so that torch.optim.Adam / SGD run in float64 are their exact-arithmetic twin and
every difference the GPU tests measure is rounding of the step itself.

Bars of the GPU tests that come from here:
  reduction    a fixed-order fp64 sum of n <= 2^20 + 3 non-negative terms is off by at most n 2^-53 = 1.2e-10 relative
               (squares of floats are exact in fp64); the issue's bar is 2e-10
  finalize     fp64 expressions rounded once to fp32: 1 ulp of fp32 covers a last-bit difference of the fp64 square root
  clipped step the bar of tests/test_gpu_heatmap_kernels.py for an unclipped step: max(4 x the error of the fp32 CPU formula
               against fp64, 2^-23), p relative to |p| before + the updates so far, moments relative to their largest
               element
"""
import math

import numpy as np
import torch

CHUNK = 8192                    # BUCTD_GRAD_SUMSQ_CHUNK of include/buctd_hip.h
LENGTHS = (1, 63, 64, 65, 4095, 4096, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 2 ** 20 + 3)
FLOOR = 2.0 ** -23              # floor of the measured bars (tests/helpers/stream_cases.py)

# exactly representable in fp32 (and therefore the same numbers in the float64 torch optimizers)
ADAM_HYPER = (2.0 ** -10, 0.875, 1.0 - 2.0 ** -9, 2.0 ** -27)          # lr, beta1, beta2, eps
SGD_HYPER = (2.0 ** -4, 0.875, 2.0 ** -10)                             # lr, momentum, weight decay


def f32(x):
    return float(np.float32(x))


def sumsq(values):
    """exact sum of squares of fp32 values (a sequence of numpy arrays or one array), correctly rounded to fp64"""
    arrays = values if isinstance(values, (list, tuple)) else [values]
    return math.fsum(v for a in arrays for v in np.square(np.asarray(a, dtype=np.float64).ravel()).tolist())


def norm_coef(sumsq_value, max_norm, gscale=1.0):
    """-> (total_norm, coef) in fp64: torch's expressions, clip_grad_norm_(error_if_nonfinite=False)"""
    total = gscale * math.sqrt(sumsq_value) if not math.isnan(sumsq_value) else float("nan")
    c = max_norm / (total + 1e-6)
    return total, (1.0 if c > 1.0 else c)


def within_one_ulp(got, ref64):
    """fp32 tensor `got` against fp64 values rounded to fp32: equal, or a neighbour"""
    r = torch.as_tensor(ref64, dtype=torch.float64).to(torch.float32).reshape(got.shape)
    lo = torch.nextafter(r, torch.full_like(r, -math.inf))
    hi = torch.nextafter(r, torch.full_like(r, math.inf))
    return bool(((got >= lo) & (got <= hi)).all())


def log_uniform(n, gen, lo=-20.0, hi=15.0):
    """n fp32 values of either sign with magnitudes 1e-20 ... 1e+15, log-uniform: an fp32 accumulator loses the small squares
    (they underflow) and the precision of the large ones"""
    e = torch.rand(n, generator=gen, dtype=torch.float64) * (hi - lo) + lo
    s = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    return (s * 10.0 ** e).float()


def adam32(p, g, m, v, step, scale):
    """one step of adam_kernel in fp32, its order (loss_decode.hip); scale: the fp32 product gscale * coef"""
    lr, b1, b2, eps = (torch.tensor(x, dtype=torch.float32) for x in ADAM_HYPER)
    one = torch.tensor(1.0, dtype=torch.float32)
    bc1 = torch.tensor(1.0 - ADAM_HYPER[1] ** step, dtype=torch.float32)
    bc2s = torch.tensor(math.sqrt(1.0 - ADAM_HYPER[2] ** step), dtype=torch.float32)
    gg = g * torch.tensor(scale, dtype=torch.float32)
    m = b1 * m + (one - b1) * gg
    v = b2 * v + (one - b2) * gg * gg
    return p - (lr / bc1) * (m / (torch.sqrt(v) / bc2s + eps)), m, v


def sgd32(p, g, buf, nesterov, scale):
    """one step of sgd_kernel in fp32, its order; a zero buffer makes the first step's 'buf = g'"""
    lr, mu, wd = (torch.tensor(x, dtype=torch.float32) for x in SGD_HYPER)
    gg = g * torch.tensor(scale, dtype=torch.float32) + wd * p
    b = mu * buf + gg
    gg = gg + mu * b if nesterov else b
    return p - lr * gg, b
