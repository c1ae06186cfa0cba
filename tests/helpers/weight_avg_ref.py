"""fp64 restatement of the weight-averaging recurrence and of its schedules (engine.WeightAverage, csrc/weight_avg.hip), in
numpy; shares no code with the product.

    avg_{t+1} = avg_t + w_t (p_t - avg_t)
    ema:  w_t = 1 - d_t,  d_t = min(decay, (1 + t) / (10 + t)) with warm-up, decay without     (t counts the updates from 0)
    swa:  w_t = 1 / (t + 1)

The recurrence takes the weight as the launch receives it - the double rounded once to fp32 (f32()) - so the rounding of w
itself is not part of the compared error."""
import numpy as np

EPS = 2.0 ** -24        # half an ulp of 1.0 in fp32: the relative error of one rounding


def f32(w):
    """the fp32 value a double becomes when it is passed as a float argument, as a Python float"""
    return float(np.float32(w))


def decay_at(decay, t, warmup=True):
    if not warmup:
        return decay
    ramp = (1.0 + t) / (10.0 + t)
    return ramp if ramp < decay else decay


def weight(mode, decay, warmup, t):
    if mode == "swa":
        return 1.0 / (t + 1.0)
    assert mode == "ema"
    return 1.0 - decay_at(decay, t, warmup)


def due(step, start_step, update_every):
    """step counts the optimizer's steps from 1"""
    return step >= start_step and step % update_every == 0


def update(avg, p, w):
    """one update in fp64; avg, p: arrays of any float type, w: the fp32-rounded weight as a Python float"""
    avg = np.asarray(avg, dtype=np.float64)
    return avg + w * (np.asarray(p, dtype=np.float64) - avg)


def chain(avg0, ps, ws):
    avg = np.asarray(avg0, dtype=np.float64)
    for p, w in zip(ps, ws):
        avg = update(avg, p, w)
    return avg


def bound(updates, magnitude):
    """4 S 2^-24 M: see tests/test_gpu_weight_avg.py"""
    return 4.0 * updates * EPS * magnitude


def magnitude(*arrays):
    return max((float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in arrays if np.size(a)), default=0.0)
