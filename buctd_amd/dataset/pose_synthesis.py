"""Generative pose synthesis on the device - drop-in for reference lib/dataset/pose_synthesis.py:779-817
(synthesize_pose and its variants: coco 505-775, crowdpose 234-501, and synthesize_pose_fish 6-231, the generic one that
every other DATASET.DATASET takes - fish, marmosets, multimouse, a custom data set): the training-time condition of every
"generative sampling" recipe (DATASET.SYNTHESIS_POSE True).  synthesize_pose keeps the reference signature for one person;
synthesize_pose_batch does a whole batch in one kernel launch (one wavefront per person and joint)."""
import ctypes as C
import functools

import numpy as np
import torch

from .._C import check, lib, ptr, stream_ptr

_MAXK = 32


class _Tables(C.Structure):
    _fields_ = [("sigmas", C.c_double * _MAXK), ("pair", C.c_int * _MAXK), ("jitter_cls", C.c_int * _MAXK),
                ("miss_cls", C.c_int * _MAXK), ("inv_cls", C.c_int * _MAXK), ("swap_cls", C.c_int * _MAXK),
                ("jitter_p", (C.c_double * 3) * 2), ("miss_p", (C.c_double * 3) * 3), ("inv_p", C.c_double * 3),
                ("swap_p", (C.c_double * 3) * 2), ("out_vis", C.c_double), ("jitter_nv", C.c_int),
                ("miss_nv", C.c_int * 2), ("crowd_nv", C.c_int * 2), ("crowd_ov", C.c_int * 2)]


# The probability ladders [row][class] and the thresholds that pick the row: jitter row 0 while num_valid <= jitter_nv;
# miss row 0 / 1 while num_valid <= miss_nv[0] / [1]; swap row 0 when "crowded" = for one of the two (nv, ov) pairs
# num_valid <= nv and num_overlap >= ov.  coco and crowdpose share theirs (pose_synthesis.py:56-72, 91-112, 146-152,
# 176-190 / 561-575, 597-618, 651-657, 680-694: `num_overlap > 0` is `>= 1`).
_HUMAN_LADDERS = dict(jitter_p=[[0.15, 0.20, 0.25], [0.10, 0.15, 0.20]],
                      miss_p=[[0.15, 0.20, 0.25], [0.10, 0.13, 0.15], [0.02, 0.05, 0.10]], inv_p=[0.01, 0.03, 0.06],
                      swap_p=[[0.02, 0.15, 0.10], [0.01, 0.06, 0.03]],
                      jitter_nv=10, miss_nv=(5, 10), crowd=((10, 1), (15, 3)))
# synthesize_pose_fish (pose_synthesis.py:61-64, 86-91, 126, 150-153): one class, other thresholds
_GENERIC_LADDERS = dict(jitter_p=[[0.20] * 3, [0.15] * 3], miss_p=[[0.20] * 3, [0.13] * 3, [0.05] * 3], inv_p=[0.03] * 3,
                        swap_p=[[0.10] * 3, [0.04] * 3], jitter_nv=4, miss_nv=(2, 4), crowd=((4, 1), (5, 1)))


def _joint_classes(dataset, k):
    """Per-joint probability classes of the reference's if / elif ladders (pose_synthesis.py:56-72, 91-112, 146-152,
    176-190 for crowdpose; 561-575, 597-618, 651-657, 680-694 for coco).  Crowdpose joints 12 and 13 fall through the
    jitter ladder and inherit what joint 11 left in the variable: class 0.  Any other data set is the generic variant
    (pose_synthesis.py:798-800, 815-816): k joints of sigma 0.1, no symmetry, no classes, visibility column 0 (line 229)."""
    if dataset == "coco":
        jit = [0 if (j == 0 or 13 <= j <= 16) else (1 if 1 <= j <= 10 else 2) for j in range(k)]
        miss = [0 if j <= 4 else (1 if j in (5, 6, 15, 16) else 2) for j in range(k)]
        inv = [0 if j <= 4 else (1 if 5 <= j <= 10 else 2) for j in range(k)]
        swap = list(inv)
        sym = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
        sig = [.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]
        vis = 1.0
    elif dataset == "crowdpose":
        jit = [0 if 8 <= j <= 11 else (1 if j <= 5 else (2 if j <= 7 else 0)) for j in range(k)]
        miss = [0 if j in (12, 13) else (1 if j in (0, 1, 8, 9) else 2) for j in range(k)]
        inv = [0 if j >= 12 else (1 if j <= 5 else 2) for j in range(k)]
        swap = [0 if j in (12, 13) else (1 if j <= 5 else 2) for j in range(k)]
        sym = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)]
        sig = [.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .79, .79]
        vis = 0.0
    else:
        jit = miss = inv = swap = [0] * k
        sym, sig, vis = [], [1.] * k, 0.0
    return jit, miss, inv, swap, sym, np.array(sig) / 10.0, vis


def default_ladders(dataset):
    """A copy of the ladders `dataset` takes without a `ladders` argument (the reference's numbers)."""
    lad = _HUMAN_LADDERS if dataset in ("coco", "crowdpose") else _GENERIC_LADDERS
    return {k: _thaw(_freeze(v)) for k, v in lad.items()}


def _freeze(v):
    """Nested lists / tuples / arrays -> nested tuples of Python numbers (hashable: the key of the tables' cache)."""
    if isinstance(v, (list, tuple, np.ndarray)):
        return tuple(_freeze(x) for x in v)
    return v.item() if isinstance(v, np.generic) else v


def _thaw(v):
    return [_thaw(x) for x in v] if isinstance(v, tuple) else v


_LADDER_SHAPES = dict(jitter_p=(2, 3), miss_p=(3, 3), inv_p=(3,), swap_p=(2, 3), jitter_nv=(), miss_nv=(2,), crowd=(2, 2))


def _ladders_key(ladders):
    """ladders (a dict with keys of _HUMAN_LADDERS: the four probability ladders alone, or the row thresholds as well) ->
    a sorted tuple of (key, nested tuples), checked for keys, shapes and 0 <= p <= 1."""
    unknown = sorted(set(ladders) - set(_LADDER_SHAPES))
    if unknown:
        raise ValueError(f"ladders: unknown keys {unknown}; known: {sorted(_LADDER_SHAPES)}")
    key = []
    for name in sorted(ladders):
        val = _freeze(ladders[name])
        if np.shape(val) != _LADDER_SHAPES[name]:
            raise ValueError(f"ladders[{name!r}] has shape {np.shape(val)}, expected {_LADDER_SHAPES[name]}")
        if name.endswith("_p") and not all(0.0 <= p <= 1.0 for p in np.ravel(val)):
            raise ValueError(f"ladders[{name!r}] holds a probability outside [0, 1]")
        key.append((name, val))
    return tuple(key)


def make_tables(dataset, num_joints, ladders=None):
    """Per-dataset constants of the kernel (buctd_synth_tables), built once per (dataset, K, ladders); callers do not
    modify it.  dataset: 'coco', 'crowdpose', or any other name for the generic variant with num_joints (1...32) key
    points.  ladders: None = the reference's numbers; or a dict with keys of default_ladders(dataset) - the probability
    ladders jitter_p / miss_p / inv_p / swap_p, any subset, and optionally the row thresholds - that replaces those
    entries (ErrorProfile.ladders of dataset.error_diagnosis makes one from a bottom-up model's measured errors)."""
    return _make_tables(dataset, num_joints, None if ladders is None else _ladders_key(ladders))


@functools.lru_cache(maxsize=None)
def _make_tables(dataset, num_joints, ladders_key):
    if not 1 <= num_joints <= _MAXK:
        raise ValueError(f"pose synthesis takes 1 to {_MAXK} key points, MODEL.NUM_JOINTS is {num_joints}")
    jit, miss, inv, swap, sym, sig, vis = _joint_classes(dataset, num_joints)
    if len(sig) != num_joints:
        raise ValueError(f"{dataset} has {len(sig)} key points, MODEL.NUM_JOINTS is {num_joints}")
    lad = _HUMAN_LADDERS if dataset in ("coco", "crowdpose") else _GENERIC_LADDERS
    if ladders_key is not None:
        lad = dict(lad, **dict(ladders_key))
    t = _Tables()
    pair = [-1] * _MAXK
    for a, b in sym:
        pair[a], pair[b] = b, a
    for j in range(_MAXK):
        t.pair[j] = pair[j]
        t.sigmas[j] = float(sig[j]) if j < num_joints else 0.0
        t.jitter_cls[j] = jit[j] if j < num_joints else 0
        t.miss_cls[j] = miss[j] if j < num_joints else 0
        t.inv_cls[j] = inv[j] if j < num_joints else 0
        t.swap_cls[j] = swap[j] if j < num_joints else 0
    for name in ("jitter_p", "miss_p", "swap_p"):
        for r, row in enumerate(lad[name]):
            for c, v in enumerate(row):
                getattr(t, name)[r][c] = v
    for c, v in enumerate(lad["inv_p"]):
        t.inv_p[c] = v
    t.out_vis = vis
    t.jitter_nv = lad["jitter_nv"]
    for i in range(2):
        t.miss_nv[i] = lad["miss_nv"][i]
        t.crowd_nv[i], t.crowd_ov[i] = lad["crowd"][i]
    return t


def synthesize_pose_batch(dataset, joints, estimated_joints, near_joints, area, num_overlap, seed, device=None,
                          ladders=None):
    """joints, estimated_joints [B, K, 3]; near_joints [B, M, K, 3] (pad absent neighbours with visibility 0);
    area [B]; num_overlap [B].  numpy arrays or tensors; returns a float64 device tensor [B, K, 3].
    ladders: see make_tables (None: the reference's)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device

    def dev64(a):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a, dtype=torch.float64).to(dev).contiguous()
    J, E, A = dev64(joints), dev64(estimated_joints), dev64(area)
    B, K = J.shape[0], J.shape[1]
    NR = dev64(near_joints) if near_joints is not None and len(near_joints) else None
    M = 0 if NR is None else NR.shape[1]
    ov = torch.as_tensor(np.asarray(num_overlap), dtype=torch.int32).to(dev).contiguous()
    out = torch.empty((B, K, 3), dtype=torch.float64, device=dev)
    tables = make_tables(dataset, K, ladders)
    check(lib().buctd_synthesize_pose(C.byref(tables), ptr(J), ptr(E), ptr(NR), ptr(A), ptr(ov), B, K, M,
                                      C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), ptr(out), stream_ptr()),
          "synthesize_pose")
    return out


_calls = {"n": 0}


def synthesize_pose(cfg, joints, estimated_joints, near_joints, area, num_overlap, seed=None):
    """Reference signature (one person, numpy in / numpy out).  seed None: torch's seed mixed with a call counter."""
    if seed is None:
        _calls["n"] += 1
        seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + _calls["n"]) & 0xFFFFFFFFFFFFFFFF
    near = np.asarray(near_joints, dtype=np.float64).reshape(-1, cfg.MODEL.NUM_JOINTS, 3)
    out = synthesize_pose_batch(cfg.DATASET.DATASET, np.asarray(joints)[None], np.asarray(estimated_joints)[None],
                                near[None] if near.shape[0] else None, [area], [num_overlap], seed)
    return out[0].cpu().numpy()
