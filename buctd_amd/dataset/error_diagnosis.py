"""Pose error diagnosis on the device: which error type every key point of a bottom-up model is, in the synthesiser's own
geometry, and probability ladders for the synthesiser calibrated from the result.

buctd_pose_error_types (csrc/synth_diag.hip) is the inverse of buctd_synthesize_pose: per labelled joint the code
0 good / 1 jitter / 2 inversion / 3 swap / 4 miss / 5 absent (-1: unlabelled), the key point similarity, and the counts per
(type, ladder row, joint class) the ladders are made of.  DESIGN.md "Pose error diagnosis" has the definition.

    records = ConditionSource(cfg, annotated, device=dev).train_records(model_key='bu_w32')
    profile = diagnose_records(pipe, records)
    pipe = DeviceSamplePipeline(cfg, ..., is_train=True, synth_ladders=profile.ladders(default_ladders(dataset)))
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from .._C import check, lib, ptr, stream_ptr
from .pose_synthesis import _LADDER_SHAPES, _freeze, _thaw, default_ladders, make_tables

CODES = ("good", "jitter", "inversion", "swap", "miss", "absent")
TYPES = ("jitter_p", "miss_p", "inv_p", "swap_p")            # hist's first axis; its rows: 2, 3, 1, 2
_ROWS = (2, 3, 1, 2)


class ErrorProfile:
    """Result of diagnose() / diagnose_records().  Device tensors: code int32 [N, K], ks float64 [N, K] (N persons,
    concatenated over batches), hist int64 [4, 3, 3, 2] (type jitter / miss / inversion / swap, ladder row, joint class,
    {hits, eligible}), per_joint int64 [K, 6] (counts of the codes 0...5)."""

    def __init__(self, dataset, code, ks, hist, per_joint, tables=None):
        self.dataset, self.code, self.ks, self.hist, self.per_joint = dataset, code, ks, hist, per_joint
        self.tables = tables

    def table(self):
        """OrderedDict code name -> numpy [K]: per joint the fraction of its scored (labelled) instances with that code;
        a joint never scored has zeros.  np.stack(list(table().values()), 1) is the [K, 6] array."""
        pj = self.per_joint.cpu().numpy().astype(np.float64)
        frac = pj / np.maximum(pj.sum(1, keepdims=True), 1.0)
        return OrderedDict((name, frac[:, c].copy()) for c, name in enumerate(CODES))

    def ladders(self, base=None, min_count=100):
        """Probability ladders for make_tables / DeviceSamplePipeline(synth_ladders=...): every (type, row, class) cell
        with at least min_count eligible joints becomes hits / eligible, every other cell (and the row thresholds) keeps
        base's value (base None: the data set's default ladders).  min_count is a policy constant, not a measurement.

        A cell is the FREQUENCY of the type among the joints eligible for it (inversion: the partner is labelled; swap:
        a neighbour has the joint or its partner).  The synthesiser renormalises its probabilities when a type has no
        source or no surviving candidate, so the frequency equals the ladder that generated a data set exactly only when
        every type is eligible and feasible for every joint; this is not a maximum-likelihood fit under renormalisation.

        Raises ValueError when for some joint and some combination of rows jitter + miss + inversion + swap > 1: the
        synthesiser needs p_good >= 0."""
        base = default_ladders(self.dataset) if base is None else base
        out = {k: _thaw(_freeze(v)) for k, v in base.items()}
        missing = [k for k in _LADDER_SHAPES if k not in out]
        if missing:
            out.update({k: v for k, v in default_ladders(self.dataset).items() if k in missing})
        hist = self.hist.cpu().numpy()
        for t, name in enumerate(TYPES):
            for r in range(_ROWS[t]):
                for c in range(3):
                    hits, eligible = int(hist[t, r, c, 0]), int(hist[t, r, c, 1])
                    if eligible >= min_count and eligible > 0:
                        if name == "inv_p":
                            out[name][c] = hits / eligible
                        else:
                            out[name][r][c] = hits / eligible
        self._check_sum(out)
        return out

    def _check_sum(self, lad):
        t = self.tables
        if t is None:
            classes = {(a, b, c, d) for a in range(3) for b in range(3) for c in range(3) for d in range(3)}
        else:
            K = int(self.per_joint.shape[0])
            classes = {(t.jitter_cls[j], t.miss_cls[j], t.inv_cls[j], t.swap_cls[j]) for j in range(K)}
        for cj, cm, ci, cs in sorted(classes):
            for rj in range(2):
                for rm in range(3):
                    for rs in range(2):
                        total = lad["jitter_p"][rj][cj] + lad["miss_p"][rm][cm] + lad["inv_p"][ci] + lad["swap_p"][rs][cs]
                        if total > 1.0:
                            raise ValueError(
                                f"ladders: joint classes (jitter {cj}, miss {cm}, inversion {ci}, swap {cs}) at rows (jitter "
                                f"{rj}, miss {rm}, swap {rs}) sum to {total:.6f} > 1: the synthesiser needs p_good >= 0")


def _dev64(a, dev):
    if not torch.is_tensor(a):
        a = torch.tensor(np.asarray(a), dtype=torch.float64)            # a copy: the caller's array may be read-only
    return a.to(device=dev, dtype=torch.float64).contiguous()


def diagnose(dataset, joints, estimated, near_joints, area, num_overlap=None, *, tables=None, profile=None, device=None):
    """One buctd_pose_error_types launch.  joints, estimated [B, K, 3]; near_joints [B, M, K, 3] or None (absent
    neighbours: visibility 0); area [B]; num_overlap [B] (None: zeros, as DeviceSamplePipeline passes them) - numpy arrays
    or tensors, the arguments of synthesize_pose_batch with the pose to diagnose as `estimated`.  tables: a
    make_tables() result (None: the data set's default - only sigmas, pairs, classes and row thresholds are read, never
    the probabilities).  profile: an ErrorProfile to continue - its counters are added to and code / ks appended; None
    starts one.  Returns the ErrorProfile; nothing is copied to the host and the call does not wait for the device."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    J, E, A = _dev64(joints, dev), _dev64(estimated, dev), _dev64(area, dev)
    B, K = int(J.shape[0]), int(J.shape[1])
    if E.shape != J.shape or J.shape[2] != 3 or A.shape != (B,):
        raise ValueError(f"diagnose: joints {tuple(J.shape)}, estimated {tuple(E.shape)}, area {tuple(A.shape)}")
    NR = _dev64(near_joints, dev) if near_joints is not None and len(near_joints) else None
    M = 0 if NR is None else int(NR.shape[1])
    if NR is not None and NR.shape != (B, M, K, 3):
        raise ValueError(f"diagnose: near_joints {tuple(NR.shape)}, expected {(B, M, K, 3)}")
    ov = np.zeros(B, dtype=np.int32) if num_overlap is None else num_overlap
    ov = (ov if torch.is_tensor(ov) else torch.tensor(np.asarray(ov))).to(device=dev, dtype=torch.int32).contiguous()
    if ov.shape != (B,):
        raise ValueError(f"diagnose: num_overlap {tuple(ov.shape)}, expected {(B,)}")
    tables = make_tables(dataset, K) if tables is None else tables
    if profile is None:
        profile = ErrorProfile(dataset, None, None, torch.zeros((4, 3, 3, 2), dtype=torch.int64, device=dev),
                               torch.zeros((K, 6), dtype=torch.int64, device=dev), tables)
    elif profile.per_joint.shape[0] != K or profile.hist.device != J.device:
        raise ValueError("diagnose: the profile to continue has another joint count or device")
    code = torch.empty((B, K), dtype=torch.int32, device=dev)
    ks = torch.empty((B, K), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().buctd_pose_error_types(C.byref(tables), ptr(J), ptr(E), ptr(NR), ptr(A), ptr(ov), B, K, M, ptr(code),
                                           ptr(ks), ptr(profile.hist), ptr(profile.per_joint), stream_ptr()),
              "pose_error_types")
    profile.code = code if profile.code is None else torch.cat([profile.code, code])
    profile.ks = ks if profile.ks is None else torch.cat([profile.ks, ks])
    return profile


def diagnose_records(pipeline, records, batch=4096):
    """Diagnoses the conditions of train records - the output of ConditionSource.train_records(model_key=...) or any
    records DeviceSamplePipeline takes - packed by the pipeline's own synthesis_inputs: the condition as the pose to
    diagnose, synthesis_area of it as the area (the rings are the ones training uses) and pad_near_joints.  The loader
    leaves the third column of joints_3d at 0 and keeps the label in joints_3d_vis (dataloader.py:177-188); a joint counts
    as labelled here when either is > 0 - without that no joint of such a record could be scored.  Records without a
    condition are diagnosed as their own ground truth under DATASET.SYNTHESIS_POSE (every joint good), as the pipeline
    conditions them."""
    if not records:
        raise ValueError("diagnose_records: no records")
    image = records[0].get("image")
    dev = image.device if torch.is_tensor(image) else None
    K = pipeline.num_joints
    profile = None
    for at in range(0, len(records), int(batch)):
        part = records[at:at + int(batch)]
        J, E, _, near, area = pipeline.synthesis_inputs(part)
        label = np.stack([np.asarray(r["joints_3d_vis"], dtype=np.float64).reshape(K, 3)[:, 0] for r in part])
        J = J.copy()
        J[:, :, 2] = np.maximum(J[:, :, 2], label)
        profile = diagnose(pipeline.dataset, J, E, near, area, profile=profile, device=dev)
    return profile
