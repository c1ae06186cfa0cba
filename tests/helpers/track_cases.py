"""Fixtures of the CTD tracking tests (test_sequence_tracker.py on the CPU, test_gpu_sequence_tracker.py on the GPU).

scripted(K): a T = 6, M = 4 sequence told in image space - who is where in which frame - turned into the heat-map peaks of
a stand-in network by simulating the sequence once with track_ref's book-keeping and the pipeline's own box and crop
functions: the peak of (frame, slot, joint) is the integer heat-map position nearest to where the script wants that joint,
seen through the slot's box of that frame.  A Gaussian at an integer position decodes to that position exactly (no
quarter-pixel shift: its neighbours are equal), so every prediction is transform_preds of the table, in closed form.

step_case(M, K, D): state, decode outputs and detections of one buctd_track_step call."""
import functools

import numpy as np
import torch

from refine_cases import CROP, HEATMAP, IN_VIS_THRE, MARGIN, SCALE_THRE
from tests.helpers import track_ref

IW, IH = 400, 300
T, M = 6, 4
PARAMS = dict(birth_oks=0.3, merge_oks=0.25, death_score=0.2, max_misses=2)
ASPECT = CROP[0] * 1.0 / CROP[1]
HIGH, LOW = 0.8, 0.1                       # peak heights: counted, and below IN_VIS_THRE (key-point score 0)


def sigmas_for(K):
    from buctd_amd.nms.nms import COCO_SIGMAS
    return COCO_SIGMAS if K == 17 else np.linspace(0.05, 0.1, K)


def ref_params(K):
    return dict(PARAMS, sigmas=np.asarray(sigmas_for(K), dtype=np.float64), margin=MARGIN, iw=IW, ih=IH)


def box_cs(pose):
    """center, scale of the crop around a pose: the pipeline's own functions"""
    from buctd_amd.dataset.pipeline import box_from_keypoints, xywh2cs
    return xywh2cs(*box_from_keypoints(np.asarray(pose, dtype=np.float64), MARGIN, IW, IH), ASPECT, SCALE_THRE)


def empty_cs():
    from buctd_amd.dataset.pipeline import xywh2cs
    return xywh2cs(0, 0, IW, IH, ASPECT, SCALE_THRE)


def predictions(peaks, heights, center, scale):
    """[K, 2] integer heat-map positions -> float32 [K, 3] image-space predictions, as the decode leaves them"""
    from buctd_amd.utils.transforms import transform_preds
    xy = transform_preds(peaks.astype(np.float32), center, scale, list(HEATMAP))[:, :2].astype(np.float32)
    return np.concatenate([xy, np.asarray(heights, dtype=np.float32).reshape(-1, 1)], axis=1)


def keypoint_score(maxvals):
    mv = np.asarray(maxvals, dtype=np.float32)
    counted = mv > np.float32(IN_VIS_THRE)
    return float(mv[counted].astype(np.float64).mean()) if counted.any() else 0.0


def _shape(rng, K):
    s = np.stack([rng.uniform(-20, 20, K), rng.uniform(-30, 30, K)], axis=1)
    s[0], s[1] = (-20, -30), (20, 30)                                    # the extent is the same for everyone
    return s


def _pose(centre, shape, score):
    return np.concatenate([shape + np.asarray(centre, dtype=np.float64), np.full((shape.shape[0], 1), score)], axis=1)


@functools.lru_cache(maxsize=None)
def scripted(K):
    """Returns dict(dets [T] of [n, K, 3], peaks [T, M, K, 2], heights [T, M, K], expected [T] of per-frame dicts, margins)."""
    from buctd_amd.utils.transforms import affine_transform, get_affine_transform
    rng = np.random.RandomState(100 + K)
    shapes = {n: _shape(rng, K) for n in "ABCDEFZ"}
    zshape = shapes["Z"]
    zshape[:, 0] = rng.uniform(-15, 15, K); zshape[:, 1] = rng.uniform(-20, 20, K)
    zshape[0], zshape[1] = (-15, -20), (15, 20)                        # x in [35, 65], y in [60, 100] around (50, 80)
    where = {"A": lambda t: (130 + 4 * t, 90), "B": lambda t: (300, 80 + 3 * t), "C": lambda t: (80, 225),
             "D": lambda t: (135, 225) if t <= 2 else (80, 225), "F": lambda t: (200, 60), "Z": lambda t: (50, 80)}
    low = {("B", 2), ("B", 3), ("C", 3)}                                # B: max_misses low frames; C: one fewer
    det = lambda name, t, score=0.9, shift=(0, 0): (name, _pose(np.add(where[name](t), shift), shapes[name], score))
    script = [[det("A", 0), det("B", 0, 0.85), det("A", 0, 0.6, (3, -2))],        # the copy of A is covered by A's track
              [det("A", 1, 0.7), det("C", 1)],                                     # A again: covered; C is born
              [det("D", 2, 0.9), ("E", _pose((200, 60), shapes["E"], 0.5))],       # D takes the last slot, E finds none
              [],                                                                  # nothing detected
              [det("F", 4), det("A", 4, 0.5)],                                     # F takes the slot B left in frame 3
              [det("Z", 5)]]                                                       # born and dead in one frame
    par = ref_params(K)
    margins = track_ref.Margins()
    ids, misses, next_id = np.full(M, -1, dtype=np.int64), np.zeros(M, dtype=np.int64), 0
    pose, area = np.zeros((M, K, 3)), np.zeros(M)
    names = {}
    peaks, heights = np.ones((T, M, K, 2)), np.full((T, M, K), HIGH)
    expected, dets = [], []
    for t in range(T):
        d = np.stack([p for _, p in script[t]]) if script[t] else np.zeros((0, K, 3))
        dets.append(d)
        born, next_id = track_ref.birth(ids, pose, area, next_id, d, par, margins)
        for s in np.nonzero(born)[0]:
            names[ids[s]] = next(n for n, p in script[t] if np.array_equal(p, pose[s]))
        preds, score = np.zeros((M, K, 3), dtype=np.float32), np.zeros(M)
        for s in np.nonzero(ids >= 0)[0]:
            name = names[ids[s]]
            c, sc = box_cs(pose[s])
            fwd = get_affine_transform(c, sc, 0, np.array(CROP))
            want = shapes[name] + np.asarray(where[name](t), dtype=np.float64)
            hm = np.stack([affine_transform(w, fwd) for w in want]) / (CROP[0] / HEATMAP[0])
            peaks[t, s] = np.clip(np.rint(hm), 1, (HEATMAP[0] - 2, HEATMAP[1] - 2))
            if name == "Z":
                peaks[t, s, :, 0] = 0                                  # image x = 0 for every joint: no box
            if (name, t) in low:
                heights[t, s] = LOW
            preds[s] = predictions(peaks[t, s], heights[t, s], c, sc)
            score[s] = keypoint_score(heights[t, s])
        frame = dict(ids=ids.copy(), preds=preds, score=score, born=born)
        frame["died"] = track_ref.death_and_merge(ids, misses, pose, area, preds, score, par, margins)
        frame["names"] = [names.get(i) for i in frame["ids"]]
        expected.append(frame)
    return dict(dets=dets, peaks=peaks, heights=heights, expected=expected, margins=margins)


def peak_maps(case):
    """float32 [T, M, K, h, w]: FixedPeaks' Gaussians (sigma 2) at the script's peaks"""
    pos, peak = case["peaks"], case["heights"]
    ys = np.arange(HEATMAP[1], dtype=np.float64).reshape(1, 1, 1, -1, 1)
    xs = np.arange(HEATMAP[0], dtype=np.float64).reshape(1, 1, 1, 1, -1)
    d2 = (xs - pos[..., 0, None, None]) ** 2 + (ys - pos[..., 1, None, None]) ** 2
    return (peak[..., None, None] * np.exp(-d2 / (2 * 2.0 ** 2))).astype(np.float32)


class ScriptedPeaks(torch.nn.Module):
    """Returns, whatever its input, the heat-maps of frame number `calls` of a script (refine_cases.FixedPeaks per frame)."""

    def __init__(self, maps):
        super().__init__()
        self.register_buffer("maps", torch.as_tensor(maps))
        self.calls = 0

    def forward(self, x):
        assert x.shape[0] == self.maps.shape[1]
        out = self.maps[self.calls % self.maps.shape[0]].clone()
        self.calls += 1
        return out


def compare_frames(got, want, what, preds_tol=0.0, score_tol=0.0):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        for k in ("ids", "born", "died"):
            assert np.array_equal(g[k], w[k]), f"{what} frame {t}: {k} {g[k]} != {w[k]}"
        assert g["ids"].dtype == np.int64 and g["born"].dtype == bool and g["died"].dtype == bool
        dp = np.abs(g["preds"][:, :, :2].astype(np.float64) - w["preds"][:, :, :2]).max()
        ds = np.abs(g["score"] - w["score"]).max()
        print(f"{what} frame {t}: preds {dp:.3e} px, score {ds:.3e}")
        assert dp <= preds_tol and ds <= score_tol, f"{what} frame {t}: preds {dp:.3e} px, score {ds:.3e}"
        assert np.array_equal(g["preds"][:, :, 2], w["preds"][:, :, 2]), f"{what} frame {t}: maxvals"


# ---- one buctd_track_step call ------------------------------------------------------------------------------------------
STEP_SIZES = [(1, 14, 0), (4, 14, 3), (5, 17, 7), (64, 17, 64), (3, 32, 2)]


@functools.lru_cache(maxsize=None)
def step_case(Ms, K, D):
    """Slots: about two thirds live, each with the box of a random pose; slot 1 (where there is one) decodes to the same
    pose as slot 0 and is younger: merged away; the last live slot scores below death_score with one miss on its record.
    Detections: copies of live slots' poses a few pixels off (covered), pairs of near-copies of each other, and new ones -
    more than there are free slots when D is large."""
    rng = np.random.RandomState(7 * Ms + K + D)
    live = np.array([s < 2 or s % 3 != 2 for s in range(Ms)])
    ids = np.where(live, rng.permutation(Ms) + 5, -1).astype(np.int32)
    if Ms > 1:
        ids[0], ids[1] = 2, 3
    next_id = int(Ms + 5)
    misses = np.zeros(Ms, dtype=np.int32)
    centres = np.stack([rng.uniform(40, IW - 40, Ms), rng.uniform(50, IH - 50, Ms)], axis=1)
    if Ms > 1:
        centres[1] = centres[0]
    center, scale = np.zeros((Ms, 2), dtype=np.float32), np.zeros((Ms, 2), dtype=np.float32)
    state_pose = np.zeros((Ms, K, 3))
    shape0 = _shape(np.random.RandomState(1), K)
    for s in range(Ms):
        state_pose[s] = _pose(centres[s], shape0 if s < 2 else _shape(rng, K), 0.5)
        center[s], scale[s] = box_cs(state_pose[s]) if live[s] else empty_cs()
    coords = np.stack([rng.randint(2, HEATMAP[0] - 2, (Ms, K)), rng.randint(2, HEATMAP[1] - 2, (Ms, K))], axis=2).astype(np.float32)
    if Ms > 1:
        coords[1] = coords[0]
    maxvals = (0.3 + 0.6 * rng.rand(Ms, K, 1)).astype(np.float32)
    last = int(np.nonzero(live)[0][-1])
    if last > 1:
        maxvals[last], misses[last] = 0.15, 1
    offset = rng.choice([-0.25, 0.0, 0.25], (Ms, K, 2)).astype(np.float32)
    host_preds = np.stack([predictions(coords[s] + offset[s], maxvals[s], center[s], scale[s]) for s in range(Ms)])
    dets = np.zeros((D, K, 3))
    live_slots = np.nonzero(live)[0]
    for d in range(D):
        kind = d % 4
        if kind == 0 and d // 4 < len(live_slots):                      # covered by a track
            dets[d] = host_preds[live_slots[d // 4]]
            dets[d][:, :2] += rng.uniform(-2, 2, (K, 2))
            dets[d][:, 2] = rng.uniform(0.3, 0.9)
        elif kind == 1 and d >= 4:                                      # a near-copy of the detection before the last new one
            dets[d] = dets[d - 2]
            dets[d][:, :2] += rng.uniform(-2, 2, (K, 2))
            dets[d][:, 2] = rng.uniform(0.3, 0.9)
        else:
            dets[d] = _pose((rng.uniform(40, IW - 40), rng.uniform(50, IH - 50)), _shape(rng, K), rng.uniform(0.3, 0.9))
    return dict(ids=ids, misses=misses, next_id=next_id, center=center, scale=scale, state_pose=state_pose, coords=coords,
                maxvals=maxvals, offset=offset, host_preds=host_preds, dets=dets, live=live)


def step_expected(case, preds, K):
    """Everything after the predictions, from track_ref and the pipeline's host functions, for the float32 predictions it
    is given (the kernel's own: see tests/test_gpu_refine_step.py)."""
    from buctd_amd.utils.transforms import affine_transform, get_affine_transform
    par = ref_params(K)
    margins = track_ref.Margins()
    ids, misses = case["ids"].astype(np.int64), case["misses"].astype(np.int64)
    Ms = ids.shape[0]
    pose, area = case["state_pose"].copy(), np.zeros(Ms)
    score = np.array([keypoint_score(case["maxvals"][s]) if ids[s] >= 0 else 0.0 for s in range(Ms)])
    died = track_ref.death_and_merge(ids, misses, pose, area, preds, score, par, margins)
    born, next_id = track_ref.birth(ids, pose, area, case["next_id"], case["dets"], par, margins)
    center, scale = np.zeros((Ms, 2), dtype=np.float32), np.zeros((Ms, 2), dtype=np.float32)
    mats, cond = np.zeros((Ms, 2, 3)), np.zeros((Ms, K, 2))
    for s in range(Ms):
        center[s], scale[s] = box_cs(pose[s]) if ids[s] >= 0 else empty_cs()
        mats[s] = get_affine_transform(center[s], scale[s], 0, np.array(CROP))
        if ids[s] >= 0:
            cond[s] = np.stack([affine_transform(pose[s][k, :2], mats[s]) for k in range(K)])
    return dict(score=score, died=died, born=born, ids=ids, misses=misses, next_id=next_id, center=center, scale=scale,
                mats=mats, cond=cond, pose=pose, margins=margins)
