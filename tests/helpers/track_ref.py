"""CTD tracking, the book-keeping of one frame boundary restated in numpy float64 from the rules of DESIGN.md section 21 -
birth, death, merge - independently of dataset.pipeline.SequenceTracker and of buctd_track_step.  Every OKS and score a
decision compares with a threshold is recorded, so a fixture can be checked for decisions that sit on their threshold."""
import numpy as np


class Margins:
    """|value - threshold| of every comparison made, by kind."""

    def __init__(self):
        self.seen = {"birth": [], "merge": [], "death": []}

    def note(self, kind, values, threshold):
        self.seen[kind].extend(np.abs(np.atleast_1d(np.asarray(values, dtype=np.float64)) - threshold).tolist())

    def smallest(self):
        return min((min(v) for v in self.seen.values() if v), default=np.inf)


def pose_box(pose, margin, iw, ih):
    """(x, y, w, h) around the non-zero x and the non-zero y of a pose, each widened by margin and clipped to the image;
    None without a non-zero x or without a non-zero y."""
    xs, ys = pose[:, 0][pose[:, 0] != 0], pose[:, 1][pose[:, 1] != 0]
    if xs.size == 0 or ys.size == 0:
        return None
    x0, x1 = min(max(xs.min() - margin, 0.0), iw), min(max(xs.max() + margin, 0.0), iw)
    y0, y1 = min(max(ys.min() - margin, 0.0), ih), min(max(ys.max() + margin, 0.0), ih)
    return x0, y0, x1 - x0, y1 - y0


def area_of(pose, margin, iw, ih):
    box = pose_box(np.asarray(pose, dtype=np.float64), margin, iw, ih)
    return None if box is None or (box[2] == 0 and box[3] == 0) else box[2] * box[3]


def oks(a, b, area_a, area_b, sigmas):
    """Object-keypoint similarity of two poses [K, 3], every joint counted."""
    var = (2.0 * np.asarray(sigmas, dtype=np.float64)) ** 2
    d2 = (a[:, 0] - b[:, 0]) ** 2 + (a[:, 1] - b[:, 1]) ** 2
    scale = (area_a + area_b) / 2 + np.spacing(1)
    return float(np.mean(np.exp(-d2 / var / scale / 2)))


def mean_score(pose):
    total = 0.0
    for v in np.asarray(pose, dtype=np.float64)[:, 2]:
        total = total + v
    return total / pose.shape[0]


def birth(ids, pose, area, next_id, dets, par, margins=None):
    """The detections of one frame against the slots (ids [M], -1 empty; pose [M, K, 3]; area [M]), all updated in place.
    par: dict(birth_oks, sigmas, margin, iw, ih).  Returns (born [M] bool, next_id)."""
    M = ids.shape[0]
    born = np.zeros(M, dtype=bool)
    dets = np.asarray(dets, dtype=np.float64).reshape(-1, pose.shape[1], 3)
    means = [mean_score(d) for d in dets]
    order = sorted(range(len(means)), key=lambda i: (-means[i], i))
    for i in order:
        a = area_of(dets[i], par["margin"], par["iw"], par["ih"])
        if a is None:
            continue
        values = [oks(dets[i], pose[s], a, area[s], par["sigmas"]) for s in range(M) if ids[s] >= 0]
        if margins is not None:
            margins.note("birth", values, par["birth_oks"])
        if values and max(values) >= par["birth_oks"]:
            continue
        free = [s for s in range(M) if ids[s] < 0]
        if not free:
            continue
        s = free[0]
        ids[s], pose[s], area[s], born[s] = next_id, dets[i], a, True
        next_id += 1
    return born, next_id


def death_and_merge(ids, misses, pose, area, preds, score, par, margins=None):
    """After the forward pass of a frame: preds [M, K, 3] and score [M] of the slots.  par adds death_score, max_misses,
    merge_oks.  ids, misses, pose, area are updated in place.  Returns died [M] bool."""
    M = ids.shape[0]
    died = np.zeros(M, dtype=bool)
    live = [s for s in range(M) if ids[s] >= 0]
    for s in live:
        pose[s] = np.asarray(preds[s], dtype=np.float64)
        a = area_of(pose[s], par["margin"], par["iw"], par["ih"])
        if a is None:
            died[s] = True
            continue
        area[s] = a
        if margins is not None:
            margins.note("death", score[s], par["death_score"])
        misses[s] = misses[s] + 1 if score[s] < par["death_score"] else 0
        died[s] = misses[s] >= par["max_misses"]
    kept = []
    for s in sorted((s for s in live if not died[s]), key=lambda s: ids[s]):
        values = [oks(pose[s], pose[q], area[s], area[q], par["sigmas"]) for q in kept]
        if margins is not None:
            margins.note("merge", values, par["merge_oks"])
        if values and max(values) >= par["merge_oks"]:
            died[s] = True
        else:
            kept.append(s)
    ids[died], misses[died] = -1, 0
    return died
