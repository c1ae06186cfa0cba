"""TEST INFRASTRUCTURE - inputs for the pose error diagnosis tests (tests/test_error_diagnosis.py on the CPU,
tests/test_gpu_error_diagnosis.py on the device), numpy only.

seeded(dataset, B, K, M, seed)  random persons with unlabelled joints, absent predictions, joints whose partner is
    unlabelled, neighbours with visibility 0, num_valid on each side of every row threshold of the data set and
    num_overlap 0 / 3; predictions are placed around a randomly chosen source at 0 ... 1.6 d50, so every code occurs.
spread(...)  the closed-loop layout: crowdpose, one neighbour, every source at least 10 px from every other with
    area 1 (d10 <= 0.46 px: more than 2 d10 apart), so every error type is feasible for every joint and the synthesiser's
    renormalisation is the identity wherever every type is eligible.  Labelled sets are whole symmetric pairs (and
    joints 12 + 13, which have no partner), so every labelled joint with a partner can be inverted."""
import functools
import math

import numpy as np

from tests.helpers import error_types_ref as ref

GENERIC_PAIRS_32 = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (30, 31)]
SHAPES = [("crowdpose", 1, 14, 0), ("coco", 3, 17, 2), ("fish", 5, 5, 31), ("crowdpose", 65, 14, 1), ("fish", 4, 32, 3)]


def pairs_of(dataset, K):
    return GENERIC_PAIRS_32 if (dataset not in ("coco", "crowdpose") and K == 32) else None


def nv_cycle(T, K):
    """num_valid values on each side of every row threshold of the tables (those that K allows), and K itself."""
    marks = {T["jitter_nv"], T["miss_nv"][0], T["miss_nv"][1], T["crowd"][0][0], T["crowd"][1][0]}
    return sorted({min(max(v, 1), K) for m in marks for v in (m, m + 1)} | {K})


@functools.lru_cache(maxsize=None)
def seeded(dataset, B, K, M, seed=0):
    T = ref.tables(dataset, K, pairs_of(dataset, K))
    rng = np.random.RandomState(1000 * seed + 17 * B + K + M)
    cyc = nv_cycle(T, K)
    J = np.zeros((B, K, 3))
    J[:, :, :2] = 50 + rng.rand(B, K, 2) * 200
    for b in range(B):
        nv = cyc[(b + seed) % len(cyc)] if B > 1 else min(K, 11)
        J[b, rng.permutation(K)[:nv], 2] = 1 + (b % 2)                    # visibility 1 or 2
    near = np.zeros((B, M, K, 3))
    near[:, :, :, :2] = 50 + rng.rand(B, M, K, 2) * 200
    near[:, :, :, 2] = (rng.rand(B, M, K) > 0.3) * 2.0
    if M > 1:
        near[:, M - 1] = 0.0                                              # a padded (absent) neighbour
    area = 2000 + rng.rand(B) * 6000
    ov = np.array([0 if b % 2 == 0 else 3 for b in range(B)], dtype=np.int32)
    E = np.zeros((B, K, 3))
    for b in range(B):
        for j in range(K):
            d50 = math.sqrt(-2.0 * area[b] * (2 * T["sigmas"][j]) ** 2 * math.log(0.5))
            srcs = [J[b, j, :2]]
            p = T["pair"][j]
            if p >= 0:
                srcs.append(J[b, p, :2])
            for m in range(M):
                srcs += [near[b, m, q, :2] for q in ([j] if p < 0 else [j, p]) if near[b, m, q, 2] > 0]
            s = srcs[rng.randint(len(srcs))] if rng.rand() < 0.5 else srcs[0]
            r, ang = rng.rand() * 1.6 * d50, rng.rand() * 2 * math.pi
            E[b, j] = (s[0] + r * math.cos(ang), s[1] + r * math.sin(ang), 0.7)
            if rng.rand() < 0.08:
                E[b, j] = 0.0                                              # an absent prediction
    for a in (J, E, near, area, ov):
        a.setflags(write=False)
    return dict(dataset=dataset, T=T, joints=J, estimated=E, near=near if M else None, area=area, num_overlap=ov)


@functools.lru_cache(maxsize=None)
def seeded_reference(dataset, B, K, M, seed=0):
    """The restatement's result for seeded(...), computed once (read only)."""
    c = seeded(dataset, B, K, M, seed)
    out = ref.error_types(c["T"], c["joints"], c["estimated"], c["near"], c["area"], c["num_overlap"])
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the closed-loop layout ----------------------------------------------------------------------------------------------
UNITS = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13)]         # crowdpose pairs, and the two unpaired joints
FOUR = [(6, 0), (6, 4), (1, 3)]                                            # num_valid 4: units, cycled (classes balanced)


def spread_labels(i, nv):
    """Labelled joints of person i of the group with num_valid nv (4, 8 or 14)."""
    if nv == 14:
        units = range(7)
    elif nv == 8:
        units = [6] + [(i + k) % 6 for k in range(3)]
    else:
        units = FOUR[i % 3]
    return sorted(j for u in units for j in UNITS[u])


@functools.lru_cache(maxsize=None)
def spread(groups=((4, 0, 450), (4, 3, 450), (8, 0, 287), (8, 1, 287), (14, 0, 287), (14, 3, 287))):
    """groups: (num_valid, num_overlap, persons).  Default: 2048 persons that populate every row of every crowdpose
    ladder: jitter rows by nv <= 10, miss rows by nv <= 5 / <= 10, swap rows by crowded = (nv <= 10 and ov >= 1) or
    (nv <= 15 and ov >= 3)."""
    K = 14
    B = sum(g[2] for g in groups)
    J, near = np.zeros((B, K, 3)), np.ones((B, 1, K, 3))
    J[:, :, 0] = near[:, 0, :, 0] = 100.0 + 10.0 * np.arange(K)
    J[:, :, 1], near[:, 0, :, 1] = 100.0, 200.0
    ov = np.zeros(B, dtype=np.int32)
    b = 0
    for nv, o, n in groups:
        for i in range(n):
            J[b, spread_labels(i, nv), 2] = 1.0
            ov[b] = o
            b += 1
    E = J.copy()
    E[:, :, 1] = 150.0                                                     # the own source of an unlabelled joint
    area = np.ones(B)
    for a in (J, E, near, area, ov):
        a.setflags(write=False)
    return dict(dataset="crowdpose", T=ref.tables("crowdpose", K), joints=J, estimated=E, near=near, area=area,
                num_overlap=ov)


# a ladder that is not the default and keeps jitter + miss + inversion + swap <= 0.80; inversion class 0 (joints without a
# partner) is never eligible and keeps the default's 0.01
LADDER = dict(jitter_p=[[0.32, 0.36, 0.08], [0.28, 0.32, 0.04]],
              miss_p=[[0.10, 0.12, 0.18], [0.16, 0.08, 0.20], [0.06, 0.10, 0.04]], inv_p=[0.01, 0.08, 0.02],
              swap_p=[[0.06, 0.05, 0.16], [0.04, 0.12, 0.08]])
DEFAULT = dict(jitter_p=[[0.15, 0.20, 0.25], [0.10, 0.15, 0.20]],
               miss_p=[[0.15, 0.20, 0.25], [0.10, 0.13, 0.15], [0.02, 0.05, 0.10]], inv_p=[0.01, 0.03, 0.06],
               swap_p=[[0.02, 0.15, 0.10], [0.01, 0.06, 0.03]])
TYPES = ("jitter_p", "miss_p", "inv_p", "swap_p")


def cell(lad, t, r, c):
    return lad["inv_p"][c] if t == 2 else lad[TYPES[t]][r][c]


def check_cells(hist, lad, min_eligible, want_close=True, types=(0, 1, 2, 3)):
    """Per populated cell of hist (numpy [4, 3, 3, 2]): n = eligible >= min_eligible, and hits / n within (want_close) or
    farther than (not want_close) 5 sqrt(p (1 - p) / n) of the ladder's p.  Returns the number of cells looked at."""
    seen = 0
    for t in types:
        for r in range(3):
            for c in range(3):
                hits, n = int(hist[t, r, c, 0]), int(hist[t, r, c, 1])
                if n == 0:
                    continue
                seen += 1
                assert n >= min_eligible, (t, r, c, n)
                p = cell(lad, t, r, c)
                bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
                gap = abs(hits / n - p)
                print(f"cell type {t} row {r} class {c}: n {n} freq {hits / n:.4f} p {p:.4f} gap {gap:.4f} bound {bound:.4f}")
                assert (gap <= bound) if want_close else (gap > bound), (t, r, c, hits, n, p, bound)
    return seen
