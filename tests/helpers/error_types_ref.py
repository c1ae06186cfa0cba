"""TEST INFRASTRUCTURE - plain-loop float64 restatement of the pose error diagnosis (DESIGN.md "Pose error diagnosis"),
written from the definition alone: it imports nothing of buctd_amd and carries its own per-data-set constants.

error_types(T, joints, estimated, near, area, num_overlap) -> dict(code [B, K], ks [B, K], hist [4, 3, 3, 2],
per_joint [K, 6], margin [B, K]).  margin is, per scored and present joint, the smallest relative distance of any
comparison the definition makes from its threshold: min(r0, rI, rS) against d50, r0 against d85, and the finite source
distances r0, rI, rS against each other (inf for joints that are not scored or not present).  A bit-equal pair of
distances has margin 0: exact ties are decided by the tie order and tested on their own."""
import math

import numpy as np

INF = float("inf")


def tables(dataset, K, pairs=None):
    """sigmas, pair, per-type classes and row thresholds of coco / crowdpose / the generic variant (any other name: sigma
    0.1, no classes, `pairs` = a list of (a, b) or none)."""
    if dataset == "coco":
        sig = [.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]
        sym = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
        jit = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 0, 0, 0, 0]
        miss = [0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1]
        inv = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2]
        swap = list(inv)
    elif dataset == "crowdpose":
        sig = [.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .79, .79]
        sym = [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11)]
        jit = [1, 1, 1, 1, 1, 1, 2, 2, 0, 0, 0, 0, 0, 0]
        miss = [1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 2, 2, 0, 0]
        inv = [1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 0, 0]
        swap = list(inv)
    else:
        sig, sym = [1.0] * K, list(pairs or [])
        jit = miss = inv = swap = [0] * K
    assert len(sig) == K
    pair = [-1] * K
    for a, b in sym:
        pair[a], pair[b] = b, a
    human = dataset in ("coco", "crowdpose")
    return dict(sigmas=[s / 10.0 for s in sig], pair=pair, jitter_cls=jit, miss_cls=miss, inv_cls=inv, swap_cls=swap,
                jitter_nv=10 if human else 4, miss_nv=(5, 10) if human else (2, 4),
                crowd=((10, 1), (15, 3)) if human else ((4, 1), (5, 1)))


def _dist(px, py, qx, qy):
    dx, dy = px - qx, py - qy
    return math.sqrt(dx * dx + dy * dy)


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b)) if max(abs(a), abs(b)) > 0 else 0.0


def error_types(T, joints, estimated, near, area, num_overlap):
    J, E = np.asarray(joints, dtype=np.float64), np.asarray(estimated, dtype=np.float64)
    B, K = J.shape[0], J.shape[1]
    NR = np.zeros((B, 0, K, 3)) if near is None else np.asarray(near, dtype=np.float64)
    M = NR.shape[1]
    code = np.full((B, K), -1, dtype=np.int32)
    ks = np.zeros((B, K), dtype=np.float64)
    margin = np.full((B, K), INF, dtype=np.float64)
    hist = np.zeros((4, 3, 3, 2), dtype=np.int64)
    per_joint = np.zeros((K, 6), dtype=np.int64)
    for b in range(B):
        nv = 0
        for q in range(K):
            if J[b, q, 2] > 0:
                nv += 1
        ov = int(num_overlap[b])
        a = float(area[b])
        for j in range(K):
            if not J[b, j, 2] > 0:
                continue
            px, py = float(E[b, j, 0]), float(E[b, j, 1])
            if px == 0.0 and py == 0.0:
                code[b, j] = 5
                per_joint[j, 5] += 1
                continue
            var = (2.0 * T["sigmas"][j]) * (2.0 * T["sigmas"][j])
            d85 = math.sqrt(-2.0 * a * var * math.log(0.85))
            d50 = math.sqrt(-2.0 * a * var * math.log(0.50))
            p = T["pair"][j]
            r0 = _dist(px, py, float(J[b, j, 0]), float(J[b, j, 1]))
            rI = INF
            if p >= 0 and J[b, p, 2] > 0:
                rI = _dist(px, py, float(J[b, p, 0]), float(J[b, p, 1]))
            rS, has_swap = INF, False
            for m in range(M):
                for q in ([j] if p < 0 else [j, p]):
                    if NR[b, m, q, 2] > 0:
                        has_swap = True
                        rS = min(rS, _dist(px, py, float(NR[b, m, q, 0]), float(NR[b, m, q, 1])))
            lo = min(r0, rI, rS)
            if lo >= d50:
                c = 4
            elif r0 <= rI and r0 <= rS:
                c = 0 if r0 < d85 else 1
            elif rI <= rS:
                c = 2
            else:
                c = 3
            code[b, j] = c
            per_joint[j, c] += 1
            ks[b, j] = math.exp(-(r0 * r0) / (2.0 * a * var))
            finite = [r for r in (r0, rI, rS) if r != INF]
            rels = [_rel(lo, d50), _rel(r0, d85)]
            for i in range(len(finite)):
                for k in range(i + 1, len(finite)):
                    rels.append(_rel(finite[i], finite[k]))
            margin[b, j] = min(rels)
            row_jit = 0 if nv <= T["jitter_nv"] else 1
            row_miss = 0 if nv <= T["miss_nv"][0] else (1 if nv <= T["miss_nv"][1] else 2)
            crowded = False
            for cnv, cov in T["crowd"]:
                if nv <= cnv and ov >= cov:
                    crowded = True
            row_swap = 0 if crowded else 1
            cells = [(0, row_jit, T["jitter_cls"][j], c == 1), (1, row_miss, T["miss_cls"][j], c == 4)]
            if rI != INF:
                cells.append((2, 0, T["inv_cls"][j], c == 2))
            if has_swap:
                cells.append((3, row_swap, T["swap_cls"][j], c == 3))
            for t, r, cl, hit in cells:
                hist[t, r, cl, 1] += 1
                if hit:
                    hist[t, r, cl, 0] += 1
    return dict(code=code, ks=ks, hist=hist, per_joint=per_joint, margin=margin)
