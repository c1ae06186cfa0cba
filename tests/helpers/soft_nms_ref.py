"""TEST INFRASTRUCTURE - plain-loop fp64 restatement of the soft OKS suppression as include/buctd_hip.h states it for
buctd_soft_oks_nms_grouped (the reference's soft_oks_nms / rescore, lib/nms/nms.py:150-200, with the re-sort of every
round written as an arg-max).  Key points are widened to fp64 before they are subtracted.  Shares no code with the
product; tests/test_soft_nms.py pins it against tests/golden/nms.npz and against the two host implementations."""
import math

SPACING1 = 2.220446049250313e-16        # np.spacing(1)


def oks(g, d, a_g, a_d, sigmas, in_vis_thre=None):
    """OKS of candidate d against head g, both [K][3] (x, y, joint score): the joints whose score in d is > in_vis_thre
    where a threshold is given (0.0 if there is none), summed in joint order."""
    scale = (float(a_g) + float(a_d)) / 2 + SPACING1
    total, count = 0.0, 0
    for j in range(len(sigmas)):
        if in_vis_thre is not None and not float(d[j][2]) > in_vis_thre:
            continue
        dx = float(d[j][0]) - float(g[j][0])
        dy = float(d[j][1]) - float(g[j][1])
        var = (float(sigmas[j]) * 2) * (float(sigmas[j]) * 2)
        total += math.exp(-((dx * dx + dy * dy) / var / scale / 2))
        count += 1
    return total / count if count > 0 else 0.0


def soft_nms(kpts, areas, scores, sigmas, thresh, decay='gaussian', in_vis_thre=None, max_keep=20):
    """One image: kpts [n][K][3], areas [n], scores [n] in the caller's order.  Returns a dict:
      rank [n]        the round in which a person was taken, -1 if it never was;
      soft_score [n]  its live score when it was taken, or after the last round;
      compared        per round the (position, live score) pairs the arg-max looked at;
      formed          every (round, head, candidate, OKS, live score after the decay) of the run."""
    assert decay in ('gaussian', 'linear')
    n = len(scores)
    live = [float(s) for s in scores]
    rank = [-1] * n
    compared, formed = [], []
    for r in range(min(n, max_keep)):
        head = -1
        looked_at = []
        for p in range(n):
            if rank[p] >= 0:
                continue
            looked_at.append((p, live[p]))
            if head < 0 or live[p] > live[head]:        # strict: the lowest position among equal live scores
                head = p
        compared.append(looked_at)
        rank[head] = r
        for c in range(n):
            if rank[c] >= 0:
                continue
            v = oks(kpts[head], kpts[c], areas[head], areas[c], sigmas, in_vis_thre)
            if decay == 'gaussian':
                live[c] = live[c] * math.exp(-(v * v) / thresh)
            elif v >= thresh:
                live[c] = live[c] * (1 - v)
            formed.append((r, head, c, v, live[c]))
    return dict(rank=rank, soft_score=live, compared=compared, formed=formed)


def selection(rank):
    """Positions in the order they were taken."""
    return [p for _, p in sorted((r, p) for p, r in enumerate(rank) if r >= 0)]
