"""TEST INFRASTRUCTURE - the seeded case table of the OKS merge (tests/test_oks_merge.py, tests/test_gpu_oks_merge.py) in
the grouped layout of buctd_oks_merge_grouped: L = 3 levels, ten images in one call.

  a  no persons at all
  b  level 0 only
  c  level 1 only: nothing accepted precedes, all kept with max_oks -1
  d  1 against 1, an exact duplicate: OKS exactly 1.0 - dropped at thresh 0.5, kept at thresh 1.0
  e  70 candidates against 3 accepted: more candidates than lanes
  f  3 candidates against 70 accepted (nothing is staged in chunks: there is no boundary to cross)
  g  the chain.  Level 0: A.  Level 1: X, 0.6 pose sizes from A (accepted at 0.5), and R, close to A with three times
     A's area (rejected at 0.5).  Level 2: a duplicate of X (dropped); a duplicate of R's key points with a twentieth of
     A's area, which shrinks the OKS scale (kept: R takes no part, and against A alone it stays below 0.5); two poses
     that duplicate each other and nothing else (both kept: one level is never compared with itself)
  h  two identical accepted poses, one candidate near them: best is the lower index
  i  an accepted pose with every joint score below VIS_THRE and a candidate on the same key points with every joint score
     above it: with in_vis_thre the OKS is 0 and the candidate is kept; the other direction of the test would give 1.0
  j  a candidate 1e6 px away: every exp underflows, the OKS is exactly 0.0 - kept at thresh 0.0

Poses are float32 [K][3]; all other poses of an image lie within 0.6 pose sizes of an accepted one, so that no OKS but the
exact 0.0 of j (and of i with in_vis_thre) comes near 0."""
import numpy as np

from tests.helpers.kpt_eval_cases import COCO_SIGMAS

L = 3
VIS_THRE = 0.2
IMAGES = 'abcdefghij'
# name -> (K, seed, sigmas, thresh, in_vis_thre)
CONFIGS = {
    'k17': (17, 41, COCO_SIGMAS, 0.5, None),
    'k14_vis': (14, 42, np.array([0.1] * 14), 0.5, VIS_THRE),
    'k5': (5, 43, np.array([0.1] * 5), 0.5, None),
    'k17_vis_thresh1': (17, 41, COCO_SIGMAS, 1.0, VIS_THRE),
    'k5_thresh0': (5, 43, np.array([0.1] * 5), 0.0, None),
}


def _oks(g, d, sigmas):
    """Plain OKS of two (xy float32 [K][2], joint scores, area) poses without a joint-score threshold, for the search in g."""
    e = ((d[0].astype(np.float64) - g[0].astype(np.float64)) ** 2).sum(1) / (np.asarray(sigmas) * 2) ** 2 \
        / ((g[2] + d[2]) / 2 + np.spacing(1)) / 2
    return float(np.exp(-e).mean())


class _Poses:
    def __init__(self, K, seed):
        self.K, self.rng = K, np.random.RandomState(seed)

    def scores(self):
        return self.rng.rand(self.K) * 0.9 + 0.1

    def new(self, center, size):
        xy = np.asarray(center, dtype=np.float64) + self.rng.randn(self.K, 2) * size * 0.3
        return (xy.astype(np.float32), self.scores(), size * size * (0.8 + 0.4 * self.rng.rand()), size)

    def near(self, pose, noise):
        xy = pose[0].astype(np.float64) + self.rng.randn(self.K, 2) * noise * pose[3]
        return (xy.astype(np.float32), self.scores(), pose[3] ** 2 * (0.8 + 0.4 * self.rng.rand()), pose[3])

    def dup(self, pose, area=None, scores=None):
        return (pose[0].copy(), self.scores() if scores is None else scores, pose[2] * 1.1 if area is None else area, pose[3])


def _search(draw, accept):
    for _ in range(1000):
        x = draw()
        if accept(x):
            return x
    raise AssertionError("the seeded stream holds no such pose")


def _images(K, seed, sigmas):
    """{letter: [level 0, level 1, level 2]}, a level being a list of poses."""
    p = _Poses(K, seed)
    rng = p.rng
    spot = lambda: rng.rand(2) * 1500 + 250
    noises = (0.02, 0.05, 0.1, 0.2, 0.35, 0.6)
    im = {'a': [[], [], []]}
    im['b'] = [[p.new(spot(), 60.0) for _ in range(3)], [], []]
    im['c'] = [[], [p.new(spot(), 40.0) for _ in range(4)], []]
    d0 = p.new(spot(), 90.0)
    im['d'] = [[d0], [p.dup(d0)], []]
    e0 = [p.new(spot(), s) for s in (40.0, 90.0, 200.0)]
    im['e'] = [e0, [p.near(e0[i % 3], noises[i % 6]) for i in range(70)], []]
    centers = [p.new(spot(), s) for s in (28.0, 60.0, 120.0, 90.0, 40.0)]
    f0 = centers + [p.near(centers[i % 5], noises[(i // 5) % 6]) for i in range(65)]
    im['f'] = [f0, [p.near(f0[69], 0.02), p.near(f0[1], 0.35), p.near(f0[33], 0.1)], []]
    # g: search the seeded stream for an X below and an (R, small-area duplicate) pair on both sides of 0.5, well clear of it
    A = p.new(spot(), 100.0)
    X = _search(lambda: p.near(A, 0.6), lambda x: _oks(x, A, sigmas) < 0.4)

    def rejected_pair():
        r = p.near(A, (0.03, 0.05, 0.08, 0.12, 0.15)[rng.randint(5)])
        r = (r[0], r[1], A[2] * 3.0, r[3])
        return r, p.dup(r, area=A[2] / 20.0)
    R, R2 = _search(rejected_pair, lambda q: _oks(q[0], A, sigmas) > 0.6 and _oks(q[1], A, sigmas) < 0.4
                    and _oks(q[1], X, sigmas) < 0.4)
    T = _search(lambda: p.near(A, 0.6), lambda x: max(_oks(x, A, sigmas), _oks(x, X, sigmas)) < 0.4)
    im['g'] = [[A], [X, R], [p.dup(X), R2, T, p.dup(T)]]
    h0 = p.new(spot(), 60.0)
    im['h'] = [[h0, (h0[0].copy(), h0[1].copy(), h0[2], h0[3])], [p.near(h0, 0.05)], []]
    i0 = p.new(spot(), 90.0)
    i0 = (i0[0], rng.rand(K) * 0.1 + 0.05, i0[2], i0[3])
    im['i'] = [[i0], [p.dup(i0, scores=rng.rand(K) * 0.5 + 0.4)], []]
    j0 = p.new(spot(), 60.0)
    far = ((j0[0].astype(np.float64) + 1.0e6).astype(np.float32), p.scores(), j0[2], j0[3])
    im['j'] = [[j0], [far], []]
    return im


_cache = {}


def table(name):
    """dict(K, sigmas, thresh, in_vis_thre, cells int32 [10 * L + 1], kpts float32 [N][K][3], areas fp64 [N],
    cell: {letter: the L + 1 offsets of the image})."""
    if name not in _cache:
        K, seed, sigmas, thresh, vis = CONFIGS[name]
        im = _images(K, seed, sigmas)
        kpts, areas, cells, cell = [], [], [0], {}
        for letter in IMAGES:
            start = len(cells) - 1
            for level in im[letter]:
                for xy, js, area, _ in level:
                    kpts.append(np.concatenate([xy, js[:, None].astype(np.float32)], 1))
                    areas.append(area)
                cells.append(len(kpts))
            cell[letter] = cells[start:start + L + 1]
        t = dict(K=K, sigmas=np.asarray(sigmas, dtype=np.float64), thresh=thresh, in_vis_thre=vis,
                 cells=np.array(cells, dtype=np.int32), kpts=np.asarray(kpts, dtype=np.float32).reshape(-1, K, 3),
                 areas=np.asarray(areas, dtype=np.float64), cell=cell)
        for k in ('sigmas', 'cells', 'kpts', 'areas'):
            t[k].setflags(write=False)
        _cache[name] = t
    return _cache[name]


def reference(name):
    """(keep, max_oks, best) of nms.oks_merge_levels on a table, computed once and read-only."""
    key = ('ref', name)
    if key not in _cache:
        from buctd_amd.nms.nms import oks_merge_levels
        t = table(name)
        out = oks_merge_levels(t['cells'], t['kpts'], t['areas'], t['sigmas'], t['thresh'], t['in_vis_thre'], levels=L)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def pose_lists(name):
    """Per image (in table order) its L levels as fresh lists of pose dicts like lib/nms/nms.py takes them; 'index' is the
    grouped index of a pose."""
    t = table(name)
    out = []
    for n, letter in enumerate(IMAGES):
        c = t['cells'][n * L:n * L + L + 1]
        out.append([[{'keypoints': t['kpts'][p].astype(np.float64), 'score': float(t['kpts'][p][:, 2].mean()),
                      'area': float(t['areas'][p]), 'index': p} for p in range(c[l], c[l + 1])] for l in range(L)])
    return out
