"""Post-evaluation suppression - drop-in for reference lib/nms/nms.py:17-200 plus the two native extensions it imports
(lib/nms/cpu_nms.pyx -> buctd_cpu_nms, host C++; lib/nms/gpu_nms.pyx + nms_kernel.cu -> buctd_nms, HIP).  Same function
names and return conventions.  None of this runs on the BUCTD path itself (keep = [] there); it serves detector-box
evaluation.  The OKS functions evaluate a whole candidate set per step as one numpy expression
instead of the reference's per-candidate Python loop."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def py_nms_wrapper(thresh):
    return lambda dets: nms(dets, thresh)


def cpu_nms_wrapper(thresh):
    return lambda dets: cpu_nms(dets, thresh)


def gpu_nms_wrapper(thresh, device_id):
    return lambda dets: gpu_nms(dets, thresh, device_id)


def _iou_one_to_many(box, others):
    """IoU with the +1 pixel convention of box [4] against others [m, 4]."""
    w = np.maximum(0.0, np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]) + 1)
    h = np.maximum(0.0, np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]) + 1)
    inter = w * h
    area = lambda b: (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1)
    return inter / (area(box) + area(others) - inter)


def nms(dets, thresh):
    """Greedy NMS on [[x1, y1, x2, y2, score]]: walk the boxes by descending score, drop every later box whose IoU with
    a kept one exceeds thresh.  Returns the kept indices (into dets) in score order."""
    if dets.shape[0] == 0:
        return []
    remaining = dets[:, 4].argsort()[::-1]
    keep = []
    while remaining.size:
        head, rest = remaining[0], remaining[1:]
        keep.append(head)
        remaining = rest[_iou_one_to_many(dets[head, :4], dets[rest, :4]) <= thresh]
    return keep


def cpu_nms(dets, thresh):
    """lib/nms/cpu_nms.pyx:20-71 (float32 arithmetic, suppression at IoU >= thresh) through the host C++ entry point."""
    from .._C import check, lib
    d = np.ascontiguousarray(dets, dtype=np.float32)
    n = d.shape[0]
    if n == 0:
        return []
    order = np.ascontiguousarray(d[:, 4].argsort()[::-1], dtype=np.int32)
    keep = np.zeros(n, dtype=np.int32)
    num = C.c_int(0)
    check(lib().buctd_cpu_nms(d.ctypes.data_as(C.c_void_p), n, order.ctypes.data_as(C.c_void_p), float(thresh),
                              keep.ctypes.data_as(C.c_void_p), C.byref(num)), "cpu_nms")
    return [int(i) for i in keep[:num.value]]


def gpu_nms(dets, thresh, device_id=0):
    """lib/nms/gpu_nms.pyx:19-33: sort by score, suppression mask + greedy sweep on the device (buctd_nms)."""
    import torch
    from .. import ops
    from .._C import check, lib, ptr, stream_ptr
    n = dets.shape[0]
    if n == 0:
        return []
    dev = torch.device("cuda", device_id)
    with torch.cuda.device(dev):
        d = torch.as_tensor(np.ascontiguousarray(dets, dtype=np.float32)).to(dev) if not torch.is_tensor(dets) \
            else dets.to(dev, torch.float32).contiguous()
        order = torch.argsort(d[:, 4], descending=True, stable=True)
        boxes = d[order].contiguous()
        keep = torch.empty(n, dtype=torch.int32, device=dev)
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = ops.workspace(lib().buctd_nms_workspace(n), dev)
        check(lib().buctd_nms(ptr(keep), ptr(num), ptr(boxes), n, boxes.shape[1], float(thresh), ptr(ws), ws.numel(),
                              stream_ptr()), "nms")
        k = int(num.item())
        return [int(i) for i in order[keep[:k].long()].cpu()]


def oks_iou(g, d, a_g, a_d, sigmas=None, in_vis_thre=None):
    """Object-keypoint similarity of pose g [3K] against poses d [m, 3K] (areas a_g, a_d [m]).  With in_vis_thre only
    the joints whose score in d exceeds it count (the reference's `list(vg > t) and list(vd > t)` evaluates to the
    second list, nms.py:90 - kept)."""
    if not isinstance(sigmas, np.ndarray):
        sigmas = COCO_SIGMAS
    variances = (sigmas * 2) ** 2
    d = np.asarray(d)
    if d.shape[0] == 0:
        return np.zeros(0)
    dx = d[:, 0::3] - g[0::3]
    dy = d[:, 1::3] - g[1::3]
    scale = (a_g + np.asarray(a_d, dtype=np.float64)) / 2 + np.spacing(1)
    e = (dx ** 2 + dy ** 2) / variances / scale[:, None] / 2
    sim = np.exp(-e)
    if in_vis_thre is None:
        return sim.sum(1) / sim.shape[1]
    counted = d[:, 2::3] > in_vis_thre
    n = counted.sum(1)
    return np.where(n > 0, (sim * counted).sum(1) / np.maximum(n, 1), 0.0)


def _db_arrays(kpts_db):
    scores = np.array([p['score'] for p in kpts_db])
    kpts = np.array([p['keypoints'].flatten() for p in kpts_db])
    areas = np.array([p['area'] for p in kpts_db])
    return scores, kpts, areas


def oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None):
    """Greedy suppression with OKS as the overlap: keep the best-scoring pose, drop poses with OKS > thresh to it."""
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    remaining = scores.argsort()[::-1]
    keep = []
    while remaining.size:
        head, rest = remaining[0], remaining[1:]
        keep.append(head)
        remaining = rest[oks_iou(kpts[head], kpts[rest], areas[head], areas[rest], sigmas, in_vis_thre) <= thresh]
    return keep


def oks_merge(kpts_db_mode0, kpts_db_mode1, min_oks_thres=0.5, sigmas=None, in_vis_thre=None):
    """Append to mode-1 detections every mode-0 pose whose best OKS against the ORIGINAL mode-1 set is <= min_oks_thres
    (the returned list is kpts_db_mode1 itself, extended in place, like the reference)."""
    if len(kpts_db_mode1) == 0:
        return kpts_db_mode0
    _, k0, a0 = _db_arrays(kpts_db_mode0)
    _, k1, a1 = _db_arrays(kpts_db_mode1)
    for i in range(len(k0)):
        if oks_iou(k0[i], k1, a0[i], a1, sigmas, in_vis_thre).max() <= min_oks_thres:
            kpts_db_mode1.append(kpts_db_mode0[i])
    return kpts_db_mode1


def rescore(overlap, scores, thresh, type='gaussian'):
    assert overlap.shape[0] == scores.shape[0]
    if type == 'linear':
        hit = overlap >= thresh
        scores[hit] = scores[hit] * (1 - overlap[hit])
        return scores
    return scores * np.exp(-overlap ** 2 / thresh)


def soft_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None):
    """Soft suppression: the scores of the remaining poses decay with their OKS to the pose just taken; at most 20
    poses are returned."""
    if len(kpts_db) == 0:
        return []
    scores, kpts, areas = _db_arrays(kpts_db)
    order = scores.argsort()[::-1]
    scores = scores[order]
    limit = 20
    keep = []
    while order.size and len(keep) < limit:
        head, order = order[0], order[1:]
        decayed = rescore(oks_iou(kpts[head], kpts[order], areas[head], areas[order], sigmas, in_vis_thre), scores[1:],
                          thresh)
        rank = decayed.argsort()[::-1]
        order, scores = order[rank], decayed[rank]
        keep.append(head)
    return np.array(keep, dtype=np.intp)


# ---- grouped OKS operations on the device (csrc/keypoint_eval.hip, csrc/oks_merge.hip)
def _pose_set(kpts, areas, sigmas, in_vis_thre, scores=None, offsets=None):
    """A pose set as every grouped kernel takes it, checked, then staged on kpts.device: kpts float32 [N][K][3], areas /
    scores fp64 [N], sigmas fp64 [K], offsets int32 [images + 1] (scores, offsets: None stays None), N, K, images (of
    offsets) and vis, the kernels' (use_vis, in_vis_thre) argument pair."""
    import torch
    if kpts.dim() != 3 or kpts.shape[2] != 3:
        raise ValueError(f"kpts is {tuple(kpts.shape)}, expected [N, K, 3]")
    N, K = int(kpts.shape[0]), int(kpts.shape[1])
    sizes = {name: t.numel() for name, t in dict(areas=areas, scores=scores, sigmas=sigmas, offsets=offsets).items()
             if t is not None}
    fits = lambda name, n: n >= 1 if name == 'offsets' else n == (K if name == 'sigmas' else N)
    if not all(fits(name, n) for name, n in sizes.items()):
        raise ValueError(" / ".join(f"{name} ({n})" for name, n in sizes.items())
                         + f" do not describe {N} persons with {K} key points")
    stage = lambda t, dtype: t if t is None else t.to(kpts.device, dtype).contiguous()
    use_vis = in_vis_thre is not None
    return SimpleNamespace(N=N, K=K, images=sizes.get('offsets', 0) - 1, kpts=stage(kpts, torch.float32),
                           areas=stage(areas, torch.float64), scores=stage(scores, torch.float64),
                           sigmas=stage(sigmas, torch.float64), offsets=stage(offsets, torch.int32),
                           vis=(int(use_vis), float(in_vis_thre) if use_vis else 0.0))


def oks_nms_grouped(offsets, kpts, areas, sigmas, thresh, *, in_vis_thre=None, max_per_image=None):
    """OKS suppression (oks_nms) of every image at once (buctd_oks_nms_grouped, one wavefront per image).  Device tensors:
    offsets int32 [images + 1] (CSR of the groups), kpts float32 [N][K][3] and areas fp64 [N] in grouped order, within an
    image by descending score, sigmas fp64 [K].  max_per_image, the largest group's size, sizes the kernel's LDS bitmap;
    None reads it from offsets, which waits for the device: a caller that has the counts on the host passes it.  Returns
    keep int32 [N]: 0 where the OKS to a kept, better-scored person of the image exceeds thresh, else 1."""
    import torch
    from .._C import check, lib, ptr, stream_ptr
    s = _pose_set(kpts, areas, sigmas, in_vis_thre, offsets=offsets)
    with torch.cuda.device(kpts.device):
        keep = torch.ones(s.N, dtype=torch.int32, device=kpts.device)
        if s.N and s.images:
            if max_per_image is None:
                max_per_image = (s.offsets[1:] - s.offsets[:-1]).max()
            check(lib().buctd_oks_nms_grouped(ptr(s.offsets), s.images, int(max_per_image), ptr(s.kpts), ptr(s.areas),
                                              ptr(s.sigmas), s.K, float(thresh), *s.vis, ptr(keep), stream_ptr()),
                  "oks_nms_grouped")
    return keep


def soft_oks_nms_grouped(offsets, kpts, areas, scores, sigmas, thresh, *, decay='gaussian', in_vis_thre=None,
                         max_keep=20):
    """Soft OKS suppression of every image at once (buctd_soft_oks_nms_grouped, one wavefront per image).  Device
    tensors: offsets int32 [images + 1] (CSR of the groups), kpts float32 [N][K][3], areas / scores fp64 [N] in grouped
    order, sigmas fp64 [K].  Returns (rank, soft_score): rank int32 [N], the round in which a person was taken (-1: never;
    at most max_keep per image); soft_score fp64 [N], its live score at that moment, or after the last round.  In every
    round the head is the untaken person with the largest live score, the lowest position among equal ones."""
    import torch
    from .._C import check, lib, ptr, stream_ptr
    if decay not in ('gaussian', 'linear'):
        raise ValueError(f"decay is 'gaussian' or 'linear', not {decay!r}")
    s = _pose_set(kpts, areas, sigmas, in_vis_thre, scores, offsets)
    with torch.cuda.device(kpts.device):
        rank = torch.full((s.N,), -1, dtype=torch.int32, device=kpts.device)
        soft_score = s.scores.clone()
        if s.N and s.images:
            check(lib().buctd_soft_oks_nms_grouped(ptr(s.offsets), s.images, ptr(s.kpts), ptr(s.areas), ptr(s.scores),
                                                   ptr(s.sigmas), s.K, float(thresh), int(decay == 'linear'), *s.vis,
                                                   int(max_keep), ptr(soft_score), ptr(rank), stream_ptr()),
                  "soft_oks_nms_grouped")
    return rank, soft_score


def _db_pose_set(dbs, sigmas, device_id):
    """Non-empty kpts_db lists, one after the other, as one pose set on the device: kpts float32 [N][K][3], areas and
    scores fp64 [N], sigmas fp64 [K] (COCO_SIGMAS by default), and the sizes of the lists."""
    import torch
    scores, kpts, areas = (np.concatenate(a) for a in zip(*map(_db_arrays, dbs)))
    kpts = kpts.reshape(kpts.shape[0], -1, 3)
    sig = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, dtype=np.float64).reshape(-1)
    if sig.shape[0] != kpts.shape[1]:
        raise ValueError(f"sigmas has {sig.shape[0]} entries, the poses {kpts.shape[1]} key points")
    dev = torch.device("cuda", device_id)
    t = lambda a, dt: torch.as_tensor(np.array(a, dtype=dt)).to(dev)          # a copy: the caller's array may be read-only
    return t(kpts, np.float32), t(areas, np.float64), t(scores, np.float64), t(sig, np.float64), [len(db) for db in dbs]


def gpu_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None, device_id=0):
    """oks_nms on the device (oks_nms_grouped over a one-image group): the kept indices into kpts_db in score order;
    equal scores in input order.  The key points enter as float32."""
    if len(kpts_db) == 0:
        return []
    import torch
    kpts, areas, scores, sig, (n,) = _db_pose_set([kpts_db], sigmas, device_id)
    order = torch.argsort(scores, descending=True, stable=True)
    keep = oks_nms_grouped(torch.tensor([0, n], dtype=torch.int32), kpts[order], areas[order], sig, thresh,
                           in_vis_thre=in_vis_thre, max_per_image=n)
    return [int(i) for i in order[keep != 0].cpu()]


def gpu_soft_oks_nms(kpts_db, thresh, sigmas=None, in_vis_thre=None, device_id=0):
    """soft_oks_nms on the device (soft_oks_nms_grouped over a one-image group): the indices into kpts_db in selection
    order, at most 20; equal live scores in input order.  The key points enter as float32."""
    if len(kpts_db) == 0:
        return []
    import torch
    kpts, areas, scores, sig, (n,) = _db_pose_set([kpts_db], sigmas, device_id)
    order = torch.argsort(scores, descending=True, stable=True)
    rank, _ = soft_oks_nms_grouped(torch.tensor([0, n], dtype=torch.int32), kpts[order], areas[order], scores[order], sig,
                                   thresh, in_vis_thre=in_vis_thre, max_keep=20)
    taken = torch.nonzero(rank >= 0).reshape(-1)
    taken = taken[torch.argsort(rank[taken])]
    return order[taken].cpu().numpy().astype(np.intp)


# ---- OKS merge of prioritised prediction sets (csrc/oks_merge.hip)
def _merge_images(cells, levels, N):
    """The number of images a cell table [images * levels + 1] describes; its values are checked, they index memory."""
    L = int(levels)
    if L <= 0:
        raise ValueError(f"levels is {levels!r}, expected at least one priority level")
    if len(cells.shape) != 1 or cells.shape[0] < 1 or (cells.shape[0] - 1) % L:
        raise ValueError(f"cells is {tuple(cells.shape)}, expected [images * {L} + 1]")
    if int(cells[0]) != 0 or int(cells[-1]) != N or bool((cells[1:] < cells[:-1]).any()):
        raise ValueError(f"cells does not ascend from 0 to the {N} persons")
    return (int(cells.shape[0]) - 1) // L


def oks_merge_levels(cells, kpts, areas, sigmas, thresh, in_vis_thre=None, levels=2):
    """`merged = level 0; for l in 1 .. levels - 1: merged = oks_merge(level l, merged)` for every image, as one host
    function on the layout of buctd_oks_merge_grouped - the statement the device is tested against.  Persons in grouped
    order (image-major, within an image level-major, level 0 the highest priority); cells int [images * levels + 1], the
    CSR offsets over the (image, level) cells; kpts [N][K][3], areas [N], sigmas [K].  Returns (keep int32 [N], max_oks
    fp64 [N], best int32 [N]): a person of level l >= 1 is kept iff its largest OKS (oks_iou, g the person, d the kept
    persons of the levels < l of its image) is <= thresh or there is no such person; max_oks is that OKS, best the
    grouped index that gave it (the lowest of equal ones); -1.0 / -1 for level 0 and where nothing precedes."""
    kpts = np.asarray(kpts, dtype=np.float64)
    if kpts.ndim != 3 or kpts.shape[2] != 3:
        raise ValueError(f"kpts is {kpts.shape}, expected [N, K, 3]")
    N, K = kpts.shape[0], kpts.shape[1]
    areas = np.asarray(areas, dtype=np.float64).reshape(-1)
    sigmas = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    if areas.shape[0] != N or sigmas.shape[0] != K:
        raise ValueError(f"areas ({areas.shape[0]}) / sigmas ({sigmas.shape[0]}) do not describe {N} persons with {K} key "
                         f"points")
    cells = np.asarray(cells, dtype=np.int64)
    images, L = _merge_images(cells, levels, N), int(levels)
    flat = kpts.reshape(N, K * 3)
    keep, max_oks, best = np.ones(N, dtype=np.int32), np.full(N, -1.0), np.full(N, -1, dtype=np.int32)
    for i in range(images):
        cell = cells[i * L:i * L + L + 1]
        merged = np.arange(cell[0], cell[1])
        for l in range(1, L):
            if merged.size:
                for c in range(cell[l], cell[l + 1]):
                    oks = oks_iou(flat[c], flat[merged], areas[c], areas[merged], sigmas, in_vis_thre)
                    at = int(np.argmax(oks))
                    keep[c], max_oks[c], best[c] = oks[at] <= thresh, oks[at], merged[at]
            level = np.arange(cell[l], cell[l + 1])
            merged = np.concatenate([merged, level[keep[level] != 0]])
    return keep, max_oks, best


def oks_merge_grouped(cells, levels, kpts, areas, sigmas, thresh, *, in_vis_thre=None):
    """OKS merge of every image and every priority level at once (buctd_oks_merge_grouped, one wavefront per image).
    Device tensors in the layout of oks_merge_levels: cells int32 [images * levels + 1], kpts float32 [N][K][3], areas
    fp64 [N], sigmas fp64 [K].  Returns (keep int32 [N], max_oks fp64 [N], best int32 [N])."""
    import torch
    from .._C import check, lib, ptr, stream_ptr
    s = _pose_set(kpts, areas, sigmas, in_vis_thre)
    N, images, L = s.N, _merge_images(cells, levels, s.N), int(levels)
    dev = kpts.device
    with torch.cuda.device(dev):
        cell_t = cells.to(dev, torch.int32).contiguous()
        keep = torch.ones(N, dtype=torch.int32, device=dev)
        max_oks = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
        best = torch.full((N,), -1, dtype=torch.int32, device=dev)
        if N and images:
            check(lib().buctd_oks_merge_grouped(ptr(cell_t), images, L, N, ptr(s.kpts), ptr(s.areas), ptr(s.sigmas), s.K,
                                                float(thresh), *s.vis, ptr(keep), ptr(max_oks), ptr(best), stream_ptr()),
                  "oks_merge_grouped")
    return keep, max_oks, best


def gpu_oks_merge(kpts_db_mode0, kpts_db_mode1, min_oks_thres=0.5, sigmas=None, in_vis_thre=None, device_id=0):
    """oks_merge on the device (oks_merge_grouped over one image with two levels: mode 1 is level 0, mode 0 the
    candidates).  Same returns: kpts_db_mode0 when mode 1 is empty, otherwise kpts_db_mode1 itself, extended in place by
    the mode-0 poses it accepts, in mode-0 order.  The key points enter as float32."""
    if len(kpts_db_mode1) == 0:
        return kpts_db_mode0
    if len(kpts_db_mode0) == 0:
        return kpts_db_mode1
    import torch
    kpts, areas, _, sig, (n1, n0) = _db_pose_set([kpts_db_mode1, kpts_db_mode0], sigmas, device_id)
    keep, _, _ = oks_merge_grouped(torch.tensor([0, n1, n1 + n0], dtype=torch.int32), 2, kpts, areas, sig, min_oks_thres,
                                   in_vis_thre=in_vis_thre)
    for i in np.flatnonzero(keep[n1:].cpu().numpy()):
        kpts_db_mode1.append(kpts_db_mode0[i])
    return kpts_db_mode1

