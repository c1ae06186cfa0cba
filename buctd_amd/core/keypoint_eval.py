"""Keypoint evaluation: validate()'s tables `all_preds` / `all_boxes` -> the ten COCO keypoint figures (AP first), the
step the reference's data set classes implement in `evaluate` with Python loops around lib/nms/nms.py and with
pycocotools.COCOeval (lib/dataset/dataloader.py:538-735).  No pycocotools object is involved.

What runs where
  device (csrc/keypoint_eval.hip, fp64): rescoring, OKS NMS (hard or soft) grouped by image, the per-image OKS
      matrices and the 3 x 10 greedy matchings of COCOeval.evaluateImg;
  host: grouping persons by image, the results JSON, and the accumulation over the small match tables (numpy, fp64).

A data set class opts in by delegating:
    self.evaluator = KeypointEvaluator(gt_dict, sigmas=..., image_dir=self.image_dir)
    def evaluate(self, *a, **kw): return self.evaluator.evaluate(*a, **kw)
"""
import ctypes as C
import json
import logging
import os
from collections import OrderedDict, namedtuple

import numpy as np

logger = logging.getLogger(__name__)

STATS_NAMES = ['AP', 'AP .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
# COCOeval's keypoint parameters
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)   # all, medium, large


def accumulate(dt_scores, dt_matched, dt_ignored, npig, rec_thrs=REC_THRS):
    """COCOeval.accumulate for one category and one detection limit.  dt_scores [D] in evaluation order (images by id,
    detections by score within an image), dt_matched / dt_ignored [A][T][D] (non-zero = matched / ignored), npig [A] the
    number of non-ignored ground truths per area range.  Returns precision [T][R][A] and recall [T][A]; entries of an
    area range without a non-ignored ground truth stay -1."""
    dt_scores = np.asarray(dt_scores, dtype=np.float64)
    dtm = np.asarray(dt_matched) != 0
    dti = np.asarray(dt_ignored) != 0
    A, T, D = dtm.shape
    R = len(rec_thrs)
    precision = -np.ones((T, R, A))
    recall = -np.ones((T, A))
    inds = np.argsort(-dt_scores, kind='mergesort')
    for a in range(A):
        if npig[a] == 0:
            continue
        m, ig = dtm[a][:, inds], dti[a][:, inds]
        tp_sum = np.cumsum(m & ~ig, axis=1).astype(np.float64)
        fp_sum = np.cumsum(~m & ~ig, axis=1).astype(np.float64)
        for t in range(T):
            tp, fp = tp_sum[t], fp_sum[t]
            q = np.zeros(R)
            if D == 0:
                recall[t, a] = 0
                precision[t, :, a] = q
                continue
            rc = tp / npig[a]
            pr = tp / (fp + tp + np.spacing(1))
            recall[t, a] = rc[-1]
            pr = np.maximum.accumulate(pr[::-1])[::-1]          # the precision envelope
            at = np.searchsorted(rc, rec_thrs, side='left')
            ok = at < D
            q[ok] = pr[at[ok]]
            precision[t, :, a] = q
    return precision, recall


def summarize(precision, recall):
    """The ten figures of COCOeval.summarize for key points, in the order of STATS_NAMES; -1 where nothing counts."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    half, three_q = 0, 5                                          # IOU_THRS[0] = .5, IOU_THRS[5] = .75
    return [mean(precision[:, :, 0]), mean(precision[half, :, 0]), mean(precision[three_q, :, 0]),
            mean(precision[:, :, 1]), mean(precision[:, :, 2]),
            mean(recall[:, 0]), mean(recall[half, 0]), mean(recall[three_q, 0]), mean(recall[:, 1]), mean(recall[:, 2])]


# What the suppression leaves of one prediction table, or of a merged ensemble: preds / all_boxes as checked,
# person_image_id, img (image position per person), order_h (input row of each grouped person), keep_h (mask over the
# grouped persons), offsets / counts (CSR of the groups), kp_s (the grouped key points on the device), the three score
# vectors on the host per input row and, under soft suppression, rank and live score per grouped person (else None).
KeptPersons = namedtuple('KeptPersons', 'preds all_boxes person_image_id img order_h keep_h offsets counts kp_s score_h '
                                        'box_score_h kpt_score_h soft_rank_s soft_score_s', defaults=(None, None))


class KeypointEvaluator:
    """ev = KeypointEvaluator(gt, ...); name_value, ap = ev.evaluate(cfg, preds, output_dir, all_boxes, img_path, epoch).

    gt: loaded COCO-format annotation dict (`images`, `annotations` with keypoints, num_keypoints, area, bbox, iscrowd,
    image_id, id; one category).  sigmas: per-joint OKS sigmas of the evaluation (default nms.COCO_SIGMAS);
    nms_sigmas: those of the suppression (the reference passes joints_weight / 10, dataloader.py:614-625; default: sigmas).
    use_nms=False is the BUCTD setting `keep = []`: every person is kept.  nms_in_vis_thre: joint-score threshold inside
    the suppression's OKS (the reference passes none).  suppression='soft' is TEST.SOFT_NMS: soft_oks_nms instead of
    oks_nms (dataloader.py:614-625) - at most max_dets persons per image are chosen by decayed scores (`tables` gains
    soft_rank / soft_score per input row); the scores that are written and matched stay the rescored ones.  img_path entries are mapped to image ids through `image_ids`, a
    dict or callable path -> id; by default the dict {join(image_dir, file_name): id} of gt['images'].
    `tables` holds what the last call produced.  evaluate_merged(cfg, sets, output_dir, epoch) scores an ensemble of
    prediction sets, merged per image by the reference's oks_merge on the device."""

    def __init__(self, gt, sigmas=None, nms_sigmas=None, oks_thre=0.5, in_vis_thre=0.0, use_nms=True, max_dets=20,
                 device=None, *, image_dir='', image_ids=None, soft_nms=False, nms_in_vis_thre=None, mode='val',
                 category_id=1, suppression='hard'):
        import torch
        from ..nms.nms import COCO_SIGMAS
        if soft_nms:
            raise NotImplementedError("soft_nms is not an option of the evaluator: pass suppression='soft' for the "
                                      "device's soft OKS NMS (nms.soft_oks_nms is the host form)")
        if suppression not in ('hard', 'soft'):
            raise ValueError(f"suppression is 'hard' or 'soft', not {suppression!r}")
        if suppression == 'soft' and not use_nms:
            raise ValueError("suppression='soft' needs use_nms=True: without the suppression every person is kept")
        self.suppression = suppression
        self.sigmas = np.asarray(COCO_SIGMAS if sigmas is None else sigmas, dtype=np.float64).reshape(-1)
        self.nms_sigmas = self.sigmas if nms_sigmas is None else np.asarray(nms_sigmas, dtype=np.float64).reshape(-1)
        self.K = self.sigmas.shape[0]
        if self.nms_sigmas.shape[0] != self.K:
            raise ValueError(f"nms_sigmas has {self.nms_sigmas.shape[0]} entries, sigmas {self.K}")
        self.oks_thre, self.in_vis_thre, self.nms_in_vis_thre = float(oks_thre), float(in_vis_thre), nms_in_vis_thre
        self.use_nms, self.max_dets, self.mode, self.category_id = bool(use_nms), int(max_dets), mode, category_id
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.tables = None

        images = sorted(gt['images'], key=lambda im: im['id'])
        self.image_ids = np.array([im['id'] for im in images], dtype=np.int64)
        self._image_pos = {int(i): p for p, i in enumerate(self.image_ids)}
        if image_ids is None:
            image_ids = {os.path.join(image_dir, im['file_name']): im['id'] for im in images}
        self._path_to_id = image_ids
        per_image = [[] for _ in images]
        for ann in gt['annotations']:
            per_image[self._image_pos[int(ann['image_id'])]].append(ann)
        anns = [a for group in per_image for a in group]
        for a in anns:
            if len(a['keypoints']) != 3 * self.K:
                raise ValueError(f"annotation {a['id']} has {len(a['keypoints']) // 3} key points, sigmas {self.K}")
        G = len(anns)
        self.gt_ids = np.array([a['id'] for a in anns], dtype=np.int64)
        self.gt_counts = np.array([len(g) for g in per_image], dtype=np.int64)
        self.gt_offsets = np.concatenate([[0], np.cumsum(self.gt_counts)]).astype(np.int32)
        self.gt_area = np.array([a['area'] for a in anns], dtype=np.float64).reshape(G)
        self.gt_flags = np.array([(1 if a.get('iscrowd', 0) else 0) | (2 if a['num_keypoints'] == 0 else 0) for a in anns],
                                 dtype=np.int32).reshape(G)
        # what core.keypoint_analysis reads besides the tables above: image sizes (nan where the set carries none), the
        # annotations' num_keypoints field and a stored num_overlaps (-1 where there is none)
        self.image_wh = np.array([[im.get('width', np.nan), im.get('height', np.nan)] for im in images],
                                 dtype=np.float64).reshape(len(images), 2)
        self.gt_image = np.repeat(np.arange(len(images), dtype=np.int64), self.gt_counts)
        self.gt_num_keypoints = np.array([int(a['num_keypoints']) for a in anns], dtype=np.int64).reshape(G)
        self.gt_num_overlaps = np.array([int(a.get('num_overlaps', -1)) for a in anns], dtype=np.int64).reshape(G)
        self.gt_has_num_overlaps = np.array(['num_overlaps' in a for a in anns], dtype=bool).reshape(G)
        kp = np.array([a['keypoints'] for a in anns], dtype=np.float64).reshape(G, self.K, 3)
        bb = np.array([a['bbox'] for a in anns], dtype=np.float64).reshape(G, 4)
        out = (self.gt_area[None, :] < AREA_RNG[:, :1]) | (self.gt_area[None, :] > AREA_RNG[:, 1:])
        self.npig = np.count_nonzero(~((self.gt_flags[None, :] != 0) | out), axis=1)
        dev = self.device
        self._d = dict(gt_off=torch.as_tensor(self.gt_offsets).to(dev), gt_kpts=torch.as_tensor(kp).to(dev),
                       gt_area=torch.as_tensor(self.gt_area).to(dev), gt_bbox=torch.as_tensor(bb).to(dev),
                       gt_flags=torch.as_tensor(self.gt_flags).to(dev), sigmas=torch.as_tensor(self.sigmas).to(dev),
                       nms_sigmas=torch.as_tensor(self.nms_sigmas).to(dev), thrs=torch.as_tensor(IOU_THRS).to(dev),
                       area_rng=torch.as_tensor(AREA_RNG).to(dev))

    def _image_id(self, path):
        try:
            return self._path_to_id(path) if callable(self._path_to_id) else self._path_to_id[path]
        except KeyError:
            raise KeyError(f"img_path entry {path!r} has no image id in the annotation set") from None

    def _kept_persons(self, preds, all_boxes, img_path):
        """Steps 1-2 of evaluate(), shared with core.keypoint_analysis: the tables are checked, every person is rescored,
        the persons are grouped (images by id, descending score within an image, equal scores in input order) and the
        suppression runs within every image.  Returns a KeptPersons."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        from ..nms import nms
        preds = np.ascontiguousarray(preds, dtype=np.float32)
        all_boxes = np.asarray(all_boxes, dtype=np.float64)
        N = preds.shape[0]
        if preds.ndim != 3 or preds.shape[1:] != (self.K, 3):
            raise ValueError(f"preds is {preds.shape}, expected [N, {self.K}, 3] (one sigma per joint)")
        if all_boxes.shape != (N, 7) or len(img_path) != N:
            raise ValueError(f"all_boxes {all_boxes.shape} / img_path ({len(img_path)}) do not describe {N} persons")
        person_image_id = [self._image_id(p) for p in img_path]
        try:
            img = np.array([self._image_pos[int(i)] for i in person_image_id], dtype=np.int64).reshape(N)
        except KeyError as e:
            raise KeyError(f"image id {e.args[0]} is not in the annotation set") from None
        I, K, dev, d = len(self.image_ids), self.K, self.device, self._d

        with torch.cuda.device(dev):
            # 1. rescoring
            preds_t = torch.as_tensor(preds).to(dev)
            box_in = torch.as_tensor(np.ascontiguousarray(all_boxes[:, 5])).to(dev)
            area_t = torch.as_tensor(np.ascontiguousarray(all_boxes[:, 4])).to(dev)
            score, box_score, kpt_score = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
            check(lib().buctd_kpt_rescore(ptr(preds_t), ptr(box_in), N, K, self.in_vis_thre, ptr(score), ptr(box_score),
                                          ptr(kpt_score), stream_ptr()), "kpt_rescore")
            # grouping: images by id, persons by descending score within an image, equal scores in input order
            img_t = torch.as_tensor(img).to(dev)
            by_score = torch.sort(score, descending=True, stable=True).indices
            order = by_score[torch.sort(img_t[by_score], stable=True).indices]
            counts = np.bincount(img, minlength=I)
            offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            kp_s = preds_t[order].contiguous()
            # 2. OKS NMS within every image
            keep_s, soft = torch.ones(N, dtype=torch.int32, device=dev), ()
            if self.use_nms:
                off_t = torch.as_tensor(offsets).to(dev)
                area_s = area_t[order].contiguous()
                if self.suppression == 'soft':
                    # the decayed scores choose the persons and nothing else: the reference takes indices only
                    rank_s, soft_s = nms.soft_oks_nms_grouped(off_t, kp_s, area_s, score[order], d['nms_sigmas'],
                                                              self.oks_thre, in_vis_thre=self.nms_in_vis_thre,
                                                              max_keep=self.max_dets)
                    keep_s, soft = (rank_s >= 0).to(torch.int32), (rank_s.cpu().numpy(), soft_s.cpu().numpy())
                else:
                    keep_s = nms.oks_nms_grouped(off_t, kp_s, area_s, d['nms_sigmas'], self.oks_thre,
                                                 in_vis_thre=self.nms_in_vis_thre,
                                                 max_per_image=int(counts.max(initial=0)))
            return KeptPersons(preds, all_boxes, person_image_id, img, order.cpu().numpy(),
                               keep_s.cpu().numpy().astype(bool), offsets, counts, kp_s, score.cpu().numpy(),
                               box_score.cpu().numpy(), kpt_score.cpu().numpy(), *soft)

    def _match(self, dt_kpts, dt_counts, gt_counts, gt=None):
        """Step 3 of evaluate(), shared with core.keypoint_analysis: the OKS matrices and the A x T greedy matchings of
        `images` = len(dt_counts) detection / ground-truth groups.  dt_kpts: device tensor [Dt][K][3] in group order;
        gt: the device tables gt_kpts / gt_area / gt_bbox / gt_flags in group order (default: the evaluator's own).
        Returns oks_offsets (host) and the device tensors oks, dt_matched, dt_ignored."""
        import torch
        from .. import ops
        from .._C import KptMatchArgs, check, lib, ptr, stream_ptr
        dev, d = self.device, self._d
        gt = d if gt is None else gt
        A, T = AREA_RNG.shape[0], IOU_THRS.shape[0]
        dt_counts, gt_counts = np.asarray(dt_counts, dtype=np.int64), np.asarray(gt_counts, dtype=np.int64)
        dt_offsets = np.concatenate([[0], np.cumsum(dt_counts)]).astype(np.int32)
        gt_offsets = np.concatenate([[0], np.cumsum(gt_counts)]).astype(np.int32)
        oks_offsets = np.concatenate([[0], np.cumsum(dt_counts * gt_counts)]).astype(np.int64)
        Dt, G = int(dt_offsets[-1]), int(gt_offsets[-1])
        with torch.cuda.device(dev):
            oks = torch.zeros(max(int(oks_offsets[-1]), 1), dtype=torch.float64, device=dev)
            dt_matched = torch.zeros((A, T, Dt), dtype=torch.int32, device=dev)
            dt_ignored = torch.zeros((A, T, Dt), dtype=torch.int32, device=dev)
            if Dt:
                dt_off_t = torch.as_tensor(dt_offsets).to(dev)
                gt_off_t = torch.as_tensor(gt_offsets).to(dev)
                oks_off_t = torch.as_tensor(oks_offsets).to(dev)
                ws = ops.workspace(lib().buctd_coco_kpt_match_workspace(G, T, A), dev)
                m = KptMatchArgs(images=len(dt_counts), K=self.K, n_thr=T, n_area=A, dt_total=Dt, gt_total=G,
                                 dt_offsets=ptr(dt_off_t), gt_offsets=ptr(gt_off_t), oks_offsets=ptr(oks_off_t),
                                 dt_kpts=ptr(dt_kpts), gt_kpts=ptr(gt['gt_kpts']), gt_area=ptr(gt['gt_area']),
                                 gt_bbox=ptr(gt['gt_bbox']), gt_flags=ptr(gt['gt_flags']), sigmas=ptr(d['sigmas']),
                                 thresholds=ptr(d['thrs']), area_ranges=ptr(d['area_rng']), oks=ptr(oks),
                                 dt_matched=ptr(dt_matched), dt_ignored=ptr(dt_ignored))
                check(lib().buctd_coco_kpt_match(C.byref(m), ptr(ws), ws.numel(), stream_ptr()), "coco_kpt_match")
        return oks_offsets, oks, dt_matched, dt_ignored

    def evaluate(self, cfg, preds, output_dir, all_boxes, img_path, epoch=-1, *args, **kwargs):
        return self._finish(cfg, self._kept_persons(preds, all_boxes, img_path), img_path, output_dir, epoch)

    def evaluate_merged(self, cfg, sets, output_dir, epoch=-1, *, min_oks_thres=0.5, merge_in_vis_thre=None):
        """evaluate() of an ensemble: sets = [(preds, all_boxes, img_path), ...] in priority order, each a table like
        evaluate()'s.  Every set is rescored and suppressed on its own, as configured; its kept persons are level l of
        their image, and one launch of nms.oks_merge_grouped chains the reference's oks_merge (lib/nms/nms.py:127-148)
        over the levels: a person of a later set is accepted iff its largest OKS to the accepted persons of the earlier
        sets in its image is <= min_oks_thres (areas all_boxes[:, 4], nms_sigmas - the merge is a suppression;
        merge_in_vis_thre: joint-score threshold on the accepted pose, none by default).  The accepted persons of an image
        are ordered by rescored score (equal scores: by level, then by position within the set's own order), cut at
        max_dets, matched and summarised as in evaluate(); the results file holds them, within an image in that order
        (with one set and use_nms=False: in input order, like evaluate()).  Rows are those of the concatenated sets.
        `tables` gains per row: level, merge_keep (accepted by the merge; False where the set's own suppression dropped
        the row, which then never entered the merge), merge_max_oks and merge_best (the row that gave it, or -1).
        With one set every figure, table and the results file equal evaluate()'s."""
        import torch
        from ..nms.nms import oks_merge_grouped
        sets = list(sets)
        if not sets:
            raise ValueError("evaluate_merged needs at least one (preds, all_boxes, img_path) set")
        ps = [self._kept_persons(*s) for s in sets]
        L, I, dev = len(ps), len(self.image_ids), self.device
        sizes = [q.preds.shape[0] for q in ps]
        base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        N = int(base[-1])
        cat = lambda k: np.concatenate([getattr(q, k) for q in ps])
        all_boxes, score_h = cat('all_boxes'), cat('score_h')
        # per position of the sets' grouped orders, one after the other: input row, level, position, image, kept by its set
        row_g = np.concatenate([base[l] + q.order_h for l, q in enumerate(ps)]).astype(np.int64)
        lvl_g = np.repeat(np.arange(L, dtype=np.int64), sizes)
        pos_g = np.concatenate([np.arange(n, dtype=np.int64) for n in sizes])
        img_g = np.concatenate([q.img[q.order_h] for q in ps]).astype(np.int64)
        kept_g = cat('keep_h')
        # the merge: kept persons in cells, image-major and level-major, within a cell in the set's own order
        cell_order = np.lexsort((pos_g, lvl_g, img_g))
        m_idx = cell_order[kept_g[cell_order]]
        cells = np.concatenate([[0], np.cumsum(np.bincount(img_g[m_idx] * L + lvl_g[m_idx], minlength=I * L))])
        rows_m = row_g[m_idx]
        with torch.cuda.device(dev):
            kp_g = torch.cat([q.kp_s for q in ps])
            keep_m, max_m, best_m = oks_merge_grouped(
                torch.as_tensor(cells.astype(np.int32)), L, kp_g[torch.as_tensor(m_idx).to(dev)],
                torch.as_tensor(np.ascontiguousarray(all_boxes[rows_m, 4])).to(dev), self._d['nms_sigmas'], min_oks_thres,
                in_vis_thre=merge_in_vis_thre)
            keep_m, max_m, best_m = keep_m.cpu().numpy() != 0, max_m.cpu().numpy(), best_m.cpu().numpy()
        level, merge_keep = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
        merge_max_oks, merge_best = np.full(N, -1.0), np.full(N, -1, dtype=np.int64)
        level[row_g] = lvl_g
        merge_keep[rows_m], merge_max_oks[rows_m] = keep_m, max_m
        merge_best[rows_m] = np.where(best_m >= 0, rows_m[np.maximum(best_m, 0)], -1) if rows_m.size else rows_m
        # the merged set in evaluate()'s grouped form: images by id, within an image by score, then level, then position
        accepted_g = np.zeros(N, dtype=bool)
        accepted_g[m_idx] = keep_m
        final = np.lexsort((pos_g, lvl_g, -score_h[row_g], img_g))
        counts = np.sum([q.counts for q in ps], axis=0)
        with torch.cuda.device(dev):
            kp_s = kp_g[torch.as_tensor(final).to(dev)].contiguous()
        soft = [cat(k)[final] for k in ('soft_rank_s', 'soft_score_s') if getattr(ps[0], k) is not None]
        p = KeptPersons(cat('preds'), all_boxes, [i for q in ps for i in q.person_image_id], cat('img'), row_g[final],
                        accepted_g[final], np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), counts, kp_s, score_h,
                        cat('box_score_h'), cat('kpt_score_h'), *soft)
        img_path = [path for s in sets for path in s[2]]
        return self._finish(cfg, p, img_path, output_dir, epoch, by_score=self.use_nms or L > 1,
                            extra=dict(level=level, merge_keep=merge_keep, merge_max_oks=merge_max_oks,
                                       merge_best=merge_best))

    def _finish(self, cfg, p, img_path, output_dir, epoch, by_score=None, extra=None):
        """Steps 3-5 of evaluate() on what _kept_persons returned: the detections, the matching, the figures, `tables` and
        the results file."""
        import torch
        preds, all_boxes, person_image_id = p.preds, p.all_boxes, p.person_image_id
        N, I, dev = preds.shape[0], len(self.image_ids), self.device
        order_h, keep_h, offsets, counts, score_h = p.order_h, p.keep_h, p.offsets, p.counts, p.score_h
        # detections: the kept persons of an image by score, at most max_dets
        img_s = p.img[order_h]
        rank = np.cumsum(keep_h) - keep_h
        rank = rank - np.repeat(rank[offsets[:-1][counts > 0]], counts[counts > 0])
        dt_pos = np.flatnonzero(keep_h & (rank < self.max_dets))
        dt_counts = np.bincount(img_s[dt_pos], minlength=I)
        dt_offsets = np.concatenate([[0], np.cumsum(dt_counts)]).astype(np.int32)
        # 3. OKS matrices + the A x T greedy matchings per image
        with torch.cuda.device(dev):
            dt_kpts = p.kp_s[torch.as_tensor(dt_pos).to(dev)].contiguous()
            oks_offsets, oks, dt_matched, dt_ignored = self._match(dt_kpts, dt_counts, self.gt_counts)
            oks_h = oks.cpu().numpy()[:int(oks_offsets[-1])]
            dtm_h, dti_h = dt_matched.cpu().numpy(), dt_ignored.cpu().numpy()
        box_score_h, kpt_score_h = p.box_score_h, p.kpt_score_h

        dt_rows = order_h[dt_pos]
        precision, recall = accumulate(score_h[dt_rows], dtm_h, dti_h, self.npig)
        stats = summarize(precision, recall)
        keep = np.zeros(N, dtype=bool)
        keep[order_h] = keep_h
        self.tables = dict(
            score=score_h, box_score=box_score_h, keypoint_score=kpt_score_h, keep=keep, order=order_h, offsets=offsets,
            dt_rows=dt_rows, dt_offsets=dt_offsets, gt_offsets=self.gt_offsets, gt_ids=self.gt_ids,
            image_ids=self.image_ids, oks_offsets=oks_offsets, oks_flat=oks_h,
            oks=[oks_h[oks_offsets[i]:oks_offsets[i + 1]].reshape(int(dt_counts[i]), int(self.gt_counts[i]))
                 for i in range(I)],
            dt_matched=dtm_h, dt_ignored=dti_h, precision=precision, recall=recall, stats=stats)
        if p.soft_rank_s is not None:                       # per input row: the round a person was taken in, its live score
            soft_rank, soft_score = np.full(N, -1, dtype=np.int32), np.zeros(N)
            soft_rank[order_h], soft_score[order_h] = p.soft_rank_s, p.soft_score_s
            self.tables.update(soft_rank=soft_rank, soft_score=soft_score)
        if extra:
            self.tables.update(extra)
        if output_dir:
            self._write_results(cfg, output_dir, epoch, preds, all_boxes, img_path, person_image_id,
                                self.use_nms if by_score is None else by_score)
        name_value = OrderedDict(zip(STATS_NAMES, stats))
        return name_value, name_value['AP']

    def _write_results(self, cfg, output_dir, epoch, preds, all_boxes, img_path, person_image_id, by_score):
        """The reference's results file (dataloader.py:541-553, 652-717): the kept persons, images in order of first
        appearance; within an image by score where a suppression or a merge ran (by_score), in input order where not."""
        res_file = getattr(cfg, 'OUTPUT_JSON', '') if cfg is not None else ''
        if not res_file:
            res_folder = os.path.join(output_dir, 'results')
            os.makedirs(res_folder, exist_ok=True)
            res_file = os.path.join(res_folder, 'keypoints_{}_results_epoch{}.json'.format(self.mode, epoch))
        t = self.tables
        rows = t['order'][t['keep'][t['order']]] if by_score else np.arange(preds.shape[0])
        first = {}
        for r in range(preds.shape[0]):
            first.setdefault(person_image_id[r], len(first))
        rows = sorted(rows, key=lambda r: first[person_image_id[r]])       # stable: keeps the order within an image
        results = [{
            'image_id': person_image_id[r] if not isinstance(person_image_id[r], np.integer) else int(person_image_id[r]),
            'image_path': os.path.join(*img_path[r].split('/')[-3:]),
            'category_id': self.category_id,
            'keypoints': [float(v) for v in preds[r].reshape(-1)],
            'score': float(t['score'][r]),
            'center': [float(v) for v in all_boxes[r, 0:2]],
            'scale': [float(v) for v in all_boxes[r, 2:4]],
            'annotation_id': int(all_boxes[r, 6]),
            'box_score': float(t['box_score'][r]),
            'keypoint_score': float(t['keypoint_score'][r]),
        } for r in rows]
        logger.info('=> writing results json to %s' % res_file)
        with open(res_file, 'w') as f:
            json.dump(results, f, sort_keys=True, indent=4)
        self.tables['res_file'] = res_file
