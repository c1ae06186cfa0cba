"""Crowding analysis of a keypoint evaluation: the ten COCO keypoint figures per (overlap count, labelled key points)
bin and per annotated person - what the reference's lib/analysis/evaluation.py prints with `coco_evaluation`
(12 COCOeval runs over trimmed copies of the annotation set, lines 25-129) and `sort_instance_ap` (one deep copy, one
loadRes and one COCOeval per person, lines 240-314).  No pycocotools object is involved, and no plot is drawn: the
matrices are returned and written as JSON.

What runs where
  device, once per analysis (csrc/keypoint_eval.hip, fp64): `buctd_kpt_crowding` - which annotations count
      (check_valid_annotations) and how many others each overlaps;
  device, per call: the evaluator's rescoring and suppression (KeypointEvaluator._kept_persons, the steps evaluate()
      runs), one `buctd_coco_kpt_match` launch over pseudo-images, and for the persons one `buctd_kpt_segment_ap`
      launch (accumulate + summarize of every person at once);
  host: the filters that choose the detections of a bin / a person (numpy, no loop over persons), and for the bins
      12 calls of keypoint_eval.accumulate / summarize, which sort across images.

    an = CrowdingAnalysis(evaluator)
    tables = an.bins(preds, all_boxes, img_path)        # {'num_instances': [3][4], 'AP': [3][4], ...}
    per = an.instances(preds, all_boxes, img_path)      # {annotation id: {'AP': ..., ...}}
    an.write(output_dir)                                # benchmark_tables.json, instance_ap.json

Where it departs from the reference's letter: the bin figures are not rounded to three decimals (the reference rounds
them for its plots), and `instances` covers every valid annotation (the reference leaves out persons with 30 or more
overlaps or with a num_keypoints outside 1..17)."""
import json
import os
from collections import OrderedDict

import numpy as np

from .keypoint_eval import AREA_RNG, IOU_THRS, REC_THRS, STATS_NAMES, accumulate, summarize

OVERLAP_GROUPS = ((0,), (1, 2), (3, 4, 5, 6, 7, 8))
NUM_KPT_GROUPS = ((1, 2, 3, 4, 5), (6, 7, 8, 9, 10), (11, 12, 13, 14, 15), (16, 17))


def _group_index(groups, what):
    """count -> index of the group that holds it; a count may stand in one group only."""
    index = {}
    if len(groups) == 0:
        raise ValueError(f"{what} is empty")
    for i, group in enumerate(groups):
        for c in group:
            if int(c) != c or int(c) in index:
                raise ValueError(f"{what}: {c!r} is no integer or stands in more than one group")
            index[int(c)] = i
    return index


def _ranks(key):
    """Position of every element within its run of equal keys (key is sorted)."""
    return np.arange(key.shape[0]) - np.searchsorted(key, key, side='left')


class CrowdingAnalysis:
    """See the module's docstring.  `evaluator` is a KeypointEvaluator: its ground-truth tables, sigmas, suppression
    settings (suppression='soft' included: the persons analysed are the ones its soft OKS NMS selects), detection limit
    and device are used, and it is left as it was.  num_overlaps / valid / bin_of_gt are per
    annotation in evaluator.gt_ids order: valid as check_valid_annotations decides it, num_overlaps the stored count
    of an annotation that carries one, otherwise the number of other valid annotations of the image whose box IoU is
    > iou_for_overlap (-1 where not valid), bin_of_gt = overlap group * len(num_kpt_groups) + key point group, -1 for
    a person in no bin.  `bin_tables` / `instance_tables` hold what the last bins() / instances() call evaluated."""

    def __init__(self, evaluator, overlap_groups=OVERLAP_GROUPS, num_kpt_groups=NUM_KPT_GROUPS, iou_for_overlap=0.1):
        import torch
        from .._C import check, lib, ptr, stream_ptr
        ev = self.evaluator = evaluator
        self.overlap_groups = tuple(tuple(g) for g in overlap_groups)
        self.num_kpt_groups = tuple(tuple(g) for g in num_kpt_groups)
        self.iou_for_overlap = float(iou_for_overlap)
        by_overlap = _group_index(self.overlap_groups, "overlap_groups")
        by_kpts = _group_index(self.num_kpt_groups, "num_kpt_groups")
        if np.isnan(ev.image_wh).any():
            missing = ev.image_ids[np.isnan(ev.image_wh).any(1)]
            raise ValueError(f"{missing.shape[0]} images carry no width / height (first id: {missing[0]}); the crowding "
                             "analysis cuts every box to its image")
        self.tables = self.per_instance = self.bin_tables = self.instance_tables = None
        I, G, dev, d = len(ev.image_ids), int(ev.gt_offsets[-1]), ev.device, ev._d
        with torch.cuda.device(dev):
            wh = torch.as_tensor(ev.image_wh).to(dev)
            valid_t = torch.zeros(G, dtype=torch.int32, device=dev)
            count_t = torch.full((G,), -1, dtype=torch.int32, device=dev)
            check(lib().buctd_kpt_crowding(ptr(d['gt_off']), I, G, ev.K, ptr(d['gt_bbox']), ptr(d['gt_kpts']),
                                           ptr(d['gt_area']), ptr(wh), self.iou_for_overlap, ptr(valid_t), ptr(count_t),
                                           stream_ptr()), "kpt_crowding")
            self.valid = valid_t.cpu().numpy().astype(bool)
            counted = count_t.cpu().numpy().astype(np.int64)
        stored = self.valid & ev.gt_has_num_overlaps
        self.num_overlaps = np.where(stored, ev.gt_num_overlaps, counted)
        row = np.array([by_overlap.get(int(n), -1) for n in self.num_overlaps], dtype=np.int64).reshape(G)
        col = np.array([by_kpts.get(int(n), -1) for n in ev.gt_num_keypoints], dtype=np.int64).reshape(G)
        self.bin_of_gt = np.where(self.valid & (row >= 0) & (col >= 0), row * len(self.num_kpt_groups) + col, -1)
        self._sorted_ids = np.argsort(ev.gt_ids, kind='stable')
        out = (ev.gt_area[:, None] < AREA_RNG[None, :, 0]) | (ev.gt_area[:, None] > AREA_RNG[None, :, 1])
        self._counts_in_range = ~((ev.gt_flags[:, None] != 0) | out)                    # [G][A]: not ignored
        # ground truths in pseudo-image order, once: (bin, image) for the bins, one per segment for the persons
        NB = len(self.overlap_groups) * len(self.num_kpt_groups)
        in_bin = np.flatnonzero(self.bin_of_gt >= 0)
        key = self.bin_of_gt[in_bin] * I + ev.gt_image[in_bin]
        by_key = np.argsort(key, kind='stable')
        self._bin_gt = in_bin[by_key]
        self._bin_gt_counts = np.bincount(key, minlength=NB * I)
        self._bin_has = self._bin_gt_counts.reshape(NB, I) > 0
        self._seg_gt = np.flatnonzero(self.valid)
        self._seg_of_gt = np.full(G, -1, dtype=np.int64)
        self._seg_of_gt[self._seg_gt] = np.arange(self._seg_gt.shape[0])
        with torch.cuda.device(dev):
            gather = lambda rows: {k: d[k][torch.as_tensor(rows).to(dev)].contiguous()
                                   for k in ('gt_kpts', 'gt_area', 'gt_bbox', 'gt_flags')}
            self._bin_gt_dev, self._seg_gt_dev = gather(self._bin_gt), gather(self._seg_gt)
            self._rec_thrs = torch.as_tensor(REC_THRS).to(dev)

    def _kept(self, preds, all_boxes, img_path):
        """The persons the evaluator keeps, in (image, descending score, input order): position among the grouped persons,
        input row, image position, and the row of the annotation column 6 of all_boxes names (-1: none)."""
        ev = self.evaluator
        p = ev._kept_persons(preds, all_boxes, img_path)
        pos = np.flatnonzero(p.keep_h)
        rows = p.order_h[pos]
        ann = p.all_boxes[rows, 6].astype(np.int64)
        gt = np.full(rows.shape[0], -1, dtype=np.int64)
        if ev.gt_ids.shape[0]:
            at = np.minimum(np.searchsorted(ev.gt_ids, ann, sorter=self._sorted_ids), ev.gt_ids.shape[0] - 1)
            cand = self._sorted_ids[at]
            gt = np.where(ev.gt_ids[cand] == ann, cand, -1)
        return p, pos, rows, p.img[rows], gt

    def _cut(self, cand, key):
        """Candidates (indices into the kept persons, in their order) with a pseudo-image key each: sorted by key, equal keys
        in the given order, at most max_dets per key."""
        by_key = np.argsort(key, kind='stable')
        cand, key = cand[by_key], key[by_key]
        first = _ranks(key) < self.evaluator.max_dets
        return cand[first], key[first]

    def bins(self, preds, all_boxes, img_path):
        """bin_evaluate of the reference for every bin at once.  Returns {'num_instances': int [n_overlap][n_kpt], and
        one fp64 matrix of the same shape per name of STATS_NAMES}."""
        import torch
        ev = self.evaluator
        I, dev = len(ev.image_ids), ev.device
        shape = (len(self.overlap_groups), len(self.num_kpt_groups))
        NB = shape[0] * shape[1]
        p, pos, rows, img, gt = self._kept(preds, all_boxes, img_path)
        b = np.where(gt >= 0, self.bin_of_gt[np.maximum(gt, 0)], -1)
        ok = b >= 0
        ok[ok] = self._bin_has[b[ok], img[ok]]            # an image without an annotation of the bin is not evaluated
        cand = np.flatnonzero(ok)
        sel, key = self._cut(cand, b[cand] * I + img[cand])
        dt_counts = np.bincount(key, minlength=NB * I)
        with torch.cuda.device(dev):
            dt_kpts = p.kp_s[torch.as_tensor(pos[sel]).to(dev)].contiguous()
            _, _, dt_matched, dt_ignored = ev._match(dt_kpts, dt_counts, self._bin_gt_counts, gt=self._bin_gt_dev)
            dtm, dti = dt_matched.cpu().numpy(), dt_ignored.cpu().numpy()
        dt_end = np.cumsum(dt_counts.reshape(NB, I).sum(1))
        gt_end = np.cumsum(self._bin_gt_counts.reshape(NB, I).sum(1))
        tables = OrderedDict(num_instances=np.zeros(shape, dtype=np.int64))
        for name in STATS_NAMES:
            tables[name] = np.zeros(shape, dtype=np.float64)
        self.bin_tables = []
        for k in range(NB):
            d0, d1 = (int(dt_end[k - 1]) if k else 0), int(dt_end[k])
            gts = self._bin_gt[(int(gt_end[k - 1]) if k else 0):int(gt_end[k])]
            npig = np.count_nonzero(self._counts_in_range[gts], axis=0)
            dt_rows = rows[sel[d0:d1]]
            precision, recall = accumulate(p.score_h[dt_rows], dtm[:, :, d0:d1], dti[:, :, d0:d1], npig)
            stats = summarize(precision, recall)
            i, j = divmod(k, shape[1])
            tables['num_instances'][i, j] = gts.shape[0]
            for name, v in zip(STATS_NAMES, stats):
                tables[name][i, j] = v
            m = dtm[:, :, d0:d1]
            self.bin_tables.append(dict(
                gt_ids=ev.gt_ids[gts], dt_rows=dt_rows, npig=npig, dt_ignored=dti[:, :, d0:d1] != 0,
                dt_matched=np.where(m > 0, ev.gt_ids[self._bin_gt[np.maximum(m - 1, 0)]], 0) if m.size else m.astype(np.int64),
                precision=precision, recall=recall, stats=stats))
        self.tables = tables
        return tables

    def instances(self, preds, all_boxes, img_path):
        """instance_evaluate of the reference for every valid annotation at once: {annotation id: {name: figure}}."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        ev = self.evaluator
        dev = ev.device
        A, T = AREA_RNG.shape[0], IOU_THRS.shape[0]
        S = int(self._seg_gt.shape[0])
        p, pos, rows, img, gt = self._kept(preds, all_boxes, img_path)
        seg = np.where(gt >= 0, self._seg_of_gt[np.maximum(gt, 0)], -1)
        cand = np.flatnonzero((seg >= 0) & (ev.gt_image[np.maximum(gt, 0)] == img))     # the person's own image only
        sel, key = self._cut(cand, seg[cand])
        dt_counts = np.bincount(key, minlength=S)
        npig = np.ascontiguousarray(self._counts_in_range[self._seg_gt].astype(np.int32)).reshape(S, A)
        with torch.cuda.device(dev):
            dt_kpts = p.kp_s[torch.as_tensor(pos[sel]).to(dev)].contiguous()
            _, _, dt_matched, dt_ignored = ev._match(dt_kpts, dt_counts, np.ones(S, dtype=np.int64), gt=self._seg_gt_dev)
            seg_off = torch.as_tensor(np.concatenate([[0], np.cumsum(dt_counts)]).astype(np.int32)).to(dev)
            npig_t = torch.as_tensor(npig).to(dev)
            stats_t = torch.zeros((S, 10), dtype=torch.float64, device=dev)
            recall_t = torch.zeros((S, T, A), dtype=torch.float64, device=dev)
            check(lib().buctd_kpt_segment_ap(ptr(seg_off), S, int(dt_counts.max()) if S else 0, int(sel.shape[0]),
                                             ptr(dt_matched), ptr(dt_ignored), A, T, ptr(npig_t), ptr(self._rec_thrs),
                                             int(REC_THRS.shape[0]), 0, 5, ptr(stats_t), ptr(recall_t), stream_ptr()),
                  "kpt_segment_ap")                                                      # IOU_THRS[0] = .5, IOU_THRS[5] = .75
            stats, recall = stats_t.cpu().numpy(), recall_t.cpu().numpy()
            dtm, dti = dt_matched.cpu().numpy(), dt_ignored.cpu().numpy()
        ids = ev.gt_ids[self._seg_gt]
        self.instance_tables = dict(gt_ids=ids, dt_rows=rows[sel], dt_offsets=np.concatenate([[0], np.cumsum(dt_counts)]),
                                    dt_matched=dtm, dt_ignored=dti, npig=npig, stats=stats, recall=recall)
        self.per_instance = OrderedDict((int(i), OrderedDict(zip(STATS_NAMES, (float(v) for v in s))))
                                        for i, s in zip(ids, stats))
        return self.per_instance

    def write(self, output_dir):
        """benchmark_tables.json (the matrices of the last bins() call, with the groups) and instance_ap.json (the last
        instances() call, under the reference's file name); what has not been computed is not written."""
        if self.tables is None and self.per_instance is None:
            raise RuntimeError("nothing to write: call bins() or instances() first")
        os.makedirs(output_dir, exist_ok=True)
        written = []
        if self.tables is not None:
            out = dict(overlap_groups=self.overlap_groups, num_kpt_groups=self.num_kpt_groups,
                       iou_for_overlap=self.iou_for_overlap, **{k: v.tolist() for k, v in self.tables.items()})
            written.append(os.path.join(output_dir, 'benchmark_tables.json'))
            with open(written[-1], 'w') as f:
                json.dump(out, f, indent=4)
        if self.per_instance is not None:
            written.append(os.path.join(output_dir, 'instance_ap.json'))
            with open(written[-1], 'w') as f:
                json.dump(self.per_instance, f, indent=4)
        return written
