"""TEST INFRASTRUCTURE - loop-by-loop restatement of the reference's crowding analysis (lib/analysis/evaluation.py:
check_valid_annotations, bin_evaluate, instance_evaluate; lib/utils/utils.py: compute_iou, compute_ious).  For every bin
and every person it builds the trimmed ground-truth dict and the trimmed result list as those functions do and hands
them to the COCOeval restatement tests/helpers/coco_kpt_eval_ref.KeypointEvalRef.  Shares no code with buctd_amd/.

Like coco_kpt_eval_ref it is NOT pinned against pycocotools, which the project's image does not carry.  Two things the
product states about itself are followed here: figures are not rounded to three decimals, and every valid annotation
gets a per-person evaluation."""
import numpy as np

from tests.helpers import coco_kpt_eval_ref as R

OVERLAP_GROUPS = ((0,), (1, 2), (3, 4, 5, 6, 7, 8))
NUM_KPT_GROUPS = ((1, 2, 3, 4, 5), (6, 7, 8, 9, 10), (11, 12, 13, 14, 15), (16, 17))


def compute_iou(bbox_1, bbox_2):
    """utils.py:557-588, Python floats, the operations in their order."""
    left_1, top_1, w_1, h_1 = bbox_1[0], bbox_1[1], bbox_1[2], bbox_1[3]
    right_1 = bbox_1[0] + bbox_1[2]
    bottom_1 = bbox_1[1] + bbox_1[3]
    left_2, top_2, w_2, h_2 = bbox_2[0], bbox_2[1], bbox_2[2], bbox_2[3]
    right_2 = bbox_2[0] + bbox_2[2]
    bottom_2 = bbox_2[1] + bbox_2[3]
    left = max(left_1, left_2)
    right = min(right_1, right_2)
    top = max(top_1, top_2)
    bottom = min(bottom_1, bottom_2)
    width = max(0, right - left)
    height = max(0, bottom - top)
    area_1 = w_1 * h_1
    area_2 = w_2 * h_2
    if float(area_1 + area_2 - (width * height)) == 0:
        return 0
    return (width * height) / float(area_1 + area_2 - (width * height))


def compute_ious(anns):
    """utils.py:590-599: the upper triangle computed, the lower mirrored."""
    n = len(anns)
    ious = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            ious[i, j] = compute_iou(anns[i]['bbox'], anns[j]['bbox'])
            if i != j:
                ious[j, i] = ious[i, j]
    return ious


def valid_annotations(annotations, image_info):
    """The first half of check_valid_annotations (evaluation.py:136-154): the annotations of one image that count."""
    width, height = image_info['width'], image_info['height']
    kept = []
    for obj in annotations:
        if max(obj['keypoints']) == 0:
            continue
        x, y, w, h = obj['bbox']
        x1 = np.max((0, x))
        y1 = np.max((0, y))
        x2 = np.min((width - 1, x1 + np.max((0, w - 1))))
        y2 = np.min((height - 1, y1 + np.max((0, h - 1))))
        if obj['area'] > 0 and x2 >= x1 and y2 >= y1:
            kept.append(obj)
    return kept


def overlap_counts(annotations, iou_for_overlap):
    """The second half (evaluation.py:157-170): (num_overlaps, num_keypoints) per counted annotation, and the IoU matrix."""
    ious = compute_ious(annotations)
    eye = np.eye(len(annotations))
    out = []
    for idx, ann in enumerate(annotations):
        if 'num_overlaps' in ann.keys():
            num_keypoints = int(ann['num_keypoints'])
            num_overlaps = int(ann['num_overlaps'])
        else:
            num_overlaps = int(sum((ious[idx, :] - eye[idx, :]) > iou_for_overlap))
            num_keypoints = ann['num_keypoints']
        out.append((num_overlaps, num_keypoints))
    return out, ious


class AnalysisRef:
    """gt: COCO dict; preds / all_boxes / image_of: validate()'s tables with the image id per person.  run() fills
    valid / num_overlaps / bin_of (per annotation id), ious (every off-diagonal IoU looked at), bins[(i, j)] and
    persons[annotation id], each a dict of num_instances / stats / dt_rows / dt_matched / dt_ignored / oks."""

    def __init__(self, gt, preds, all_boxes, image_of, sigmas, oks_thre=0.5, in_vis_thre=0.0, use_nms=True,
                 overlap_groups=OVERLAP_GROUPS, num_kpt_groups=NUM_KPT_GROUPS, iou_for_overlap=0.1):
        self.gt, self.sigmas = gt, np.asarray(sigmas, dtype=np.float64)
        self.overlap_groups, self.num_kpt_groups, self.iou_for_overlap = overlap_groups, num_kpt_groups, iou_for_overlap
        self.score, _, _, self.keep, self.nms_oks = R.rescore_and_nms(preds, all_boxes, image_of, in_vis_thre, oks_thre,
                                                                      self.sigmas, use_nms)
        self.oks_thre = oks_thre
        # the results file: the kept persons (input order; COCOeval's stable sorts order equal scores by it)
        self.results = [{'image_id': image_of[r], 'keypoints': preds[r].astype(np.float64).reshape(-1),
                         'score': float(self.score[r]), 'annotation_id': int(all_boxes[r][6]), 'row': r}
                        for r in range(preds.shape[0]) if self.keep[r]]
        self.images = {im['id']: im for im in gt['images']}
        self.image_ids = sorted(self.images)
        self.anns = {a['id']: a for a in gt['annotations']}
        self.anns_of = {i: [a for a in gt['annotations'] if a['image_id'] == i] for i in self.image_ids}

    def check_valid_annotations(self, image_id, NUM_OVERLAPS, NUM_KEYPOINTS):
        annotations = valid_annotations(self.anns_of[image_id], self.images[image_id])
        counts, _ = overlap_counts(annotations, self.iou_for_overlap)
        ann_ids = [a['id'] for a, (n_ov, n_kp) in zip(annotations, counts) if n_ov in NUM_OVERLAPS and n_kp in NUM_KEYPOINTS]
        return ann_ids, ([image_id] if len(ann_ids) > 0 else [])

    def _evaluate(self, ann_ids, image_ids, results):
        gt = {'images': [self.images[i] for i in image_ids], 'annotations': [self.anns[i] for i in ann_ids]}
        ev = R.KeypointEvalRef(gt, results, self.sigmas)
        stats = [float(s) for s in ev.run()]
        scores, dtm, dti, npig = ev.match_tables()
        first = ev.evalImgs[:len(ev.imgIds)]
        return dict(num_instances=len(ann_ids), ann_ids=list(ann_ids), image_ids=list(image_ids), stats=stats,
                    dt_rows=np.array([results[d - 1]['row'] for e in first if e is not None for d in e['dtIds']], dtype=np.int64),
                    dt_matched=dtm, dt_ignored=dti, npig=npig, oks=[np.asarray(ev.ious[i]) for i in ev.imgIds])

    def bin_evaluate(self, overlap_group, num_kpt_group):
        ann_ids, image_ids = [], []
        for image_id in self.image_ids:
            a, i = self.check_valid_annotations(image_id, overlap_group, num_kpt_group)
            ann_ids.extend(a)
            image_ids.extend(i)
        results = [r for r in self.results if r['annotation_id'] in ann_ids]
        return self._evaluate(ann_ids, image_ids, results)

    def instance_evaluate(self, instance_id, image_id):
        results = [r for r in self.results if r['annotation_id'] == instance_id]
        return self._evaluate([instance_id], [image_id], results)

    def run(self):
        self.valid, self.num_overlaps, self.bin_of, ious = {}, {}, {}, []
        for image_id in self.image_ids:
            annotations = valid_annotations(self.anns_of[image_id], self.images[image_id])
            counts, m = overlap_counts(annotations, self.iou_for_overlap)
            ious.append(m[~np.eye(len(annotations), dtype=bool)])
            for a in self.anns_of[image_id]:
                self.valid[a['id']], self.num_overlaps[a['id']], self.bin_of[a['id']] = False, -1, -1
            for a, (n_ov, n_kp) in zip(annotations, counts):
                self.valid[a['id']], self.num_overlaps[a['id']] = True, n_ov
        self.ious = np.concatenate(ious) if ious else np.zeros(0)
        self.bins = {}
        for i, og in enumerate(self.overlap_groups):
            for j, ng in enumerate(self.num_kpt_groups):
                self.bins[(i, j)] = self.bin_evaluate(og, ng)
                for ann_id in self.bins[(i, j)]['ann_ids']:
                    assert self.bin_of[ann_id] == -1, "an annotation in two bins"
                    self.bin_of[ann_id] = i * len(self.num_kpt_groups) + j
        self.persons = {ann_id: self.instance_evaluate(ann_id, self.anns[ann_id]['image_id'])
                        for ann_id in self.anns if self.valid[ann_id]}
        return self

    def threshold_margin(self):
        """Smallest distance of an OKS from a threshold it is compared with, over every evaluation made."""
        thrs = np.linspace(.5, 0.95, 10)
        m = [np.abs(o.reshape(-1, 1) - thrs).min() for e in list(self.bins.values()) + list(self.persons.values())
             for o in e['oks'] if o.size]
        if self.nms_oks.size:
            m.append(np.abs(self.nms_oks - self.oks_thre).min())
        return min(m)
