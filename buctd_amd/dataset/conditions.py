"""Condition records from a bottom-up (BU) model's output: the step that turns BU poses into what DeviceSamplePipeline,
IterativeRefiner and the evaluators consume.  The reference does it in three places with Python loops over boxes:
data_preprocessing/match_coco_cond.py:79-103 (every annotation gets the BU pose of its image with the largest box IoU,
stored as cond_kpts[model]), lib/dataset/dataloader.py:335-393 (_load_coco_person_BU_detection_results: a record per BU
pose with its box and cond_max_iou) and dataloader.py:213-241 (cond_max_iou and near_joints of a training annotation).

What runs where
  host, once per call: the flat lists are grouped by image (numpy, a stable sort) and uploaded as fp64 tables with
      int32 CSR offsets; the records (dicts, lists) are assembled from what comes back; center / scale are
      pipeline.xywh2cs of the device's box;
  device (csrc/conditions.hip, fp64, one wavefront per image): `buctd_pose_boxes` (boxes of the poses),
      `buctd_match_boxes` (argmax of _get_iou per annotation), `buctd_group_max_iou` (largest overlap with the other
      members of the image, test and train form) and `buctd_group_near_list` (the near lists as CSR).

    src = ConditionSource(cfg, gt)                      # gt: the COCO annotation dict
    m = src.match(results, 'bu_w32')                    # cond_kpts / matched / best_iou / status per annotation
    gt2 = src.annotate({'bu_w32': results})             # ann['cond_kpts']['bu_w32'] as the script writes it
    train = ConditionSource(cfg, gt2).train_records(image_dir=..., model_key='bu_w32')
    test = src.test_records(bu_results)                 # the kpt_db of a BU-conditioned validation run

Where it departs from the reference's letter (each case is one the reference raises or divides by zero on):
  match: an image without predictions, or an annotation without a joint whose two coordinates are non-zero (status 1),
      gets matched = -1 and an all-zero condition, and annotate() leaves its cond_kpts entry out;
  train_records: a zero union yields overlap 0 and status 2; a group whose overlaps all equal 1 has cond_max_iou 0;
      an annotation that already carries 'bbox_overlaps' is refused (the stored-overlap branches are out of scope);
  test_records: a pose without a non-zero x or y raises a ValueError that names it.
The reference's own letter is kept where it is merely odd: if every IoU is 0 the first prediction of the image is the
match (np.argmax), and best_iou tells."""
import copy
import os

import numpy as np

from .pipeline import xywh2cs

POSE_BOX_ALL_POINTS, POSE_BOX_NONZERO = 0, 1       # include/buctd_hip.h
GROUP_IOU_TEST, GROUP_IOU_TRAIN = 0, 1


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _group(keys):
    """keys: hashable per row -> (group index per row, {key: group index}), groups numbered by first appearance."""
    index = {}
    return np.array([index.setdefault(k, len(index)) for k in keys], dtype=np.int64).reshape(len(keys)), index


class ConditionSource:
    """See the module's docstring.  gt: a COCO keypoint annotation dict ('images', 'annotations'); match / annotate /
    train_records need it, test_records does not.  gt_ids: the annotation ids in annotation order, the order of every
    per-annotation result of match().  category_id: the category train_records keeps (the reference's class 1)."""

    def __init__(self, cfg, gt=None, device=None, category_id=1):
        import torch
        self.cfg = cfg
        self.num_joints = int(cfg.MODEL.NUM_JOINTS)
        size = cfg.MODEL.IMAGE_SIZE
        self.aspect_ratio = size[0] * 1.0 / size[1]
        self.bu_bbox_margin = getattr(cfg.DATASET, "BU_BBOX_MARGIN", 25)
        self.image_thre = getattr(cfg.TEST, "IMAGE_THRE", 0.0)
        self.scale_thre = getattr(cfg.TEST, "SCALE_THRE", 1.25)
        self.category_id = category_id
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.gt = gt
        self.gt_ids = None
        if gt is not None:
            anns = gt['annotations']
            K = self.num_joints
            self.gt_ids = np.array([a['id'] for a in anns], dtype=np.int64).reshape(len(anns))
            self._gt_kpts = np.array([a['keypoints'] for a in anns], dtype=np.float64).reshape(len(anns), K, 3)

    # ---- device calls ---------------------------------------------------------------------------------------
    def _up(self, a, dtype):
        import torch
        return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def _pose_boxes(self, poses_t, form, mask_t=None, margin=0.0):
        """poses_t fp64 [N][K][3] on the device -> (boxes fp64 [N][4], status int32 [N]), device tensors."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        N = int(poses_t.shape[0])
        boxes = torch.zeros((N, 4), dtype=torch.float64, device=self.device)
        status = torch.zeros(N, dtype=torch.int32, device=self.device)
        check(lib().buctd_pose_boxes(ptr(poses_t), N, self.num_joints, form, ptr(mask_t), float(margin), ptr(boxes),
                                     ptr(status), stream_ptr()), "pose_boxes")
        return boxes, status

    def _group_max_iou(self, off_t, images, boxes_t, form):
        """-> (max_iou fp64 [N], status int32 [N], near_count int32 [N] or None), device tensors."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        N = int(boxes_t.shape[0])
        max_iou = torch.zeros(N, dtype=torch.float64, device=self.device)
        status = torch.zeros(N, dtype=torch.int32, device=self.device)
        near = torch.zeros(N, dtype=torch.int32, device=self.device) if form == GROUP_IOU_TRAIN else None
        check(lib().buctd_group_max_iou(ptr(off_t), images, ptr(boxes_t), form, ptr(max_iou), ptr(status), ptr(near),
                                        stream_ptr()), "group_max_iou")
        return max_iou, status, near

    def _need_gt(self, what):
        if self.gt is None:
            raise ValueError(f"ConditionSource.{what} needs the annotation dict (gt=...)")

    # ---- match_coco_cond.py ---------------------------------------------------------------------------------
    def match(self, results, model_key=None):
        """results: the flat COCO results list of one BU model ('image_id', 'category_id', 'keypoints').  Every annotation
        is matched to the result of its image and category whose all-joint box has the largest _get_iou with the box of
        the annotation's joints that have two non-zero coordinates.  Returns a dict, per annotation in gt_ids order:
        cond_kpts fp64 [G][K][3] - (0, 0, 0) for a joint with annotation v == 0, else the matched (x, y) with the
        annotation's v - matched (the row of `results`, -1: none), best_iou, status (1: the annotation has no box);
        plus model_key."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        self._need_gt("match")
        anns, K = self.gt['annotations'], self.num_joints
        G, P = len(anns), len(results)
        ann_group, index = _group([(a['image_id'], a['category_id']) for a in anns])
        n = len(index)
        res_group = np.array([index.get((r['image_id'], r['category_id']), -1) for r in results],
                             dtype=np.int64).reshape(P)
        ann_rows = np.argsort(ann_group, kind='stable')
        res_rows = np.flatnonzero(res_group >= 0)
        res_rows = res_rows[np.argsort(res_group[res_rows], kind='stable')]    # a result of no annotated group is left out
        pred = np.array([r['keypoints'] for r in results], dtype=np.float64).reshape(P, K, 3)
        gt_kpts = self._gt_kpts[ann_rows]
        labelled = (gt_kpts[:, :, 0] != 0) & (gt_kpts[:, :, 1] != 0)
        matched = np.full(G, -1, dtype=np.int64)
        best_iou, status = np.zeros(G, dtype=np.float64), np.zeros(G, dtype=np.int32)
        if G:
            with torch.cuda.device(self.device):
                gt_off = self._up(_offsets(np.bincount(ann_group, minlength=n)), np.int32)
                pr_off = self._up(_offsets(np.bincount(res_group[res_rows], minlength=n)), np.int32)
                gt_boxes, gt_status = self._pose_boxes(self._up(gt_kpts, np.float64), POSE_BOX_ALL_POINTS,
                                                       self._up(labelled, np.int32))
                pr_boxes, _ = self._pose_boxes(self._up(pred[res_rows], np.float64), POSE_BOX_ALL_POINTS)
                matched_t = torch.full((G,), -1, dtype=torch.int32, device=self.device)
                iou_t = torch.zeros(G, dtype=torch.float64, device=self.device)
                if res_rows.shape[0]:
                    check(lib().buctd_match_boxes(ptr(gt_off), ptr(pr_off), n, ptr(gt_boxes), ptr(gt_status), ptr(pr_boxes),
                                                  ptr(matched_t), ptr(iou_t), stream_ptr()), "match_boxes")
                m = matched_t.cpu().numpy().astype(np.int64)
                matched[ann_rows] = np.where(m >= 0, res_rows[np.maximum(m, 0)] if res_rows.shape[0] else -1, -1)
                best_iou[ann_rows] = iou_t.cpu().numpy()
                status[ann_rows] = gt_status.cpu().numpy()
        v = self._gt_kpts[:, :, 2]
        cond = np.zeros((G, K, 3), dtype=np.float64)
        has = matched >= 0
        cond[has, :, :2] = pred[matched[has], :, :2]
        cond[:, :, 2] = v
        cond[(v == 0) | ~has[:, None]] = 0.0
        return dict(model_key=model_key, cond_kpts=cond, matched=matched, best_iou=best_iou, status=status)

    def annotate(self, results_by_model):
        """{model key: results list} -> a deep copy of gt whose annotations carry cond_kpts[model] = the flat list the
        script writes (x, y, v per joint; 0, 0, v where v == 0) for every model; an annotation without a match keeps
        its cond_kpts (an empty dict if it had none) without that model's entry."""
        self._need_gt("annotate")
        out = copy.deepcopy(self.gt)
        for ann in out['annotations']:
            ann.setdefault('cond_kpts', {})
        for model, results in results_by_model.items():
            m = self.match(results, model)
            for ann, row, cond in zip(out['annotations'], m['matched'], m['cond_kpts']):
                if row < 0:
                    continue
                flat = []
                for (x, y, _), v in zip(cond, ann['keypoints'][2::3]):
                    flat.extend([0, 0, v] if v == 0 else [float(x), float(y), v])
                ann['cond_kpts'][model] = flat
        return out

    # ---- dataloader.py:136-299 ------------------------------------------------------------------------------
    def train_records(self, image_dir='', bu_bbox=False, best_model_key=None, model_key=None):
        """The gt_db of _load_coco_keypoint_annotations for annotations without stored overlaps: per image (in 'images'
        order) the non-crowd annotations whose box, cut to the image, is not empty form the group; every member's
        calc_bbox_overlap with the group gives cond_max_iou and near_joints (the key points [K][3] of the members it
        overlaps by > 0, in annotation order).  A record is written for the members of category_id that have a non-zero
        key point value: image, center, scale, joints_3d, joints_3d_vis, use_bu_bbox, filename, imgnum, annotation_id,
        cond_max_iou, near_joints, bbox (the cut box), best_model_key, image_id, overlap_status, and for an annotation
        with cond_kpts cond_joints / cond_joints_vis: dicts by model as the reference has them, or, with model_key, that
        model's arrays - the form the sample pipeline takes (an annotation without that model's entry gets none)."""
        import torch
        from .._C import check, lib, ptr, stream_ptr
        self._need_gt("train_records")
        K = self.num_joints
        images = self.gt['images']
        position = {im['id']: i for i, im in enumerate(images)}
        members = [[] for _ in images]
        for a in self.gt['annotations']:
            if a['image_id'] not in position or a.get('iscrowd', 0) != 0:
                continue
            if 'bbox_overlaps' in a:
                raise ValueError(f"annotation {a['id']} carries stored 'bbox_overlaps': that branch of the loader is out of scope")
            members[position[a['image_id']]].append(a)
        flat = [(i, a) for i, group in enumerate(members) for a in group]
        raw = np.array([a['bbox'][:4] for _, a in flat], dtype=np.float64).reshape(len(flat), 4)
        wh = np.array([[images[i]['width'], images[i]['height']] for i, _ in flat], dtype=np.float64).reshape(len(flat), 2)
        x1, y1 = np.maximum(0, raw[:, 0]), np.maximum(0, raw[:, 1])
        x2 = np.minimum(wh[:, 0] - 1, x1 + np.maximum(0, raw[:, 2] - 1))
        y2 = np.minimum(wh[:, 1] - 1, y1 + np.maximum(0, raw[:, 3] - 1))
        ok = np.flatnonzero((x2 >= x1) & (y2 >= y1))
        clean = np.stack([x1, y1, x2 - x1, y2 - y1], axis=1)[ok]
        flat = [flat[i] for i in ok]
        N = len(flat)
        if N == 0:
            return []
        counts = np.bincount(np.array([i for i, _ in flat], dtype=np.int64), minlength=len(images))
        with torch.cuda.device(self.device):
            off_t, boxes_t = self._up(_offsets(counts), np.int32), self._up(clean, np.float64)
            max_iou_t, status_t, count_t = self._group_max_iou(off_t, len(images), boxes_t, GROUP_IOU_TRAIN)
            near_off = np.concatenate([[0], np.cumsum(count_t.cpu().numpy().astype(np.int64))])
            near_t = torch.zeros(max(int(near_off[-1]), 1), dtype=torch.int32, device=self.device)
            near_off_t = self._up(near_off, np.int64)
            if near_off[-1]:
                check(lib().buctd_group_near_list(ptr(off_t), len(images), ptr(boxes_t), ptr(near_off_t), ptr(near_t),
                                                  stream_ptr()), "group_near_list")
            max_iou, status, near = max_iou_t.cpu().numpy(), status_t.cpu().numpy(), near_t.cpu().numpy()
        kpts = [np.array(a['keypoints']).reshape((-1, 3)) for _, a in flat]
        records = []
        for n, (i, a) in enumerate(flat):
            if a['category_id'] != self.category_id or max(a['keypoints']) == 0:
                continue
            joints, vis = self._joints(a['keypoints'])
            center, scale = xywh2cs(*clean[n], self.aspect_ratio, self.scale_thre)
            rec = {'image': os.path.join(image_dir, images[i]['file_name']), 'center': center, 'scale': scale,
                   'joints_3d': joints, 'joints_3d_vis': vis}
            if 'cond_kpts' in a:
                conds = {k: self._cond_joints(c) for k, c in a['cond_kpts'].items()}
                if model_key is None:
                    rec['cond_joints'] = {k: c[0] for k, c in conds.items()}
                    rec['cond_joints_vis'] = {k: c[1] for k, c in conds.items()}
                elif model_key in conds:
                    rec['cond_joints'], rec['cond_joints_vis'] = conds[model_key]
            rec.update({'use_bu_bbox': bu_bbox, 'filename': '', 'imgnum': 0, 'annotation_id': a['id'],
                        'cond_max_iou': float(max_iou[n]),
                        'near_joints': [kpts[j] for j in near[near_off[n]:near_off[n + 1]]],
                        'bbox': [float(v) for v in clean[n]], 'best_model_key': best_model_key,
                        'image_id': a['image_id'], 'overlap_status': int(status[n])})
            records.append(rec)
        return records

    def _joints(self, flat):
        """joints_3d / joints_3d_vis of an annotation's key point list (dataloader.py:177-188)."""
        kp = np.array(flat, dtype=np.float64).reshape(self.num_joints, 3)
        joints, vis = np.zeros((self.num_joints, 3)), np.zeros((self.num_joints, 3))
        joints[:, :2] = kp[:, :2]
        vis[:, 0] = vis[:, 1] = np.minimum(kp[:, 2], 1)
        return joints, vis

    def _cond_joints(self, flat):
        """cond_joints / cond_joints_vis of one cond_kpts list (dataloader.py:193-210): visible where x + y > 0."""
        kp = np.array(flat, dtype=np.float64).reshape(self.num_joints, 3)
        joints, vis = np.zeros((self.num_joints, 3)), np.zeros((self.num_joints, 3))
        joints[:, :2] = kp[:, :2]
        vis[:, 0] = vis[:, 1] = (joints.sum(axis=1) > 0).astype(np.float64)
        return joints, vis

    # ---- dataloader.py:335-393 ------------------------------------------------------------------------------
    def test_records(self, bu_results):
        """bu_results: per image a dict with 'preds' [P][K][3] (x, y, joint score), 'scores' [P] and 'image_paths'.  Per
        pose the box of its non-zero coordinates +- DATASET.BU_BBOX_MARGIN and cond_max_iou = the largest compute_iou
        with any other pose of the image; only then are the poses with score < TEST.IMAGE_THRE dropped.  Returns the
        kpt_db in input order: image, center, scale, score, joints_3d (zeros), joints_3d_vis (ones), cond_joints,
        cond_joints_vis, cond_max_iou."""
        import torch
        K = self.num_joints
        counts = np.array([len(r['preds']) for r in bu_results], dtype=np.int64).reshape(len(bu_results))
        N = int(counts.sum())
        if N == 0:
            return []
        poses = np.concatenate([np.array(r['preds'], dtype=np.float64).reshape(-1, K, 3) for r in bu_results])
        with torch.cuda.device(self.device):
            boxes_t, status_t = self._pose_boxes(self._up(poses, np.float64), POSE_BOX_NONZERO, margin=self.bu_bbox_margin)
            max_iou_t, _, _ = self._group_max_iou(self._up(_offsets(counts), np.int32), len(bu_results), boxes_t, GROUP_IOU_TEST)
            boxes, status, max_iou = boxes_t.cpu().numpy(), status_t.cpu().numpy(), max_iou_t.cpu().numpy()
        if status.any():
            n = int(np.flatnonzero(status)[0])
            i = int(np.searchsorted(np.cumsum(counts), n, side='right'))
            raise ValueError(f"{int(np.count_nonzero(status))} poses have no non-zero x or no non-zero y and so no box "
                             f"(first: pose {n - int(counts[:i].sum())} of {bu_results[i]['image_paths'][0]})")
        records, n = [], 0
        for r in bu_results:
            for i in range(len(r['preds'])):
                score = r['scores'][i]
                if not score < self.image_thre:
                    center, scale = xywh2cs(*boxes[n], self.aspect_ratio, self.scale_thre)
                    cond, vis = np.zeros((K, 3)), np.zeros((K, 3))
                    cond[:, :2] = poses[n, :, :2]
                    vis[:, 0] = vis[:, 1] = poses[n, :, 2]
                    records.append({'image': r['image_paths'][0], 'center': center, 'scale': scale, 'score': score,
                                    'joints_3d': np.zeros((K, 3)), 'joints_3d_vis': np.ones((K, 3)), 'cond_joints': cond,
                                    'cond_joints_vis': vis, 'cond_max_iou': float(max_iou[n])})
                n += 1
        return records
