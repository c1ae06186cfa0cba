"""TEST INFRASTRUCTURE - restatement of the three reference passages behind buctd_amd/dataset/conditions.py, loop by
loop in numpy / plain Python, sharing no code with the package:

  match_annotations   data_preprocessing/match_coco_cond.py:79-103 with its helpers (lines 19-50)
  bu_test_records     lib/dataset/dataloader.py:335-393 with JointsDataset.compute_iou (JointsDataset.py:566-597)
  train_records       lib/dataset/dataloader.py:136-299 (the branch without stored overlaps) with calc_bbox_overlap
                      (lines 512-535) and _xywh2cs (lines 305-321)

Where the reference raises or divides by zero the restatement does what the package documents: no prediction for the
image or no labelled joint -> no match (row -1, status 1 for the latter); zero union -> overlap 0 and status 2; every
overlap equal to 1 -> cond_max_iou 0.  Each function also returns the raw IoU lists, so that a test can state its
conditions on them."""
import copy
import os

import numpy as np

PIXEL_STD = 200


# ---- match_coco_cond.py ---------------------------------------------------------------------------------------------
def corner_boxes(points):
    """lines 19-30 with slack 0, offset 0, clip: [n][m][2] -> [n][4] x1 y1 x2 y2; None where there is no point."""
    data = np.asarray(points, dtype=np.float64)
    if data.ndim != 3:
        data = data[None]
    if data.ndim != 3 or data.shape[1] == 0:
        return None
    boxes = np.full((data.shape[0], 4), np.nan)
    boxes[:, :2] = np.nanmin(data[..., :2], axis=1)
    boxes[:, 2:4] = np.nanmax(data[..., :2], axis=1)
    boxes[boxes < 0] = 0
    return boxes


def corner_iou(a, b):
    """lines 33-50"""
    xa, ya = max(a[0], b[0]), max(a[1], b[1])
    xb, yb = min(a[2], b[2]), min(a[3], b[3])
    inter = abs(max((xb - xa, 0)) * max((yb - ya), 0))
    if inter == 0:
        return 0
    area_a = abs((a[2] - a[0]) * (a[3] - a[1]))
    area_b = abs((b[2] - b[0]) * (b[3] - b[1]))
    return inter / float(area_a + area_b - inter)


def match_annotations(gt, results, model):
    """The loop over gt['annotations'] on a deep copy.  Returns (annotated copy, rows): per annotation a dict with
    matched (row of `results`, -1), best_iou, status, ious (the list np.argmax saw), gt_box, flat (the cond_kpts list)."""
    out = copy.deepcopy(gt)
    rows = []
    for ann in out['annotations']:
        ann.setdefault('cond_kpts', {})
        kp = np.array(ann['keypoints'], dtype=np.float64).reshape(-1, 3)
        labelled = [p for p in kp[:, :2].tolist() if all(p) != 0]
        gt_boxes = corner_boxes(labelled)
        where = [i for i, r in enumerate(results)
                 if r['image_id'] == ann['image_id'] and r['category_id'] == ann['category_id']]
        poses = [np.array(results[i]['keypoints'], dtype=np.float64).reshape(-1, 3)[:, :2] for i in where]
        row = dict(matched=-1, best_iou=0.0, status=0 if gt_boxes is not None else 1, ious=[], gt_box=None,
                   flat=[0.0] * (3 * kp.shape[0]))
        rows.append(row)
        if gt_boxes is None or not poses:
            continue
        row['gt_box'] = gt_boxes[0]
        row['ious'] = [corner_iou(gt_boxes[0], b) for b in corner_boxes(poses)]
        at = int(np.argmax(row['ious']))
        row['matched'], row['best_iou'] = where[at], float(row['ious'][at])
        flat = []
        for i, p in enumerate(poses[at]):
            v = ann['keypoints'][3 * i + 2]
            if v == 0:
                p = (0, 0)
            flat.extend([p[0], p[1], v])
        row['flat'] = flat
        ann['cond_kpts'][model] = [v if isinstance(v, int) else float(v) for v in flat]
    return out, rows


# ---- dataloader.py: test ------------------------------------------------------------------------------------------------
def xywh2cs(x, y, w, h, aspect_ratio, scale_thre):
    """lines 305-321"""
    center = np.zeros((2), dtype=np.float32)
    center[0] = x + w * 0.5
    center[1] = y + h * 0.5
    if w > aspect_ratio * h:
        h = w * 1.0 / aspect_ratio
    elif w < aspect_ratio * h:
        w = h * aspect_ratio
    scale = np.array([w * 1.0 / PIXEL_STD, h * 1.0 / PIXEL_STD], dtype=np.float32)
    if center[0] != -1:
        scale = scale * scale_thre
    return center, scale


def xywh_iou(b1, b2):
    """JointsDataset.py:566-597"""
    l1, r1, t1, u1 = b1[0], b1[0] + b1[2], b1[1], b1[1] + b1[3]
    l2, r2, t2, u2 = b2[0], b2[0] + b2[2], b2[1], b2[1] + b2[3]
    left, right = max(l1, l2), min(r1, r2)
    top, bottom = max(t1, t2), min(u1, u2)
    width, height = max(0, right - left), max(0, bottom - top)
    a1, a2 = b1[2] * b1[3], b2[2] * b2[3]
    if float(a1 + a2 - (width * height)) == 0:
        return 0
    return (width * height) / float(a1 + a2 - (width * height))


def nonzero_box(pose, margin):
    """lines 357-361: x, y, w, h, or None where a coordinate has no non-zero value."""
    xs, ys = pose[:, 0][np.nonzero(pose[:, 0])], pose[:, 1][np.nonzero(pose[:, 1])]
    if xs.size == 0 or ys.size == 0:
        return None
    xmin, ymin = np.min(xs) - margin, np.min(ys) - margin
    xmax, ymax = np.max(xs) + margin, np.max(ys) + margin
    return [xmin, ymin, xmax - xmin, ymax - ymin]


def bu_test_records(bu_results, num_joints, margin, image_thre, aspect_ratio, scale_thre):
    """Returns (kpt_db, boxes per image, IoU lists per image and pose)."""
    db, all_boxes, all_ious = [], [], []
    for img in bu_results:
        preds, scores, name = img['preds'], img['scores'], img['image_paths'][0]
        boxes, conds, vises = [], [], []
        for i in range(len(preds)):
            pred = np.array(preds[i], dtype=np.float64)
            cond, vis = np.zeros((num_joints, 3)), np.zeros((num_joints, 3))
            cond[:, :2] = pred[:, :2]
            vis[:, 0] = pred[:, 2]
            vis[:, 1] = pred[:, 2]
            conds.append(cond)
            vises.append(vis)
            boxes.append(nonzero_box(cond, margin))
        all_boxes.append(boxes)
        image_ious = []
        for i in range(len(preds)):
            ious = [xywh_iou(boxes[i], boxes[j]) for j in range(len(preds)) if not i == j]
            image_ious.append(ious)
            cond_max_iou = 0 if len(ious) == 0 else max(ious)
            if scores[i] < image_thre:
                continue
            center, scale = xywh2cs(*boxes[i], aspect_ratio, scale_thre)
            db.append({'image': name, 'center': center, 'scale': scale, 'score': scores[i],
                       'joints_3d': np.zeros((num_joints, 3)), 'joints_3d_vis': np.ones((num_joints, 3)),
                       'cond_joints': conds[i], 'cond_joints_vis': vises[i], 'cond_max_iou': cond_max_iou})
        all_ious.append(image_ious)
    return db, all_boxes, all_ious


# ---- dataloader.py: train -----------------------------------------------------------------------------------------------
def xywh_overlap(b1, b2):
    """lines 512-535; (overlap, union was zero)"""
    x1, y1, w1, h1 = b1
    x2, y2, w2, h2 = b2
    x_overlap = max(0, min(x1 + w1, x2 + w2) - max(x1, x2))
    y_overlap = max(0, min(y1 + h1, y2 + h2) - max(y1, y2))
    inter = x_overlap * y_overlap
    union = w1 * h1 + w2 * h2 - inter
    if union == 0:
        return 0.0, True
    return inter / union, False


def train_records(gt, num_joints, aspect_ratio, scale_thre, image_dir='', category_id=1, bu_bbox=False,
                  best_model_key=None, model_key=None):
    """Returns (gt_db, overlap lists per record's annotation id)."""
    db, overlaps_of = [], {}
    for im in gt['images']:
        width, height = im['width'], im['height']
        objs = []
        for obj in gt['annotations']:
            if obj['image_id'] != im['id'] or obj.get('iscrowd', 0):
                continue
            x, y, w, h = obj['bbox']
            x1, y1 = np.max((0, x)), np.max((0, y))
            x2 = np.min((width - 1, x1 + np.max((0, w - 1))))
            y2 = np.min((height - 1, y1 + np.max((0, h - 1))))
            if x2 >= x1 and y2 >= y1:
                objs.append(dict(obj, clean_bbox=[x1, y1, x2 - x1, y2 - y1]))
        for obj in objs:
            if obj['category_id'] != category_id or max(obj['keypoints']) == 0:
                continue
            joints, vis = np.zeros((num_joints, 3)), np.zeros((num_joints, 3))
            for k in range(num_joints):
                joints[k, 0], joints[k, 1] = obj['keypoints'][k * 3], obj['keypoints'][k * 3 + 1]
                vis[k, 0] = vis[k, 1] = min(obj['keypoints'][k * 3 + 2], 1)
            rec = {'image': os.path.join(image_dir, im['file_name'])}
            rec['center'], rec['scale'] = xywh2cs(*obj['clean_bbox'], aspect_ratio, scale_thre)
            rec['joints_3d'], rec['joints_3d_vis'] = joints, vis
            if 'cond_kpts' in obj:
                cj, cv = {}, {}
                for key, cond in obj['cond_kpts'].items():
                    cj[key], cv[key] = np.zeros((num_joints, 3)), np.zeros((num_joints, 3))
                    for k in range(num_joints):
                        cj[key][k, 0], cj[key][k, 1] = cond[k * 3], cond[k * 3 + 1]
                        cv[key][k, 0] = cv[key][k, 1] = 1 if sum(cj[key][k]) > 0 else 0
                if model_key is None:
                    rec['cond_joints'], rec['cond_joints_vis'] = cj, cv
                elif model_key in cj:
                    rec['cond_joints'], rec['cond_joints_vis'] = cj[model_key], cv[model_key]
            pairs = [xywh_overlap(obj['clean_bbox'], other['clean_bbox']) for other in objs]
            overlaps = np.array([p[0] for p in pairs])
            near = [np.array(other['keypoints']).reshape((-1, 3)) for k, other in enumerate(objs) if overlaps[k] > 0]
            max_iou = 0
            if len(overlaps) > 1:
                left = overlaps[overlaps != 1]
                max_iou = max(left) if len(left) else 0
            overlaps_of[obj['id']] = overlaps
            rec.update({'use_bu_bbox': bu_bbox, 'filename': '', 'imgnum': 0, 'annotation_id': obj['id'],
                        'cond_max_iou': max_iou, 'near_joints': near, 'bbox': obj['clean_bbox'][:4],
                        'best_model_key': best_model_key, 'image_id': obj['image_id'],
                        'overlap_status': 2 if any(p[1] for p in pairs) else 0})
            db.append(rec)
    return db, overlaps_of
