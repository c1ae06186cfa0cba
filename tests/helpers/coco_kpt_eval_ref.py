"""TEST INFRASTRUCTURE - loop-by-loop numpy restatement of the published COCO keypoint evaluation (COCOeval with
iouType 'keypoints': _prepare, computeOks, evaluateImg, accumulate, summarize, and the part of COCO.loadRes that gives
a keypoint result its id and area), and of the reference's rescoring + oks_nms step (lib/dataset/dataloader.py:590-634,
the suppression itself through oracle.nms).  Shares no code with buctd_amd/core/keypoint_eval.py.

NOT pinned against pycocotools (it is not part of the project's image): this file has the standing of the other
restatements of third-party code; tests/test_keypoint_eval.py compares against pycocotools where it imports."""
from collections import defaultdict

import numpy as np

from oracle import nms as onms

STATS_NAMES = ['AP', 'AP .5', 'AP .75', 'AP (M)', 'AP (L)', 'AR', 'AR .5', 'AR .75', 'AR (M)', 'AR (L)']
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


class Params:
    def __init__(self, sigmas):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [20]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'medium', 'large']
        self.kpt_oks_sigmas = np.asarray(sigmas, dtype=np.float64)


def rescore_and_nms(preds, all_boxes, image_of, in_vis_thre, oks_thre, nms_sigmas, use_nms, nms_in_vis_thre=None):
    """dataloader.py:565-634.  preds [N][K][3], all_boxes [N][7] (area in column 4, box score in 5), image_of [N] image
    ids.  Returns score, box_score, keypoint_score [N], the keep mask [N], and the per-(head, candidate) OKS values the
    suppression looked at (for the tests' condition on the inputs).  The joint scores are added in fp64 (the reference's
    Python loop promotes them); key points enter the suppression widened to fp64."""
    N, K = preds.shape[0], preds.shape[1]
    score, box_score, keypoint_score = np.zeros(N), np.zeros(N), np.zeros(N)
    kpts = defaultdict(list)
    for idx in range(N):
        kpts[image_of[idx]].append(idx)
    keep_mask = np.zeros(N, dtype=bool)
    seen = []
    for img in kpts.keys():
        rows = kpts[img]
        for r in rows:
            bs = float(all_boxes[r][5])
            kpt_score = 0.0
            valid_num = 0
            for n_jt in range(0, K):
                t_s = float(preds[r][n_jt][2])
                if t_s > in_vis_thre:
                    kpt_score = kpt_score + t_s
                    valid_num = valid_num + 1
            if valid_num != 0:
                kpt_score = kpt_score / valid_num
            score[r] = kpt_score * bs
            box_score[r] = bs
            keypoint_score[r] = kpt_score
        db = [{'keypoints': preds[r].astype(np.float64), 'score': score[r], 'area': float(all_boxes[r][4])} for r in rows]
        keep = onms.oks_nms(db, oks_thre, np.asarray(nms_sigmas, dtype=np.float64), nms_in_vis_thre) if use_nms else []
        if len(keep) == 0:
            keep = range(len(rows))
        for k in keep:
            keep_mask[rows[k]] = True
        if use_nms:         # every OKS a greedy sweep in any tie order could look at
            flat = np.array([p['keypoints'].flatten() for p in db])
            areas = np.array([p['area'] for p in db])
            for i in range(len(db)):
                others = [j for j in range(len(db)) if j != i]
                if others:
                    seen.append(onms.oks_iou(flat[i], flat[others], areas[i], areas[others],
                                             np.asarray(nms_sigmas, dtype=np.float64), nms_in_vis_thre))
    return score, box_score, keypoint_score, keep_mask, (np.concatenate(seen) if seen else np.zeros(0))


def load_res(results, K):
    """COCO.loadRes for key points: id = position + 1, area = extent box of the key points."""
    anns = []
    for i, r in enumerate(results):
        ann = dict(r)
        s = ann['keypoints']
        x = s[0::3]
        y = s[1::3]
        x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
        ann['area'] = (x1 - x0) * (y1 - y0)
        ann['id'] = i + 1
        ann['bbox'] = [x0, y0, x1 - x0, y1 - y0]
        anns.append(ann)
    return anns


class KeypointEvalRef:
    """COCOeval(cocoGt, cocoDt, 'keypoints') for one category.  gt: COCO dict; results: list of dicts with image_id,
    keypoints (flat, 3K floats) and score, in results-file order."""

    def __init__(self, gt, results, sigmas):
        self.params = Params(sigmas)
        self.imgIds = sorted(im['id'] for im in gt['images'])
        self._gts = defaultdict(list)
        self._dts = defaultdict(list)
        for g in gt['annotations']:
            g = dict(g)
            g['ignore'] = g['ignore'] if 'ignore' in g else 0
            g['ignore'] = 'iscrowd' in g and g['iscrowd']
            g['ignore'] = (g['num_keypoints'] == 0) or g['ignore']
            self._gts[g['image_id']].append(g)
        for d in load_res(results, len(self.params.kpt_oks_sigmas)):
            self._dts[d['image_id']].append(d)
        self.ious = {}
        self.evalImgs = []
        self.eval = {}
        self.stats = []

    def run(self):
        p = self.params
        self.ious = {i: self.computeOks(i) for i in self.imgIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(i, areaRng, maxDet) for areaRng in p.areaRng for i in self.imgIds]
        self.accumulate()
        self.summarize()
        return self.stats

    def computeOks(self, imgId):
        p = self.params
        gts = self._gts[imgId]
        dts = self._dts[imgId]
        inds = np.argsort([-d['score'] for d in dts], kind='mergesort')
        dts = [dts[i] for i in inds]
        if len(dts) > p.maxDets[-1]:
            dts = dts[0:p.maxDets[-1]]
        if len(gts) == 0 or len(dts) == 0:
            return []
        ious = np.zeros((len(dts), len(gts)))
        sigmas = p.kpt_oks_sigmas
        vars = (sigmas * 2) ** 2
        k = len(sigmas)
        for j, gt in enumerate(gts):
            g = np.array(gt['keypoints'])
            xg = g[0::3]; yg = g[1::3]; vg = g[2::3]
            k1 = np.count_nonzero(vg > 0)
            bb = gt['bbox']
            x0 = bb[0] - bb[2]; x1 = bb[0] + bb[2] * 2
            y0 = bb[1] - bb[3]; y1 = bb[1] + bb[3] * 2
            for i, dt in enumerate(dts):
                d = np.array(dt['keypoints'])
                xd = d[0::3]; yd = d[1::3]
                if k1 > 0:
                    dx = xd - xg
                    dy = yd - yg
                else:
                    z = np.zeros((k))
                    dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                    dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
                e = (dx ** 2 + dy ** 2) / vars / (gt['area'] + np.spacing(1)) / 2
                if k1 > 0:
                    e = e[vg > 0]
                ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
        return ious

    def evaluateImg(self, imgId, aRng, maxDet):
        p = self.params
        gt = self._gts[imgId]
        dt = self._dts[imgId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId][:, gtind] if len(self.ious[imgId]) > 0 else self.ious[imgId]
        T = len(p.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {'image_id': imgId, 'aRng': aRng, 'maxDet': maxDet, 'dtIds': [d['id'] for d in dt],
                'gtIds': [g['id'] for g in gt], 'dtMatches': dtm, 'gtMatches': gtm,
                'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg}

    def accumulate(self):
        p = self.params
        T = len(p.iouThrs)
        R = len(p.recThrs)
        A = len(p.areaRng)
        precision = -np.ones((T, R, A))
        recall = -np.ones((T, A))
        I0 = len(self.imgIds)
        maxDet = p.maxDets[-1]
        for a in range(A):
            Na = a * I0
            E = [self.evalImgs[Na + i] for i in range(I0)]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
            inds = np.argsort(-dtScores, kind='mergesort')
            dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
            dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
            gtIg = np.concatenate([e['gtIgnore'] for e in E])
            npig = np.count_nonzero(gtIg == 0)
            if npig == 0:
                continue
            tps = np.logical_and(dtm, np.logical_not(dtIg))
            fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
            tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
            fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
            for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                tp = np.array(tp)
                fp = np.array(fp)
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                q = np.zeros((R,))
                if nd:
                    recall[t, a] = rc[-1]
                else:
                    recall[t, a] = 0
                pr = pr.tolist()
                q = q.tolist()
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                inds = np.searchsorted(rc, p.recThrs, side='left')
                try:
                    for ri, pi in enumerate(inds):
                        q[ri] = pr[pi]
                except IndexError:
                    pass
                precision[t, :, a] = np.array(q)
        self.eval = {'precision': precision, 'recall': recall}

    def summarize(self):
        p = self.params

        def _summarize(ap=1, iouThr=None, areaRng='all'):
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, aind]
            if len(s[s > -1]) == 0:
                return -1
            return np.mean(s[s > -1])
        self.stats = [_summarize(1), _summarize(1, iouThr=.5), _summarize(1, iouThr=.75),
                      _summarize(1, areaRng='medium'), _summarize(1, areaRng='large'),
                      _summarize(0), _summarize(0, iouThr=.5), _summarize(0, iouThr=.75),
                      _summarize(0, areaRng='medium'), _summarize(0, areaRng='large')]

    # ---- the tables in the layout of the product's device outputs (images by id, detections by score)
    def match_tables(self):
        """dt_scores [D], dt_matched / dt_ignored [A][T][D] (dt_matched: the ground truth's id, 0 unmatched), npig [A],
        and per image the matched ground-truth ids / OKS matrices, for a comparison table by table."""
        p = self.params
        A, I0 = len(p.areaRng), len(self.imgIds)
        scores, dtm, dti, npig = None, [], [], []
        for a in range(A):
            E = [e for e in self.evalImgs[a * I0:(a + 1) * I0] if e is not None]
            T = len(p.iouThrs)
            scores = np.concatenate([np.asarray(e['dtScores'], dtype=np.float64) for e in E]) if E else np.zeros(0)
            dtm.append(np.concatenate([e['dtMatches'] for e in E], axis=1) if E else np.zeros((T, 0)))
            dti.append(np.concatenate([e['dtIgnore'] for e in E], axis=1) if E else np.zeros((T, 0)))
            npig.append(int(sum(np.count_nonzero(e['gtIgnore'] == 0) for e in E)))
        return scores, np.stack(dtm).astype(np.int64), np.stack(dti).astype(bool), np.array(npig)


def evaluate_ref(gt, preds, all_boxes, image_of, sigmas, nms_sigmas=None, oks_thre=0.5, in_vis_thre=0.0, use_nms=True,
                 nms_in_vis_thre=None):
    """The whole host path: rescoring + oks_nms per image, a results list (kept persons in input order, so that equal
    scores keep input order), COCOeval.  Returns a dict of everything the tests compare."""
    nms_sigmas = sigmas if nms_sigmas is None else nms_sigmas
    score, box_score, keypoint_score, keep, nms_oks = rescore_and_nms(preds, all_boxes, image_of, in_vis_thre, oks_thre,
                                                                      nms_sigmas, use_nms, nms_in_vis_thre)
    results = [{'image_id': image_of[r], 'keypoints': preds[r].astype(np.float64).reshape(-1), 'score': float(score[r]),
                'row': r} for r in range(preds.shape[0]) if keep[r]]
    ev = KeypointEvalRef(gt, results, sigmas)
    stats = ev.run()
    dt_scores, dtm, dti, npig = ev.match_tables()
    dt_rows = [results[d - 1]['row'] for e in ev.evalImgs[:len(ev.imgIds)] if e is not None for d in e['dtIds']]
    return dict(dt_rows=np.array(dt_rows, dtype=np.int64),score=score, box_score=box_score, keypoint_score=keypoint_score, keep=keep, nms_oks=nms_oks, ev=ev,
                stats=[float(s) for s in stats], dt_scores=dt_scores, dt_matched=dtm, dt_ignored=dti, npig=npig,
                oks={i: ev.ious[i] for i in ev.imgIds})
