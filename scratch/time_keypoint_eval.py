"""Times the keypoint evaluation on a synthetic COCO-val-sized set (about 5000 images, 1-20 persons each, K = 17):
  (a) KeypointEvaluator.evaluate (core/keypoint_eval.py: rescoring, OKS NMS and matching on the MI355X, accumulation on the
      host), wall clock per call with a device synchronize on both sides, median [min, max] of SAMPLES calls after a warm-up;
  (b) the host path on the same inputs: rescoring + nms.oks_nms per image (buctd_amd/nms/nms.py) followed by the COCOeval
      restatement of tests/helpers/coco_kpt_eval_ref.py - Python loops, timed once.
The ten figures of the two paths are compared, so the two clocks time the same work.

    python scratch/time_keypoint_eval.py [--images 5000] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, SAMPLES = 17, 7


def make_set(images, seed=5):
    from tests.helpers import kpt_eval_cases as cases
    b = cases.CaseBuilder(K, seed)
    rng = b.rng
    for i in range(images):
        image_id = b.image(1 + i)
        for _ in range(rng.randint(1, 21)):
            g = b.gt(image_id, rng.rand(2) * 1500 + 250, cases.SIZES[rng.randint(len(cases.SIZES))])
            b.det_near(g, cases.NOISES[rng.randint(len(cases.NOISES))])
            if rng.rand() < 0.15:
                b.det_near(g, 0.03)                       # a duplicate for the suppression to remove
    return b.build()


def host_path(gt, preds, boxes, image_of, sigmas, in_vis_thre, oks_thre):
    from buctd_amd.nms import nms
    from tests.helpers import coco_kpt_eval_ref as R
    N = preds.shape[0]
    vis = preds[:, :, 2].astype(np.float64)
    counted = vis > in_vis_thre
    kpt_score = np.where(counted.any(1), (vis * counted).sum(1) / np.maximum(counted.sum(1), 1), 0.0)
    score = kpt_score * boxes[:, 5]
    rows_of = {}
    for r in range(N):
        rows_of.setdefault(image_of[r], []).append(r)
    keep = np.zeros(N, dtype=bool)
    for rows in rows_of.values():
        db = [{'keypoints': preds[r].astype(np.float64), 'score': score[r], 'area': boxes[r, 4]} for r in rows]
        for k in nms.oks_nms(db, oks_thre, sigmas):
            keep[rows[k]] = True
    results = [{'image_id': image_of[r], 'keypoints': preds[r].astype(np.float64).reshape(-1), 'score': float(score[r])}
               for r in range(N) if keep[r]]
    return [float(s) for s in R.KeypointEvalRef(gt, results, sigmas).run()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from types import SimpleNamespace
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    from buctd_amd.nms.nms import COCO_SIGMAS
    from tests.helpers import kpt_eval_cases as cases
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    gt, preds, boxes, paths = make_set(a.images)
    image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
    cfg = SimpleNamespace(OUTPUT_JSON='')
    res = {"images": a.images, "persons": int(preds.shape[0]), "ground_truths": len(gt['annotations']), "K": K,
           "device": torch.cuda.get_device_name(0), "samples": SAMPLES}
    t0 = time.perf_counter()
    ev = KeypointEvaluator(gt, sigmas=COCO_SIGMAS, image_dir=cases.IMAGE_DIR)
    torch.cuda.synchronize()
    res["a_construct_s"] = round(time.perf_counter() - t0, 4)
    ev.evaluate(cfg, preds, None, boxes, paths)             # warm-up
    times = []
    for _ in range(SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ap_dev = ev.evaluate(cfg, preds, None, boxes, paths)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["a_evaluate_s"] = [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]
    res["a_kept_persons"] = int(ev.tables['keep'].sum())
    print("a", res["a_evaluate_s"], flush=True)
    t0 = time.perf_counter()
    stats = host_path(gt, preds, boxes, image_of, COCO_SIGMAS, 0.0, 0.5)
    res["b_host_path_s_single_run"] = round(time.perf_counter() - t0, 2)
    res["figures_device"] = ev.tables['stats']
    res["figures_host"] = stats
    res["max_abs_difference"] = float(np.abs(np.asarray(stats) - np.asarray(ev.tables['stats'])).max())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
