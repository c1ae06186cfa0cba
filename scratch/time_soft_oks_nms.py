"""Times the soft OKS suppression on the synthetic COCO-val-sized set of scratch/time_keypoint_eval.py (about 5000 images,
K = 17), in one process:
  (a) KeypointEvaluator.evaluate with suppression='soft' (the whole call: rescoring, buctd_soft_oks_nms_grouped, matching,
      accumulation), and with suppression='hard' for comparison;
  (b) the host loop the reference's evaluate runs instead of the one launch: nms.soft_oks_nms per image
      (buctd_amd/nms/nms.py, numpy) on the same rescored scores - the suppression step alone.
Wall clock with a device synchronize on both sides of (a); each figure is the median [min, max] of SAMPLES runs after a
warm-up.  The two selections are compared, so the two clocks time the same decisions.

    python scratch/time_soft_oks_nms.py [--images 5000] [--out profiles/soft_oks_nms_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SAMPLES = 7


def host_loop(preds, boxes, image_of, score, sigmas, thresh):
    from buctd_amd.nms import nms
    rows_of = {}
    for r in range(preds.shape[0]):
        rows_of.setdefault(image_of[r], []).append(r)
    keep = np.zeros(preds.shape[0], dtype=bool)
    for rows in rows_of.values():
        db = [{'keypoints': preds[r].astype(np.float64), 'score': score[r], 'area': boxes[r, 4]} for r in rows]
        for k in nms.soft_oks_nms(db, thresh, sigmas):
            keep[rows[k]] = True
    return keep


def timed(fn, sync):
    fn()                                                     # warm-up
    times = []
    for _ in range(SAMPLES):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from types import SimpleNamespace
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    from buctd_amd.nms.nms import COCO_SIGMAS
    from scratch.time_keypoint_eval import K, make_set
    from tests.helpers import kpt_eval_cases as cases
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    gt, preds, boxes, paths = make_set(a.images)
    image_of = [int(p.split('/')[-1].split('.')[0]) for p in paths]
    cfg = SimpleNamespace(OUTPUT_JSON='')
    res = {"images": a.images, "persons": int(preds.shape[0]), "K": K, "device": torch.cuda.get_device_name(0),
           "samples": SAMPLES, "oks_thre": 0.5}
    for mode in ('soft', 'hard'):
        ev = KeypointEvaluator(gt, sigmas=COCO_SIGMAS, image_dir=cases.IMAGE_DIR, suppression=mode)
        _, res[f"a_evaluate_{mode}_s"] = timed(lambda: ev.evaluate(cfg, preds, None, boxes, paths), True)
        res[f"a_kept_persons_{mode}"] = int(ev.tables['keep'].sum())
        if mode == 'soft':
            keep_dev, score = ev.tables['keep'].copy(), ev.tables['score'].copy()
        print(mode, res[f"a_evaluate_{mode}_s"], flush=True)
    keep_host, res["b_host_soft_oks_nms_loop_s"] = timed(
        lambda: host_loop(preds, boxes, image_of, score, COCO_SIGMAS, 0.5), False)
    res["persons_selected_differently"] = int(np.count_nonzero(keep_host != keep_dev))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
