"""Times the crowding analysis (core/keypoint_analysis.py) on a synthetic COCO-val-sized set (about 2300 images and 6400
persons, K = 17, tests/helpers/kpt_analysis_cases.coco_sized_set):
  (a) CrowdingAnalysis.bins and .instances, wall clock per call with a device synchronize on both sides, median
      [min, max] of SAMPLES calls after a warm-up; the construction (buctd_kpt_crowding + uploads) once;
  (b) the per-person figures again on the host of the same machine: this package's accumulate / summarize called once per
      person on the match tables of (a) - the same work as the one buctd_kpt_segment_ap launch - median of SAMPLES runs.
The two sets of per-person figures are compared.  The reference's own path (pycocotools, one deep copy of the ground
truth per person) is not timed: pycocotools is not installed.

    python scratch/time_keypoint_analysis.py [--images 2300] [--out FILE.json]"""
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


def timed(fn):
    times = []
    for _ in range(SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def host_per_person(an, scores):
    from buctd_amd.core.keypoint_eval import accumulate, summarize
    t = an.instance_tables
    out = np.zeros((len(t['gt_ids']), 10))
    for s in range(out.shape[0]):
        d0, d1 = t['dt_offsets'][s], t['dt_offsets'][s + 1]
        out[s] = summarize(*accumulate(scores[t['dt_rows'][d0:d1]], t['dt_matched'][:, :, d0:d1],
                                       t['dt_ignored'][:, :, d0:d1], t['npig'][s]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from buctd_amd.core.keypoint_analysis import CrowdingAnalysis
    from buctd_amd.core.keypoint_eval import KeypointEvaluator
    from buctd_amd.nms.nms import COCO_SIGMAS
    from tests.helpers import kpt_analysis_cases as cases
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    gt, preds, boxes, paths = cases.coco_sized_set(17, 3, a.images)
    ev = KeypointEvaluator(gt, sigmas=COCO_SIGMAS, image_dir=cases.IMAGE_DIR)
    res = {"images": a.images, "ground_truths": len(gt['annotations']), "persons": int(preds.shape[0]), "K": 17,
           "device": torch.cuda.get_device_name(0), "samples": SAMPLES}
    CrowdingAnalysis(ev)                                      # warm-up of the construction
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    an = CrowdingAnalysis(ev)
    torch.cuda.synchronize()
    res["a_construct_s"] = round(time.perf_counter() - t0, 4)
    res["valid_annotations"] = int(an.valid.sum())
    res["annotations_in_a_bin"] = int((an.bin_of_gt >= 0).sum())
    an.bins(preds, boxes, paths)
    an.instances(preds, boxes, paths)
    tables, res["a_bins_s"] = timed(lambda: an.bins(preds, boxes, paths))
    _, res["a_instances_s"] = timed(lambda: an.instances(preds, boxes, paths))
    res["num_instances"] = tables['num_instances'].tolist()
    res["AP"] = tables['AP'].tolist()
    scores = ev._kept_persons(preds, boxes, paths).score_h
    host, res["b_host_accumulate_per_person_s"] = timed(lambda: host_per_person(an, scores))
    res["max_abs_difference_per_person"] = float(np.abs(host - an.instance_tables['stats']).max())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
