// Box overlaps of the reference, restated operation by operation in fp64.  The library is built with -ffp-contract=off,
// so each function returns the bits the reference's Python expression returns for the same float64 inputs.
#pragma once

// max / min as Python's built-ins state them for two arguments (the second only where it compares strictly).
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// compute_iou of lib/utils/utils.py:557-588 (and, with the same operations, JointsDataset.compute_iou,
// lib/dataset/JointsDataset.py:566-597) on two (x, y, w, h) boxes; 0 where the denominator is 0.
__device__ __forceinline__ double box_iou(const double* __restrict__ b1, const double* __restrict__ b2) {
  const double x1_l = b1[0], x1_r = b1[0] + b1[2], y1_t = b1[1], y1_b = b1[1] + b1[3], w1 = b1[2], h1 = b1[3];
  const double x2_l = b2[0], x2_r = b2[0] + b2[2], y2_t = b2[1], y2_b = b2[1] + b2[3], w2 = b2[2], h2 = b2[3];
  const double xi_l = py_max(x1_l, x2_l), xi_r = py_min(x1_r, x2_r);
  const double yi_t = py_max(y1_t, y2_t), yi_b = py_min(y1_b, y2_b);
  const double width = py_max(0.0, xi_r - xi_l), height = py_max(0.0, yi_b - yi_t);
  const double a1 = w1 * h1, a2 = w2 * h2;
  const double inter = width * height;
  const double den = a1 + a2 - inter;
  if (den == 0) return 0.0;
  return inter / den;
}

// _get_iou of data_preprocessing/match_coco_cond.py:33-50 on two (x1, y1, x2, y2) boxes: max((d, 0)) keeps d unless
// 0 is strictly greater, the intersection goes through abs, and an intersection of 0 returns 0 before any division.
__device__ __forceinline__ double corner_iou(const double* __restrict__ a, const double* __restrict__ b) {
  const double xA = py_max(a[0], b[0]), yA = py_max(a[1], b[1]);
  const double xB = py_min(a[2], b[2]), yB = py_min(a[3], b[3]);
  const double inter = fabs(py_max(xB - xA, 0.0) * py_max(yB - yA, 0.0));
  if (inter == 0) return 0.0;
  const double area_a = fabs((a[2] - a[0]) * (a[3] - a[1]));
  const double area_b = fabs((b[2] - b[0]) * (b[3] - b[1]));
  return inter / (area_a + area_b - inter);
}

// calc_bbox_overlap of lib/dataset/dataloader.py:512-535 on two (x, y, w, h) boxes.  The reference divides by a zero
// union; here that pair yields 0 and *zero_union is set.
__device__ __forceinline__ double bbox_overlap(const double* __restrict__ b1, const double* __restrict__ b2,
                                               bool* zero_union) {
  const double x1 = b1[0], y1 = b1[1], w1 = b1[2], h1 = b1[3];
  const double x2 = b2[0], y2 = b2[1], w2 = b2[2], h2 = b2[3];
  const double x1_max = x1 + w1, y1_max = y1 + h1, x2_max = x2 + w2, y2_max = y2 + h2;
  const double x_overlap = py_max(0.0, py_min(x1_max, x2_max) - py_max(x1, x2));
  const double y_overlap = py_max(0.0, py_min(y1_max, y2_max) - py_max(y1, y2));
  const double inter = x_overlap * y_overlap;
  const double uni = w1 * h1 + w2 * h2 - inter;
  if (uni == 0) {
    *zero_union = true;
    return 0.0;
  }
  return inter / uni;
}
