// Condition records on the device (dataset/conditions.py): the boxes of bottom-up poses, the match of every annotation
// to the prediction of its image with the largest box IoU (data_preprocessing/match_coco_cond.py:79-103), and the
// largest overlap of every pose with the others of its image (lib/dataset/dataloader.py:213-241, 335-393).
// Everything is fp64 in plain C++ and, with -ffp-contract=off, equal to the reference's Python values bit for bit.
//
// MI355X shape of the problem (as in keypoint_eval.hip): an image is a wave-sized job that exists thousands of times,
// so one wave64 wavefront takes one image and its lanes stride over the members of the group.  Latency kernels; no
// atomics, no LDS, nothing tuned.
#include <climits>

#include "common.h"
#include "box_iou.h"
#include "../../include/buctd_hip.h"

// One thread per pose.  form 0: x1, y1, x2, y2 over the joints of the mask (all joints without one), negative corners
// cut to 0.  form 1: x, y, w, h over the non-zero x and, separately, the non-zero y, widened by the margin.
__global__ __launch_bounds__(64) void pose_boxes_kernel(int n, int K, int form, double margin,
                                                        const double* __restrict__ poses, const int* __restrict__ mask,
                                                        double* __restrict__ boxes, int* __restrict__ status) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n) return;
  const double* kp = poses + (long)p * K * 3;
  double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
  int nx = 0, ny = 0;
  for (int j = 0; j < K; ++j) {
    const double x = kp[j * 3], y = kp[j * 3 + 1];
    const bool in = form == BUCTD_POSE_BOX_NONZERO || !mask || mask[(long)p * K + j] != 0;
    if (in && (form != BUCTD_POSE_BOX_NONZERO || x != 0)) {
      x0 = nx ? fmin(x0, x) : x;
      x1 = nx ? fmax(x1, x) : x;
      ++nx;
    }
    if (in && (form != BUCTD_POSE_BOX_NONZERO || y != 0)) {
      y0 = ny ? fmin(y0, y) : y;
      y1 = ny ? fmax(y1, y) : y;
      ++ny;
    }
  }
  double* b = boxes + (long)p * 4;
  if (nx == 0 || ny == 0) {
    b[0] = b[1] = b[2] = b[3] = 0.0;
    status[p] = 1;
    return;
  }
  if (form == BUCTD_POSE_BOX_NONZERO) {
    const double xmin = x0 - margin, ymin = y0 - margin, xmax = x1 + margin, ymax = y1 + margin;
    b[0] = xmin; b[1] = ymin; b[2] = xmax - xmin; b[3] = ymax - ymin;
  } else {
    b[0] = x0 < 0 ? 0.0 : x0; b[1] = y0 < 0 ? 0.0 : y0; b[2] = x1 < 0 ? 0.0 : x1; b[3] = y1 < 0 ? 0.0 : y1;
  }
  status[p] = 0;
}

// One wavefront per image.  Per annotation the lanes stride over the image's predictions, each keeping its first
// largest IoU; the butterfly then reduces the pair (IoU, index): larger IoU, and among equal ones the lower index -
// np.argmax over the reference's list, whose all-zero case is index 0.
__global__ __launch_bounds__(64) void match_boxes_kernel(const int* __restrict__ gt_off, const int* __restrict__ pr_off,
                                                         const double* __restrict__ gt_boxes,
                                                         const int* __restrict__ gt_status,
                                                         const double* __restrict__ pr_boxes, int* __restrict__ matched,
                                                         double* __restrict__ best_iou) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int g0 = gt_off[img], G = gt_off[img + 1] - g0;
  const int p0 = pr_off[img], P = pr_off[img + 1] - p0;
  for (int g = 0; g < G; ++g) {
    const bool skip = P <= 0 || (gt_status && gt_status[g0 + g] != 0);     // uniform over the wavefront
    double best = -1.0;
    int at = INT_MAX;
    if (!skip) {
      const double* gb = gt_boxes + (long)(g0 + g) * 4;
      for (int p = lane; p < P; p += 64) {
        const double v = corner_iou(gb, pr_boxes + (long)(p0 + p) * 4);
        if (v > best) {
          best = v;
          at = p;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(best, o, 64);
        const int i = __shfl_xor(at, o, 64);
        if (v > best || (v == best && i < at)) {
          best = v;
          at = i;
        }
      }
    }
    if (lane == 0) {
      const bool none = skip || at == INT_MAX;                              // INT_MAX: every IoU was NaN
      matched[g0 + g] = none ? -1 : p0 + at;
      best_iou[g0 + g] = none ? 0.0 : best;
    }
  }
}

// One wavefront per image, lanes stride over its members; a member walks the whole group.
// form 0 (test): max over j != i of compute_iou, 0 for a single member.
// form 1 (train): calc_bbox_overlap with every member, itself included: max over the overlaps != 1 of a group of more
// than one (0 if none is left), the number of overlaps > 0, status 2 where a union was 0.
__global__ __launch_bounds__(64) void group_max_iou_kernel(int form, const int* __restrict__ off,
                                                           const double* __restrict__ boxes, double* __restrict__ max_iou,
                                                           int* __restrict__ status, int* __restrict__ near_count) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int g0 = off[img], G = off[img + 1] - g0;
  for (int i = lane; i < G; i += 64) {
    const double* bi = boxes + (long)(g0 + i) * 4;
    double m = 0.0;
    bool any = false, zero_union = false;
    int near = 0;
    for (int j = 0; j < G; ++j) {
      const double* bj = boxes + (long)(g0 + j) * 4;
      double v;
      if (form == BUCTD_GROUP_IOU_TRAIN) {
        v = bbox_overlap(bi, bj, &zero_union);
        near += v > 0 ? 1 : 0;
        if (G <= 1 || !(v != 1)) continue;
      } else {
        if (j == i) continue;
        v = box_iou(bi, bj);
      }
      m = any ? py_max(m, v) : v;
      any = true;
    }
    max_iou[g0 + i] = any ? m : 0.0;
    status[g0 + i] = zero_union ? 2 : 0;
    if (near_count) near_count[g0 + i] = near;
  }
}

// The near lists of the train form: member i writes the rows of the members it overlaps (> 0), in ascending order, to
// near_index[near_off[i] ...]; near_off is the prefix sum of the counts of the first launch.
__global__ __launch_bounds__(64) void group_near_list_kernel(const int* __restrict__ off, const double* __restrict__ boxes,
                                                             const long* __restrict__ near_off,
                                                             int* __restrict__ near_index) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int g0 = off[img], G = off[img + 1] - g0;
  for (int i = lane; i < G; i += 64) {
    const double* bi = boxes + (long)(g0 + i) * 4;
    long w = near_off[g0 + i];
    const long end = near_off[g0 + i + 1];
    bool zero_union = false;
    for (int j = 0; j < G && w < end; ++j)
      if (bbox_overlap(bi, boxes + (long)(g0 + j) * 4, &zero_union) > 0) near_index[w++] = g0 + j;
  }
}

extern "C" int buctd_pose_boxes(const double* poses, int n, int K, int form, const int* joint_mask, double margin,
                                double* boxes, int* status, void* stream) {
  BUCTD_CHECK_ARG(n >= 0 && K >= 1, "buctd_pose_boxes: bad argument (n < 0 or K < 1)");
  BUCTD_CHECK_ARG(form == BUCTD_POSE_BOX_ALL_POINTS || form == BUCTD_POSE_BOX_NONZERO, "buctd_pose_boxes: unknown form");
  if (n == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(poses && boxes && status, "buctd_pose_boxes: null pointer");
  hipLaunchKernelGGL(pose_boxes_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, (hipStream_t)stream, n, K, form, margin, poses,
                     form == BUCTD_POSE_BOX_NONZERO ? nullptr : joint_mask, boxes, status);
  BUCTD_CHECK_LAUNCH("buctd_pose_boxes");
  return BUCTD_OK;
}

extern "C" int buctd_match_boxes(const int* gt_offsets, const int* pred_offsets, int images, const double* gt_boxes,
                                 const int* gt_status, const double* pred_boxes, int* matched, double* best_iou,
                                 void* stream) {
  BUCTD_CHECK_ARG(images >= 0, "buctd_match_boxes: bad argument (images < 0)");
  if (images == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(gt_offsets && pred_offsets && gt_boxes && pred_boxes && matched && best_iou,
                  "buctd_match_boxes: null pointer");
  hipLaunchKernelGGL(match_boxes_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, gt_offsets, pred_offsets, gt_boxes,
                     gt_status, pred_boxes, matched, best_iou);
  BUCTD_CHECK_LAUNCH("buctd_match_boxes");
  return BUCTD_OK;
}

extern "C" int buctd_group_max_iou(const int* offsets, int images, const double* boxes, int form, double* max_iou,
                                   int* status, int* near_count, void* stream) {
  BUCTD_CHECK_ARG(images >= 0, "buctd_group_max_iou: bad argument (images < 0)");
  BUCTD_CHECK_ARG(form == BUCTD_GROUP_IOU_TEST || form == BUCTD_GROUP_IOU_TRAIN, "buctd_group_max_iou: unknown form");
  if (images == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(offsets && boxes && max_iou && status, "buctd_group_max_iou: null pointer");
  hipLaunchKernelGGL(group_max_iou_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, form, offsets, boxes, max_iou,
                     status, form == BUCTD_GROUP_IOU_TRAIN ? near_count : nullptr);
  BUCTD_CHECK_LAUNCH("buctd_group_max_iou");
  return BUCTD_OK;
}

extern "C" int buctd_group_near_list(const int* offsets, int images, const double* boxes, const long* near_offsets,
                                     int* near_index, void* stream) {
  BUCTD_CHECK_ARG(images >= 0, "buctd_group_near_list: bad argument (images < 0)");
  if (images == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(offsets && boxes && near_offsets && near_index, "buctd_group_near_list: null pointer");
  hipLaunchKernelGGL(group_near_list_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, offsets, boxes, near_offsets,
                     near_index);
  BUCTD_CHECK_LAUNCH("buctd_group_near_list");
  return BUCTD_OK;
}
