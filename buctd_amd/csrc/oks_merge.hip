// OKS merge of prioritised prediction sets on the device (nms/nms.py: oks_merge_grouped; core/keypoint_eval.py:
// evaluate_merged): the reference's oks_merge (lib/nms/nms.py:127-148) chained over L priority levels,
//     merged = level 0;  for l in 1 .. L-1: merged = oks_merge(level l, merged)
// for every image in one launch.  fp64 like the other OKS kernels: accepting a pose is a comparison against a threshold.
//
// MI355X shape of the problem (as in keypoint_eval.hip): an image is a wave-sized job that exists thousands of times, so
// one wave64 wavefront takes one image.  Lanes stride over the candidates of a level; every lane walks the accepted
// poses of the earlier levels in index order, so the maximum and its position need no shuffle and no atomics.  The
// levels run in sequence inside the wavefront, with a barrier between them: the keep flags of a level are written by the
// lanes that own its candidates and read by every lane at the next level.  A latency kernel of fp64 exps; not tuned, no LDS.
#include "common.h"
#include "oks.h"
#include "../../include/buctd_hip.h"

// cell = cells + img * L: persons [cell[l], cell[l + 1]) are level l of the image.  nms_oks(g = candidate, d = accepted
// pose): oks_iou(kpts_mode0[i], kpts_mode1, ...) of nms.py:142, so use_vis looks at the accepted pose's joint scores.
// The running maximum follows numpy's max / argmax: the first of equal values, and a NaN, once met, stays - then
// `m <= thresh` is false and the candidate is dropped, as `max_oks_ovr <= min_oks_thres` drops it (nms.py:145).
__global__ __launch_bounds__(64) void oks_merge_grouped_kernel(int L, int K, double thresh, int use_vis, double in_vis_thre,
                                                               const int* __restrict__ cells,
                                                               const float* __restrict__ kpts,
                                                               const double* __restrict__ areas,
                                                               const double* __restrict__ sigmas, int* keep,
                                                               double* __restrict__ max_oks, int* __restrict__ best) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int* cell = cells + (long)img * L;
  const int first = cell[0];
  for (int c = first + lane; c < cell[1]; c += 64) {                // level 0: accepted as it is
    keep[c] = 1;
    max_oks[c] = -1.0;
    best[c] = -1;
  }
  for (int l = 1; l < L; ++l) {                                     // L is uniform: every lane meets every barrier
    __syncthreads();                                                // the keep flags of the levels < l are visible
    const int lo = cell[l], hi = cell[l + 1];
    for (int c = lo + lane; c < hi; c += 64) {
      const float* g = kpts + (long)c * K * 3;
      const double a_g = areas[c];
      double m = -1.0;
      int b = -1;
      for (int a = first; a < lo; ++a) {                            // same address in every lane
        if (!keep[a]) continue;                                     // a rejected pose takes part in nothing
        const double v = nms_oks(g, kpts + (long)a * K * 3, a_g, areas[a], sigmas, K, use_vis, in_vis_thre);
        if (b < 0 || v > m || (v != v && m == m)) {
          m = v;
          b = a;
        }
      }
      keep[c] = (b < 0 || m <= thresh) ? 1 : 0;                     // an empty accepted set accepts (nms.py:128-129)
      max_oks[c] = b < 0 ? -1.0 : m;
      best[c] = b;
    }
  }
}

extern "C" int buctd_oks_merge_grouped(const int* cells, int images, int levels, int n, const float* kpts,
                                       const double* areas, const double* sigmas, int K, double thresh, int use_vis,
                                       double in_vis_thre, int* keep, double* max_oks, int* best, void* stream) {
  BUCTD_CHECK_ARG(images >= 0 && levels > 0 && n >= 0 && K > 0, "buctd_oks_merge_grouped: bad argument");
  BUCTD_CHECK_ARG((long)images * levels < (1l << 31) - 1, "buctd_oks_merge_grouped: more than 2^31 - 2 cells");
  if (images == 0 || n == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(cells && kpts && areas && sigmas && keep && max_oks && best, "buctd_oks_merge_grouped: null pointer");
  hipLaunchKernelGGL(oks_merge_grouped_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, levels, K, thresh, use_vis,
                     in_vis_thre, cells, kpts, areas, sigmas, keep, max_oks, best);
  BUCTD_CHECK_LAUNCH("buctd_oks_merge_grouped");
  return BUCTD_OK;
}
