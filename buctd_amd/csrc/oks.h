// Object-keypoint similarity of one pose pair in fp64: oks_iou of nms/nms.py:86-105.  The one statement of it on the
// device, for the grouped suppression kernels of keypoint_eval.hip (float32 poses) and the track step of sample.hip
// (float64 poses).
#pragma once
#include "common.h"

#define KPT_SPACING1 2.220446049250313e-16   // np.spacing(1)

// g, d: [K][3] rows (x, y, score) of float32 or float64; a_g, a_d: the areas.  With use_vis only the joints whose score in
// d exceeds in_vis_thre count.  Joint order, one rounding per operation.
template <typename TG, typename TD>
__device__ __forceinline__ double nms_oks(const TG* __restrict__ g, const TD* __restrict__ d, double a_g, double a_d,
                                          const double* __restrict__ sigmas, int K, int use_vis, double in_vis_thre) {
  const double scale = (a_g + a_d) / 2 + KPT_SPACING1;
  double sum = 0.0;
  int cnt = 0;
  for (int j = 0; j < K; ++j) {
    if (use_vis && !((double)d[j * 3 + 2] > in_vis_thre)) continue;
    const double dx = (double)d[j * 3 + 0] - (double)g[j * 3 + 0];
    const double dy = (double)d[j * 3 + 1] - (double)g[j * 3 + 1];
    const double var = (sigmas[j] * 2) * (sigmas[j] * 2);
    const double e = (dx * dx + dy * dy) / var / scale / 2;
    sum += exp(-e);
    ++cnt;
  }
  return cnt > 0 ? sum / cnt : 0.0;
}
