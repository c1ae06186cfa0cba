// Pose error diagnosis on the device: the inverse of synth_pose_kernel (synth.hip).  Given the ground truth, a predicted
// pose (the bottom-up condition) and the neighbours, every labelled joint gets the error type whose candidate region of
// the synthesiser the prediction lies in - good / jitter / inversion / swap / miss, or absent - by the synthesiser's own
// rings (d85, d50 from sigma_j and the area) and sources (own joint, the symmetric partner, the neighbours' joint j and
// pair[j]).  The nearest source decides (ties: own, inversion, swap); at least d50 from every source is a miss.
// DESIGN.md "Pose error diagnosis" holds the definition and why it inverts the synthesiser.
//
// One wavefront per person, lanes over joints (the shape of sample_geometry_kernel): num_valid is a ballot, each lane
// walks the M neighbours of its joint.  The counters (per joint and code; per type, ladder row and class: hits and
// eligible joints) are 64-bit integer atomics and are accumulated into, so a data set is diagnosed batch by batch and
// the result does not depend on scheduling.  float64 throughout, products and sums never fused (-ffp-contract=off).
#include "common.h"
#include "../../include/buctd_hip.h"

struct DiagArgs {
  const double* joints;     // [B][K][3]
  const double* estimated;  // [B][K][3]
  const double* near;       // [B][M][K][3]
  const double* area;       // [B]
  const int* num_overlap;   // [B]
  int* code;                // [B][K]
  double* ks;               // [B][K]
  unsigned long long* hist;       // [4][3][3][2]
  unsigned long long* per_joint;  // [K][6]
  int B, K, M;
  buctd_synth_tables t;
};

__device__ __forceinline__ double sd_dist(double ax, double ay, double bx, double by) {
  const double dx = ax - bx, dy = ay - by;
  return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(256) void pose_error_types_kernel(DiagArgs a) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), j = threadIdx.x & 63;
  if (b >= a.B) return;                                   // whole wavefronts leave: the ballot below sees 64 lanes
  const bool on = j < a.K;
  const int jj = on ? j : 0;
  const double* J = a.joints + (long)b * a.K * 3;
  const double* E = a.estimated + (long)b * a.K * 3;
  const bool scored = on && J[jj * 3 + 2] > 0.0;
  const int nv = __popcll(__ballot(scored));
  if (!on) return;
  const double px = E[j * 3], py = E[j * 3 + 1];
  const bool present = px != 0.0 || py != 0.0;
  int code = -1;
  double ks = 0.0;
  if (scored && !present) code = 5;
  if (scored && present) {
    const double area = a.area[b];
    const double var = (a.t.sigmas[j] * 2.0) * (a.t.sigmas[j] * 2.0);
    const double d50 = sqrt(-2.0 * area * var * log(0.50)), d85 = sqrt(-2.0 * area * var * log(0.85));
    const int pair = a.t.pair[j];
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    const double r0 = sd_dist(px, py, J[j * 3], J[j * 3 + 1]);
    const bool has_inv = pair >= 0 && J[pair * 3 + 2] > 0.0;
    const double rI = has_inv ? sd_dist(px, py, J[pair * 3], J[pair * 3 + 1]) : inf;
    double rS = inf;
    bool has_swap = false;
    for (int m = 0; m < a.M; ++m) {
      const double* N = a.near + (((long)b * a.M + m) * a.K) * 3;
      if (N[j * 3 + 2] > 0.0) { has_swap = true; rS = fmin(rS, sd_dist(px, py, N[j * 3], N[j * 3 + 1])); }
      if (pair >= 0 && N[pair * 3 + 2] > 0.0) {
        has_swap = true;
        rS = fmin(rS, sd_dist(px, py, N[pair * 3], N[pair * 3 + 1]));
      }
    }
    if (fmin(r0, fmin(rI, rS)) >= d50) code = 4;
    else if (r0 <= rI && r0 <= rS) code = r0 < d85 ? 0 : 1;
    else code = rI <= rS ? 2 : 3;
    ks = exp(-(r0 * r0) / (2.0 * area * var));
    // which row of a ladder: synth.hip, the probability lookup of synth_pose_kernel
    const int ov = a.num_overlap[b];
    const int row_jit = nv <= a.t.jitter_nv ? 0 : 1;
    const int row_miss = nv <= a.t.miss_nv[0] ? 0 : (nv <= a.t.miss_nv[1] ? 1 : 2);
    const bool crowded = (nv <= a.t.crowd_nv[0] && ov >= a.t.crowd_ov[0]) ||
                         (nv <= a.t.crowd_nv[1] && ov >= a.t.crowd_ov[1]);
    const int row_swap = crowded ? 0 : 1;
    auto count = [&](int type, int row, int cls, bool hit) {
      unsigned long long* h = a.hist + ((type * 3 + row) * 3 + cls) * 2;
      if (hit) atomicAdd(h, 1ull);
      atomicAdd(h + 1, 1ull);
    };
    count(0, row_jit, a.t.jitter_cls[j], code == 1);
    count(1, row_miss, a.t.miss_cls[j], code == 4);
    if (has_inv) count(2, 0, a.t.inv_cls[j], code == 2);
    if (has_swap) count(3, row_swap, a.t.swap_cls[j], code == 3);
  }
  if (code >= 0) atomicAdd(a.per_joint + j * 6 + code, 1ull);
  a.code[(long)b * a.K + j] = code;
  a.ks[(long)b * a.K + j] = ks;
}

extern "C" int buctd_pose_error_types(const buctd_synth_tables* tables, const double* joints, const double* estimated,
                                      const double* near_joints, const double* area, const int* num_overlap, int B, int K,
                                      int M, int* code, double* ks, long long* hist, long long* per_joint, void* stream) {
  BUCTD_CHECK_ARG(tables && joints && estimated && area && num_overlap && code && ks && hist && per_joint && B > 0 &&
                      K > 0 && K <= 32 && M >= 0 && (M == 0 || near_joints) && M <= 31 && B < (1 << 20),
                  "buctd_pose_error_types: bad argument (K <= 32, M <= 31)");
  for (int j = 0; j < K; ++j) {                 // the tables index the counters and the pose: refuse what would leave them
    const bool cls_ok = tables->jitter_cls[j] >= 0 && tables->jitter_cls[j] < 3 && tables->miss_cls[j] >= 0 &&
                        tables->miss_cls[j] < 3 && tables->inv_cls[j] >= 0 && tables->inv_cls[j] < 3 &&
                        tables->swap_cls[j] >= 0 && tables->swap_cls[j] < 3;
    BUCTD_CHECK_ARG(cls_ok && tables->pair[j] < K,
                    "buctd_pose_error_types: joint %d has a class outside [0, 3) or a pair outside the pose", j);
  }
  DiagArgs a;
  a.joints = joints; a.estimated = estimated; a.near = near_joints; a.area = area; a.num_overlap = num_overlap;
  a.code = code; a.ks = ks; a.hist = (unsigned long long*)hist; a.per_joint = (unsigned long long*)per_joint;
  a.B = B; a.K = K; a.M = M; a.t = *tables;
  hipLaunchKernelGGL(pose_error_types_kernel, dim3(ceil_div(B, 4)), dim3(256), 0, (hipStream_t)stream, a);
  BUCTD_CHECK_LAUNCH("buctd_pose_error_types");
  return BUCTD_OK;
}
