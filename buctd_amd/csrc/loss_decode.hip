// Heat-map side of the path: JointsMSELoss (reference lib/core/loss.py:23-41), arg-max decode
// (lib/core/inference.py:19-47), Gaussian target rendering (lib/dataset/JointsDataset.py:397-453),
// condition heat-map rendering (JointsDataset.py:457-543), flip-test merge (lib/core/function.py:226-236),
// and the fused Adam update (lib/utils/utils.py:268-272).  All HBM-bound; one pass per tensor.
#include "common.h"
#include "step_math.h"
#include "../../include/buctd_hip.h"

// --------------------------------------------------------------- joints MSE ----
// one block per (n,k) heat-map: partial = sum w^2 (p-g)^2 ; grad written in the same pass
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const float* __restrict__ w, int HW, float gcoef,
                                                          float* __restrict__ part, float* __restrict__ grad) {
  __shared__ float sm[4];
  const long row = blockIdx.x;
  const float wt = w ? w[row] : 1.f;
  const float w2 = wt * wt;
  float s = 0.f;
  for (int i = threadIdx.x; i < HW; i += 256) {
    const float d = pred[row * HW + i] - gt[row * HW + i];
    s += d * d;
    if (grad) grad[row * HW + i] = gcoef * w2 * d;
  }
  s = block_sum_256(s, sm);
  if (threadIdx.x == 0) part[row] = s * w2;
}
__global__ __launch_bounds__(256) void mse_final_kernel(const float* __restrict__ part, int n, float coef,
                                                        float* __restrict__ loss) {
  __shared__ float sm[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)part[i];
  // fp64 partial per thread, fp32 across the block is enough for <= 256 addends
  float f = block_sum_256((float)s, sm);
  if (threadIdx.x == 0) loss[0] = f * coef;
}
extern "C" int buctd_joints_mse(const float* pred, const float* gt, const float* w, int N, int K, int HW, float* loss,
                                float* grad, float gscale, void* workspace, size_t workspace_bytes, void* stream) {
  BUCTD_CHECK_ARG(pred && gt && loss && N > 0 && K > 0 && HW > 0, "buctd_joints_mse: bad argument");
  const size_t need = (size_t)N * K * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    buctd_set_error("buctd_joints_mse: workspace %zu bytes < required %zu", workspace_bytes, need);
    return BUCTD_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  // L = 0.5/(K*N*HW) sum w^2 d^2 ; dL/dp = w^2 d / (K*N*HW)
  const float denom = (float)((double)K * (double)N * (double)HW);
  hipLaunchKernelGGL(mse_partial_kernel, dim3(N * K), dim3(256), 0, st, pred, gt, w, HW, gscale / denom,
                     (float*)workspace, grad);
  BUCTD_CHECK_LAUNCH("buctd_joints_mse(partial)");
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, N * K, 0.5f / denom, loss);
  BUCTD_CHECK_LAUNCH("buctd_joints_mse(final)");
  return BUCTD_OK;
}

// ----------------------------------------------------------- joints OHKM MSE ----
// JointsOHKMMSELoss (reference lib/core/loss.py:140-182): the mean over the samples of the mean of each sample's topk
// largest per-joint losses.  The selection needs every per-joint sum first, so the heat-maps are read twice:
//   rows   - one workgroup per (n,k) heat-map: l[n][k] = 0.5/HW w^2 sum (p-g)^2, accumulated in fp64 (the pass is
//            HBM-bound, the fp64 adds are free) and rounded to fp32 once;
//   select - one wavefront per sample ranks its K values in registers (rank = values that are greater + equal values at
//            a lower joint index: ties go to the lower index), writes the per-(n,k) gradient scale - 0 for the joints
//            that were not selected - and sums the selected losses in a fixed order (no atomics);
//   grad   - one workgroup per heat-map: scale * (p-g), or zeros without reading p and g where the scale is 0.
//
// A heat-map starts at float offset row*HW, which is 16-byte aligned only when that is a multiple of 4: `head` scalar
// elements lead up to the first aligned one, `nv` float4s follow, the rest is a scalar tail.  vec == 0 (a base pointer
// off 16 bytes): everything goes through the scalar loop.
struct RowSplit {
  int head, nv, tail0, nscalar;
};
__device__ __forceinline__ RowSplit row_split(long base, int HW, int vec) {
  RowSplit r;
  r.head = vec ? min(HW, (int)((4 - (base & 3)) & 3)) : 0;
  r.nv = vec ? (HW - r.head) >> 2 : 0;
  r.tail0 = r.head + 4 * r.nv;
  r.nscalar = r.head + (HW - r.tail0);
  return r;
}
// i-th scalar element of the row: the head first, then the tail
__device__ __forceinline__ int row_scalar_index(const RowSplit& r, int i) { return i < r.head ? i : r.tail0 + (i - r.head); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void ohkm_rows_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ w, int HW, int vec,
                                                        float* __restrict__ l) {
  __shared__ double sm[4];
  const long row = blockIdx.x;
  const long base = row * HW;
  const RowSplit rs = row_split(base, HW, vec);
  double s = 0.0;
  const f32x4* pv = reinterpret_cast<const f32x4*>(pred + base + rs.head);
  const f32x4* gv = reinterpret_cast<const f32x4*>(gt + base + rs.head);
#pragma unroll 2
  for (int i = threadIdx.x; i < rs.nv; i += 256) {
    const f32x4 p = pv[i], g = gv[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)p[j] - (double)g[j];
      s += d * d;
    }
  }
  for (int i = threadIdx.x; i < rs.nscalar; i += 256) {
    const int e = row_scalar_index(rs, i);
    const double d = (double)pred[base + e] - (double)gt[base + e];
    s += d * d;
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double wt = w ? (double)w[row] : 1.0;
    l[row] = (float)(0.5 / (double)HW * (wt * wt) * (((sm[0] + sm[1]) + sm[2]) + sm[3]));
  }
}

// One workgroup of 16 wavefronts; wavefront v takes the samples v, v + 16, ...  gcoef = gscale / (HW * N * topk).
__global__ __launch_bounds__(1024) void ohkm_select_kernel(const float* __restrict__ l, const float* __restrict__ w,
                                                           int N, int K, int topk, double gcoef,
                                                           float* __restrict__ scale, float* __restrict__ loss) {
  __shared__ double sm[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double s = 0.0;
  for (int n = wave; n < N; n += 16) {  // uniform over the wavefront
    const long row = (long)n * K + lane;
    const float v = lane < K ? l[row] : 0.f;
    const float key = v != v ? INFINITY : v;  // torch.topk's order: a NaN is the largest value
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const float o = __shfl(key, j, 64);
      rank += (o > key || (o == key && j < lane)) ? 1 : 0;
    }
    const bool sel = lane < K && rank < topk;
    if (lane < K) {
      const double wt = w ? (double)w[row] : 1.0;
      scale[row] = sel ? (float)(wt * wt * gcoef) : 0.f;
    }
    s += wave_sum_f64(sel ? (double)v : 0.0);
  }
  if (lane == 0) sm[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 16; ++i) t += sm[i];
    loss[0] = (float)(t / ((double)N * (double)topk));
  }
}

__global__ __launch_bounds__(256) void ohkm_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ scale, int HW, int vec,
                                                        float* __restrict__ grad) {
  const long row = blockIdx.x;
  const long base = row * HW;
  const RowSplit rs = row_split(base, HW, vec);
  const float s = scale[row];  // uniform over the workgroup
  f32x4* dv = reinterpret_cast<f32x4*>(grad + base + rs.head);
  if (s == 0.f) {  // not selected (or weight 0): zeros, pred and gt are not read
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < rs.nv; i += 256) dv[i] = z;
    for (int i = threadIdx.x; i < rs.nscalar; i += 256) grad[base + row_scalar_index(rs, i)] = 0.f;
    return;
  }
  const f32x4* pv = reinterpret_cast<const f32x4*>(pred + base + rs.head);
  const f32x4* gv = reinterpret_cast<const f32x4*>(gt + base + rs.head);
#pragma unroll 2
  for (int i = threadIdx.x; i < rs.nv; i += 256) dv[i] = (pv[i] - gv[i]) * s;
  for (int i = threadIdx.x; i < rs.nscalar; i += 256) {
    const int e = row_scalar_index(rs, i);
    grad[base + e] = (pred[base + e] - gt[base + e]) * s;
  }
}

extern "C" size_t buctd_joints_ohkm_mse_workspace(int N, int K) {
  return N > 0 && K > 0 ? 2 * (size_t)N * (size_t)K * sizeof(float) : 0;
}
extern "C" int buctd_joints_ohkm_mse(const float* pred, const float* gt, const float* w, int N, int K, int HW, int topk,
                                     float* loss, float* grad, float gscale, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  BUCTD_CHECK_ARG(pred && gt && loss && N > 0 && K > 0 && HW > 0, "buctd_joints_ohkm_mse: bad argument");
  BUCTD_CHECK_ARG(K <= BUCTD_OHKM_MAX_JOINTS, "buctd_joints_ohkm_mse: K = %d exceeds the limit of %d joints", K,
                  BUCTD_OHKM_MAX_JOINTS);
  BUCTD_CHECK_ARG(topk >= 1 && topk <= K, "buctd_joints_ohkm_mse: topk = %d is outside 1..K = %d", topk, K);
  BUCTD_CHECK_ARG((long)N * K <= 0x7fffffffL, "buctd_joints_ohkm_mse: N * K = %ld heat-maps exceed the grid limit",
                  (long)N * K);
  const size_t need = buctd_joints_ohkm_mse_workspace(N, K);
  if (!workspace || workspace_bytes < need) {
    buctd_set_error("buctd_joints_ohkm_mse: workspace %zu bytes < required %zu", workspace_bytes, need);
    return BUCTD_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* l = (float*)workspace;
  float* scale = l + (size_t)N * K;
  const int vec = (((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)grad) & 15) == 0;
  hipLaunchKernelGGL(ohkm_rows_kernel, dim3(N * K), dim3(256), 0, st, pred, gt, w, HW, vec, l);
  BUCTD_CHECK_LAUNCH("buctd_joints_ohkm_mse(rows)");
  const double gcoef = (double)gscale / ((double)HW * (double)N * (double)topk);
  hipLaunchKernelGGL(ohkm_select_kernel, dim3(1), dim3(1024), 0, st, (const float*)l, w, N, K, topk, gcoef, scale, loss);
  BUCTD_CHECK_LAUNCH("buctd_joints_ohkm_mse(select)");
  if (grad) {
    hipLaunchKernelGGL(ohkm_grad_kernel, dim3(N * K), dim3(256), 0, st, pred, gt, (const float*)scale, HW, vec, grad);
    BUCTD_CHECK_LAUNCH("buctd_joints_ohkm_mse(grad)");
  }
  return BUCTD_OK;
}

// ------------------------------------------------------------ argmax decode ----
// First-index arg-max of one row h[0..HW) over a 256-thread block (numpy argmax order); the result is valid in thread 0.
__device__ __forceinline__ void block_argmax_256(const float* __restrict__ h, int HW, float& best_out, int& bi_out,
                                                 float* sv /* >= 4 */, int* si /* >= 4 */) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < HW; i += 256) {
    const float v = h[i];
    if (v > best || (v == best && i < bi)) {
      best = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = best;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k)
      if (sv[k] > best || (sv[k] == best && si[k] < bi)) {
        best = sv[k];
        bi = si[k];
      }
    if (bi == 0x7fffffff) bi = 0;  // all-NaN row: numpy argmax would return the first NaN; not reachable here
  }
  best_out = best;
  bi_out = bi;
}

// get_max_preds' outputs for one row from its arg-max (thread 0 only)
__device__ __forceinline__ void store_max_preds(long row, int W, float best, int bi, float* __restrict__ preds,
                                                float* __restrict__ maxvals, int32_t* __restrict__ idx) {
  const float m = best > 0.f ? 1.f : 0.f;
  preds[row * 2 + 0] = (float)(bi % W) * m;
  preds[row * 2 + 1] = floorf((float)bi / (float)W) * m;
  maxvals[row] = best;
  if (idx) idx[row] = bi;
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ hm, int HW, int W,
                                                     float* __restrict__ preds, float* __restrict__ maxvals,
                                                     int32_t* __restrict__ idx, float* __restrict__ quarter) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const long row = blockIdx.x;
  float best;
  int bi;
  block_argmax_256(hm + row * HW, HW, best, bi, sv, si);
  if (threadIdx.x == 0) {
    store_max_preds(row, W, best, bi, preds, maxvals, idx);
    if (quarter) {
      // reference core/inference.py:68-77 (POST_PROCESS): a quarter pixel towards the higher neighbour, only for
      // peaks with 1 < px < W-1 and 1 < py < H-1 (a masked peak decodes to (0,0) and never qualifies)
      const int H = HW / W;
      const int px = best > 0.f ? bi % W : 0, py = best > 0.f ? bi / W : 0;
      float qx = 0.f, qy = 0.f;
      if (px > 1 && px < W - 1 && py > 1 && py < H - 1) {
        const float* h = hm + row * HW;
        const float dx = h[py * W + px + 1] - h[py * W + px - 1];
        const float dy = h[(py + 1) * W + px] - h[(py - 1) * W + px];
        qx = dx > 0.f ? 0.25f : (dx < 0.f ? -0.25f : 0.f);
        qy = dy > 0.f ? 0.25f : (dy < 0.f ? -0.25f : 0.f);
      }
      quarter[row * 2 + 0] = qx;
      quarter[row * 2 + 1] = qy;
    }
  }
}
extern "C" int buctd_argmax_decode(const float* hm, int rows, int H, int W, float* preds, float* maxvals,
                                   int32_t* idx, void* stream) {
  BUCTD_CHECK_ARG(hm && preds && maxvals && rows > 0 && H > 0 && W > 0, "buctd_argmax_decode: bad argument");
  hipLaunchKernelGGL(argmax_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, hm, H * W, W, preds, maxvals, idx,
                     (float*)nullptr);
  BUCTD_CHECK_LAUNCH("buctd_argmax_decode");
  return BUCTD_OK;
}
extern "C" int buctd_argmax_decode_refined(const float* hm, int rows, int H, int W, float* preds, float* maxvals,
                                           int32_t* idx, float* quarter, void* stream) {
  BUCTD_CHECK_ARG(hm && preds && maxvals && quarter && rows > 0 && H > 0 && W > 0,
                  "buctd_argmax_decode_refined: bad argument");
  hipLaunchKernelGGL(argmax_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, hm, H * W, W, preds, maxvals, idx,
                     quarter);
  BUCTD_CHECK_LAUNCH("buctd_argmax_decode_refined");
  return BUCTD_OK;
}

// -------------------------------------------------------------- DARK decode ----
// get_final_preds(use_dark=True) (DarkPose; reference lib/core/inference.py:90-151): arg-max of the unblurred map as
// above, then, for peaks with 1 < px < W-2 and 1 < py < H-2, the 11x11 Gaussian blur of the zero-padded map (float64,
// stored to float32), float32 renormalisation to the original peak, log(max(., 1e-10)) and one Newton step at the peak.
// One 256-thread workgroup per map.  The vertical pass is kept in LDS as float64 ([H*W] doubles, hence the size limit);
// the horizontal pass reduces the blurred map's max; thread 0 then recomputes the 13 blurred samples it needs and solves
// the 2x2 system.  Both passes add the taps in the order of core/inference.py's numpy restatement (rows first, tap 0
// first, -ffp-contract=off), so the blurred float32 values are bit-equal to it.
// gaussian_kernel_1d(11): sigma 0.3*((11-1)*0.5-1)+0.8 = 2, exp(-x^2/(2 sigma^2)) normalised to sum 1 in float64
__constant__ double kDarkTaps[11] = {0.008812229292562283, 0.027143577143479373, 0.06511405659938267, 0.1216490730138096,
                                     0.17699835683135567,  0.20056541423882085,  0.17699835683135567, 0.1216490730138096,
                                     0.06511405659938267,  0.027143577143479373, 0.008812229292562283};

__device__ __forceinline__ double dark_vpass(const float* __restrict__ h, int H, int W, int y, int x) {
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 11; ++t) {
    const int yy = y + t - 5;
    if (yy >= 0 && yy < H) acc = acc + kDarkTaps[t] * (double)h[yy * W + x];
  }
  return acc;
}
__device__ __forceinline__ float dark_hpass(const double* mid, int W, int y, int x) {
  double acc = 0.0;
#pragma unroll
  for (int t = 0; t < 11; ++t) {
    const int xx = x + t - 5;
    if (xx >= 0 && xx < W) acc = acc + kDarkTaps[t] * mid[y * W + xx];
  }
  return (float)acc;
}

__global__ __launch_bounds__(256) void dark_kernel(const float* __restrict__ hm, int H, int W, float* __restrict__ preds,
                                                   float* __restrict__ maxvals, int32_t* __restrict__ idx,
                                                   float* __restrict__ offset) {
  extern __shared__ double mid[];  // [H*W]: the vertical pass
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int s_peak;           // bi of an eligible peak, -1 when the reference leaves the coordinate unchanged
  const long row = blockIdx.x;
  const int HW = H * W;
  const float* h = hm + row * HW;
  float best;
  int bi;
  block_argmax_256(h, HW, best, bi, sv, si);
  if (threadIdx.x == 0) {
    store_max_preds(row, W, best, bi, preds, maxvals, idx);
    // a masked peak (best <= 0) decodes to (0, 0) and never qualifies
    const int px = best > 0.f ? bi % W : 0, py = best > 0.f ? bi / W : 0;
    const bool go = px > 1 && px < W - 2 && py > 1 && py < H - 2;
    s_peak = go ? bi : -1;
    if (!go) {
      offset[row * 2 + 0] = 0.f;
      offset[row * 2 + 1] = 0.f;
    }
  }
  __syncthreads();
  const int peak = s_peak;
  if (peak < 0) return;  // uniform over the workgroup
  for (int i = threadIdx.x; i < HW; i += 256) mid[i] = dark_vpass(h, H, W, i / W, i % W);
  __syncthreads();
  float m = -INFINITY;
  for (int i = threadIdx.x; i < HW; i += 256) m = fmaxf(m, dark_hpass(mid, W, i / W, i % W));
  m = block_max_256(m, sv);
  if (threadIdx.x == 0) {
    const float ratio = best / m;  // reference: hm *= origin_max / np.max(hm), float32
    const int px = peak % W, py = peak / W;
    // log(max(blurred * ratio, 1e-10)) at (y, x), rounded to float32 (np.maximum keeps a NaN)
    auto L = [&](int y, int x) -> double {
      float v = dark_hpass(mid, W, y, x) * ratio;
      v = v < 1e-10f ? 1e-10f : v;
      return (double)(float)log((double)v);
    };
    const double c = L(py, px);
    const double dx = 0.5 * (L(py, px + 1) - L(py, px - 1));
    const double dy = 0.5 * (L(py + 1, px) - L(py - 1, px));
    const double dxx = 0.25 * (L(py, px + 2) - 2.0 * c + L(py, px - 2));
    const double dxy = 0.25 * (L(py + 1, px + 1) - L(py - 1, px + 1) - L(py + 1, px - 1) + L(py - 1, px - 1));
    const double dyy = 0.25 * (L(py + 2, px) - 2.0 * c + L(py - 2, px));
    const double det = dxx * dyy - dxy * dxy;
    double ox = 0.0, oy = 0.0;
    if (det != 0.0) {  // offset = -H^-1 [dx, dy]
      ox = -((dyy * dx - dxy * dy) / det);
      oy = -((dxx * dy - dxy * dx) / det);
    }
    offset[row * 2 + 0] = (float)ox;
    offset[row * 2 + 1] = (float)oy;
  }
}
extern "C" int buctd_argmax_decode_dark(const float* hm, int rows, int H, int W, float* preds, float* maxvals,
                                        int32_t* idx, float* offset, void* stream) {
  BUCTD_CHECK_ARG(hm && preds && maxvals && offset && rows > 0 && H > 0 && W > 0,
                  "buctd_argmax_decode_dark: bad argument");
  BUCTD_CHECK_ARG((long)H * W <= BUCTD_DARK_MAX_PIXELS,
                  "buctd_argmax_decode_dark: %dx%d heat-map exceeds the %d-pixel limit", H, W, BUCTD_DARK_MAX_PIXELS);
  hipLaunchKernelGGL(dark_kernel, dim3(rows), dim3(256), (size_t)H * W * sizeof(double), (hipStream_t)stream, hm, H, W,
                     preds, maxvals, idx, offset);
  BUCTD_CHECK_LAUNCH("buctd_argmax_decode_dark");
  return BUCTD_OK;
}

// ---------------------------------------------------------- gaussian target ----
// one block per (b,k) map
__global__ __launch_bounds__(256) void gaussian_target_kernel(const float* __restrict__ joints,
                                                              const float* __restrict__ vis, int Hh, int Wh,
                                                              float stride_x, float stride_y, float sigma,
                                                              float* __restrict__ target,
                                                              float* __restrict__ weight) {
  const long row = blockIdx.x;
  const float jx = joints[row * 3 + 0], jy = joints[row * 3 + 1];
  float wgt = vis[row];
  // tmp_size = sigma * 3 stays a float in the reference: with sigma = 1.5 the patch is 10 wide, ul and br are truncated
  // toward zero one by one, and the patch's centre is its column size // 2 counted from ul - which is mu only while
  // mu - tmp did not truncate upward (a whole tmp, or ul >= 0)
  const float tmp = sigma * 3.f;
  // int() truncates toward zero, exactly like the reference
  const int mu_x = (int)(jx / stride_x + 0.5f), mu_y = (int)(jy / stride_y + 0.5f);
  const int ulx = (int)((float)mu_x - tmp), uly = (int)((float)mu_y - tmp);
  const int brx = (int)((float)mu_x + tmp + 1.f), bry = (int)((float)mu_y + tmp + 1.f);
  const float c0 = floorf((2.f * tmp + 1.f) * 0.5f);
  const bool outside = ulx >= Wh || uly >= Hh || brx < 0 || bry < 0;
  if (outside) wgt = 0.f;
  const bool paint = !outside && wgt > 0.5f;
  const float inv2s2 = 1.f / (2.f * sigma * sigma);
  for (int i = threadIdx.x; i < Hh * Wh; i += 256) {
    const int y = i / Wh, x = i - y * Wh;
    float v = 0.f;
    if (paint && x >= ulx && x < brx && y >= uly && y < bry) {
      const float dx = (float)(x - ulx) - c0, dy = (float)(y - uly) - c0;
      v = expf(-(dx * dx + dy * dy) * inv2s2);
    }
    target[row * Hh * Wh + i] = v;
  }
  if (threadIdx.x == 0) weight[row] = wgt;
}
extern "C" int buctd_gaussian_target(const float* joints, const float* vis, int B, int K, int Hh, int Wh,
                                     float stride_x, float stride_y, float sigma, float* target, float* weight,
                                     void* stream) {
  BUCTD_CHECK_ARG(joints && vis && target && weight && B > 0 && K > 0 && Hh > 0 && Wh > 0 && sigma > 0.f,
                  "buctd_gaussian_target: bad argument");
  hipLaunchKernelGGL(gaussian_target_kernel, dim3(B * K), dim3(256), 0, (hipStream_t)stream, joints, vis, Hh, Wh,
                     stride_x, stride_y, sigma, target, weight);
  BUCTD_CHECK_LAUNCH("buctd_gaussian_target");
  return BUCTD_OK;
}

// ---------------------------------------------------------- condition render ----
// cv2.GaussianBlur(ksize 15, sigma 0 -> 0.3*((15-1)*0.5-1)+0.8 = 2.6), BORDER_REFLECT_101, separable.
// The impulse image is K points, so instead of a dense blur each output pixel sums the K
// (reflected) point responses: out(y,x) = sum_k col_k * gy(y, py_k) * gx(x, px_k), where g?(.,.)
// accumulates the 1-D taps that land on the impulse after reflection.
struct CondTaps {
  float t[15];
};
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
  }
  return i;
}
__device__ __forceinline__ float tap_response(int out_pos, int src_pos, int n, const CondTaps& tp) {
  // sum of taps d in [-7,7] with reflect101(out_pos + d) == src_pos
  float s = 0.f;
#pragma unroll
  for (int d = -7; d <= 7; ++d)
    if (reflect101(out_pos + d, n) == src_pos) s += tp.t[d + 7];
  return s;
}
__global__ __launch_bounds__(256) void cond_render_kernel(const float* __restrict__ joints, int js,
                                                          const float* __restrict__ colors, int K, int Cc, int H,
                                                          int W, CondTaps tp, float* __restrict__ raw,
                                                          float* __restrict__ maxbuf) {
  // grid: (pixel blocks, B); impulses of image b are cached in LDS
  __shared__ int s_px[64], s_py[64];
  __shared__ float s_col[64][4];
  __shared__ int s_cnt;
  __shared__ float sm[4];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    int cnt = 0;
    for (int k = 0; k < K && cnt < 64; ++k) {
      // np.array(kpts).astype(int): truncation toward zero
      const int kx = (int)joints[((long)b * K + k) * js + 0], ky = (int)joints[((long)b * K + k) * js + 1];
      if (0 < kx && kx < W && 0 < ky && ky < H) {
        // later keypoints overwrite earlier ones at the same pixel (zero_matrix[y][x] = color)
        int slot = cnt;
        for (int q = 0; q < cnt; ++q)
          if (s_px[q] == kx - 1 && s_py[q] == ky - 1) slot = q;
        s_px[slot] = kx - 1;
        s_py[slot] = ky - 1;
        for (int c = 0; c < Cc && c < 4; ++c) s_col[slot][c] = colors ? colors[k * Cc + c] : 255.f;
        if (slot == cnt) ++cnt;
      }
    }
    s_cnt = cnt;
  }
  __syncthreads();
  const int cnt = s_cnt;
  float lmax = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < cnt; ++q) {
      const int dy = s_py[q] - y, dx = s_px[q] - x;
      // reflection can only matter within 7 px of a border; fast reject otherwise
      if ((dy > 7 || dy < -7) && y >= 7 && y < H - 7) continue;
      if ((dx > 7 || dx < -7) && x >= 7 && x < W - 7) continue;
      const float gy = tap_response(y, s_py[q], H, tp);
      if (gy == 0.f) continue;
      const float gx = tap_response(x, s_px[q], W, tp);
      const float g = gy * gx;
      for (int c = 0; c < Cc && c < 4; ++c) acc[c] += s_col[q][c] * g;
    }
    for (int c = 0; c < Cc && c < 4; ++c) {
      raw[(((long)b * Cc + c) * H) * W + i] = acc[c];
      lmax = fmaxf(lmax, acc[c]);
    }
  }
  lmax = block_max_256(lmax, sm);
  // values are >= 0, so the int ordering of the float bits matches the float ordering
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<int*>(maxbuf + b), __float_as_int(lmax));
}
__global__ __launch_bounds__(256) void cond_normalise_kernel(const float* __restrict__ raw,
                                                             const float* __restrict__ maxbuf, long per_img,
                                                             int truncate, float* __restrict__ cond, long cond_stride) {
  const int b = blockIdx.y;
  const float am = maxbuf[b];
  // heatmap /= am / 255  (skipped when the image is empty)
  const float div = am / 255.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_img; i += (long)gridDim.x * 256) {
    const float v = raw[b * per_img + i];
    const float o = am == 0.f ? v : v / div;
    cond[b * cond_stride + i] = truncate ? truncf(o) : o;
  }
}
extern "C" size_t buctd_cond_render_workspace(int B, int Cc, int H, int W) {
  return ((size_t)B * Cc * H * W + (size_t)B) * sizeof(float);
}
extern "C" int buctd_cond_render(const float* joints, int js, const float* colors, int B, int K, int Cc, int H, int W,
                                 int truncate, float* cond, void* workspace, size_t workspace_bytes, void* stream) {
  return buctd_cond_render_into(joints, js, colors, B, K, Cc, H, W, truncate, cond, (long)Cc * H * W, workspace,
                                workspace_bytes, stream);
}
extern "C" int buctd_cond_render_into(const float* joints, int js, const float* colors, int B, int K, int Cc, int H,
                                      int W, int truncate, float* cond, long cond_batch_stride, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  BUCTD_CHECK_ARG(cond_batch_stride >= (long)Cc * H * W, "buctd_cond_render_into: batch stride smaller than one image");
  BUCTD_CHECK_ARG(joints && cond && B > 0 && K > 0 && K <= 64 && Cc >= 1 && Cc <= 4 && H > 0 && W > 0 && js >= 2,
                  "buctd_cond_render: bad argument (K<=64, 1<=Cc<=4)");
  const size_t need = buctd_cond_render_workspace(B, Cc, H, W);
  if (!workspace || workspace_bytes < need) {
    buctd_set_error("buctd_cond_render: workspace %zu bytes < required %zu", workspace_bytes, need);
    return BUCTD_EWORKSPACE;
  }
  // cv2.getGaussianKernel(15, sigma<=0): sigma = 0.3*((ksize-1)*0.5 - 1) + 0.8 ; taps normalised to sum 1
  CondTaps tp;
  const double sigma = 0.3 * ((15 - 1) * 0.5 - 1.0) + 0.8;
  double sum = 0.0, tv[15];
  for (int i = 0; i < 15; ++i) {
    const double x = (double)i - 7.0;
    tv[i] = exp(-(x * x) / (2.0 * sigma * sigma));
    sum += tv[i];
  }
  for (int i = 0; i < 15; ++i) tp.t[i] = (float)(tv[i] / sum);
  hipStream_t st = (hipStream_t)stream;
  float* raw = (float*)workspace;
  float* maxbuf = raw + (size_t)B * Cc * H * W;
  hipError_t e = hipMemsetAsync(maxbuf, 0, (size_t)B * sizeof(float), st);
  if (e != hipSuccess) {
    buctd_set_error("buctd_cond_render: memset failed: %s", hipGetErrorString(e));
    return BUCTD_ELAUNCH;
  }
  dim3 grid(ceil_div(H * W, 256 * 4), B);
  hipLaunchKernelGGL(cond_render_kernel, grid, dim3(256), 0, st, joints, js, colors, K, Cc, H, W, tp, raw, maxbuf);
  BUCTD_CHECK_LAUNCH("buctd_cond_render(render)");
  const long per_img = (long)Cc * H * W;
  dim3 grid2(ceil_div(per_img, 256 * 4), B);
  hipLaunchKernelGGL(cond_normalise_kernel, grid2, dim3(256), 0, st, (const float*)raw, (const float*)maxbuf, per_img,
                     truncate, cond, cond_batch_stride);
  BUCTD_CHECK_LAUNCH("buctd_cond_render(normalise)");
  return BUCTD_OK;
}

// --------------------------------------------------------------- flip-back ----
__global__ __launch_bounds__(256) void flipback_avg_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const int32_t* __restrict__ perm, int K, int H, int W,
                                                           int shift, long total, float* __restrict__ out) {
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const int x = (int)(i % W);
    long r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int k = (int)(r % K);
    const long n = r / K;
    // flipped[n][k][y][x'] = b[n][perm[k]][y][W-1-x'] ; shift: out x reads flipped x-1 for x >= 1, x = 0 keeps x = 0
    const int xs = (shift && x >= 1) ? x - 1 : x;
    const float fv = b[((n * K + perm[k]) * H + y) * W + (W - 1 - xs)];
    out[i] = (a[i] + fv) * 0.5f;
  }
}
extern "C" int buctd_flipback_avg(const float* a, const float* b, const int32_t* perm, int N, int K, int H, int W,
                                  int shift, float* out, void* stream) {
  BUCTD_CHECK_ARG(a && b && perm && out && N > 0 && K > 0 && H > 0 && W > 0, "buctd_flipback_avg: bad argument");
  const long total = (long)N * K * H * W;
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(flipback_avg_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, perm, K, H,
                     W, shift, total, out);
  BUCTD_CHECK_LAUNCH("buctd_flipback_avg");
  return BUCTD_OK;
}

// --------------------------------------------------------------------- adam ----
// DSCALE: the _dscale entry - gscale is multiplied by the clip coefficient read from device memory (one wave-uniform load at
// kernel start); everything behind that line is the plain step's code, so *coef == 1.0f returns its bits.
template <bool DSCALE>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                   float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   float gscale, const float* __restrict__ coef) {
  if (DSCALE) gscale = gscale * coef[0];
  // torch.optim.Adam (no amsgrad, no weight decay): adam_update of step_math.h on every element
  const float step_size = lr / bc1;
  const long n4 = n >> 2;
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pp[j], mj = mm[j], vj = vv[j];
      adam_update(pj, gg[j], mj, vj, b1, b2, eps, step_size, bc2_sqrt);
      pp[j] = pj, mm[j] = mj, vv[j] = vj;
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
  }
  for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_update(pp, g[i] * gscale, mm, vv, b1, b2, eps, step_size, bc2_sqrt);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
}
template <bool DSCALE>
static int adam_launch(const char* who, float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                       float beta2, float eps, int step, float gscale, const float* coef, void* stream) {
  BUCTD_CHECK_ARG(p && g && m && v && n > 0 && step >= 1 && (!DSCALE || coef), "%s: bad argument", who);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  long blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adam_kernel<DSCALE>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                     beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), gscale, coef);
  BUCTD_CHECK_LAUNCH(who);
  return BUCTD_OK;
}
extern "C" int buctd_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                               float beta2, float eps, int step, float gscale, void* stream) {
  return adam_launch<false>("buctd_adam_step", p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, nullptr, stream);
}
extern "C" int buctd_adam_step_dscale(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                                      float beta2, float eps, int step, float gscale, const float* coef, void* stream) {
  return adam_launch<true>("buctd_adam_step_dscale", p, g, m, v, n, lr, beta1, beta2, eps, step, gscale, coef, stream);
}

// ---------------------------------------------------------------------- sgd ----
// torch.optim.SGD(lr, momentum, dampening = 0, weight_decay, nesterov) on the flat arena - the 'sgd' branch of the
// reference's get_optimizer (lib/utils/utils.py:260-267):
//   g += wd p ;  buf = g (first step) | mu buf + g ;  g = nesterov ? g + mu buf : buf ;  p -= lr g        (mu = 0: no buffer)
// DSCALE: as in adam_kernel - the clipped gradient is g * (gscale * *coef), formed before the weight-decay term
template <bool DSCALE>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  long n, float lr, float mu, float wd, int nesterov, int first, float gscale,
                                                  const float* __restrict__ coef) {
  if (DSCALE) gscale = gscale * coef[0];
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    float pp = p[i];
    float b = (mu != 0.f && !first) ? buf[i] : 0.f;
    sgd_update(pp, g[i] * gscale, b, lr, mu, wd, nesterov, first);
    if (mu != 0.f) buf[i] = b;
    p[i] = pp;
  }
}
template <bool DSCALE>
static int sgd_launch(const char* who, float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                      float weight_decay, int nesterov, int first_step, float gscale, const float* coef, void* stream) {
  BUCTD_CHECK_ARG(p && g && n > 0 && (momentum == 0.f || momentum_buf) && (!DSCALE || coef), "%s: bad argument", who);
  long blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(sgd_kernel<DSCALE>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, momentum_buf, n,
                     lr, momentum, weight_decay, nesterov, first_step, gscale, coef);
  BUCTD_CHECK_LAUNCH(who);
  return BUCTD_OK;
}
extern "C" int buctd_sgd_step(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                              float weight_decay, int nesterov, int first_step, float gscale, void* stream) {
  return sgd_launch<false>("buctd_sgd_step", p, g, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step, gscale,
                           nullptr, stream);
}
extern "C" int buctd_sgd_step_dscale(float* p, const float* g, float* momentum_buf, long n, float lr, float momentum,
                                     float weight_decay, int nesterov, int first_step, float gscale, const float* coef,
                                     void* stream) {
  return sgd_launch<true>("buctd_sgd_step_dscale", p, g, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step,
                          gscale, coef, stream);
}
