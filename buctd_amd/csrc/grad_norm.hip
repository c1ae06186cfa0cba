// Gradient-norm clipping on the flat gradient arena (engine.FusedAdam / FusedSGD max_grad_norm, engine.clip_grad_norm_,
// engine.grad_stats): the reference clips between backward() and step() (lib/core/train.py:138-141) and watches the
// gradient flow with get_network_grad_flow (lib/utils/utils.py:293-300).
//
//   buctd_grad_sumsq          sum of g^2 over [start, end) runs of the arena, fp64, into one device double
//   buctd_grad_clip_coef      total_norm = gscale sqrt(sumsq), coef = min(1, max_norm / (total_norm + 1e-6)): fp64, stored fp32
//   buctd_grad_segment_stats  mean |g| and ||g||_2 of P parameter spans, fp64
//
// Order guarantee of the reduction.  A run is cut into chunks of GN_CHUNK elements counted from the run's first element;
// one workgroup of 256 threads owns a chunk.  Element j of the chunk belongs to thread (j / 4) % 256 and a thread adds its
// squares in ascending j (a float's square is exact in fp64, so only the additions round); the 256 thread sums meet in a
// xor butterfly per wave and the four wave sums are added in wave order.  The chunk sums (runs in the order given, chunks
// ascending) go to the workspace; one workgroup adds them - thread t takes partials t, t + 256, ... ascending, then the same
// butterfly.  Nothing depends on the grid, on the number of CUs or on the order in which workgroups run, and there are no
// floating-point atomics: the same runs give the same bits.  The 16-byte path (run start 16-byte aligned) loads the four
// elements a thread owns at once; the scalar path loads them one by one - the same elements, the same order, the same bits.
#include "common.h"
#include "../../include/buctd_hip.h"

#define GN_CHUNK BUCTD_GRAD_SUMSQ_CHUNK
#define GN_TRIPS (GN_CHUNK / 1024)       // 16-byte groups of a thread per chunk
static_assert(GN_CHUNK % 1024 == 0, "a chunk is a whole number of 256 x 4-element rounds");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// 256 threads; the result is valid in every thread.  sm: >= 4 doubles
__device__ __forceinline__ double block_sum_256_f64(double v, double* sm) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm[0] + sm[1]) + sm[2]) + sm[3];
}

// one workgroup per chunk of the run g[0, len): partial[blockIdx.x] = sum of squares of its elements
template <bool VEC>
__global__ __launch_bounds__(256) void sumsq_chunk_kernel(const float* __restrict__ g, long len, double* __restrict__ partial) {
  __shared__ double sm[4];
  const long base = (long)blockIdx.x * GN_CHUNK;
  const float* p = g + base;
  const long left = len - base;          // > 0: the grid is ceil(len / GN_CHUNK)
  float x[GN_TRIPS][4];
#pragma unroll
  for (int k = 0; k < GN_TRIPS; ++k) {
    const long j = ((long)k * 256 + threadIdx.x) * 4;
    if (VEC && j + 4 <= left) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + j);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[k][e] = v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[k][e] = j + e < left ? p[j + e] : 0.f;      // +0 adds nothing to a sum of squares
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < GN_TRIPS; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (double)x[k][e];
      acc += d * d;
    }
  acc = block_sum_256_f64(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const double* __restrict__ partial, long count, double* __restrict__ out) {
  __shared__ double sm[4];
  double acc = 0.0;
  // thread t adds partials t, t + 256, ... in ascending order; eight loads are in flight per trip (a partial past the end
  // reads as +0, which changes no sum of non-negative terms), so the one workgroup waits for memory count / 2048 times
  for (long i = threadIdx.x; i < count; i += 256 * 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i + k * 256 < count ? partial[i + k * 256] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += v[k];
  }
  acc = block_sum_256_f64(acc, sm);
  if (threadIdx.x == 0) out[0] = acc;
}

static long gn_chunks(long len) { return (len + GN_CHUNK - 1) / GN_CHUNK; }

extern "C" size_t buctd_grad_sumsq_workspace(const long* runs, int nruns) {
  if (!runs || nruns <= 0) return 0;
  long chunks = 0;
  for (int r = 0; r < nruns; ++r) {
    if (runs[2 * r] < 0 || runs[2 * r + 1] <= runs[2 * r]) return 0;
    chunks += gn_chunks(runs[2 * r + 1] - runs[2 * r]);
  }
  return (size_t)chunks * sizeof(double);
}

extern "C" int buctd_grad_sumsq(const float* g, const long* runs, int nruns, double* sumsq, void* workspace,
                                size_t workspace_bytes, void* stream) {
  BUCTD_CHECK_ARG(g && runs && nruns > 0 && sumsq && workspace, "buctd_grad_sumsq: bad argument");
  const size_t need = buctd_grad_sumsq_workspace(runs, nruns);
  BUCTD_CHECK_ARG(need > 0, "buctd_grad_sumsq: every run needs 0 <= start < end");
  if (workspace_bytes < need || (uintptr_t)workspace % 8 != 0 || (uintptr_t)sumsq % 8 != 0) {
    buctd_set_error("buctd_grad_sumsq: workspace of %zu bytes (8-byte aligned) needed, %zu given", need, workspace_bytes);
    return BUCTD_EWORKSPACE;
  }
  double* partial = (double*)workspace;
  long done = 0;
  for (int r = 0; r < nruns; ++r) {
    const float* p = g + runs[2 * r];
    const long len = runs[2 * r + 1] - runs[2 * r];
    const long chunks = gn_chunks(len);
    BUCTD_CHECK_ARG(chunks <= 0x7fffffffL, "buctd_grad_sumsq: run too long");
    if ((uintptr_t)p % 16 == 0)
      hipLaunchKernelGGL(sumsq_chunk_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, p, len,
                         partial + done);
    else
      hipLaunchKernelGGL(sumsq_chunk_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, p, len,
                         partial + done);
    BUCTD_CHECK_LAUNCH("buctd_grad_sumsq");
    done += chunks;
  }
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, done, sumsq);
  BUCTD_CHECK_LAUNCH("buctd_grad_sumsq");
  return BUCTD_OK;
}

// torch.nn.utils.clip_grad_norm_'s expressions in fp64 (error_if_nonfinite = False: a non-finite norm goes through them like
// any other; the comparison is written so that a NaN coefficient stays NaN, as torch.clamp(max = 1) leaves it)
__global__ void clip_coef_kernel(const double* __restrict__ sumsq, double gscale, double max_norm, float* __restrict__ coef,
                                 float* __restrict__ total_norm) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double tn = gscale * sqrt(sumsq[0]);
  const double c = max_norm / (tn + 1e-6);
  coef[0] = (float)(c > 1.0 ? 1.0 : c);
  total_norm[0] = (float)tn;
}
extern "C" int buctd_grad_clip_coef(const double* sumsq, double gscale, double max_norm, float* coef, float* total_norm,
                                    void* stream) {
  BUCTD_CHECK_ARG(sumsq && coef && total_norm && (uintptr_t)sumsq % 8 == 0, "buctd_grad_clip_coef: bad argument");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, gscale, max_norm, coef, total_norm);
  BUCTD_CHECK_LAUNCH("buctd_grad_clip_coef");
  return BUCTD_OK;
}

// one workgroup per segment [spans[2 s], spans[2 s + 1]): thread t adds elements t, t + 256, ... ascending in fp64, then the
// butterfly of the reduction above - a fixed order.  Off the step's critical path: a monitor.
__global__ __launch_bounds__(256) void segment_stats_kernel(const float* __restrict__ g, const long* __restrict__ spans,
                                                            double* __restrict__ abs_mean, double* __restrict__ norm) {
  __shared__ double sm[4];
  const long s = spans[2 * (long)blockIdx.x], e = spans[2 * (long)blockIdx.x + 1];
  double a = 0.0, q = 0.0;
  for (long i = s + threadIdx.x; i < e; i += 256) {
    const double d = (double)g[i];
    a += fabs(d);
    q += d * d;
  }
  a = block_sum_256_f64(a, sm);
  q = block_sum_256_f64(q, sm);
  if (threadIdx.x == 0) {
    abs_mean[blockIdx.x] = a / (double)(e - s);     // an empty span gives NaN, like torch's mean of nothing
    norm[blockIdx.x] = sqrt(q);
  }
}
extern "C" int buctd_grad_segment_stats(const float* g, const long* spans, int P, double* abs_mean, double* norm,
                                        void* stream) {
  BUCTD_CHECK_ARG(g && spans && P > 0 && abs_mean && norm, "buctd_grad_segment_stats: bad argument");
  hipLaunchKernelGGL(segment_stats_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, g, spans, abs_mean, norm);
  BUCTD_CHECK_LAUNCH("buctd_grad_segment_stats");
  return BUCTD_OK;
}
