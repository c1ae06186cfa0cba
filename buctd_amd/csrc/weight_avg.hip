// Weight averaging on the flat parameter arena (engine.WeightAverage: EMA, or SWA's equal average): a shadow buffer of the
// arena's layout, updated by one streaming launch behind the optimizer step, and an in-place exchange that puts the averaged
// weights in front of the network for an evaluation and takes them out again.
//
//   buctd_ema_update          avg[i] = fmaf(w, p[i] - avg[i], avg[i]) over one flat buffer
//   buctd_ema_update_tensors  the same rule over a device table of small separate tensors (BatchNorm running statistics)
//   buctd_swap                a[i] <-> b[i], no third buffer
//
// The lerp form is the contract: where p[i] == avg[i] the difference is +0, the product is a zero and the sum is avg[i] again -
// frozen spans, the sine position embedding and the arena's zero padding keep their bits without a table of what to skip,
// and so does everything at w == 0.  One case would slip through: a sum that is zero takes the sign +0 even where avg[i] was
// -0 (fmaf(w, 0, -0) = +0).  ema_one() therefore hands back avg[i] itself whenever the result compares equal to it; the value
// is the formula's in every case, only the sign of a zero is kept.
//
// Streaming shape: 16 bytes per lane and access, 256 threads, a grid of at most 8 workgroups per CU that strides over the
// buffer, no LDS.  12 bytes of traffic per element (two loads, one store) for the update, 16 for the exchange.  Every element
// is computed from its own two inputs alone, so the 16-byte path and the scalar path return the same bits.
#include "common.h"
#include "../../include/buctd_hip.h"

#define WA_MAX_BLOCKS 2048      // 256 CUs x 8 workgroups of 256 threads

__device__ __forceinline__ float ema_one(float p, float a, float w) {
  const float r = __builtin_fmaf(w, p - a, a);
  return r == a ? a : r;
}

// elements [0, n) of one tensor, walked by `threads` threads of which this one is number `first`.  VEC: both pointers are
// 16-byte aligned - n / 4 whole 16-byte pieces, then a scalar tail of n % 4 elements.  p and avg may be the same buffer.
template <bool VEC>
__device__ __forceinline__ void ema_span(const float* p, float* avg, long n, float w, long first, long threads) {
  long done = 0;
  if (VEC) {
    const long n4 = n >> 2;
    for (long i = first; i < n4; i += threads) {
      const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
      f32x4 aa = reinterpret_cast<f32x4*>(avg)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) aa[j] = ema_one(pp[j], aa[j], w);
      reinterpret_cast<f32x4*>(avg)[i] = aa;
    }
    done = n4 << 2;
  }
  for (long i = done + first; i < n; i += threads) avg[i] = ema_one(p[i], avg[i], w);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* p, float* avg, long n, float w) {
  ema_span<VEC>(p, avg, n, w, (long)blockIdx.x * 256 + threadIdx.x, (long)gridDim.x * 256);
}

// workgroup b takes items b, b + gridDim.x, ...; the 256 threads of a workgroup share one item
__global__ __launch_bounds__(256) void ema_update_tensors_kernel(const buctd_avg_item* __restrict__ items, int nitems, float w) {
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const buctd_avg_item item = items[it];
    if ((((uintptr_t)item.src | (uintptr_t)item.avg) & 15) == 0)       // uniform over the workgroup
      ema_span<true>(item.src, item.avg, item.n, w, threadIdx.x, 256);
    else
      ema_span<false>(item.src, item.avg, item.n, w, threadIdx.x, 256);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
  const long first = (long)blockIdx.x * 256 + threadIdx.x, threads = (long)gridDim.x * 256;
  long done = 0;
  if (VEC) {
    const long n4 = n >> 2;
    for (long i = first; i < n4; i += threads) {
      const f32x4 aa = reinterpret_cast<const f32x4*>(a)[i];
      const f32x4 bb = reinterpret_cast<const f32x4*>(b)[i];
      reinterpret_cast<f32x4*>(a)[i] = bb;
      reinterpret_cast<f32x4*>(b)[i] = aa;
    }
    done = n4 << 2;
  }
  for (long i = done + first; i < n; i += threads) {
    const float aa = a[i], bb = b[i];
    a[i] = bb;
    b[i] = aa;
  }
}

static unsigned wa_blocks(long n, bool vec) {
  long blocks = ((vec ? (n + 3) / 4 : n) + 255) / 256;
  return (unsigned)(blocks > WA_MAX_BLOCKS ? WA_MAX_BLOCKS : blocks);
}
static bool wa_aligned(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
// the byte ranges of two n-element float buffers share at least one byte
static bool wa_overlap(const void* a, const void* b, long n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x < y + bytes && y < x + bytes;
}

extern "C" int buctd_ema_update(const float* p, float* avg, long n, float w, void* stream) {
  BUCTD_CHECK_ARG(n >= 0, "buctd_ema_update: n = %ld is negative", n);
  if (n == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(p && avg, "buctd_ema_update: NULL pointer with n = %ld", n);
  BUCTD_CHECK_ARG(p == avg || !wa_overlap(p, avg, n), "buctd_ema_update: p and avg overlap without being the same buffer");
  const bool vec = wa_aligned(p, avg);
  if (vec)
    hipLaunchKernelGGL(ema_update_kernel<true>, dim3(wa_blocks(n, true)), dim3(256), 0, (hipStream_t)stream, p, avg, n, w);
  else
    hipLaunchKernelGGL(ema_update_kernel<false>, dim3(wa_blocks(n, false)), dim3(256), 0, (hipStream_t)stream, p, avg, n, w);
  BUCTD_CHECK_LAUNCH("buctd_ema_update");
  return BUCTD_OK;
}

extern "C" int buctd_ema_update_tensors(const buctd_avg_item* items_device, int nitems, float w, void* stream) {
  BUCTD_CHECK_ARG(nitems >= 0, "buctd_ema_update_tensors: nitems = %d is negative", nitems);
  if (nitems == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(items_device && (uintptr_t)items_device % 8 == 0,
                  "buctd_ema_update_tensors: the item table is NULL or not 8-byte aligned");
  const unsigned blocks = nitems > WA_MAX_BLOCKS ? WA_MAX_BLOCKS : (unsigned)nitems;
  hipLaunchKernelGGL(ema_update_tensors_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, items_device, nitems, w);
  BUCTD_CHECK_LAUNCH("buctd_ema_update_tensors");
  return BUCTD_OK;
}

extern "C" int buctd_swap(float* a, float* b, long n, void* stream) {
  BUCTD_CHECK_ARG(n >= 0, "buctd_swap: n = %ld is negative", n);
  if (n == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(a && b, "buctd_swap: NULL pointer with n = %ld", n);
  BUCTD_CHECK_ARG(!wa_overlap(a, b, n), "buctd_swap: the two buffers overlap");
  const bool vec = wa_aligned(a, b);
  if (vec)
    hipLaunchKernelGGL(swap_kernel<true>, dim3(wa_blocks(n, true)), dim3(256), 0, (hipStream_t)stream, a, b, n);
  else
    hipLaunchKernelGGL(swap_kernel<false>, dim3(wa_blocks(n, false)), dim3(256), 0, (hipStream_t)stream, a, b, n);
  BUCTD_CHECK_LAUNCH("buctd_swap");
  return BUCTD_OK;
}
