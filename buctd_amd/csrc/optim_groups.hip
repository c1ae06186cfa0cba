// Optimizer steps over parameter groups (engine.FusedAdam / FusedSGD with groups=): the Adam and SGD updates of
// loss_decode.hip applied to chosen spans of the flat arena, each span with its own group's hyper-parameters, in one launch.
// The reference's fine-tuning entry freezes all but the last layer and runs Adam over the rest
// (get_last_layer_optimizer, lib/utils/utils.py:277-290); torch's param_groups give the head another learning rate than
// the trunk and keep weight decay off the norm weights and biases.
//
//   buctd_step_chunks       host: cut [start, end) runs, each owned by one group, into chunks of <= BUCTD_STEP_CHUNK elements
//   buctd_adam_step_groups  one launch over a chunk table in device memory, group table in the kernel arguments
//   buctd_sgd_step_groups   the same for SGD
//
// A workgroup of 256 threads takes chunk blockIdx.x, blockIdx.x + gridDim.x, ... ; a chunk is at most 16 rounds of 256 16-byte
// accesses per array, so 1,900 small tensors and one 48-million-element matrix load the CUs alike.  The chunk record (16
// bytes) and the group's entry depend on the workgroup's counter alone: wave-uniform loads, no divergence.  Pure streaming,
// 28 B (Adam) or 12-16 B (SGD) per element.  The per-element arithmetic is step_math.h's, shared with the plain kernels.
#include "common.h"
#include "step_math.h"
#include "../../include/buctd_hip.h"
#include <math.h>

static_assert(BUCTD_STEP_CHUNK % 4 == 0, "a chunk is a whole number of 16-byte accesses");
static_assert(sizeof(buctd_step_chunk) == 16, "one 16-byte record per chunk");

// what the kernels read of a group: everything that needs double arithmetic is formed by the host
struct adam_group_k {
  float lr, b1, b2, eps, bc1, bc2_sqrt;
  float wd;          // coupled decay: g += wd p; 0 in a decoupled group
  float decay_mul;   // decoupled decay: p *= decay_mul; 1 in a coupled group
};
struct adam_table_k { adam_group_k g[BUCTD_STEP_MAX_GROUPS]; };
struct sgd_group_k { float lr, mu, wd; int nesterov; };
struct sgd_table_k { sgd_group_k g[BUCTD_STEP_MAX_GROUPS]; };

template <bool DSCALE>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          const buctd_step_chunk* __restrict__ chunks, long nchunks,
                                                          adam_table_k tab, float gscale, const float* __restrict__ coef) {
  if (DSCALE) gscale = gscale * coef[0];
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const buctd_step_chunk ch = chunks[c];
    const adam_group_k G = tab.g[ch.group];
    const float step_size = G.lr / G.bc1;
    const long base = ch.start >> 2;
    const int n4 = ch.len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[base + i];
      f32x4 gg = reinterpret_cast<const f32x4*>(g)[base + i] * gscale;
      f32x4 mm = reinterpret_cast<f32x4*>(m)[base + i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[base + i];
      if (G.wd != 0.f) gg = gg + G.wd * pp;            // torch.optim.Adam(weight_decay): grad.add(param, alpha = wd)
      if (G.decay_mul != 1.f) pp = pp * G.decay_mul;   // torch.optim.AdamW: param.mul_(1 - lr * wd)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], mj = mm[j], vj = vv[j];
        adam_update(pj, gg[j], mj, vj, G.b1, G.b2, G.eps, step_size, G.bc2_sqrt);
        pp[j] = pj, mm[j] = mj, vv[j] = vj;
      }
      reinterpret_cast<f32x4*>(p)[base + i] = pp;
      reinterpret_cast<f32x4*>(m)[base + i] = mm;
      reinterpret_cast<f32x4*>(v)[base + i] = vv;
    }
  }
}

// buf is dereferenced only in chunks of a group with momentum
template <bool DSCALE>
__global__ __launch_bounds__(256) void sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ buf, const buctd_step_chunk* __restrict__ chunks,
                                                         long nchunks, sgd_table_k tab, float gscale,
                                                         const float* __restrict__ coef) {
  if (DSCALE) gscale = gscale * coef[0];
  for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const buctd_step_chunk ch = chunks[c];
    const sgd_group_k G = tab.g[ch.group];
    const long base = ch.start >> 2;
    const int n4 = ch.len >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[base + i];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[base + i] * gscale;
      f32x4 bb = {0.f, 0.f, 0.f, 0.f};
      if (G.mu != 0.f) bb = reinterpret_cast<f32x4*>(buf)[base + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], bj = bb[j];
        sgd_update(pj, gg[j], bj, G.lr, G.mu, G.wd, G.nesterov, 0);
        pp[j] = pj, bb[j] = bj;
      }
      if (G.mu != 0.f) reinterpret_cast<f32x4*>(buf)[base + i] = bb;
      reinterpret_cast<f32x4*>(p)[base + i] = pp;
    }
  }
}

extern "C" long buctd_step_chunks(const long* runs, const int* run_group, int nruns, buctd_step_chunk* out) {
  if (!runs || !run_group || nruns <= 0) {
    buctd_set_error("buctd_step_chunks: bad argument");
    return -1;
  }
  long count = 0, prev_end = 0;
  for (int r = 0; r < nruns; ++r) {
    const long s = runs[2 * r], e = runs[2 * r + 1];
    if (s < 0 || e <= s || s % 4 != 0 || e % 4 != 0) {
      buctd_set_error("buctd_step_chunks: run %d = [%ld, %ld) is empty or not 16-byte aligned", r, s, e);
      return -1;
    }
    if (s < prev_end) {
      buctd_set_error("buctd_step_chunks: run %d = [%ld, %ld) overlaps or precedes the run before it (ends at %ld)", r, s, e,
                      prev_end);
      return -1;
    }
    if (run_group[r] < 0 || run_group[r] >= BUCTD_STEP_MAX_GROUPS) {
      buctd_set_error("buctd_step_chunks: run %d names group %d, outside [0, %d)", r, run_group[r], BUCTD_STEP_MAX_GROUPS);
      return -1;
    }
    prev_end = e;
    for (long at = s; at < e; at += BUCTD_STEP_CHUNK) {
      if (out) {
        out[count].start = at;
        out[count].len = (int)(e - at < BUCTD_STEP_CHUNK ? e - at : BUCTD_STEP_CHUNK);
        out[count].group = run_group[r];
      }
      ++count;
    }
  }
  return count;
}

// Workgroups of the launch: enough to keep every CU's 32 wave slots busy (8 workgroups of 4 waves per CU), never more than
// the plain kernels' cap or than there are chunks.  The CU count is asked once per device.
static long groups_grid(long nchunks) {
  static int cus[BUCTD_MAX_DEVICES];
  int dev = 0, n = 256;
  if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < BUCTD_MAX_DEVICES) {
    if (cus[dev] == 0) {
      int q = 0;
      cus[dev] = hipDeviceGetAttribute(&q, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && q > 0 ? q : 256;
    }
    n = cus[dev];
  }
  long blocks = (long)n * 8;
  if (blocks > 4096) blocks = 4096;
  return nchunks < blocks ? nchunks : blocks;
}

extern "C" int buctd_adam_step_groups(float* p, const float* g, float* m, float* v, const buctd_step_chunk* chunks_device,
                                      long nchunks, const buctd_adam_group* groups, int ngroups, float gscale,
                                      const float* coef, void* stream) {
  BUCTD_CHECK_ARG(p && g && m && v && chunks_device && groups, "buctd_adam_step_groups: null pointer");
  BUCTD_CHECK_ARG(nchunks > 0, "buctd_adam_step_groups: nchunks = %ld", nchunks);
  BUCTD_CHECK_ARG(ngroups >= 1 && ngroups <= BUCTD_STEP_MAX_GROUPS, "buctd_adam_step_groups: %d groups, 1 .. %d are possible",
                  ngroups, BUCTD_STEP_MAX_GROUPS);
  BUCTD_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)chunks_device) % 16 == 0,
                  "buctd_adam_step_groups: the buffers and the chunk table are 16-byte aligned");
  adam_table_k tab;
  memset(&tab, 0, sizeof tab);
  for (int i = 0; i < ngroups; ++i) {
    const buctd_adam_group& s = groups[i];
    // a group that no chunk names this step may carry step 0 (it has never stepped); its entry is not read
    BUCTD_CHECK_ARG(s.step >= 0, "buctd_adam_step_groups: group %d has step %d", i, s.step);
    const int step = s.step > 0 ? s.step : 1;
    const double bc1 = 1.0 - pow((double)s.beta1, (double)step);      // as adam_launch forms them
    const double bc2 = 1.0 - pow((double)s.beta2, (double)step);
    adam_group_k& d = tab.g[i];
    d.lr = s.lr, d.b1 = s.beta1, d.b2 = s.beta2, d.eps = s.eps;
    d.bc1 = (float)bc1, d.bc2_sqrt = (float)sqrt(bc2);
    d.wd = s.decoupled ? 0.f : s.weight_decay;
    d.decay_mul = s.decoupled ? (float)(1.0 - (double)s.lr * (double)s.weight_decay) : 1.f;
  }
  const long blocks = groups_grid(nchunks);
  if (coef)
    hipLaunchKernelGGL(adam_groups_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       chunks_device, nchunks, tab, gscale, coef);
  else
    hipLaunchKernelGGL(adam_groups_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       chunks_device, nchunks, tab, gscale, coef);
  BUCTD_CHECK_LAUNCH("buctd_adam_step_groups");
  return BUCTD_OK;
}

extern "C" int buctd_sgd_step_groups(float* p, const float* g, float* buf, const buctd_step_chunk* chunks_device, long nchunks,
                                     const buctd_sgd_group* groups, int ngroups, float gscale, const float* coef,
                                     void* stream) {
  BUCTD_CHECK_ARG(p && g && chunks_device && groups, "buctd_sgd_step_groups: null pointer");
  BUCTD_CHECK_ARG(nchunks > 0, "buctd_sgd_step_groups: nchunks = %ld", nchunks);
  BUCTD_CHECK_ARG(ngroups >= 1 && ngroups <= BUCTD_STEP_MAX_GROUPS, "buctd_sgd_step_groups: %d groups, 1 .. %d are possible",
                  ngroups, BUCTD_STEP_MAX_GROUPS);
  BUCTD_CHECK_ARG(((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf | (uintptr_t)chunks_device) % 16 == 0,
                  "buctd_sgd_step_groups: the buffers and the chunk table are 16-byte aligned");
  sgd_table_k tab;
  memset(&tab, 0, sizeof tab);
  for (int i = 0; i < ngroups; ++i) {
    BUCTD_CHECK_ARG(groups[i].momentum == 0.f || buf, "buctd_sgd_step_groups: group %d has a momentum but there is no buffer", i);
    tab.g[i].lr = groups[i].lr, tab.g[i].mu = groups[i].momentum, tab.g[i].wd = groups[i].weight_decay;
    tab.g[i].nesterov = groups[i].nesterov;
  }
  const long blocks = groups_grid(nchunks);
  if (coef)
    hipLaunchKernelGGL(sgd_groups_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                       chunks_device, nchunks, tab, gscale, coef);
  else
    hipLaunchKernelGGL(sgd_groups_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                       chunks_device, nchunks, tab, gscale, coef);
  BUCTD_CHECK_LAUNCH("buctd_sgd_step_groups");
  return BUCTD_OK;
}
