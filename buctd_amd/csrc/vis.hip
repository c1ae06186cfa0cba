// Debug pictures on the device (utils/vis.py): the heat-map grid of save_batch_heatmaps (reference utils/vis.py:269-332)
// and the joint grid of save_batch_image_with_joints (utils/vis.py:75-141), rendered from the tensors of the step into
// uint8 RGB, plus the min / max of the batch image that both normalise with.  The arithmetic is the one stated in
// include/buctd_hip.h, operation by operation: fp32 where it says fp32 (the library is built without contraction),
// integers elsewhere - tests/helpers/vis_ref.py restates it in numpy and the bytes are equal.
//
// MI355X shape of the problem: a few bytes per pixel, memory-bound, nothing reused.  The output is taken as a flat list
// of pixels; a thread renders 4 consecutive ones and writes their 12 bytes as three dwords, so a wavefront writes 768
// contiguous bytes whatever the row length is (a row of (K+1)*Wh*3 bytes is rarely a multiple of 4).  The image taps are
// gathers; the peaks and joints are a few hundred bytes per image, read by every pixel from cache.
#include "common.h"
#include "../../include/buctd_hip.h"

namespace {

struct Image {   // fp32 [B][3][H][W] by element strides
  const float* p;
  int B, H, W;
  long sb, sc, sh, sw;
};

__device__ __forceinline__ int clamp_byte(float v) { return (int)fminf(fmaxf(v, 0.0f), 255.0f); }

// image byte: ((v - lo) / ((hi - lo) + 1e-5f)) * 255, clamped and truncated; without lo / hi, v * 255
__device__ __forceinline__ int image_byte(float v, bool norm, float lo, float den) {
  const float u = norm ? (v - lo) / den : v;
  return clamp_byte(u * 255.0f);
}

// tap position and fixed-point weight of output coordinate x on an axis shrunk from n to m
__device__ __forceinline__ void tap(int x, int n, int m, int* x0, int* x1, int* w) {
  const float fx = ((float)x + 0.5f) * ((float)n / (float)m) - 0.5f;
  const float fl = floorf(fx);
  float a = fx - fl;
  int i0 = (int)fl;
  if (i0 < 0) {
    i0 = 0;
    a = 0.0f;
  }
  int i1 = i0 + 1;
  if (i0 >= n - 1) {
    i0 = i1 = n - 1;
    a = 0.0f;
  }
  *x0 = i0;
  *x1 = i1;
  *w = (int)rintf(a * 2048.0f);
}

// pixel of a position: truncation toward zero (far-away and NaN positions land outside every picture)
__device__ __forceinline__ int pixel_of(float v) { return (int)fminf(fmaxf(v, -1e9f), 1e9f); }

__device__ __forceinline__ int jet_byte(float t, float centre) {
  const float c = fminf(fmaxf(1.5f - fabsf(4.0f * t - centre), 0.0f), 1.0f);
  return (int)floorf(c * 255.0f + 0.5f);
}

// writes the 4 pixels of a thread: three dwords, or single bytes for the last pixels of an output that is no multiple of 4
__device__ __forceinline__ void store_pixels(uint8_t* out, long first, long total, const unsigned (&rgb)[4]) {
  if (first + 4 <= total) {
    const unsigned d0 = (rgb[0] & 0xffffffu) | (rgb[1] << 24);
    const unsigned d1 = ((rgb[1] >> 8) & 0xffffu) | (rgb[2] << 16);
    const unsigned d2 = ((rgb[2] >> 16) & 0xffu) | (rgb[3] << 8);
    unsigned* o = reinterpret_cast<unsigned*>(out + first * 3);   // 12 * thread: dword-aligned
    o[0] = d0;
    o[1] = d1;
    o[2] = d2;
  } else {
    for (int q = 0; first + q < total; ++q) {
      out[(first + q) * 3] = (uint8_t)(rgb[q] & 0xffu);
      out[(first + q) * 3 + 1] = (uint8_t)((rgb[q] >> 8) & 0xffu);
      out[(first + q) * 3 + 2] = (uint8_t)((rgb[q] >> 16) & 0xffu);
    }
  }
}

__device__ __forceinline__ unsigned pack_rgb(int r, int g, int b) { return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16); }

constexpr unsigned RED = 0x0000ffu, GREEN = 0x00ff00u, BLUE = 0xff0000u;   // r | g << 8 | b << 16

__global__ void minmax_init_kernel(float* lohi) {
  lohi[0] = __int_as_float(0x7f800000);
  lohi[1] = __int_as_float(0xff800000);
}

// Grid-stride over the B*3*H*W elements, the axis with the smaller stride of (channel, column) innermost, so that
// NCHW and channels-last images are both read along their memory order.  One atomic pair per block.
__global__ __launch_bounds__(256) void minmax_kernel(Image im, long n, int c_inner, float* lohi) {
  __shared__ float sm_lo[4], sm_hi[4];
  float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    long r = i;
    int c, x, y, b;
    if (c_inner) {
      c = (int)(r % 3); r /= 3;
      x = (int)(r % im.W); r /= im.W;
      y = (int)(r % im.H); b = (int)(r / im.H);
    } else {
      x = (int)(r % im.W); r /= im.W;
      y = (int)(r % im.H); r /= im.H;
      c = (int)(r % 3); b = (int)(r / 3);
    }
    const float v = im.p[b * im.sb + c * im.sc + y * im.sh + x * im.sw];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    sm_lo[threadIdx.x >> 6] = lo;
    sm_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(lohi, fminf(fminf(sm_lo[0], sm_lo[1]), fminf(sm_lo[2], sm_lo[3])));
    atomicMax(lohi + 1, fmaxf(fmaxf(sm_hi[0], sm_hi[1]), fmaxf(sm_hi[2], sm_hi[3])));
  }
}

// byte of channel c (memory order) of the image shrunk to Hh x Wh at (x, y)
struct Shrunk {
  int x0, x1, wa, y0, y1, wb;
};
__device__ __forceinline__ int shrunk_byte(const Image& im, int b, int c, const Shrunk& s, bool norm, float lo, float den) {
  const float* base = im.p + b * im.sb + c * im.sc;
  const int p00 = image_byte(base[s.y0 * im.sh + s.x0 * im.sw], norm, lo, den);
  const int p01 = image_byte(base[s.y0 * im.sh + s.x1 * im.sw], norm, lo, den);
  const int p10 = image_byte(base[s.y1 * im.sh + s.x0 * im.sw], norm, lo, den);
  const int p11 = image_byte(base[s.y1 * im.sh + s.x1 * im.sw], norm, lo, den);
  return ((p00 * (2048 - s.wa) + p01 * s.wa) * (2048 - s.wb) + (p10 * (2048 - s.wa) + p11 * s.wa) * s.wb + (1 << 21)) >> 22;
}

__global__ __launch_bounds__(256) void heatmap_grid_kernel(Image im, const float* __restrict__ lohi,
                                                           const float* __restrict__ hm, int K, int Hh, int Wh,
                                                           const float* __restrict__ peaks, int bgr,
                                                           uint8_t* __restrict__ out, long total) {
  const long first = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (first >= total) return;
  const bool norm = lohi != nullptr;
  const float lo = norm ? lohi[0] : 0.0f;
  const float den = norm ? (lohi[1] - lo) + 1e-5f : 1.0f;
  const long row_px = (long)(K + 1) * Wh;
  unsigned rgb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long px = first + q;
    rgb[q] = 0;
    if (px >= total) continue;
    const long row = px / row_px;
    const int col = (int)(px - row * row_px);
    const int b = (int)(row / Hh), y = (int)(row - (long)b * Hh);
    const int tile = col / Wh, x = col - tile * Wh;
    // the markers drawn so far: joints 0 .. last (all of them in column block 0)
    const int last = tile == 0 ? K - 1 : tile - 1;
    bool marked = false, own = false;
    for (int j = 0; j <= last; ++j) {
      const int cx = pixel_of(peaks[((long)b * K + j) * 2]), cy = pixel_of(peaks[((long)b * K + j) * 2 + 1]);
      const bool hit = abs(x - cx) + abs(y - cy) == 1;
      marked |= hit;
      own = hit && j == last;
    }
    if (marked && (tile == 0 || own)) {
      rgb[q] = RED;
      continue;
    }
    int bg[3] = {255, 0, 0};
    if (!marked) {
      Shrunk s;
      tap(x, im.W, Wh, &s.x0, &s.x1, &s.wa);
      tap(y, im.H, Hh, &s.y0, &s.y1, &s.wb);
#pragma unroll
      for (int c = 0; c < 3; ++c) bg[c] = shrunk_byte(im, b, bgr ? 2 - c : c, s, norm, lo, den);
    }
    if (tile == 0) {
      rgb[q] = pack_rgb(bg[0], bg[1], bg[2]);
      continue;
    }
    const float h = hm[(((long)b * K + (tile - 1)) * Hh + y) * Wh + x];
    const float t = (float)clamp_byte(h * 255.0f) / 255.0f;
    rgb[q] = pack_rgb((7 * jet_byte(t, 3.0f) + 3 * bg[0]) / 10, (7 * jet_byte(t, 2.0f) + 3 * bg[1]) / 10,
                      (7 * jet_byte(t, 1.0f) + 3 * bg[2]) / 10);
  }
  store_pixels(out, first, total, rgb);
}

struct Joints {   // [B][K][2] positions in input pixels, [B][K] visibilities; cond / cond_vis may be null
  const float *pred, *pred_vis, *gt, *gt_vis, *cond, *cond_vis;
};

__global__ __launch_bounds__(256) void joint_grid_kernel(Image im, const float* __restrict__ lohi, int K, Joints jt,
                                                         int xmaps, int padding, int Wg, int bgr,
                                                         uint8_t* __restrict__ out, long total) {
  const long first = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (first >= total) return;
  const bool norm = lohi != nullptr;
  const float lo = norm ? lohi[0] : 0.0f;
  const float den = norm ? (lohi[1] - lo) + 1e-5f : 1.0f;
  const int ch = im.H + padding, cw = im.W + padding;
  unsigned rgb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long px = first + q;
    rgb[q] = 0;
    if (px >= total) continue;
    const int gy = (int)(px / Wg) - padding, gx = (int)(px % Wg) - padding;
    if (gy < 0 || gx < 0) continue;
    const int cy = gy / ch, y = gy - cy * ch, cx = gx / cw, x = gx - cx * cw;
    const long b = (long)cy * xmaps + cx;
    if (y >= im.H || x >= im.W || cx >= xmaps || b >= im.B) continue;
    int mark = -1;   // the last mark that covers the pixel, in the order pred, gt, cond of joint 0, 1, ...
    for (int j = 0; j < K; ++j) {
      const long at = b * K + j;
      if (jt.pred_vis[at] != 0.0f) {
        const int dx = x - pixel_of(jt.pred[at * 2]), dy = y - pixel_of(jt.pred[at * 2 + 1]);
        if (abs(dx) <= 2 && abs(dy) <= 2 && dx * dx + dy * dy <= 8) mark = 0;
      }
      if (jt.gt_vis[at] != 0.0f) {
        const int dx = x - pixel_of(jt.gt[at * 2]), dy = y - pixel_of(jt.gt[at * 2 + 1]);
        if ((dx == 0 && abs(dy) <= 2) || (dy == 0 && abs(dx) <= 2)) mark = 1;
      }
      if (jt.cond && jt.cond_vis[at] > 0.0f) {
        const float fx = jt.cond[at * 2], fy = jt.cond[at * 2 + 1];
        const int dx = x - pixel_of(fx), dy = y - pixel_of(fy);
        if (fx > 0.0f && fy > 0.0f && abs(dx) == abs(dy) && abs(dx) <= 2) mark = 2;
      }
    }
    if (mark >= 0) {
      rgb[q] = mark == 0 ? RED : mark == 1 ? BLUE : GREEN;
      continue;
    }
    const float* base = im.p + b * im.sb + y * im.sh + x * im.sw;
    rgb[q] = pack_rgb(image_byte(base[(bgr ? 2 : 0) * im.sc], norm, lo, den), image_byte(base[im.sc], norm, lo, den),
                      image_byte(base[(bgr ? 0 : 2) * im.sc], norm, lo, den));
  }
  store_pixels(out, first, total, rgb);
}

// blocks of 256 threads x 4 pixels for `total` pixels, or -1 if that is no valid grid size
long pixel_blocks(long total) {
  const long blocks = (total + 1023) / 1024;
  return blocks <= 0x7fffffffL ? blocks : -1;
}

}  // namespace

extern "C" int buctd_vis_minmax(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw, float* lohi,
                                void* stream) {
  BUCTD_CHECK_ARG(img && lohi, "buctd_vis_minmax: null pointer");
  BUCTD_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "buctd_vis_minmax: bad argument (B, H or W < 1)");
  const Image im{img, B, H, W, sb, sc, sh, sw};
  const long n = (long)B * 3 * H * W;
  const long want = (n + 2047) / 2048;   // 8 elements per thread before the grid strides
  hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, lohi);
  hipLaunchKernelGGL(minmax_kernel, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, (hipStream_t)stream, im, n,
                     (sc < 0 ? -sc : sc) < (sw < 0 ? -sw : sw) ? 1 : 0, lohi);
  BUCTD_CHECK_LAUNCH("buctd_vis_minmax");
  return BUCTD_OK;
}

extern "C" int buctd_vis_heatmap_grid(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw,
                                      const float* lohi, const float* heatmaps, int K, int Hh, int Wh, const float* peaks,
                                      int bgr, uint8_t* out, void* stream) {
  BUCTD_CHECK_ARG(img && heatmaps && peaks && out, "buctd_vis_heatmap_grid: null pointer");
  BUCTD_CHECK_ARG(((uintptr_t)out & 3) == 0, "buctd_vis_heatmap_grid: out must be 4-byte aligned");
  BUCTD_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && K >= 1 && Hh >= 1 && Wh >= 1,
                  "buctd_vis_heatmap_grid: bad argument (an extent < 1)");
  BUCTD_CHECK_ARG((long)(K + 1) * Wh <= 0x7fffffffL && (long)B * Hh <= 0x7fffffffL,
                  "buctd_vis_heatmap_grid: the picture is too large");
  const long total = (long)B * Hh * (K + 1) * Wh;
  const long blocks = pixel_blocks(total);
  BUCTD_CHECK_ARG(blocks > 0, "buctd_vis_heatmap_grid: the picture has too many pixels");
  const Image im{img, B, H, W, sb, sc, sh, sw};
  hipLaunchKernelGGL(heatmap_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, im, lohi, heatmaps, K,
                     Hh, Wh, peaks, bgr, out, total);
  BUCTD_CHECK_LAUNCH("buctd_vis_heatmap_grid");
  return BUCTD_OK;
}

extern "C" int buctd_vis_joint_grid(const float* img, int B, int H, int W, long sb, long sc, long sh, long sw,
                                    const float* lohi, int K, const float* pred, const float* pred_vis, const float* gt,
                                    const float* gt_vis, const float* cond, const float* cond_vis, int nrow, int padding,
                                    int bgr, uint8_t* out, void* stream) {
  BUCTD_CHECK_ARG(img && pred && pred_vis && gt && gt_vis && out, "buctd_vis_joint_grid: null pointer");
  BUCTD_CHECK_ARG(((uintptr_t)out & 3) == 0, "buctd_vis_joint_grid: out must be 4-byte aligned");
  BUCTD_CHECK_ARG((cond == nullptr) == (cond_vis == nullptr), "buctd_vis_joint_grid: cond and cond_vis go together");
  BUCTD_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && K >= 1 && nrow >= 1 && padding >= 0,
                  "buctd_vis_joint_grid: bad argument (an extent < 1 or padding < 0)");
  const int xmaps = nrow < B ? nrow : B, ymaps = (B + xmaps - 1) / xmaps;
  const long Hg = (long)ymaps * (H + (long)padding) + padding, Wg = (long)xmaps * (W + (long)padding) + padding;
  BUCTD_CHECK_ARG(Hg <= 0x7fffffffL && Wg <= 0x7fffffffL, "buctd_vis_joint_grid: the picture is too large");
  const long blocks = pixel_blocks(Hg * Wg);
  BUCTD_CHECK_ARG(blocks > 0, "buctd_vis_joint_grid: the picture has too many pixels");
  const Image im{img, B, H, W, sb, sc, sh, sw};
  const Joints jt{pred, pred_vis, gt, gt_vis, cond, cond_vis};
  hipLaunchKernelGGL(joint_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, im, lohi, K, jt, xmaps,
                     padding, (int)Wg, bgr, out, Hg * Wg);
  BUCTD_CHECK_LAUNCH("buctd_vis_joint_grid");
  return BUCTD_OK;
}
