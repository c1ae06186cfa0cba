// bf16 inference mode of the HRNet / preNet pose networks (eval forward only; buctd_amd/ops_bf16.py).
//
// Storage: activations bf16 NHWC [N][H][W][C] (raw bit patterns, uint16_t); conv filters folded with their eval
// BatchNorm and rounded once to bf16 into the image [Co][Kp], K = (r * R + s) * Ci + ci, zero for K >= R*R*Ci up to
// Kp = roundup(R*R*Ci, 32); bias fp32 [Co].  Arithmetic: ONE v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation,
// fp32 epilogue (+bias, +bf16 residual, ReLU), one rounding (nearest even) at the store.
//
// Convolution = implicit GEMM, M = N*Ho*Wo output pixels, N = Co, K = R*R*Ci.  A block is 4 waves; each wave owns
// MT x 16 pixels and the block's NT x 16 output channels.  A wave's pixel rows are its own, so the activation fragment
// goes from global memory straight into the MFMA operand registers (16 bytes per lane: 8 channels of one pixel at one
// tap; Ci % 8 == 0) and is reused from registers across the NT channel tiles; the filter fragment is the same for the
// four waves of a block and is served by the L1.  No LDS, no barriers.  The next K step's operands are loaded before
// the MFMAs of the current one.  Ci % 8 != 0 (the stem's Ci = 3) takes an element-wise gather of the same fragment:
// the K padding of such a layer lives in the filter image and in registers, never in the activation tensor.
#include "common.h"
#include "../../include/buctd_hip.h"

typedef __bf16 cb_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short cb_u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float cb_bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// fp32 -> bf16, round to nearest even (NaN stays a quiet NaN) - the rounding of torch's .to(torch.bfloat16)
__device__ __forceinline__ unsigned short cb_f2bf(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

struct Bf16ConvArgs {
  const unsigned short* x;    // [N][H][W][Ci]
  const unsigned short* w;    // [Co][Kp]
  const float* bias;          // [Co]
  const unsigned short* res;  // [N][Ho][Wo][Co] or null
  void* y;                    // bf16 [N][Ho][Wo][Co], or fp32 [N][Co][Ho][Wo] when out_f32_nchw
  int N, H, W, Ci, Co, R, stride, pad, Ho, Wo, Kt, Kp, relu, out_f32_nchw;
};

template <int MT, int NT, bool VEC>
__global__ __launch_bounds__(256) void bf16_conv_kernel(const Bf16ConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long M = (long)a.N * a.Ho * a.Wo;
  const long m0 = ((long)blockIdx.x * 4 + wave) * (MT * 16);
  if (m0 >= M) return;  // no barriers below: an idle wave may leave
  const int co0 = blockIdx.y * (NT * 16);
  const int r16 = lane & 15, kq = (lane >> 4) * 8;

  // pixel of this lane's A row in each M tile; rows past M read nothing and store nothing
  int ihb[MT], iwb[MT];
  long nb[MT];
  bool mv[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const long p = m0 + mt * 16 + r16;
    mv[mt] = p < M;
    const long pc = mv[mt] ? p : 0;
    const int ow = (int)(pc % a.Wo);
    const long t = pc / a.Wo;
    const int oh = (int)(t % a.Ho);
    nb[mt] = (t / a.Ho) * a.H;
    ihb[mt] = oh * a.stride - a.pad;
    iwb[mt] = ow * a.stride - a.pad;
  }
  // filter rows of this lane's B column in each N tile (columns past Co re-read row Co-1; never stored)
  const unsigned short* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = a.w + (long)min(co0 + nt * 16 + r16, a.Co - 1) * a.Kp + kq;

  cb_bf16x8 av[MT], bv[NT];
  int tap = 0, c = kq;  // (tap, channel) of this lane's first K element in the current step (VEC path)
  while (c >= a.Ci) { c -= a.Ci; ++tap; }

  auto load = [&](int k0, cb_bf16x8 (&A)[MT], cb_bf16x8 (&B)[NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) B[nt] = __builtin_bit_cast(cb_bf16x8, *reinterpret_cast<const cb_u16x8*>(wrow[nt] + k0));
    if constexpr (VEC) {
      const bool kv = k0 + kq < a.Kt;
      const int r = tap / a.R, s = tap - r * a.R;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int ih = ihb[mt] + r, iw = iwb[mt] + s;
        cb_u16x8 v = (cb_u16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (kv && mv[mt] && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
          v = *reinterpret_cast<const cb_u16x8*>(a.x + ((nb[mt] + ih) * a.W + iw) * a.Ci + c);
        A[mt] = __builtin_bit_cast(cb_bf16x8, v);
      }
      c += 32;
      while (c >= a.Ci) { c -= a.Ci; ++tap; }
    } else {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        cb_u16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = k0 + kq + j;
          const int tp = k / a.Ci, cc = k - tp * a.Ci, r = tp / a.R, s = tp - r * a.R;
          const int ih = ihb[mt] + r, iw = iwb[mt] + s;
          v[j] = (k < a.Kt && mv[mt] && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
                     ? a.x[((nb[mt] + ih) * a.W + iw) * a.Ci + cc] : (unsigned short)0;
        }
        A[mt] = __builtin_bit_cast(cb_bf16x8, v);
      }
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  load(0, av, bv);
  for (int k0 = 0; k0 < a.Kp; k0 += 32) {
    cb_bf16x8 an[MT], bn[NT];
    const bool more = k0 + 32 < a.Kp;
    if (more) load(k0 + 32, an, bn);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
    if (more) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) av[mt] = an[mt];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bv[nt] = bn[nt];
    }
  }

  // epilogue: lane holds rows (lane >> 4) * 4 + i of column lane & 15 of every 16 x 16 tile
  const long HoWo = (long)a.Ho * a.Wo;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = co0 + nt * 16 + r16;
    if (co >= a.Co) continue;
    const float b = a.bias[co];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long p = m0 + mt * 16 + (lane >> 4) * 4 + i;
        if (p >= M) continue;
        float v = acc[mt][nt][i] + b;
        if (a.res) v += cb_bf2f(a.res[p * a.Co + co]);
        if (a.relu) v = fmaxf(v, 0.f);
        if (a.out_f32_nchw) {
          const long n = p / HoWo;
          static_cast<float*>(a.y)[(n * a.Co + co) * HoWo + (p - n * HoWo)] = v;
        } else {
          static_cast<unsigned short*>(a.y)[p * a.Co + co] = cb_f2bf(v);
        }
      }
  }
}

template <int MT, int NT>
static void launch_conv_mt_nt(const Bf16ConvArgs& a, dim3 grid, hipStream_t st) {
  if (a.Ci % 8 == 0)
    hipLaunchKernelGGL((bf16_conv_kernel<MT, NT, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((bf16_conv_kernel<MT, NT, false>), grid, dim3(256), 0, st, a);
}

template <int NT>
static void launch_conv_nt(const Bf16ConvArgs& a, long M, hipStream_t st) {
  // the largest pixel tile that still gives >= 4 blocks per CU (256 CUs); small maps take MT = 1
  const int nN = ceil_div(a.Co, NT * 16);
  if ((long)ceil_div(M, 256) * nN >= 1024)
    launch_conv_mt_nt<4, NT>(a, dim3(ceil_div(M, 256), nN), st);
  else if ((long)ceil_div(M, 128) * nN >= 1024)
    launch_conv_mt_nt<2, NT>(a, dim3(ceil_div(M, 128), nN), st);
  else
    launch_conv_mt_nt<1, NT>(a, dim3(ceil_div(M, 64), nN), st);
}

extern "C" int buctd_bf16_conv(const uint16_t* x, int N, int H, int W, int Ci, const uint16_t* wimg, const float* bias,
                               int Co, int R, int stride, int pad, const uint16_t* residual, int relu, int out_f32_nchw,
                               void* y, void* workspace, size_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  BUCTD_CHECK_ARG(x && wimg && bias && y && N > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0,
                  "buctd_bf16_conv: null pointer or empty shape");
  BUCTD_CHECK_ARG((R == 1 || R == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad < R,
                  "buctd_bf16_conv: R must be 1 or 3, stride 1 or 2, 0 <= pad < R (got R=%d stride=%d pad=%d)", R,
                  stride, pad);
  BUCTD_CHECK_ARG(!(residual && out_f32_nchw), "buctd_bf16_conv: the fp32 NCHW output takes no residual");
  Bf16ConvArgs a;
  a.x = x;
  a.w = wimg;
  a.bias = bias;
  a.res = residual;
  a.y = y;
  a.N = N, a.H = H, a.W = W, a.Ci = Ci, a.Co = Co, a.R = R, a.stride = stride, a.pad = pad;
  a.Ho = (H + 2 * pad - R) / stride + 1;
  a.Wo = (W + 2 * pad - R) / stride + 1;
  BUCTD_CHECK_ARG(a.Ho > 0 && a.Wo > 0, "buctd_bf16_conv: empty output");
  a.Kt = R * R * Ci;
  a.Kp = (a.Kt + 31) / 32 * 32;
  a.relu = relu ? 1 : 0;
  a.out_f32_nchw = out_f32_nchw ? 1 : 0;
  const long M = (long)N * a.Ho * a.Wo;
  const hipStream_t st = (hipStream_t)stream;
  if (Co <= 32)
    launch_conv_nt<2>(a, M, st);
  else if (Co % 64 != 0 && Co % 48 == 0)
    launch_conv_nt<3>(a, M, st);
  else
    launch_conv_nt<4>(a, M, st);
  BUCTD_CHECK_LAUNCH("buctd_bf16_conv");
  return BUCTD_OK;
}

// ---- filter image: eval BatchNorm (and conv bias) folded in fp32, one rounding to bf16 -------------------------------
//   scale = fp32(gamma / sqrt(var + eps) in fp64);  w' = w * scale;  b' = (bias - mean) * scale + beta  (fp32 ops; no BN:
//   scale 1, b' = bias).  The scale goes through fp64 so that one correctly rounded result is reproducible on any host.
__global__ __launch_bounds__(256) void bf16_pack_kernel(const float* __restrict__ w, long s_co, long s_ci, long s_r,
                                                        long s_s, const float* __restrict__ cbias,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ mean, const float* __restrict__ var,
                                                        float eps, int Co, int Ci, int R, int Kt, int Kp,
                                                        unsigned short* __restrict__ wimg, float* __restrict__ bias_out) {
  const long total = (long)Co * Kp;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int co = (int)(i / Kp), k = (int)(i - (long)co * Kp);
    const float sc = gamma ? (float)((double)gamma[co] / sqrt((double)var[co] + (double)eps)) : 1.f;
    float v = 0.f;
    if (k < Kt) {
      const int tap = k / Ci, ci = k - tap * Ci, r = tap / R, s = tap - r * R;
      v = w[co * s_co + ci * s_ci + r * s_r + s * s_s] * sc;
    }
    wimg[i] = cb_f2bf(v);
    if (k == 0) {
      const float b = cbias ? cbias[co] : 0.f;
      bias_out[co] = gamma ? (b - mean[co]) * sc + beta[co] : b;
    }
  }
}

extern "C" int buctd_bf16_pack_conv(const float* w, long s_co, long s_ci, long s_r, long s_s, int Co, int Ci, int R,
                                    const float* conv_bias, const float* gamma, const float* beta,
                                    const float* running_mean, const float* running_var, float eps, uint16_t* wimg,
                                    float* bias_out, void* stream) {
  BUCTD_CHECK_ARG(w && wimg && bias_out && Co > 0 && Ci > 0 && R > 0, "buctd_bf16_pack_conv: bad argument");
  BUCTD_CHECK_ARG(!gamma || (beta && running_mean && running_var),
                  "buctd_bf16_pack_conv: a BatchNorm needs gamma, beta, running mean and running var");
  const int Kt = R * R * Ci, Kp = (Kt + 31) / 32 * 32;
  const long total = (long)Co * Kp;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(bf16_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, s_co, s_ci, s_r, s_s,
                     conv_bias, gamma, beta, running_mean, running_var, eps, Co, Ci, R, Kt, Kp, wimg, bias_out);
  BUCTD_CHECK_LAUNCH("buctd_bf16_pack_conv");
  return BUCTD_OK;
}

// ---- fuse row: out = relu(sum_j term_j(n, h >> shift_j, w >> shift_j, c)), terms read as bf16, summed in fp32 in
// the order j = 0, 1, ... (the reference's row order), rounded once --------------------------------------------------
struct Bf16FuseArgs {
  const unsigned short* t[4];
  int shift[4];
  int nterms;
};

__global__ __launch_bounds__(256) void bf16_fuse_sum_kernel(const Bf16FuseArgs a, int N, int H, int W, int C8, int relu,
                                                            unsigned short* __restrict__ out) {
  const long total = (long)N * H * W * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    long pix = i / C8;
    const int w = (int)(pix % W);
    pix /= W;
    const int h = (int)(pix % H);
    const int n = (int)(pix / H);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.nterms; ++j) {
      const int sh = a.shift[j];
      const long o = (((long)n * (H >> sh) + (h >> sh)) * (W >> sh) + (w >> sh)) * C8 + c8;
      const cb_u16x8 v = reinterpret_cast<const cb_u16x8*>(a.t[j])[o];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += cb_bf2f(v[e]);
    }
    cb_u16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = cb_f2bf(relu ? fmaxf(s[e], 0.f) : s[e]);
    reinterpret_cast<cb_u16x8*>(out)[i] = r;
  }
}

extern "C" int buctd_bf16_fuse_sum(const uint16_t* const* terms, const int* shifts, int nterms, int N, int H, int W,
                                   int C, int relu, uint16_t* out, void* stream) {
  BUCTD_CHECK_ARG(terms && shifts && out && nterms >= 1 && nterms <= 4, "buctd_bf16_fuse_sum: 1..4 terms");
  BUCTD_CHECK_ARG(C % 8 == 0 && N > 0 && H > 0 && W > 0, "buctd_bf16_fuse_sum: C must be a multiple of 8");
  Bf16FuseArgs a;
  a.nterms = nterms;
  for (int j = 0; j < 4; ++j) {
    a.t[j] = j < nterms ? terms[j] : nullptr;
    a.shift[j] = j < nterms ? shifts[j] : 0;
    if (j < nterms) {
      BUCTD_CHECK_ARG(terms[j] != nullptr && shifts[j] >= 0 && shifts[j] <= 5, "buctd_bf16_fuse_sum: bad term %d", j);
      BUCTD_CHECK_ARG((H >> shifts[j]) << shifts[j] == H && (W >> shifts[j]) << shifts[j] == W,
                      "buctd_bf16_fuse_sum: H/W not divisible by 2^shift for term %d", j);
    }
  }
  const long total = (long)N * H * W * (C / 8);
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(bf16_fuse_sum_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, N, H, W, C / 8, relu,
                     out);
  BUCTD_CHECK_LAUNCH("buctd_bf16_fuse_sum");
  return BUCTD_OK;
}

// ---- fp32 -> bf16 (nearest even): the stem input ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void bf16_from_f32_kernel(const float* __restrict__ x, long n,
                                                            unsigned short* __restrict__ y) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] = cb_f2bf(x[i]);
}

extern "C" int buctd_bf16_from_f32(const float* x, long n, uint16_t* y, void* stream) {
  BUCTD_CHECK_ARG(x && y && n > 0, "buctd_bf16_from_f32: bad argument");
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(bf16_from_f32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, y);
  BUCTD_CHECK_LAUNCH("buctd_bf16_from_f32");
  return BUCTD_OK;
}
