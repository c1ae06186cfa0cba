// Device side of the per-sample input pipeline (reference lib/dataset/JointsDataset.py:134-361):
// affine person crop + ToTensor + Normalize in one kernel, written straight into the channels [0, 3) of the NCHW network
// input.  The Gaussian target (buctd_gaussian_target) and the condition heat-map (buctd_cond_render_into, which fills
// channels [3, 3+Cc)) are the other two kernels of a batch.
//
// The crop restates cv2.warpAffine(src_u8, M, (w, h), flags=INTER_LINEAR) (JointsDataset.py:287-291) bit for bit as
// OpenCV computes it on 8-bit images (imgwarp.cpp): M inverted in double; per destination pixel the source coordinate
// in 1/1024 px (rounded half-to-even per term), + 16, >> 5 -> 1/32 px; the four neighbours weighted by
// (32-fy)(32-fx)*32 ... fy*fx*32 (sum 2^15, exact - OpenCV's table correction never fires for the bilinear table);
// (sum + 2^14) >> 15; BORDER_CONSTANT 0.  HBM-bound: one pass, ~4 source bytes read (L2-served neighbours) and 12 bytes
// written per destination pixel.
#include "common.h"
#include "oks.h"
#include "../../include/buctd_hip.h"

struct WarpParams {
  const buctd_warp_item* items;
  int dh, dw;
  float mean[3], inv_std[3];
  float* out;            // [B][>=3][dh][dw] float32, normalised
  long out_batch_stride;
  unsigned char* crop;   // optional [B][dh][dw][3] uint8 (meta['input_img'])
};

__device__ __forceinline__ int sat_int(double v) {
  v = rint(v);                                   // cvRound: half to even
  v = fmin(fmax(v, -2147483648.0), 2147483647.0);
  return (int)v;
}

__global__ __launch_bounds__(256) void warp_affine_norm_kernel(WarpParams p) {
  const int b = blockIdx.y;
  const buctd_warp_item it = p.items[b];
  // invert M exactly like cv::warpAffine (double, this operation order)
  double m0 = it.m[0], m1 = it.m[1], m2 = it.m[2], m3 = it.m[3], m4 = it.m[4], m5 = it.m[5];
  double d = m0 * m4 - m1 * m3;
  d = d != 0.0 ? 1.0 / d : 0.0;
  const double a11 = m4 * d, a22 = m0 * d;
  m0 = a11; m1 *= -d; m3 *= -d; m4 = a22;
  const double b1 = -m0 * m2 - m1 * m5, b2 = -m3 * m2 - m4 * m5;
  m2 = b1; m5 = b2;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.dh * p.dw; i += gridDim.x * 256) {
    const int y = i / p.dw, x = i - y * p.dw;
    const int adelta = sat_int(m0 * (double)x * 1024.0), bdelta = sat_int(m3 * (double)x * 1024.0);
    const int x0 = sat_int((m1 * (double)y + m2) * 1024.0) + 16, y0 = sat_int((m4 * (double)y + m5) * 1024.0) + 16;
    const int X = (x0 + adelta) >> 5, Y = (y0 + bdelta) >> 5;
    int sx = X >> 5, sy = Y >> 5;
    sx = min(max(sx, -32768), 32767);
    sy = min(max(sy, -32768), 32767);
    const int fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    int acc[3] = {0, 0, 0};
    auto tap = [&](int yy, int xx, int wgt) {
      if (wgt == 0 || yy < 0 || yy >= it.H || xx < 0 || xx >= it.W) return;
      if (it.rw > 0 && (xx < it.rx || xx >= it.rx + it.rw || yy < it.ry || yy >= it.ry + it.rh)) return;
      const int xs = it.flip ? it.W - 1 - xx : xx;
      const unsigned char* s = it.src + ((long)yy * it.W + xs) * 3;
      acc[0] += wgt * (int)s[0];
      acc[1] += wgt * (int)s[1];
      acc[2] += wgt * (int)s[2];
    };
    tap(sy, sx, w00);
    tap(sy, sx + 1, w01);
    tap(sy + 1, sx, w10);
    tap(sy + 1, sx + 1, w11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = min(max((acc[c] + (1 << 14)) >> 15, 0), 255);
      // ToTensor: v / 255 in float32; Normalize: (t - mean) / std in float32 (a division, like torchvision)
      const float t = (float)v / 255.f;
      p.out[(long)b * p.out_batch_stride + ((long)c * p.dh + y) * p.dw + x] = (t - p.mean[c]) / p.inv_std[c];
      if (p.crop) p.crop[(((long)b * p.dh + y) * p.dw + x) * 3 + c] = (unsigned char)v;
    }
  }
}

extern "C" int buctd_warp_affine_norm(const buctd_warp_item* items_device, int B, int dst_h, int dst_w,
                                      const float* mean3, const float* std3, float* out, long out_batch_stride,
                                      unsigned char* crop_u8, void* stream) {
  BUCTD_CHECK_ARG(items_device && out && mean3 && std3 && B > 0 && dst_h > 0 && dst_w > 0 &&
                      out_batch_stride >= 3L * dst_h * dst_w,
                  "buctd_warp_affine_norm: bad argument");
  WarpParams p;
  p.items = items_device; p.dh = dst_h; p.dw = dst_w; p.out = out; p.out_batch_stride = out_batch_stride; p.crop = crop_u8;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.inv_std[c] = std3[c]; }   // inv_std holds std: divided by
  dim3 grid(ceil_div((long)dst_h * dst_w, 256 * 2), B);
  hipLaunchKernelGGL(warp_affine_norm_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
  BUCTD_CHECK_LAUNCH("buctd_warp_affine_norm");
  return BUCTD_OK;
}

// np.array(kpts).astype(int) of JointsDataset.py:521 as float32: a [., 2] row of the render kernel's `joints`
__device__ __forceinline__ void store_trunc(float* dst, double x, double y) {
  dst[0] = (float)trunc(x);
  dst[1] = (float)trunc(y);
}

// fliplr_joints (utils/transforms.py:61-75) + the crop affine for joint j of one [K][js] pose, js = 2 or 3 (without a
// third column z is 0), the one statement of both on the device.  flip: x = (W - x) - 1, row and visibility taken from
// the partner, joints * joints_vis (so a "missed" joint (0, 0) comes back as (W - 1, 0) times its visibility, like in the
// reference); then through m (NULL: no affine) where vis[., 0] > 0.  vis NULL: all ones - the products with 1.0 stay,
// which is bit-identical to not multiplying for every value that is not a NaN.  Every float64 product and sum is rounded
// on its own (__dmul_rn / __dadd_rn / __dsub_rn: never contracted into an fma).
struct GeomPoint { double x, y, z, v0, v1, v2; };
__device__ __forceinline__ GeomPoint geom_point(const double* pose, int js, const double* vis, int j, int K, bool flip,
                                                const int* pair, double W, const double* m) {
  int src = j;
  if (flip) {
    const int q = pair[j];
    if (q >= 0 && q < K) src = q;
  }
  GeomPoint g = {pose[src * js], pose[src * js + 1], js > 2 ? pose[src * js + 2] : 0.0, 1.0, 1.0, 1.0};
  if (vis) { g.v0 = vis[src * 3]; g.v1 = vis[src * 3 + 1]; g.v2 = vis[src * 3 + 2]; }
  if (flip) {
    g.x = __dmul_rn(__dsub_rn(__dsub_rn(W, g.x), 1.0), g.v0);
    g.y = __dmul_rn(g.y, g.v1);
    g.z = __dmul_rn(g.z, g.v2);
  }
  if (m && g.v0 > 0.0) {
    const double tx = __dadd_rn(__dadd_rn(__dmul_rn(m[0], g.x), __dmul_rn(m[1], g.y)), m[2]);
    const double ty = __dadd_rn(__dadd_rn(__dmul_rn(m[3], g.x), __dmul_rn(m[4], g.y)), m[5]);
    g.x = tx;
    g.y = ty;
  }
  return g;
}
__device__ __forceinline__ void store_point(double* joints, double* vis, const GeomPoint& g) {
  joints[0] = g.x; joints[1] = g.y; joints[2] = g.z;
  vis[0] = g.v0; vis[1] = g.v1; vis[2] = g.v2;
}

// Condition key points of a generative-sampling train batch (JointsDataset.py:257-259, 293-295): what
// DeviceSamplePipeline.geometry does to cond_joints on the host, for poses that buctd_synthesize_pose left on the
// device.  One thread per (sample, joint): geom_point with the sample's flip and crop affine.
struct CondGeomParams {
  const double* synth;           // [B][K][3]
  const double* vis;             // [B][K][3]
  const buctd_warp_item* items;  // [B]: flip, W, m
  const int* pair;               // [K], -1 = no partner
  int B, K;
  double* out_joints;            // [B][K][3]
  double* out_vis;               // [B][K][3]
  float* out_trunc;              // [B][K][2]
};

__global__ __launch_bounds__(256) void cond_geometry_kernel(CondGeomParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.B * p.K) return;
  const int b = i / p.K, j = i - b * p.K;
  const buctd_warp_item* it = p.items + b;
  const long pose = (long)b * p.K * 3;
  const GeomPoint g = geom_point(p.synth + pose, 3, p.vis + pose, j, p.K, it->flip != 0, p.pair, (double)it->W, it->m);
  store_point(p.out_joints + (long)i * 3, p.out_vis + (long)i * 3, g);
  store_trunc(p.out_trunc + (long)i * 2, g.x, g.y);
}

extern "C" int buctd_cond_geometry(const double* synth, const double* cond_vis, const buctd_warp_item* items_device,
                                   const int* pair_device, int B, int K, double* out_joints, double* out_vis,
                                   float* out_trunc, void* stream) {
  BUCTD_CHECK_ARG(synth && cond_vis && items_device && pair_device && out_joints && out_vis && out_trunc && B > 0 &&
                      K > 0 && K <= 32 && B < (1 << 20),
                  "buctd_cond_geometry: bad argument (K <= 32)");
  CondGeomParams p;
  p.synth = synth; p.vis = cond_vis; p.items = items_device; p.pair = pair_device; p.B = B; p.K = K;
  p.out_joints = out_joints; p.out_vis = out_vis; p.out_trunc = out_trunc;
  hipLaunchKernelGGL(cond_geometry_kernel, dim3(ceil_div((long)B * K, 256)), dim3(256), 0, (hipStream_t)stream, p);
  BUCTD_CHECK_LAUNCH("buctd_cond_geometry");
  return BUCTD_OK;
}

// The mirrored half of a flip-test input (reference lib/core/function.py:213-225, lib/utils/transforms.py:33-75).
//
// cond_mirror_kernel: the condition coordinates the mirrored crop is rendered from - geom_point on the crop coordinates
// with the flip always on and no affine, then store_trunc.  One thread per (sample, joint).  It reads the coordinates
// BEFORE any truncation: trunc(W - 1 - x) is not W - 1 - trunc(x) for a non-integer x.
struct CondMirrorParams {
  const double* joints;          // [B][K][js], js = 2 or 3
  const double* vis;             // [B][K][3], NULL: all ones
  const int* pair;               // [K], -1 = no partner
  int B, K, js, width;
  float* out;                    // [B][K][2]
};

__global__ __launch_bounds__(256) void cond_mirror_kernel(CondMirrorParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.B * p.K) return;
  const int b = i / p.K, j = i - b * p.K;
  const GeomPoint g = geom_point(p.joints + (long)b * p.K * p.js, p.js, p.vis ? p.vis + (long)b * p.K * 3 : nullptr, j, p.K,
                                 true, p.pair, (double)p.width, nullptr);
  store_trunc(p.out + (long)i * 2, g.x, g.y);
}

extern "C" int buctd_cond_mirror(const double* cond_joints, int joint_stride, const double* cond_vis,
                                 const int* pair_device, int B, int K, int width, float* out, void* stream) {
  BUCTD_CHECK_ARG(cond_joints && pair_device && out && (joint_stride == 2 || joint_stride == 3) && B > 0 && K > 0 &&
                      K <= 32 && B < (1 << 20) && width > 0,
                  "buctd_cond_mirror: bad argument (K <= 32, joint_stride 2 or 3)");
  CondMirrorParams p;
  p.joints = cond_joints; p.vis = cond_vis; p.pair = pair_device; p.B = B; p.K = K; p.js = joint_stride; p.width = width;
  p.out = out;
  hipLaunchKernelGGL(cond_mirror_kernel, dim3(ceil_div((long)B * K, 256)), dim3(256), 0, (hipStream_t)stream, p);
  BUCTD_CHECK_LAUNCH("buctd_cond_mirror");
  return BUCTD_OK;
}

// mirror_rows_kernel: out[b][c0 + c][y][x] = in[b][c0 + perm[c]][y][W - 1 - x].  Grid: x over a row, y over the C * H
// rows of a sample (4 per block, one wavefront each), z = sample - one 32-bit division per thread, none per pixel.  A
// thread owns V consecutive output pixels and reads the V source pixels that mirror them as one load: consecutive lanes
// write ascending addresses and read descending ones, so a wavefront still touches one dense 64 * V * 4-byte segment of a
// source row.  V = 4 (16-byte loads and stores) where W, both batch strides and both pointers allow it, else V = 1: any W.
struct MirrorRowsParams {
  const float* in;
  float* out;
  const int* perm;               // [C], NULL: identity; an entry outside [0, C) keeps its channel
  long in_bs, out_bs;            // batch strides in floats
  int c0, C, H, W;
};

template <int V>
__global__ __launch_bounds__(256) void mirror_rows_kernel(MirrorRowsParams p) {
  const int wv = p.W / V, rows = p.C * p.H;
  const float* in = p.in + (long)blockIdx.z * p.in_bs;
  float* out = p.out + (long)blockIdx.z * p.out_bs;
  for (int row = blockIdx.y * 4 + threadIdx.y; row < rows; row += gridDim.y * 4) {
    const int c = row / p.H, y = row - c * p.H;
    int cs = c;
    if (p.perm) {
      const int q = p.perm[c];
      if (q >= 0 && q < p.C) cs = q;
    }
    const float* s = in + ((long)(p.c0 + cs) * p.H + y) * p.W;
    float* d = out + ((long)(p.c0 + c) * p.H + y) * p.W;
    for (int xv = blockIdx.x * 64 + threadIdx.x; xv < wv; xv += gridDim.x * 64) {
      const int x = xv * V;                       // source pixels [W - V - x, W - x): inside the row for x <= W - V
      if (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(s + (p.W - 4 - x));
        *reinterpret_cast<float4*>(d + x) = make_float4(v.w, v.z, v.y, v.x);
      } else {
        d[x] = s[p.W - 1 - x];
      }
    }
  }
}

extern "C" int buctd_mirror_rows(const float* in, long in_batch_stride, float* out, long out_batch_stride,
                                 const int32_t* perm, int B, int channel0, int channels, int H, int W, void* stream) {
  BUCTD_CHECK_ARG(in && out && B > 0 && B <= 65535 && channel0 >= 0 && channels > 0 && H > 0 && W > 0 &&
                      (long)(channel0 + channels) * H < (1L << 31),
                  "buctd_mirror_rows: bad argument (B <= 65535)");
  const long image = (long)(channel0 + channels) * H * W;
  BUCTD_CHECK_ARG(in_batch_stride >= image && out_batch_stride >= image,
                  "buctd_mirror_rows: batch stride smaller than the channels [0, channel0 + channels)");
  // what is read and what is written may be two row ranges of one tensor, never the same floats
  const float* in_end = in + (B - 1) * in_batch_stride + image;
  const float* out_end = out + (B - 1) * out_batch_stride + image;
  BUCTD_CHECK_ARG(in_end <= out || out_end <= in, "buctd_mirror_rows: source and destination overlap");
  MirrorRowsParams p;
  p.in = in; p.out = out; p.perm = perm; p.in_bs = in_batch_stride; p.out_bs = out_batch_stride;
  p.c0 = channel0; p.C = channels; p.H = H; p.W = W;
  const bool wide = W % 4 == 0 && in_batch_stride % 4 == 0 && out_batch_stride % 4 == 0 &&
                    ((uintptr_t)in | (uintptr_t)out) % 16 == 0;
  const long rows = (long)channels * H;
  dim3 grid((unsigned)min((long)ceil_div(wide ? W / 4 : W, 64), 64L), (unsigned)min((rows + 3) / 4, 65535L), (unsigned)B);
  if (wide) hipLaunchKernelGGL(mirror_rows_kernel<4>, grid, dim3(64, 4), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(mirror_rows_kernel<1>, grid, dim3(64, 4), 0, (hipStream_t)stream, p);
  BUCTD_CHECK_LAUNCH("buctd_mirror_rows");
  return BUCTD_OK;
}

// One pass boundary of the iterative refinement (dataset/pipeline.py IterativeRefiner; reference dataloader.py:454-508,
// 596-612): what get_final_preds, rescore, next_records and geometry() do per person on the host between the decode of
// one pass and the crop of the next.  One wavefront per person, lanes over joints (K <= 32); the box and the score are
// butterfly reductions in float64.  Every float64 product and sum is rounded on its own, like in geom_point.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __dadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// dataset/pipeline.py box_from_keypoints for the wavefront's person: (x, y) is the lane's joint, on whether the lane holds
// one.  The non-zero x and the non-zero y each on their own, -+ margin, clipped to the image.  empty: no non-zero x or no
// non-zero y (the host's min() of an empty array raises); the box means nothing then.
struct KeypointBox {
  bool empty;
  double x0, y0, w, h;
};
__device__ __forceinline__ KeypointBox keypoint_box(double x, double y, bool on, double margin, double W, double H) {
  const bool nx = on && x != 0.0, ny = on && y != 0.0;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double xlo = wave_min_f64(nx ? x : inf), xhi = wave_max_f64(nx ? x : -inf);
  const double ylo = wave_min_f64(ny ? y : inf), yhi = wave_max_f64(ny ? y : -inf);
  KeypointBox r;
  r.empty = __ballot(nx) == 0 || __ballot(ny) == 0;
  r.x0 = fmin(fmax(__dsub_rn(xlo, margin), 0.0), W);
  r.y0 = fmin(fmax(__dsub_rn(ylo, margin), 0.0), H);
  r.w = __dsub_rn(fmin(fmax(__dadd_rn(xhi, margin), 0.0), W), r.x0);
  r.h = __dsub_rn(fmin(fmax(__dadd_rn(yhi, margin), 0.0), H), r.y0);
  return r;
}

// dataset/pipeline.py xywh2cs: float32 centre and scale of a box with the network's aspect ratio
struct CenterScale { float cx, cy, s0, s1; };
__device__ __forceinline__ CenterScale xywh2cs(const KeypointBox& box, double aspect_ratio, double scale_thre) {
  double w = box.w, h = box.h;
  CenterScale r;
  r.cx = (float)__dadd_rn(box.x0, __dmul_rn(w, 0.5));
  r.cy = (float)__dadd_rn(box.y0, __dmul_rn(h, 0.5));
  const double ah = __dmul_rn(aspect_ratio, h);
  if (w > ah) h = __ddiv_rn(w, aspect_ratio);
  else if (w < ah) w = __dmul_rn(h, aspect_ratio);
  r.s0 = (float)__ddiv_rn(w, 200.0);
  r.s1 = (float)__ddiv_rn(h, 200.0);
  if (r.cx != -1.f) {
    r.s0 = __fmul_rn(r.s0, (float)scale_thre);
    r.s1 = __fmul_rn(r.s1, (float)scale_thre);
  }
  return r;
}

// utils/transforms.py crop_affine_closed_form, line by line: x' = sx * x + tx, y' = sy * y + ty.
struct CropAffine {
  double sx, sy, tx, ty;
  bool ok;               // false: the box has no extent (the host's solve is singular)
};
__device__ __forceinline__ CropAffine crop_affine(float cx, float cy, float scale0, int out_w, int out_h, bool inv) {
  const float box = scale0 * 200.0f;
  const float p1y = (float)__dadd_rn((double)cy, (double)(box * -0.5f));
  const float dy = cy - p1y;
  const float p2x = cx - dy;
  const double ex = __dsub_rn((double)cx, (double)p2x), ey = __dsub_rn((double)cy, (double)p1y);
  const double a = (double)out_w * 0.5, b = (double)out_h * 0.5;
  CropAffine t;
  t.ok = ex != 0.0 && ey != 0.0;
  if (inv) {
    t.sx = ex / a;
    t.sy = ey / a;
    t.tx = __dsub_rn((double)cx, __dmul_rn(t.sx, a));
    t.ty = __dsub_rn((double)cy, __dmul_rn(t.sy, b));
  } else {
    t.sx = a / ex;
    t.sy = a / ey;
    t.tx = __dsub_rn(a, __dmul_rn(t.sx, (double)cx));
    t.ty = __dsub_rn(b, __dmul_rn(t.sy, (double)cy));
  }
  return t;
}

__global__ __launch_bounds__(256) void refine_step_kernel(buctd_refine_args p) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), j = threadIdx.x & 63;
  if (b >= p.B) return;                                   // whole wavefronts leave: the shuffles below see 64 lanes
  const bool on = j < p.K;
  const long row = (long)p.pass * p.B + b;                // row of this person in the history buffers
  const float cx = p.center[2 * b], cy = p.center[2 * b + 1], s0 = p.scale[2 * b], s1 = p.scale[2 * b + 1];
  const double box_score = p.box_score[b];
  // predictions: coords (+ offset) in float32, inverse crop affine in float64, one rounding to float32
  const CropAffine back = crop_affine(cx, cy, s0, p.heatmap_w, p.heatmap_h, true);
  float px = 0.f, py = 0.f, mv = 0.f;
  if (on) {
    const long i = (long)b * p.K + j;
    float hx = p.coords[2 * i], hy = p.coords[2 * i + 1];
    if (p.offset) {
      hx = hx + p.offset[2 * i];
      hy = hy + p.offset[2 * i + 1];
    }
    mv = p.maxvals[i];
    px = (float)__dadd_rn(__dmul_rn((double)hx, back.sx), back.tx);
    py = (float)__dadd_rn(__dmul_rn((double)hy, back.sy), back.ty);
    float* hp = p.hist_preds + (row * p.K + j) * 3;
    hp[0] = px; hp[1] = py; hp[2] = mv;
  }
  // rescore: mean of the maxvals above the threshold (compared in float32, like numpy does), times the box score
  const bool counted = on && mv > (float)p.in_vis_thre;
  const int n = __popcll(__ballot(counted));
  const double sum = wave_sum_f64(counted ? (double)mv : 0.0);
  const double kpt_score = n > 0 ? sum / (double)n : 0.0;
  const double score = __dmul_rn(kpt_score, box_score);
  // the box around the predictions and the next pass's centre and scale
  const buctd_warp_item* it = p.items + b;
  const KeypointBox box = keypoint_box((double)px, (double)py, on, p.margin, (double)it->W, (double)it->H);
  const CenterScale next = xywh2cs(box, p.aspect_ratio, p.scale_thre);
  const CropAffine fwd = crop_affine(next.cx, next.cy, next.s0, p.crop_w, p.crop_h, false);
  const int bad = (box.empty ? 1 : 0) | (!box.empty && !fwd.ok ? 2 : 0);
  if (j == 0) {
    p.hist_score[row] = score;
    p.hist_box_score[row] = box_score;
    p.hist_keypoint_score[row] = kpt_score;
    p.hist_center[2 * row] = cx; p.hist_center[2 * row + 1] = cy;
    p.hist_scale[2 * row] = s0; p.hist_scale[2 * row + 1] = s1;
    p.box_score[b] = score;
    if (bad) p.status[b] = p.status[b] | bad;
  }
  if (bad) return;
  if (j == 0) {
    p.center[2 * b] = next.cx; p.center[2 * b + 1] = next.cy;
    p.scale[2 * b] = next.s0; p.scale[2 * b + 1] = next.s1;
    double* m = p.items[b].m;
    m[0] = fwd.sx; m[1] = 0.0; m[2] = fwd.tx;
    m[3] = 0.0; m[4] = fwd.sy; m[5] = fwd.ty;
  }
  if (on) {
    // the next condition: the prediction through the new affine (all visibilities are 1), and its trunc() for the renderer
    const long i = (long)b * p.K + j;
    const double qx = __dadd_rn(__dmul_rn(fwd.sx, (double)px), fwd.tx), qy = __dadd_rn(__dmul_rn(fwd.sy, (double)py), fwd.ty);
    if (p.cond_joints) {
      p.cond_joints[2 * i] = qx;
      p.cond_joints[2 * i + 1] = qy;
    }
    store_trunc(p.cond_trunc + 2 * i, qx, qy);
  }
}

extern "C" int buctd_refine_step(const buctd_refine_args* a, void* stream) {
  BUCTD_CHECK_ARG(a && a->coords && a->maxvals && a->center && a->scale && a->box_score && a->items && a->cond_trunc &&
                      a->status && a->hist_preds && a->hist_score && a->hist_box_score && a->hist_keypoint_score &&
                      a->hist_center && a->hist_scale,
                  "buctd_refine_step: NULL argument (only offset and cond_joints may be NULL)");
  BUCTD_CHECK_ARG(a->B > 0 && a->B < (1 << 20) && a->K > 0 && a->K <= 32, "buctd_refine_step: B > 0, 0 < K <= 32");
  BUCTD_CHECK_ARG(a->passes > 0 && a->pass >= 0 && a->pass < a->passes, "buctd_refine_step: pass outside [0, passes)");
  BUCTD_CHECK_ARG(a->heatmap_w > 0 && a->heatmap_h > 0 && a->crop_w > 0 && a->crop_h > 0 && a->aspect_ratio > 0.0,
                  "buctd_refine_step: sizes and the aspect ratio must be positive");
  hipLaunchKernelGGL(refine_step_kernel, dim3(ceil_div(a->B, 4)), dim3(256), 0, (hipStream_t)stream, *a);
  BUCTD_CHECK_LAUNCH("buctd_refine_step");
  return BUCTD_OK;
}

// One frame boundary of CTD tracking (dataset/pipeline.py SequenceTracker; no reference call site: the reference leaves
// this loop to the host).  The slot of a person is its identity; the pose of frame t is the condition of frame t + 1.  One
// workgroup of four wavefronts runs the whole step, in this order:
//   A  per slot (a wavefront per slot, lanes over joints, as refine_step_kernel): predictions of frame `frame`, key-point
//      score, the box around the predictions; the pose goes to the state, the box to LDS;
//   B  death (one thread per slot), then the M x M OKS table of the survivors (all threads, LDS), then the merge walk in
//      ascending id order (wavefront 0: lanes over the older slots, one ballot per slot);
//   C  the detections of frame + 1: box and mean score, rank by (score descending, index), the M x D table against the
//      live slots and the triangle of detection pairs (all threads, LDS), then the birth walk (wavefront 0: lanes over the
//      slots, one ballot per detection);
//   E  per slot: centre, scale, crop affine, source image and truncated condition of frame + 1, and the history rows.
// The walks read LDS only; nothing is accumulated across threads, so the result does not depend on scheduling.  The OKS
// is symmetric bit for bit without a visibility threshold (squares of differences, a commutative sum of the two areas):
// detection pairs are kept as a triangle.  LDS: 32 KiB + 15.75 KiB of tables, 6 KiB of per-slot and per-detection rows.
#define TRACK_MAX 64
struct TrackShared {
  double oks[TRACK_MAX * TRACK_MAX];              // [M][M] for the merge, then [M][D] for the birth
  double tri[TRACK_MAX * (TRACK_MAX - 1) / 2];    // detections i < j at j * (j - 1) / 2 + i
  double box[TRACK_MAX][4], dbox[TRACK_MAX][4];   // x0, y0, w, h of the slots' predictions and of the detections
  double score[TRACK_MAX], dmean[TRACK_MAX];
  int id[TRACK_MAX], alive[TRACK_MAX], nobox[TRACK_MAX], died[TRACK_MAX], src[TRACK_MAX], order[TRACK_MAX], dbad[TRACK_MAX];
  int n_order, next_id;
};

__device__ __forceinline__ void put_box(double* dst, const KeypointBox& b) {
  dst[0] = b.x0; dst[1] = b.y0; dst[2] = b.w; dst[3] = b.h;
}
__device__ __forceinline__ KeypointBox get_box(const double* src) {
  KeypointBox b;
  b.empty = false; b.x0 = src[0]; b.y0 = src[1]; b.w = src[2]; b.h = src[3];
  return b;
}

__global__ __launch_bounds__(256) void track_step_kernel(buctd_track_args p) {
  __shared__ TrackShared sh;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = p.M, K = p.K, f = p.frame;
  const bool decode = f >= 0, next = f + 1 < p.frames;
  const bool on = lane < K;
  const double W = (double)p.items[0].W, H = (double)p.items[0].H;        // one size for all frames
  if (tid < M) {
    const int id = p.ids[tid];
    sh.id[tid] = id; sh.alive[tid] = id >= 0; sh.died[tid] = 0; sh.src[tid] = -1; sh.nobox[tid] = 0; sh.score[tid] = 0.0;
  }
  if (tid == 0) { sh.next_id = *p.next_id; sh.n_order = 0; }
  __syncthreads();
  // ---- A: predictions, score and box of frame f, per slot ----------------------------------------------------------
  if (decode) {
    for (int s = wave; s < M; s += 4) {                                    // wave-uniform
      const bool live = sh.alive[s] != 0;
      const long row = (long)f * M + s;
      float px = 0.f, py = 0.f, mv = 0.f;
      if (live && on) {
        const CropAffine back = crop_affine(p.center[2 * s], p.center[2 * s + 1], p.scale[2 * s], p.heatmap_w, p.heatmap_h, true);
        const long i = (long)s * K + lane;
        float hx = p.coords[2 * i], hy = p.coords[2 * i + 1];
        if (p.offset) {
          hx = hx + p.offset[2 * i];
          hy = hy + p.offset[2 * i + 1];
        }
        mv = p.maxvals[i];
        px = (float)__dadd_rn(__dmul_rn((double)hx, back.sx), back.tx);
        py = (float)__dadd_rn(__dmul_rn((double)hy, back.sy), back.ty);
      }
      if (on) {
        float* hp = p.hist_preds + (row * K + lane) * 3;
        hp[0] = px; hp[1] = py; hp[2] = mv;
        double* ps = p.pose + ((long)s * K + lane) * 3;
        if (live) { ps[0] = (double)px; ps[1] = (double)py; ps[2] = (double)mv; }
      }
      const bool counted = live && on && mv > (float)p.in_vis_thre;          // IterativeRefiner.rescore, box score 1
      const int n = __popcll(__ballot(counted));
      const double sum = wave_sum_f64(counted ? (double)mv : 0.0);
      const double kpt_score = n > 0 ? sum / (double)n : 0.0;
      const KeypointBox box = keypoint_box((double)px, (double)py, live && on, p.margin, W, H);
      const CenterScale cs = xywh2cs(box, p.aspect_ratio, p.scale_thre);
      const CropAffine fwd = crop_affine(cs.cx, cs.cy, cs.s0, p.crop_w, p.crop_h, false);
      if (lane == 0) {
        put_box(sh.box[s], box);
        sh.nobox[s] = live && (box.empty || !fwd.ok);
        sh.score[s] = kpt_score;
        p.hist_score[row] = kpt_score;
      }
    }
    __syncthreads();
    // ---- B: death, then merge ----------------------------------------------------------------------------------------
    if (tid < M && sh.alive[tid]) {
      int misses = p.misses[tid];
      bool dies = sh.nobox[tid] != 0;
      if (!dies) {
        misses = sh.score[tid] < p.death_score ? misses + 1 : 0;
        dies = misses >= p.max_misses;
      }
      p.misses[tid] = dies ? 0 : misses;
      if (dies) { sh.alive[tid] = 0; sh.died[tid] = 1; }
    }
    __syncthreads();
    for (int idx = tid; idx < M * M; idx += 256) {
      const int i = idx / M, j = idx - i * M;
      if (i < j && sh.alive[i] && sh.alive[j]) {
        const double v = nms_oks(p.pose + (long)i * K * 3, p.pose + (long)j * K * 3, __dmul_rn(sh.box[i][2], sh.box[i][3]),
                                 __dmul_rn(sh.box[j][2], sh.box[j][3]), p.sigmas, K, 0, 0.0);
        sh.oks[i * M + j] = v;
        sh.oks[j * M + i] = v;
      }
    }
    if (tid < M && sh.alive[tid]) {                                          // rank among the survivors by id (ids are unique)
      int rank = 0;
      for (int q = 0; q < M; ++q) rank += (sh.alive[q] && sh.id[q] < sh.id[tid]) ? 1 : 0;
      sh.order[rank] = tid;
    }
    __syncthreads();
    if (wave == 0) {
      const unsigned long long alive = __ballot(lane < M && sh.alive[lane]);
      const int n = __popcll(alive);
      unsigned long long kept = 0ull;
      for (int r = 0; r < n; ++r) {
        const int s = sh.order[r];                                           // same address in every lane
        const bool hit = ((kept >> lane) & 1ull) && sh.oks[s * M + lane] >= p.merge_oks;
        if (__ballot(hit) == 0ull) kept |= 1ull << s;
      }
      if (((alive & ~kept) >> lane) & 1ull) { sh.alive[lane] = 0; sh.died[lane] = 1; }
    }
    __syncthreads();
  }
  // ---- C: birth for frame f + 1 ------------------------------------------------------------------------------------
  if (next) {
    const int base = p.det_offsets[f + 1];
    const int D = min(max(p.det_offsets[f + 2] - base, 0), p.max_dets);     // beyond the stated maximum: never indexed
    const double* dets = p.dets + (long)base * K * 3;
    for (int d = wave; d < D; d += 4) {
      const double x = on ? dets[((long)d * K + lane) * 3] : 0.0, y = on ? dets[((long)d * K + lane) * 3 + 1] : 0.0;
      const KeypointBox box = keypoint_box(x, y, on, p.margin, W, H);
      const CenterScale cs = xywh2cs(box, p.aspect_ratio, p.scale_thre);
      const CropAffine fwd = crop_affine(cs.cx, cs.cy, cs.s0, p.crop_w, p.crop_h, false);
      if (lane == 0) {
        put_box(sh.dbox[d], box);
        sh.dbad[d] = box.empty || !fwd.ok;
      }
    }
    if (tid < D) {                                                           // mean score: summed in joint order
      double sum = 0.0;
      for (int j = 0; j < K; ++j) sum = __dadd_rn(sum, dets[((long)tid * K + j) * 3 + 2]);
      sh.dmean[tid] = sum / (double)K;
    }
    __syncthreads();
    if (tid < D) {
      int rank = 0;
      const double mine = sh.dmean[tid];
      for (int q = 0; q < D; ++q) {
        const double other = sh.dmean[q];
        rank += (other > mine || (other == mine && q < tid)) ? 1 : 0;
      }
      sh.order[rank] = tid;
    }
    for (int idx = tid; idx < (M + D) * D; idx += 256) {
      const int r = idx / D, d = idx - r * D;
      const double a_d = __dmul_rn(sh.dbox[d][2], sh.dbox[d][3]);
      if (r < M) {
        if (sh.alive[r])
          sh.oks[r * D + d] = nms_oks(p.pose + (long)r * K * 3, dets + (long)d * K * 3,
                                      __dmul_rn(sh.box[r][2], sh.box[r][3]), a_d, p.sigmas, K, 0, 0.0);
      } else if (r - M < d) {
        const int i = r - M;
        sh.tri[d * (d - 1) / 2 + i] = nms_oks(dets + (long)i * K * 3, dets + (long)d * K * 3,
                                              __dmul_rn(sh.dbox[i][2], sh.dbox[i][3]), a_d, p.sigmas, K, 0, 0.0);
      }
    }
    __syncthreads();
    if (wave == 0) {
      unsigned long long live = __ballot(lane < M && sh.alive[lane]);
      const unsigned long long slots = M == 64 ? ~0ull : (1ull << M) - 1ull;
      int mysrc = -1, born = 0;
      for (int r = 0; r < D; ++r) {
        const int d = sh.order[r];                                           // same address in every lane
        if (sh.dbad[d]) continue;
        bool hit = false;
        if ((live >> lane) & 1ull) {
          const double v = mysrc < 0 ? sh.oks[lane * D + d]
                                     : (mysrc < d ? sh.tri[d * (d - 1) / 2 + mysrc] : sh.tri[mysrc * (mysrc - 1) / 2 + d]);
          hit = v >= p.birth_oks;
        }
        const unsigned long long free_slots = ~live & slots;
        if (__ballot(hit) == 0ull && free_slots != 0ull) {
          const int slot = __ffsll((long long)free_slots) - 1;               // the lowest free slot
          if (lane == slot) {
            mysrc = d;
            sh.src[lane] = d; sh.id[lane] = sh.next_id + born; sh.alive[lane] = 1;
          }
          live |= 1ull << slot;
          ++born;
        }
      }
      if (lane == 0) sh.next_id = sh.next_id + born;                         // after every read of it above: one wavefront
    }
    __syncthreads();
  }
  // ---- E: the slots of frame f + 1 and the history rows -------------------------------------------------------------
  for (int s = wave; s < M; s += 4) {
    const bool alive = sh.alive[s] != 0;
    const int src = sh.src[s];
    if (lane == 0) {
      if (decode) p.hist_died[(long)f * M + s] = (unsigned char)sh.died[s];
      p.ids[s] = alive ? sh.id[s] : -1;
      if (!alive || src >= 0) p.misses[s] = 0;
    }
    if (!next) continue;
    KeypointBox box;
    double x = 0.0, y = 0.0;
    double* ps = p.pose + ((long)s * K + lane) * 3;
    if (alive && src >= 0) {                                                 // newborn: the detection is its pose
      box = get_box(sh.dbox[src]);
      if (on) {
        const double* dp = p.dets + ((long)(p.det_offsets[f + 1] + src) * K + lane) * 3;
        x = dp[0]; y = dp[1];
        ps[0] = x; ps[1] = y; ps[2] = dp[2];
      }
    } else if (alive) {
      box = get_box(sh.box[s]);
      if (on) { x = ps[0]; y = ps[1]; }
    } else {                                                                 // empty: the whole image, no condition
      box.empty = false; box.x0 = 0.0; box.y0 = 0.0; box.w = W; box.h = H;
    }
    const CenterScale cs = xywh2cs(box, p.aspect_ratio, p.scale_thre);
    const CropAffine fwd = crop_affine(cs.cx, cs.cy, cs.s0, p.crop_w, p.crop_h, false);
    if (lane == 0) {
      const long row = (long)(f + 1) * M + s;
      p.hist_ids[row] = alive ? sh.id[s] : -1;
      p.hist_born[row] = (unsigned char)(alive && src >= 0);
      p.center[2 * s] = cs.cx; p.center[2 * s + 1] = cs.cy;
      p.scale[2 * s] = cs.s0; p.scale[2 * s + 1] = cs.s1;
      buctd_warp_item* it = p.items + s;
      it->src = p.frame_src[f + 1];
      it->m[0] = fwd.sx; it->m[1] = 0.0; it->m[2] = fwd.tx;
      it->m[3] = 0.0; it->m[4] = fwd.sy; it->m[5] = fwd.ty;
    }
    if (on) {
      double qx = 0.0, qy = 0.0;
      if (alive) {
        qx = __dadd_rn(__dmul_rn(fwd.sx, x), fwd.tx);
        qy = __dadd_rn(__dmul_rn(fwd.sy, y), fwd.ty);
      }
      store_trunc(p.cond_trunc + ((long)s * K + lane) * 2, qx, qy);
    }
  }
  if (tid == 0) *p.next_id = sh.next_id;
}

extern "C" int buctd_track_step(const buctd_track_args* a, void* stream) {
  BUCTD_CHECK_ARG(a && a->ids && a->misses && a->next_id && a->pose && a->center && a->scale && a->items && a->cond_trunc &&
                      a->dets && a->det_offsets && a->frame_src && a->sigmas && a->hist_ids && a->hist_preds &&
                      a->hist_score && a->hist_born && a->hist_died,
                  "buctd_track_step: NULL argument (only coords, maxvals and offset may be NULL, before the first frame)");
  BUCTD_CHECK_ARG(a->M > 0 && a->M <= TRACK_MAX, "buctd_track_step: 0 < M <= 64 track slots");
  BUCTD_CHECK_ARG(a->K > 0 && a->K <= 32, "buctd_track_step: 0 < K <= 32 joints");
  BUCTD_CHECK_ARG(a->max_dets >= 0 && a->max_dets <= TRACK_MAX, "buctd_track_step: at most 64 detections per frame");
  BUCTD_CHECK_ARG(a->frames > 0 && a->frame >= -1 && a->frame < a->frames, "buctd_track_step: frame outside [-1, frames)");
  BUCTD_CHECK_ARG(a->frame < 0 || (a->coords && a->maxvals), "buctd_track_step: frame >= 0 needs its decode outputs");
  BUCTD_CHECK_ARG(a->heatmap_w > 0 && a->heatmap_h > 0 && a->crop_w > 0 && a->crop_h > 0 && a->aspect_ratio > 0.0 &&
                      a->max_misses > 0,
                  "buctd_track_step: sizes, the aspect ratio and max_misses must be positive");
  hipLaunchKernelGGL(track_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
  BUCTD_CHECK_LAUNCH("buctd_track_step");
  return BUCTD_OK;
}

// Scalar geometry of a train batch (dataset/pipeline.py DeviceSamplePipeline.geometry; reference JointsDataset.py:217-295):
// box -> half-body override -> scale draw -> flip -> crop affine for any rotation -> joints, condition, target centres,
// keep-rectangle.  One wavefront per sample, lanes over joints (K <= 32), like refine_step_kernel; every float64 and
// float32 product, sum and difference is rounded on its own.  A keep-rectangle with a negative origin is cut at 0, which
// is what oracle.sample.warp_affine_u8 keeps; the reference's negative slice indices wrap around instead (out of scope).
// utils/transforms.py _two_sum, _split, _two_prod, _cross: error-free sums and products without a fused multiply-add
struct Two { double s, e; };
__device__ __forceinline__ Two two_sum(double a, double b) {
  Two r;
  r.s = __dadd_rn(a, b);
  const double bb = __dsub_rn(r.s, a);
  r.e = __dadd_rn(__dsub_rn(a, __dsub_rn(r.s, bb)), __dsub_rn(b, bb));
  return r;
}
__device__ __forceinline__ Two split_f64(double a) {
  const double c = __dmul_rn(134217729.0, a);
  Two r;
  r.s = __dsub_rn(c, __dsub_rn(c, a));
  r.e = __dsub_rn(a, r.s);
  return r;
}
__device__ __forceinline__ Two two_prod(double a, double b) {
  Two r;
  r.s = __dmul_rn(a, b);
  const Two x = split_f64(a), y = split_f64(b);
  r.e = __dadd_rn(__dadd_rn(__dadd_rn(__dsub_rn(__dmul_rn(x.s, y.s), r.s), __dmul_rn(x.s, y.e)), __dmul_rn(x.e, y.s)),
                  __dmul_rn(x.e, y.e));
  return r;
}
__device__ __forceinline__ double cross_f64(double a, Two u, double b, Two v) {   // a * (u.s + u.e) - b * (v.s + v.e)
  const Two p1 = two_prod(a, u.s), p2 = two_prod(b, v.s);
  const Two s = two_sum(p1.s, -p2.s);
  return __dadd_rn(s.s, __dadd_rn(__dadd_rn(s.e, __dsub_rn(p1.e, p2.e)), __dsub_rn(__dmul_rn(a, u.e), __dmul_rn(b, v.e))));
}

struct RotAffine {
  double m[6];
  bool ok;               // false: the box has no extent (the host's solve is singular)
};
// utils/transforms.py crop_affine_rot_closed_form, line by line (scale in float64: the train path's dtype).
__device__ __forceinline__ RotAffine crop_affine_rot(float cx, float cy, double scale0, double sn, double cs, int out_w,
                                                     int out_h) {
  const double box = __dmul_rn(scale0, 200.0);
  const double y = __dmul_rn(box, -0.5);
  const double ax = -__dmul_rn(y, sn), ay = __dmul_rn(y, cs);                   // get_dir([0, y], rot)
  const float p1x = (float)__dadd_rn((double)cx, ax), p1y = (float)__dadd_rn((double)cy, ay);
  const float dx = __fsub_rn(cx, p1x), dy = __fsub_rn(cy, p1y);                 // get_3rd_point: float32
  const float p2x = __fsub_rn(p1x, dy), p2y = __fadd_rn(p1y, dx);
  const double d1x = __dsub_rn((double)p1x, (double)cx), d1y = __dsub_rn((double)p1y, (double)cy);
  const double d2x = __dsub_rn((double)p2x, (double)p1x), d2y = __dsub_rn((double)p2y, (double)p1y);
  const double det = __dsub_rn(__dmul_rn(d1x, d2y), __dmul_rn(d2x, d1y));
  const double a = (double)out_w * 0.5, b = (double)out_h * 0.5;
  RotAffine t;
  t.ok = det != 0.0;
  t.m[0] = __dmul_rn(a, d1y) / det;
  t.m[1] = -__dmul_rn(a, d1x) / det;
  t.m[3] = -__dmul_rn(a, d2y) / det;
  t.m[4] = __dmul_rn(a, d2x) / det;
  // the translation over the same denominator, its two differences of products taken exactly
  const double cxd = (double)cx, cyd = (double)cy;
  t.m[2] = __dmul_rn(a, cross_f64(d1x, two_sum(d2y, cyd), d1y, two_sum(d2x, cxd))) / det;
  const Two qx = two_prod(b, d1x), qy = two_prod(b, d1y);
  Two wx = two_sum(qx.s, __dmul_rn(a, cxd)), wy = two_sum(qy.s, __dmul_rn(a, cyd));   // a * cx, a * cy: exact
  wx.e = __dadd_rn(wx.e, qx.e);
  wy.e = __dadd_rn(wy.e, qy.e);
  t.m[5] = cross_f64(d2y, wx, d2x, wy) / det;
  return t;
}

// target_centres(): a coordinate that buctd_gaussian_target's (int)(v / stride + 0.5f) maps to int(j / stride + 0.5)
__device__ __forceinline__ float target_centre(double v, double stride) {
  double q = __dadd_rn(v / stride, 0.5);
  q = fmin(fmax(q, -9.0e18), 9.0e18);                      // astype(int) of a finite double, kept inside int64
  long long mu = (long long)q;                             // truncates toward zero
  if (mu < 0) mu -= 1;
  return (float)__dmul_rn((double)mu, stride);
}

__device__ __forceinline__ int floor_div10(long long v) {
  long long q = v / 10;
  if (v % 10 != 0 && v < 0) q -= 1;
  return (int)q;
}

__device__ __forceinline__ int trunc_int(double v) {       // astype(int), kept inside int32 (the table's fields)
  return (int)fmin(fmax(trunc(v), -1.0e9), 1.0e9);
}

__global__ __launch_bounds__(256) void sample_geometry_kernel(buctd_sample_geom_args p) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), j = threadIdx.x & 63;
  if (b >= p.B) return;                                   // whole wavefronts leave: the shuffles below see 64 lanes
  const bool on = j < p.K;
  const long i = (long)b * p.K + j;
  const int flags = p.flags[b];
  const bool has_cond = p.cond != nullptr;
  const bool flip = (flags & BUCTD_GEOM_FLIP) != 0;
  buctd_warp_item* it = p.items + b;
  const double W = (double)it->W, H = (double)it->H;
  // 1. box: from the condition pose under use_bu_bbox, else the record's
  float cx = p.center[2 * b], cy = p.center[2 * b + 1], s0 = p.scale[2 * b], s1 = p.scale[2 * b + 1];
  bool has_box = (flags & BUCTD_GEOM_HAS_BBOX) != 0;
  double bx = 0.0, by = 0.0, bw = 0.0, bh = 0.0;
  if (has_box) { bx = p.bbox[4 * b]; by = p.bbox[4 * b + 1]; bw = p.bbox[4 * b + 2]; bh = p.bbox[4 * b + 3]; }
  int bad = 0;
  if (has_cond && (flags & BUCTD_GEOM_USE_BU_BBOX)) {     // wave-uniform
    const double ex = on ? p.cond[i * 3] : 0.0, ey = on ? p.cond[i * 3 + 1] : 0.0;
    const KeypointBox box = keypoint_box(ex, ey, on, p.margin, W, H);
    const double xsum = wave_sum_f64(ex);
    const double y_first = p.cond[(long)b * p.K * 3 + 1];
    if (box.empty) {
      bad |= 1;
    } else if (xsum != 0.0 && y_first != 0.0) {               // the host's test (geometry()), reference quirk included
      const CenterScale c = xywh2cs(box, p.aspect_ratio, p.scale_thre);
      has_box = true;
      bx = box.x0; by = box.y0; bw = box.w; bh = box.h;
      cx = c.cx; cy = c.cy; s0 = c.s0; s1 = c.s1;
    }
  }
  // 2. half-body override
  if (flags & BUCTD_GEOM_HALF_BODY) {
    cx = p.half_body[4 * b]; cy = p.half_body[4 * b + 1]; s0 = p.half_body[4 * b + 2]; s1 = p.half_body[4 * b + 3];
  }
  // 3. scale draw: float32 * float64 scalar is float64 in numpy
  const double mul = p.draws[4 * b], sn = p.draws[4 * b + 1], cs = p.draws[4 * b + 2];
  const double sc0 = __dmul_rn((double)s0, mul), sc1 = __dmul_rn((double)s1, mul);
  // 4. flip of the centre, in float32
  if (flip) cx = __fsub_rn(__fsub_rn((float)it->W, cx), 1.0f);
  // 5. crop affine
  const RotAffine t = crop_affine_rot(cx, cy, sc0, sn, cs, p.crop_w, p.crop_h);
  if (!bad && !t.ok) bad |= 2;
  if (j == 0) p.status[b] = bad;
  // 6. joints, condition, target centres
  if (on) {
    GeomPoint g = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!bad) g = geom_point(p.joints + (long)b * p.K * 3, 3, p.joints_vis + (long)b * p.K * 3, j, p.K, flip, p.pair, W, t.m);
    store_point(p.out_joints + i * 3, p.out_joints_vis + i * 3, g);
    p.target_xy[i * 3] = bad ? 0.f : target_centre(g.x, p.stride_x);
    p.target_xy[i * 3 + 1] = bad ? 0.f : target_centre(g.y, p.stride_y);
    p.target_xy[i * 3 + 2] = 0.f;
    p.target_vis[i] = (float)g.v0;
    if (has_cond) {
      GeomPoint c = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (!bad) c = geom_point(p.cond + (long)b * p.K * 3, 3, p.cond_vis + (long)b * p.K * 3, j, p.K, flip, p.pair, W, t.m);
      store_point(p.out_cond + i * 3, p.out_cond_vis + i * 3, c);
      store_trunc(p.cond_trunc + i * 2, c.x, c.y);
    }
  }
  if (j != 0) return;
  // 8. meta
  p.out_center[2 * b] = bad ? 0.f : cx; p.out_center[2 * b + 1] = bad ? 0.f : cy;
  p.out_scale[2 * b] = bad ? 0.0 : sc0; p.out_scale[2 * b + 1] = bad ? 0.0 : sc1;
  p.out_rotation[b] = p.draws[4 * b + 3];
  if (bad) return;
  // 7. keep-rectangle
  int rx = 0, ry = 0, rw = 0, rh = 0;
  if (p.keep_rect && has_box) {
    int x = trunc_int(bx), y = trunc_int(by), w = trunc_int(bw), h = trunc_int(bh);
    if (p.bbox_aug) {
      const int xd = floor_div10((long long)w * p.bbox_draws[2 * b]), yd = floor_div10((long long)h * p.bbox_draws[2 * b + 1]);
      x = x - xd > 0 ? x - xd : 0;
      y = y - yd > 0 ? y - yd : 0;
      w = w + 2 * xd;
      h = h + 2 * yd;
    }
    rx = max(x, 0); ry = max(y, 0);
    rw = x + w - rx; rh = y + h - ry;
  }
  it->flip = flip ? 1 : 0;
  it->rx = rx; it->ry = ry; it->rw = rw; it->rh = rh;
#pragma unroll
  for (int k = 0; k < 6; ++k) it->m[k] = t.m[k];
}

extern "C" int buctd_sample_geometry(const buctd_sample_geom_args* a, void* stream) {
  BUCTD_CHECK_ARG(a && a->joints && a->joints_vis && a->center && a->scale && a->bbox && a->half_body && a->draws &&
                      a->bbox_draws && a->flags && a->pair && a->items && a->out_joints && a->out_joints_vis &&
                      a->target_xy && a->target_vis && a->out_center && a->out_scale && a->out_rotation && a->status,
                  "buctd_sample_geometry: NULL argument (only the condition's five may be NULL)");
  const bool all = a->cond && a->cond_vis && a->out_cond && a->out_cond_vis && a->cond_trunc;
  const bool none = !a->cond && !a->cond_vis && !a->out_cond && !a->out_cond_vis && !a->cond_trunc;
  BUCTD_CHECK_ARG(all || none, "buctd_sample_geometry: cond, cond_vis, out_cond, out_cond_vis and cond_trunc go together");
  BUCTD_CHECK_ARG(a->B > 0 && a->B < (1 << 20) && a->K > 0 && a->K <= 32, "buctd_sample_geometry: B > 0, 0 < K <= 32");
  BUCTD_CHECK_ARG(a->crop_w > 0 && a->crop_h > 0 && a->aspect_ratio > 0.0 && a->stride_x > 0.0 && a->stride_y > 0.0,
                  "buctd_sample_geometry: sizes, strides and the aspect ratio must be positive");
  hipLaunchKernelGGL(sample_geometry_kernel, dim3(ceil_div(a->B, 4)), dim3(256), 0, (hipStream_t)stream, *a);
  BUCTD_CHECK_LAUNCH("buctd_sample_geometry");
  return BUCTD_OK;
}
