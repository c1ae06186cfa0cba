// Pose overlays on the device (utils/vis.py:draw_poses): skeletons of every person of every canvas drawn in place on
// uint8 RGB pictures, in the paint order of the reference's sequential cv2.line / cv2.circle calls (tools/vis.py:
// plot_keypoints, lib/utils/vis.py:vis_keypoints).  The pixel rules are the ones stated in include/buctd_hip.h, in 64-bit
// integers - tests/helpers/pose_overlay_ref.py restates them in numpy and the bytes are equal.
//
// MI355X shape of the problem: pixel-parallel, but ordered - the LAST primitive that covers a pixel decides it.  So no
// primitive is scattered into the picture; every pixel gathers.  One workgroup (4 wavefronts) owns a 64 x 16 tile, a
// thread 4 pixels of one column (a wavefront = one row of 64 pixels = 192 contiguous bytes).  The primitives of the
// tile's canvas are enumerated by index, never stored: primitive i is slot i % S of person i / S (S = K + L rings and
// segments, or 3 L segments and discs), 256 per round, one per lane.  A lane builds its primitive from the joints and
// tests the bounding box, clipped to the person's rectangle, against the tile; the hits are compacted into LDS in
// index order (wave ballot + popcount of the lower lanes + the counts of the earlier waves), then every thread walks
// the list - each record is one LDS broadcast - and keeps the colour of the last record that covers each of its pixels.
// After the last round a thread blends its covered pixels: one read-modify-write per pixel, no pixel shared between
// threads, no atomics, and a tile that nothing reaches writes nothing.
#include "common.h"
#include "../../include/buctd_hip.h"

namespace {

constexpr int TILE_W = BUCTD_VIS_POSE_TILE_W, TILE_H = BUCTD_VIS_POSE_TILE_H, CHUNK = BUCTD_VIS_POSE_CHUNK;
constexpr int ROWS = TILE_H / 4;                 // pixels of a thread: rows wave, wave + 4, ...
static_assert(TILE_W == 64 && CHUNK == 256 && TILE_H % 4 == 0, "one wavefront per tile row, one primitive per lane");
constexpr int COORD_MIN = -8192, COORD_MAX = 8191, EXTENT_MAX = 8192, WIDTH_MAX = 16384;
constexpr unsigned COVERED = 1u << 24;

enum { SEGMENT = 0, DISC = 1, RING = 2 };

struct Prim {      // a primitive that reaches the tile
  int kind;
  int px, py, qx, qy;        // segment P-Q; disc and ring: P is the centre
  int t, r;                  // thickness, radius
  int x0, y0, x1, y1;        // pixels it may cover: bounding box, clip rectangle and canvas intersected, [x0, x1) x [y0, y1)
  unsigned colour;           // r | g << 8 | b << 16
};

struct Point {
  int x, y;
  bool ok;
};

// pixel of joint j of person p; absent: not finite, score <= thresh (or not finite), outside [-8192, 8191]
__device__ __forceinline__ Point joint_pixel(const float* __restrict__ joints, long p, int K, int j, int dx, int dy,
                                             float thresh) {
  const float* at = joints + (p * K + j) * 3;
  const float x = at[0], y = at[1], s = at[2];
  Point o{0, 0, false};
  if (!(isfinite(x) && isfinite(y) && isfinite(s) && s > thresh)) return o;
  const long ix = (long)(int)fminf(fmaxf(x, -1e9f), 1e9f) + dx, iy = (long)(int)fminf(fmaxf(y, -1e9f), 1e9f) + dy;
  if (ix < COORD_MIN || ix > COORD_MAX || iy < COORD_MIN || iy > COORD_MAX) return o;
  o.x = (int)ix;
  o.y = (int)iy;
  o.ok = true;
  return o;
}

// end point of a limb: the floor midpoint of two joints
__device__ __forceinline__ Point end_point(const float* __restrict__ joints, long p, int K, int j0, int j1, int dx, int dy,
                                           float thresh) {
  Point a = joint_pixel(joints, p, K, j0, dx, dy, thresh);
  if (j0 == j1 || !a.ok) return a;
  const Point b = joint_pixel(joints, p, K, j1, dx, dy, thresh);
  a.x = (a.x + b.x) >> 1;
  a.y = (a.y + b.y) >> 1;
  a.ok = b.ok;
  return a;
}

// Coverage in int64: coordinates in [-8192, 8191] and pixels in [0, 8191] make every difference < 2^14 in magnitude,
// c1 and c2 < 2^29, |w|^2 * c2 < 2^58 and its fourfold < 2^60; t, r <= 16384 give t^2 * c2 < 2^57 and (2r + t)^2 < 2^32.
__device__ __forceinline__ bool covers(const Prim& m, int X, int Y) {
  if (X < m.x0 || X >= m.x1 || Y < m.y0 || Y >= m.y1) return false;
  const long wx = X - m.px, wy = Y - m.py;
  const long ww = wx * wx + wy * wy;
  if (m.kind == DISC) return ww <= (long)m.r * m.r;
  if (m.kind == RING) {
    const long hi = 2L * m.r + m.t, lo = 2L * m.r - m.t;
    return 4 * ww <= hi * hi && (lo <= 0 || 4 * ww >= lo * lo);
  }
  const long vx = m.qx - m.px, vy = m.qy - m.py;
  const long c1 = wx * vx + wy * vy, c2 = vx * vx + vy * vy, tt = (long)m.t * m.t;
  if (c1 <= 0) return 4 * ww <= tt;
  if (c1 >= c2) {
    const long ux = X - m.qx, uy = Y - m.qy;
    return 4 * (ux * ux + uy * uy) <= tt;
  }
  return 4 * (ww * c2 - c1 * c1) <= tt * c2;
}

__global__ __launch_bounds__(256) void pose_overlay_kernel(buctd_vis_pose_args a) {
  __shared__ Prim list[CHUNK];
  __shared__ int wave_hits[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the tile (block-uniform; anything that points outside the tables draws nothing)
  const int* tile = a.tiles + (long)blockIdx.x * 3;
  const int c = tile[0], tcol = tile[1], trow = tile[2];
  if (c < 0 || c >= a.C || tcol < 0 || trow < 0) return;
  const buctd_vis_canvas cv = a.canvases[c];
  if (cv.base == nullptr || cv.H < 1 || cv.W < 1 || cv.H > a.canvas_h_max || cv.W > a.canvas_w_max ||
      cv.row_stride < 3L * cv.W)
    return;
  const long tx0l = (long)tcol * TILE_W, ty0l = (long)trow * TILE_H;
  if (tx0l >= cv.W || ty0l >= cv.H) return;
  const int tx0 = (int)tx0l, ty0 = (int)ty0l;
  const int tx1 = min(tx0 + TILE_W, cv.W), ty1 = min(ty0 + TILE_H, cv.H);
  int first = a.person_offsets[c], end = a.person_offsets[c + 1];
  first = max(first, 0);
  end = min(end, a.P);
  if (end <= first) return;

  const bool pretty = a.style == BUCTD_VIS_POSE_PRETTY;
  const int slots = pretty ? 3 * a.L : a.K + a.L;          // <= 192
  const long nprim = (long)(end - first) * slots;

  const int X = tx0 + lane;
  unsigned paint[ROWS];
#pragma unroll
  for (int q = 0; q < ROWS; ++q) paint[q] = 0;

  for (long base = 0; base < nprim; base += CHUNK) {
    const long i = base + tid;
    Prim m;
    bool hit = false;
    if (i < nprim) {
      const long p = first + i / slots;
      const int slot = (int)(i % slots);
      const int* pr = a.persons + p * 7;
      // the person's rectangle inside the tile; empty for most persons of a large picture
      m.x0 = max(pr[2], tx0);
      m.y0 = max(pr[3], ty0);
      m.x1 = min(pr[4], tx1);
      m.y1 = min(pr[5], ty1);
      if (m.x0 < m.x1 && m.y0 < m.y1) {
        const int dx = pr[0], dy = pr[1];
        m.colour = (unsigned)pr[6] & 0xffffffu;
        m.t = a.thickness;
        m.r = a.radius;
        int reach = 0;         // the primitive lies within `reach` pixels of its end points
        bool ok = false;
        int limb = -1, part = 0;
        if (pretty) {
          limb = slot / 3;
          part = slot - limb * 3;
        } else if (slot >= a.K) {
          limb = slot - a.K;
        }
        if (limb < 0) {        // plain: the ring of joint `slot`
          const Point z = joint_pixel(a.joints, p, a.K, slot, dx, dy, a.score_thresh);
          m.kind = RING;
          m.px = m.qx = z.x;
          m.py = m.qy = z.y;
          ok = z.ok;
          reach = m.r + (m.t + 1) / 2;
        } else {
          const int* lb = a.skeleton + limb * 5;
          const int a0 = lb[0], a1 = lb[1], b0 = lb[2], b1 = lb[3], ci = lb[4];
          const bool in_tables = a0 >= 0 && a0 < a.K && a1 >= 0 && a1 < a.K && b0 >= 0 && b0 < a.K && b1 >= 0 &&
                                 b1 < a.K && ci >= -1 && ci < a.n_palette;
          if (in_tables) {
            if (pretty && ci >= 0) {
              const uint8_t* pal = a.palette + ci * 3;
              m.colour = (unsigned)pal[0] | ((unsigned)pal[1] << 8) | ((unsigned)pal[2] << 16);
            }
            Point A{0, 0, false}, B{0, 0, false};
            if (part != 2) A = end_point(a.joints, p, a.K, a0, a1, dx, dy, a.score_thresh);
            if (part != 1) B = end_point(a.joints, p, a.K, b0, b1, dx, dy, a.score_thresh);
            if (part == 0) {
              m.kind = SEGMENT;
              m.px = A.x; m.py = A.y; m.qx = B.x; m.qy = B.y;
              ok = A.ok && B.ok;
              reach = (m.t + 1) / 2;
            } else {
              const Point z = part == 1 ? A : B;
              m.kind = DISC;
              m.px = m.qx = z.x;
              m.py = m.qy = z.y;
              ok = z.ok;
              reach = m.r;
            }
          }
        }
        if (ok) {
          m.x0 = max(m.x0, min(m.px, m.qx) - reach);
          m.y0 = max(m.y0, min(m.py, m.qy) - reach);
          m.x1 = min(m.x1, max(m.px, m.qx) + reach + 1);
          m.y1 = min(m.y1, max(m.py, m.qy) + reach + 1);
          hit = m.x0 < m.x1 && m.y0 < m.y1;
        }
      }
    }
    // ordered compaction: position = hits of the earlier waves + hits of the lower lanes
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) wave_hits[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int n = wave_hits[w];
      before += w < wave ? n : 0;
      total += n;
    }
    if (hit) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = m;
    __syncthreads();
    if (X < tx1) {
      for (int k = 0; k < total; ++k) {
        const Prim& m2 = list[k];
        if (X < m2.x0 || X >= m2.x1) continue;
#pragma unroll
        for (int q = 0; q < ROWS; ++q)
          if (covers(m2, X, ty0 + wave + 4 * q)) paint[q] = m2.colour | COVERED;
      }
    }
    __syncthreads();         // the list and the counts are rewritten by the next round
  }

  if (X >= tx1 || a.alpha256 == 0) return;
  const int al = a.alpha256, keep = 256 - al;
#pragma unroll
  for (int q = 0; q < ROWS; ++q) {
    const int Y = ty0 + wave + 4 * q;
    if (!(paint[q] & COVERED) || Y >= ty1) continue;
    uint8_t* px = cv.base + (long)Y * cv.row_stride + 3L * X;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int col = (int)((paint[q] >> (8 * ch)) & 0xffu);
      px[ch] = (uint8_t)(((int)px[ch] * keep + col * al + 128) >> 8);
    }
  }
}

}  // namespace

extern "C" int buctd_vis_pose_overlay(const buctd_vis_pose_args* a, void* stream) {
  BUCTD_CHECK_ARG(a, "buctd_vis_pose_overlay: null argument struct");
  BUCTD_CHECK_ARG(a->canvases && a->person_offsets && a->persons && a->joints && a->skeleton && a->tiles,
                  "buctd_vis_pose_overlay: null table");
  BUCTD_CHECK_ARG(a->n_palette >= 0 && (a->palette || a->n_palette == 0),
                  "buctd_vis_pose_overlay: null palette with n_palette > 0, or n_palette < 0");
  BUCTD_CHECK_ARG(a->C >= 1 && a->P >= 0 && a->n_tiles >= 0, "buctd_vis_pose_overlay: bad argument (C < 1, P < 0 or n_tiles < 0)");
  BUCTD_CHECK_ARG(a->K >= 1 && a->K <= 64, "buctd_vis_pose_overlay: K = %d is outside 1 .. 64", a->K);
  BUCTD_CHECK_ARG(a->L >= 1 && a->L <= 64, "buctd_vis_pose_overlay: L = %d is outside 1 .. 64", a->L);
  BUCTD_CHECK_ARG(a->style == BUCTD_VIS_POSE_PLAIN || a->style == BUCTD_VIS_POSE_PRETTY,
                  "buctd_vis_pose_overlay: unknown style %d", a->style);
  BUCTD_CHECK_ARG(a->thickness >= 1 && a->thickness <= WIDTH_MAX, "buctd_vis_pose_overlay: thickness = %d is outside 1 .. %d",
                  a->thickness, WIDTH_MAX);
  BUCTD_CHECK_ARG(a->radius >= 0 && a->radius <= WIDTH_MAX, "buctd_vis_pose_overlay: radius = %d is outside 0 .. %d",
                  a->radius, WIDTH_MAX);
  BUCTD_CHECK_ARG(a->alpha256 >= 0 && a->alpha256 <= 256, "buctd_vis_pose_overlay: alpha256 = %d is outside 0 .. 256",
                  a->alpha256);
  BUCTD_CHECK_ARG(a->canvas_h_max >= 1 && a->canvas_h_max <= EXTENT_MAX && a->canvas_w_max >= 1 &&
                      a->canvas_w_max <= EXTENT_MAX,
                  "buctd_vis_pose_overlay: a canvas of %d x %d is outside 1 .. %d", a->canvas_h_max, a->canvas_w_max,
                  EXTENT_MAX);
  if (a->P == 0 || a->n_tiles == 0) return BUCTD_OK;
  hipLaunchKernelGGL(pose_overlay_kernel, dim3((unsigned)a->n_tiles), dim3(256), 0, (hipStream_t)stream, *a);
  BUCTD_CHECK_LAUNCH("buctd_vis_pose_overlay");
  return BUCTD_OK;
}
