// Keypoint evaluation on the device (core/keypoint_eval.py): the rescoring and grouped OKS NMS, hard and soft, of the
// reference's data set classes (lib/dataset/dataloader.py:590-634 around lib/nms/nms.py:75-200) and the per-image part of the
// published COCO keypoint evaluation (computeOks + evaluateImg).  Everything is fp64: a match is a comparison against
// a threshold, and the data is a few MB.  The crowding analysis (core/keypoint_analysis.py, the reference's
// lib/analysis/evaluation.py) adds the overlap count per ground truth and a per-segment accumulate + summarize.
//
// MI355X shape of the problem: each image is a wave-sized job that exists thousands of times, so one wave64 wavefront
// takes one image - lanes stride over the candidates of an NMS step, over the cells of the OKS matrix, and one lane
// runs each of the (area range, threshold) greedy matchings.  These are latency kernels; nothing here is tuned.
#include "common.h"
#include "box_iou.h"
#include "oks.h"
#include "../../include/buctd_hip.h"

// Per person: mean of the joint scores above in_vis_thre (0 if none), summed in joint order; score = mean * box score.
__global__ __launch_bounds__(64) void kpt_rescore_kernel(int n, int K, double in_vis_thre, const float* __restrict__ preds,
                                                         const double* __restrict__ box_in, double* __restrict__ score,
                                                         double* __restrict__ box_score,
                                                         double* __restrict__ keypoint_score) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n) return;
  double s = 0.0;
  int valid = 0;
  for (int j = 0; j < K; ++j) {
    const double t = (double)preds[((long)p * K + j) * 3 + 2];
    if (t > in_vis_thre) {
      s = s + t;
      ++valid;
    }
  }
  if (valid != 0) s = s / valid;
  const double b = box_in[p];
  score[p] = s * b;
  box_score[p] = b;
  keypoint_score[p] = s;
}

// nms_oks (oks.h): oks_iou of nms/nms.py:86-105 for one (head, candidate) pair; kp rows are [K][3] float32.
// One wavefront per image; persons [off[i], off[i+1]) are in descending score order.  The alive set is a bitmap in LDS
// (cap_words words); a kept head clears the later candidates it overlaps by more than thresh, 64 candidates per step.
__global__ __launch_bounds__(64) void oks_nms_grouped_kernel(int K, int cap_words, double thresh, int use_vis,
                                                             double in_vis_thre, const int* __restrict__ off,
                                                             const float* __restrict__ kpts, const double* __restrict__ areas,
                                                             const double* __restrict__ sigmas, int* __restrict__ keep) {
  extern __shared__ unsigned long long alive[];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int base = off[img];
  const int n_all = off[img + 1] - base;
  const int n = min(n_all, cap_words * 64);      // persons beyond the caller's stated maximum are dropped, never indexed
  const int words = (n + 63) >> 6;
  for (int w = lane; w < words; w += 64) {
    const int rest = n - w * 64;
    alive[w] = rest >= 64 ? ~0ull : ((1ull << rest) - 1ull);
  }
  __syncthreads();
  for (int a = 0; a < n; ++a) {
    if (!((alive[a >> 6] >> (a & 63)) & 1ull)) continue;            // same address in every lane: uniform
    const float* g = kpts + (long)(base + a) * K * 3;
    const double a_g = areas[base + a];
    for (int c0 = (a + 1) & ~63; c0 < n; c0 += 64) {
      const int c = c0 + lane;
      const unsigned long long word = alive[c0 >> 6];
      bool dead = false;
      if (c > a && c < n && ((word >> lane) & 1ull))
        dead = nms_oks(g, kpts + (long)(base + c) * K * 3, a_g, areas[base + c], sigmas, K, use_vis, in_vis_thre) > thresh;
      const unsigned long long hit = __ballot(dead);
      __syncthreads();
      if (lane == 0) alive[c0 >> 6] = word & ~hit;
      __syncthreads();
    }
  }
  for (int p = lane; p < n_all; p += 64) keep[base + p] = p < n ? (int)((alive[p >> 6] >> (p & 63)) & 1ull) : 0;
}

// Soft suppression (soft_oks_nms / rescore of nms/nms.py:150-200), one wavefront per image; persons [off[i], off[i+1])
// in the caller's grouped order.  min(n, max_keep) rounds: the head of a round is the untaken person with the largest
// live score (equal scores: the lowest position), every other untaken person's live score is multiplied by the decay of
// its OKS to the head.  The live scores sit in soft_score and rank >= 0 marks a taken person, so n has no bound.  Lane l
// alone reads and writes positions l, l + 64, ... of both arrays (the head's rank is written by the lane that owns it):
// no LDS, no barrier, no atomics.  A latency kernel like the others of this file; not tuned.
__global__ __launch_bounds__(64) void soft_oks_nms_grouped_kernel(int K, double thresh, int decay_type, int use_vis,
                                                                  double in_vis_thre, int max_keep,
                                                                  const int* __restrict__ off, const float* __restrict__ kpts,
                                                                  const double* __restrict__ areas,
                                                                  const double* __restrict__ scores,
                                                                  const double* __restrict__ sigmas, double* soft_score,
                                                                  int* rank) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int base = off[img];
  const int n = off[img + 1] - base;
  double best = 0.0;
  int best_p = -1;                                                  // this lane's best untaken (score, position)
  for (int p = lane; p < n; p += 64) {
    const double s = scores[base + p];
    soft_score[base + p] = s;
    rank[base + p] = -1;
    if (best_p < 0 || s > best) { best = s; best_p = p; }           // ascending p: the lowest position of equal scores
  }
  const int rounds = min(n, max_keep);
  for (int r = 0; r < rounds; ++r) {
    for (int o = 32; o > 0; o >>= 1) {
      const double s = __shfl_xor(best, o, 64);
      const int p = __shfl_xor(best_p, o, 64);
      if (p >= 0 && (best_p < 0 || s > best || (s == best && p < best_p))) { best = s; best_p = p; }
    }
    const int head = __shfl(best_p, 0, 64);
    if (head < 0) break;                                            // cannot happen while r < n; uniform
    if ((head & 63) == lane) rank[base + head] = r;
    const float* g = kpts + (long)(base + head) * K * 3;
    const double a_g = areas[base + head];
    best = 0.0;
    best_p = -1;
    for (int c = lane; c < n; c += 64) {
      if (c == head || rank[base + c] >= 0) continue;
      const double oks = nms_oks(g, kpts + (long)(base + c) * K * 3, a_g, areas[base + c], sigmas, K, use_vis, in_vis_thre);
      double s = soft_score[base + c];
      if (decay_type == 0) s = s * exp(-(oks * oks) / thresh);
      else if (oks >= thresh) s = s * (1 - oks);
      soft_score[base + c] = s;
      if (best_p < 0 || s > best) { best = s; best_p = c; }
    }
  }
}

struct KptMatchArgs {
  int K, n_thr, n_area;
  long gt_total, dt_total;
  const int* dt_off;
  const int* gt_off;
  const long* oks_off;
  const float* dt_kpts;
  const double* gt_kpts;
  const double* gt_area;
  const double* gt_bbox;
  const int* gt_flags;
  const double* sigmas;
  const double* thrs;
  const double* area_rng;
  double* oks;
  int* dt_matched;
  int* dt_ignored;
  int* gt_order;             // workspace [n_area][gt_total]
  unsigned char* gt_taken;   // workspace [n_area * n_thr][gt_total]
};

__device__ __forceinline__ bool out_of_range(double area, const double* __restrict__ rng) {
  return area < rng[0] || area > rng[1];
}

// Area of the extent of a detection's key points dk [K][3], the area COCOeval gives a detection without a box.
__device__ __forceinline__ double kpt_extent_area(const float* dk, int K) {
  double x0 = dk[0], x1 = dk[0], y0 = dk[1], y1 = dk[1];
  for (int j = 1; j < K; ++j) {
    x0 = fmin(x0, (double)dk[j * 3]); x1 = fmax(x1, (double)dk[j * 3]);
    y0 = fmin(y0, (double)dk[j * 3 + 1]); y1 = fmax(y1, (double)dk[j * 3 + 1]);
  }
  return (x1 - x0) * (y1 - y0);
}

// One wavefront per image.  (a) the D x G OKS matrix of computeOks; (b) evaluateImg: one lane per (area range,
// threshold) walks the detections in score order over the ground truths sorted non-ignored first.
__global__ __launch_bounds__(64) void coco_kpt_match_kernel(KptMatchArgs A) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int K = A.K;
  const int d0 = A.dt_off[img], D = A.dt_off[img + 1] - d0;
  const int g0 = A.gt_off[img], G = A.gt_off[img + 1] - g0;
  if (D <= 0 || G <= 0) {
    // no matrix: every detection is unmatched, and ignored where its own area lies outside the range
    for (int idx = lane; idx < D * A.n_area * A.n_thr; idx += 64) {
      const int d = idx % D, l = idx / D, a = l / A.n_thr;
      const float* dk = A.dt_kpts + (long)(d0 + d) * K * 3;
      A.dt_matched[(long)l * A.dt_total + d0 + d] = 0;
      A.dt_ignored[(long)l * A.dt_total + d0 + d] = out_of_range(kpt_extent_area(dk, K), A.area_rng + 2 * a) ? 1 : 0;
    }
    return;
  }
  double* oks = A.oks + A.oks_off[img];
  for (long idx = lane; idx < (long)D * G; idx += 64) {
    const int d = (int)(idx / G), g = (int)(idx % G);
    const float* dk = A.dt_kpts + (long)(d0 + d) * K * 3;
    const double* gk = A.gt_kpts + (long)(g0 + g) * K * 3;
    int k1 = 0;
    for (int j = 0; j < K; ++j) k1 += gk[j * 3 + 2] > 0 ? 1 : 0;
    const double* bb = A.gt_bbox + (long)(g0 + g) * 4;
    const double bx0 = bb[0] - bb[2], bx1 = bb[0] + bb[2] * 2, by0 = bb[1] - bb[3], by1 = bb[1] + bb[3] * 2;
    const double den = A.gt_area[g0 + g] + KPT_SPACING1;
    double sum = 0.0;
    int cnt = 0;
    for (int j = 0; j < K; ++j) {
      const double xd = dk[j * 3], yd = dk[j * 3 + 1];
      double dx, dy;
      if (k1 > 0) {
        if (!(gk[j * 3 + 2] > 0)) continue;
        dx = xd - gk[j * 3];
        dy = yd - gk[j * 3 + 1];
      } else {
        dx = fmax(0.0, bx0 - xd) + fmax(0.0, xd - bx1);
        dy = fmax(0.0, by0 - yd) + fmax(0.0, yd - by1);
      }
      const double var = (A.sigmas[j] * 2) * (A.sigmas[j] * 2);
      sum += exp(-((dx * dx + dy * dy) / var / den / 2));
      ++cnt;
    }
    oks[idx] = sum / cnt;
  }
  // ground truths stably sorted by the ignore flag, per area range (lane a), and the taken flags cleared
  if (lane < A.n_area) {
    int* ord = A.gt_order + (long)lane * A.gt_total + g0;
    int w = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int g = 0; g < G; ++g) {
        const int ig = (A.gt_flags[g0 + g] != 0 || out_of_range(A.gt_area[g0 + g], A.area_rng + 2 * lane)) ? 1 : 0;
        if (ig == pass) ord[w++] = g;
      }
  }
  for (long idx = lane; idx < (long)A.n_area * A.n_thr * G; idx += 64)
    A.gt_taken[(idx / G) * A.gt_total + g0 + idx % G] = 0;
  __syncthreads();
  if (lane >= A.n_area * A.n_thr) return;
  const int a = lane / A.n_thr;
  const double thr = A.thrs[lane % A.n_thr];
  const double* rng = A.area_rng + 2 * a;
  const int* ord = A.gt_order + (long)a * A.gt_total + g0;
  unsigned char* taken = A.gt_taken + (long)lane * A.gt_total + g0;
  for (int d = 0; d < D; ++d) {
    double best = fmin(thr, 1 - 1e-10);
    int m = -1, m_ig = 0;
    for (int gi = 0; gi < G; ++gi) {
      const int g = ord[gi];
      const int flags = A.gt_flags[g0 + g];
      const int ig = (flags != 0 || out_of_range(A.gt_area[g0 + g], rng)) ? 1 : 0;
      if (taken[g] && !(flags & 1)) continue;       // matched already and not a crowd
      if (m > -1 && m_ig == 0 && ig == 1) break;    // a non-ignored match stands; only ignored ones follow
      const double v = oks[(long)d * G + g];
      if (v < best) continue;
      best = v;
      m = g;
      m_ig = ig;
    }
    const long o = (long)lane * A.dt_total + d0 + d;
    if (m == -1) {
      const float* dk = A.dt_kpts + (long)(d0 + d) * K * 3;
      A.dt_matched[o] = 0;
      A.dt_ignored[o] = out_of_range(kpt_extent_area(dk, K), rng) ? 1 : 0;
    } else {
      A.dt_matched[o] = g0 + m + 1;
      A.dt_ignored[o] = m_ig;
      taken[m] = 1;
    }
  }
}

// check_valid_annotations of lib/analysis/evaluation.py:132-178, one wavefront per image.  Pass 1: lanes stride over
// the image's ground truths and write `valid`; pass 2: a valid one counts the other valid ones it overlaps.
__global__ __launch_bounds__(64) void kpt_crowding_kernel(int K, double thresh, const int* __restrict__ off,
                                                          const double* __restrict__ bbox, const double* __restrict__ kpts,
                                                          const double* __restrict__ area, const double* __restrict__ image_wh,
                                                          int* valid, int* __restrict__ num_overlaps) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const int g0 = off[img], G = off[img + 1] - g0;
  const double W = image_wh[img * 2], H = image_wh[img * 2 + 1];
  for (int g = lane; g < G; g += 64) {
    const double* kp = kpts + (long)(g0 + g) * K * 3;
    double top = kp[0];
    for (int j = 1; j < K * 3; ++j) top = py_max(top, kp[j]);
    const double* b = bbox + (long)(g0 + g) * 4;
    const double x1 = py_max(0.0, b[0]), y1 = py_max(0.0, b[1]);
    const double x2 = py_min(W - 1, x1 + py_max(0.0, b[2] - 1));
    const double y2 = py_min(H - 1, y1 + py_max(0.0, b[3] - 1));
    valid[g0 + g] = (top != 0 && area[g0 + g] > 0 && x2 >= x1 && y2 >= y1) ? 1 : 0;
  }
  __syncthreads();
  for (int g = lane; g < G; g += 64) {
    int n = -1;
    if (valid[g0 + g]) {
      n = 0;
      for (int h = 0; h < G; ++h) {
        if (h == g || !valid[g0 + h]) continue;
        const int lo = min(g, h), hi = max(g, h);                   // compute_ious fills [i][j] for i < j and mirrors it
        if (box_iou(bbox + (long)(g0 + lo) * 4, bbox + (long)(g0 + hi) * 4) > thresh) ++n;
      }
    }
    num_overlaps[g0 + g] = n;
  }
}

#define KPT_SEG_MAX 64

// COCOeval accumulate + summarize for one segment per wavefront (core/keypoint_eval.py: accumulate, summarize).  Lane
// l = a * n_thr + t owns the (area range, threshold) pair of the matching kernel's lane l: cumulative tp / fp over the
// segment's detections (already in descending score order), the precision envelope from the right, the left
// searchsorted of every recall threshold.  Then lanes 0-9 form the ten figures, adding over t in index order.
__global__ __launch_bounds__(64) void kpt_segment_ap_kernel(int max_len, long dt_total, int n_area, int n_thr, int n_rec,
                                                            int t_half, int t_three_q, const int* __restrict__ seg_off,
                                                            const int* __restrict__ dt_matched,
                                                            const int* __restrict__ dt_ignored, const int* __restrict__ npig,
                                                            const double* __restrict__ rec_thrs, double* __restrict__ stats,
                                                            double* __restrict__ recall) {
  __shared__ double pr[KPT_SEG_MAX][64];          // [detection][lane]: a lane's column, no bank shared within a half-wave
  __shared__ unsigned char tps[KPT_SEG_MAX][64];
  __shared__ double lane_pr[64], lane_rc[64];     // per pair: sum of its n_rec precision values, its recall; -1 = not counted
  const int seg = blockIdx.x, lane = threadIdx.x;
  const int d0 = seg_off[seg];
  const int D = min(seg_off[seg + 1] - d0, min(max_len, KPT_SEG_MAX));
  const bool active = lane < n_area * n_thr;
  const int a = lane / n_thr, t = lane % n_thr;
  double p_sum = -1.0, rc_last = -1.0;
  const int np = active ? npig[(long)seg * n_area + a] : 0;
  if (active && np != 0) {
    const int* m = dt_matched + (long)lane * dt_total + d0;
    const int* ig = dt_ignored + (long)lane * dt_total + d0;
    int tp = 0, fp = 0;
    for (int d = 0; d < D; ++d) {
      const bool matched = m[d] != 0, ignored = ig[d] != 0;
      tp += (matched && !ignored) ? 1 : 0;
      fp += (!matched && !ignored) ? 1 : 0;
      tps[d][lane] = (unsigned char)tp;
      pr[d][lane] = (double)tp / ((double)fp + (double)tp + KPT_SPACING1);
    }
    for (int d = D - 1; d > 0; --d)
      if (pr[d][lane] > pr[d - 1][lane]) pr[d - 1][lane] = pr[d][lane];
    rc_last = D > 0 ? (double)tp / (double)np : 0.0;
    p_sum = 0.0;
    int at = 0;                                   // recall thresholds ascend and rc does not descend: one walk
    for (int r = 0; r < n_rec; ++r) {
      const double thr = rec_thrs[r];
      while (at < D && (double)tps[at][lane] / (double)np < thr) ++at;
      if (at < D) p_sum = p_sum + pr[at][lane];
    }
  }
  lane_pr[lane] = p_sum;
  lane_rc[lane] = rc_last;
  if (active) recall[((long)seg * n_thr + t) * n_area + a] = rc_last;
  __syncthreads();
  if (lane >= 10) return;
  // figure f: precision (f < 5) or recall; all / one threshold; area range 0 (all), 1 (medium), 2 (large)
  const int f = lane % 5;
  const bool is_pr = lane < 5;
  const int ar = f == 3 ? 1 : f == 4 ? 2 : 0;
  const int t_lo = f == 1 ? t_half : f == 2 ? t_three_q : 0;
  const int t_hi = (f == 1 || f == 2) ? t_lo + 1 : n_thr;
  double sum = 0.0;
  long cnt = 0;
  for (int tt = t_lo; tt < t_hi; ++tt) {
    const double v = is_pr ? lane_pr[ar * n_thr + tt] : lane_rc[ar * n_thr + tt];
    if (v > -1) {
      sum = sum + v;
      cnt += is_pr ? n_rec : 1;
    }
  }
  stats[(long)seg * 10 + lane] = cnt > 0 ? sum / (double)cnt : -1.0;
}

extern "C" int buctd_kpt_rescore(const float* preds, const double* box_in, int n, int K, double in_vis_thre,
                                 double* score, double* box_score, double* keypoint_score, void* stream) {
  BUCTD_CHECK_ARG(n >= 0 && K > 0, "buctd_kpt_rescore: bad argument");
  if (n == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(preds && box_in && score && box_score && keypoint_score, "buctd_kpt_rescore: null pointer");
  hipLaunchKernelGGL(kpt_rescore_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, (hipStream_t)stream, n, K, in_vis_thre, preds,
                     box_in, score, box_score, keypoint_score);
  BUCTD_CHECK_LAUNCH("buctd_kpt_rescore");
  return BUCTD_OK;
}

extern "C" int buctd_oks_nms_grouped(const int* offsets, int images, int max_per_image, const float* kpts,
                                     const double* areas, const double* sigmas, int K, double thresh, int use_vis,
                                     double in_vis_thre, int* keep, void* stream) {
  BUCTD_CHECK_ARG(images >= 0 && K > 0 && max_per_image >= 0, "buctd_oks_nms_grouped: bad argument");
  if (images == 0 || max_per_image == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(offsets && kpts && areas && sigmas && keep, "buctd_oks_nms_grouped: null pointer");
  const int cap_words = ceil_div(max_per_image, 64);
  BUCTD_CHECK_ARG((size_t)cap_words * 8 <= 64 * 1024, "buctd_oks_nms_grouped: more than 524288 persons in one image");
  hipLaunchKernelGGL(oks_nms_grouped_kernel, dim3(images), dim3(64), (size_t)cap_words * 8, (hipStream_t)stream, K,
                     cap_words, thresh, use_vis, in_vis_thre, offsets, kpts, areas, sigmas, keep);
  BUCTD_CHECK_LAUNCH("buctd_oks_nms_grouped");
  return BUCTD_OK;
}

extern "C" int buctd_soft_oks_nms_grouped(const int* offsets, int images, const float* kpts, const double* areas,
                                          const double* scores, const double* sigmas, int K, double thresh,
                                          int decay_type, int use_vis, double in_vis_thre, int max_keep,
                                          double* soft_score, int* rank, void* stream) {
  BUCTD_CHECK_ARG(images >= 0 && K > 0 && max_keep > 0, "buctd_soft_oks_nms_grouped: bad argument");
  BUCTD_CHECK_ARG(thresh > 0, "buctd_soft_oks_nms_grouped: thresh must be > 0 (it divides the gaussian exponent)");
  BUCTD_CHECK_ARG(decay_type == 0 || decay_type == 1, "buctd_soft_oks_nms_grouped: decay_type is 0 (gaussian) or 1 (linear)");
  BUCTD_CHECK_ARG(offsets && kpts && areas && scores && sigmas && soft_score && rank,
                  "buctd_soft_oks_nms_grouped: null pointer");
  if (images == 0) return BUCTD_OK;
  hipLaunchKernelGGL(soft_oks_nms_grouped_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, K, thresh, decay_type,
                     use_vis, in_vis_thre, max_keep, offsets, kpts, areas, scores, sigmas, soft_score, rank);
  BUCTD_CHECK_LAUNCH("buctd_soft_oks_nms_grouped");
  return BUCTD_OK;
}

extern "C" size_t buctd_coco_kpt_match_workspace(long gt_total, int n_thr, int n_area) {
  if (gt_total <= 0 || n_thr <= 0 || n_area <= 0) return 0;
  return (size_t)gt_total * n_area * sizeof(int) + (size_t)gt_total * n_area * n_thr;
}

extern "C" int buctd_coco_kpt_match(const buctd_kpt_match_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  BUCTD_CHECK_ARG(a && a->images >= 0 && a->K > 0 && a->dt_total >= 0 && a->gt_total >= 0, "buctd_coco_kpt_match: bad argument");
  BUCTD_CHECK_ARG(a->n_thr > 0 && a->n_area > 0 && a->n_thr * a->n_area <= 64,
                  "buctd_coco_kpt_match: one lane per (area range, threshold): at most 64 pairs");
  if (a->images == 0 || a->dt_total == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(a->dt_total * (long)a->n_thr * a->n_area < (1l << 31) && a->gt_total < (1l << 31),
                  "buctd_coco_kpt_match: table too large");
  BUCTD_CHECK_ARG(a->dt_offsets && a->gt_offsets && a->oks_offsets && a->dt_kpts && a->sigmas && a->thresholds &&
                      a->area_ranges && a->dt_matched && a->dt_ignored,
                  "buctd_coco_kpt_match: null pointer");
  BUCTD_CHECK_ARG(a->gt_total == 0 || (a->gt_kpts && a->gt_area && a->gt_bbox && a->gt_flags && a->oks),
                  "buctd_coco_kpt_match: null ground-truth pointer");
  const size_t need = buctd_coco_kpt_match_workspace(a->gt_total, a->n_thr, a->n_area);
  if (need && (!workspace || workspace_bytes < need)) {
    buctd_set_error("buctd_coco_kpt_match: workspace %zu bytes < required %zu", workspace_bytes, need);
    return BUCTD_EWORKSPACE;
  }
  KptMatchArgs k;
  k.K = a->K; k.n_thr = a->n_thr; k.n_area = a->n_area;
  k.gt_total = a->gt_total; k.dt_total = a->dt_total;
  k.dt_off = a->dt_offsets; k.gt_off = a->gt_offsets; k.oks_off = a->oks_offsets;
  k.dt_kpts = a->dt_kpts; k.gt_kpts = a->gt_kpts; k.gt_area = a->gt_area; k.gt_bbox = a->gt_bbox;
  k.gt_flags = a->gt_flags; k.sigmas = a->sigmas; k.thrs = a->thresholds; k.area_rng = a->area_ranges;
  k.oks = a->oks; k.dt_matched = a->dt_matched; k.dt_ignored = a->dt_ignored;
  k.gt_order = (int*)workspace;
  k.gt_taken = (unsigned char*)workspace + (size_t)a->gt_total * a->n_area * sizeof(int);
  hipLaunchKernelGGL(coco_kpt_match_kernel, dim3(a->images), dim3(64), 0, (hipStream_t)stream, k);
  BUCTD_CHECK_LAUNCH("buctd_coco_kpt_match");
  return BUCTD_OK;
}

extern "C" int buctd_kpt_crowding(const int* gt_offsets, int images, long gt_total, int K, const double* gt_bbox,
                                  const double* gt_kpts, const double* gt_area, const double* image_wh, double iou_thresh,
                                  int* valid, int* num_overlaps, void* stream) {
  BUCTD_CHECK_ARG(images >= 0 && gt_total >= 0 && K > 0, "buctd_kpt_crowding: bad argument");
  if (images == 0 || gt_total == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(gt_total * (long)K * 3 < (1l << 31), "buctd_kpt_crowding: table too large");
  BUCTD_CHECK_ARG(gt_offsets && gt_bbox && gt_kpts && gt_area && image_wh && valid && num_overlaps,
                  "buctd_kpt_crowding: null pointer");
  hipLaunchKernelGGL(kpt_crowding_kernel, dim3(images), dim3(64), 0, (hipStream_t)stream, K, iou_thresh, gt_offsets, gt_bbox,
                     gt_kpts, gt_area, image_wh, valid, num_overlaps);
  BUCTD_CHECK_LAUNCH("buctd_kpt_crowding");
  return BUCTD_OK;
}

extern "C" int buctd_kpt_segment_ap(const int* seg_offsets, int segments, int max_seg_len, long dt_total,
                                    const int* dt_matched, const int* dt_ignored, int n_area, int n_thr, const int* npig,
                                    const double* rec_thrs, int n_rec, int t_half, int t_three_q, double* stats,
                                    double* recall, void* stream) {
  BUCTD_CHECK_ARG(segments >= 0 && max_seg_len >= 0 && dt_total >= 0 && n_rec >= 0, "buctd_kpt_segment_ap: bad argument");
  BUCTD_CHECK_ARG(n_thr > 0 && n_area > 0 && n_thr * n_area <= 64,
                  "buctd_kpt_segment_ap: one lane per (area range, threshold): at most 64 pairs");
  BUCTD_CHECK_ARG(n_area >= 3 && t_half >= 0 && t_half < n_thr && t_three_q >= 0 && t_three_q < n_thr,
                  "buctd_kpt_segment_ap: the figures need the area ranges all, medium, large and two threshold indices");
  BUCTD_CHECK_ARG(max_seg_len <= KPT_SEG_MAX, "buctd_kpt_segment_ap: a segment holds at most 64 detections");
  BUCTD_CHECK_ARG(n_rec <= 128, "buctd_kpt_segment_ap: at most 128 recall thresholds");
  BUCTD_CHECK_ARG(dt_total * (long)n_thr * n_area < (1l << 31), "buctd_kpt_segment_ap: table too large");
  if (segments == 0) return BUCTD_OK;
  BUCTD_CHECK_ARG(seg_offsets && npig && stats && recall && (n_rec == 0 || rec_thrs),
                  "buctd_kpt_segment_ap: null pointer");
  BUCTD_CHECK_ARG(dt_total == 0 || max_seg_len == 0 || (dt_matched && dt_ignored),
                  "buctd_kpt_segment_ap: null match table");
  hipLaunchKernelGGL(kpt_segment_ap_kernel, dim3(segments), dim3(64), 0, (hipStream_t)stream, max_seg_len, dt_total, n_area,
                     n_thr, n_rec, t_half, t_three_q, seg_offsets, dt_matched, dt_ignored, npig, rec_thrs, stats, recall);
  BUCTD_CHECK_LAUNCH("buctd_kpt_segment_ap");
  return BUCTD_OK;
}
