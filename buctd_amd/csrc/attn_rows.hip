// Chosen rows of the attention matrix of the TransPose encoder (reference lib/models/transpose_h.py:110-150, 168-243:
// return_atten_map=True hands back the head-averaged soft-max weights of nn.MultiheadAttention, [B, T, T] per layer).
//     out[b][r][j] = 1/h sum_head softmax_j(scale * q[rows[b][r]] . k[j])          (eval mode: no dropout, no mask)
// computed for R query rows per image straight from the projected q | k: the "dependency area" of a key point's token is
// ONE row of the T x T matrix, so an inspection of K joints writes K T floats, not T T.  rows == NULL is the full map.
//
// Layout.  A workgroup = 4 wavefronts owns one tile of 16 query rows of one image (grid.y) and a chunk of the keys
// (grid.x); heads run in order inside the workgroup.  There is no V and nothing to accumulate: the logits run on
// v_mfma_f32_16x16x4_f32 with the operands of mha_fwd_kernel (attn_mha.hip) - lane (i16, g) holds channels
// 16 m + 4 g + e of query / key i16, one 16-byte load feeds four MFMA steps, the contraction order is that of
// buctd_mha_heads_fwd - and a head width that is no multiple of 16 is zero-padded inside the last step.
// Keys are read from global memory (L2 resident: T d floats per image) directly into the B operand, the next 16-key block
// travelling while the current one is multiplied.
//   pass 1 (statistics): every workgroup streams ALL keys, wavefront w taking the 16-key blocks w, w + 4, ...; a lane keeps
//     a running (max, sum) per row, merged over the 16 lanes of a row and then over the wavefronts through LDS in a fixed
//     order.  The partition of the keys depends on T alone - not on R or grid.x - and there is one kernel per head width, so
//     a row's statistics, and with them its values, are bit-identical wherever it is computed (duplicates; a row query
//     against the full map).
//   pass 2 (write): the logits of the workgroup's own key chunk are recomputed and exp(s - max) / sum is stored.  The head
//     mean is a read-modify-write of out by the lane that owns (row, key) in every head: program order, no atomics.
// Recomputed: the logits once (2 T R d FLOP per head more) instead of a T x R logit buffer in memory; with grid.x > 1 (few
// rows: R = 17 would leave the GPU empty) pass 1 is repeated per key chunk, which at small R is cheaper than an idle machine.
#include "common.h"
#include "../../include/buctd_hip.h"

#define AR_WAVES 4
#define AR_THREADS (64 * AR_WAVES)

struct AttnRowsArgs {
  const float* q; const float* k; const int* rows;
  float* out; float* out_heads;
  int T, R, h, dh, ldq, ldk;
  int kb_per_split;            // 16-key blocks per workgroup along grid.x (a multiple of AR_WAVES)
  float scale, inv_h;
};

template <int DF>              // DF = ceil(dh / 16) contraction steps of 16 channels
__global__ __launch_bounds__(AR_THREADS) void attn_rows_kernel(AttnRowsArgs a) {
  __shared__ float st_m[AR_WAVES][16], st_l[AR_WAVES][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  const int T = a.T, R = a.R, dh = a.dh, ldq = a.ldq, ldk = a.ldk;
  const int b = blockIdx.z, r0 = blockIdx.y * 16;
  const int nkb = (T + 15) >> 4;
  const int kb0 = blockIdx.x * a.kb_per_split, kb1 = min(nkb, kb0 + a.kb_per_split);
  const float* qb = a.q + (long)b * T * ldq;
  const float* kb = a.k + (long)b * T * ldk;
  const int* rows = a.rows ? a.rows + (long)b * R : nullptr;

  // A operand: this lane loads query row r0 + i16; a row that is not there or names no token loads token 0
  int tok_a;
  {
    const int ri = r0 + i16;
    const int tok = ri < R ? (rows ? rows[ri] : ri) : -1;
    tok_a = (tok >= 0 && tok < T) ? tok : 0;
  }
  // C layout: this lane owns rows r0 + 4 g + r.  bit r of in_r: the row exists; of ok: it names a token
  unsigned in_r = 0, ok = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ri = r0 + 4 * g + r;
    if (ri < R) {
      in_r |= 1u << r;
      const int tok = rows ? rows[ri] : ri;
      if (tok >= 0 && tok < T) ok |= 1u << r;
    }
  }

  auto load_k = [&](f32x4 (&kf)[DF], int kbi, int c0) {
    const int key = min(kbi * 16 + i16, T - 1);      // keys past T re-read the last one; their logits are never used
    const float* kp = kb + (long)key * ldk + c0 + 4 * g;
#pragma unroll
    for (int m = 0; m < DF; ++m)
      kf[m] = 16 * m + 4 * g < dh ? *reinterpret_cast<const f32x4*>(kp + 16 * m) : (f32x4){0.f, 0.f, 0.f, 0.f};
  };

  for (int head = 0; head < a.h; ++head) {
    const int c0 = head * dh;
    f32x4 qf[DF];                                    // (scale q)[row i16][16 m + 4 g + e], zeros past dh
#pragma unroll
    for (int m = 0; m < DF; ++m) {
      if (16 * m + 4 * g < dh) {
        qf[m] = *reinterpret_cast<const f32x4*>(qb + (long)tok_a * ldq + c0 + 16 * m + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[m][e] *= a.scale;
      } else {
        qf[m] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    auto logits = [&](const f32x4 (&kf)[DF]) {
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < DF; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[m][e], kf[m][e], s, 0, 0, 0);
      return s;
    };

    // ---- pass 1: (max, sum exp) of every row over all keys; this lane sees key 16 kbi + i16 of its 4 rows
    float mx[4], ls[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mx[r] = -INFINITY; ls[r] = 0.f; }
    {
      f32x4 kf[DF], kn[DF];
      if (wave < nkb) load_k(kf, wave, c0);
      for (int kbi = wave; kbi < nkb; kbi += AR_WAVES) {
        if (kbi + AR_WAVES < nkb) load_k(kn, kbi + AR_WAVES, c0);
        const f32x4 s = logits(kf);
        if (kbi * 16 + i16 < T) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // one exponential per logit: the smaller of (running max, logit) is rescaled to the larger
            const float d = s[r] - mx[r];                        // +inf on the lane's first key
            const float e = __expf(-fabsf(d));
            ls[r] = d > 0.f ? ls[r] * e + 1.f : ls[r] + e;
            mx[r] = fmaxf(mx[r], s[r]);
          }
        }
#pragma unroll
        for (int m = 0; m < DF; ++m) kf[m] = kn[m];
      }
    }
    if (head) __syncthreads();                       // the previous head's statistics have been read by everyone
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = mx[r];
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
      // a lane (or a whole wavefront) without a key holds (-inf, 0) and contributes nothing
      float l = mx[r] == -INFINITY ? 0.f : ls[r] * __expf(mx[r] - m);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) l += __shfl_xor(l, off, 64);
      if (i16 == 0) {
        st_m[wave][4 * g + r] = m;
        st_l[wave][4 * g + r] = l;
      }
    }
    __syncthreads();
    float row_m[4], row_il[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * g + r;
      float m = st_m[0][row];                        // wavefront 0 always has key block 0: finite
#pragma unroll
      for (int w = 1; w < AR_WAVES; ++w) m = fmaxf(m, st_m[w][row]);
      float l = 0.f;
#pragma unroll
      for (int w = 0; w < AR_WAVES; ++w) {
        const float mw = st_m[w][row];
        l += mw == -INFINITY ? 0.f : st_l[w][row] * __expf(mw - m);
      }
      row_m[r] = m;
      row_il[r] = 1.f / l;
    }

    // ---- pass 2: the workgroup's key chunk, written
    {
      f32x4 kf[DF], kn[DF];
      if (kb0 + wave < kb1) load_k(kf, kb0 + wave, c0);
      for (int kbi = kb0 + wave; kbi < kb1; kbi += AR_WAVES) {
        if (kbi + AR_WAVES < kb1) load_k(kn, kbi + AR_WAVES, c0);
        const f32x4 s = logits(kf);
        const int key = kbi * 16 + i16;
        if (key < T) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (!(in_r >> r & 1u)) continue;
            const int ri = r0 + 4 * g + r;
            const float p = (ok >> r & 1u) ? __expf(s[r] - row_m[r]) * row_il[r] : 0.f;
            if (a.out_heads) a.out_heads[(((long)b * a.h + head) * R + ri) * T + key] = p;
            float* op = a.out + ((long)b * R + ri) * T + key;
            float v = head ? *op + p : p;            // heads in order, by the one lane that owns (row, key)
            if (head == a.h - 1 && a.h > 1) v *= a.inv_h;
            *op = v;
          }
        }
#pragma unroll
        for (int m = 0; m < DF; ++m) kf[m] = kn[m];
      }
    }
  }
}

extern "C" int buctd_attn_rows_supported(int T, int h, int dh) {
  return (T >= 1 && h >= 1 && h <= 4096 && dh >= 4 && dh <= 128 && dh % 4 == 0) ? 1 : 0;
}

template <int DF>
static int attn_rows_launch(int B, const AttnRowsArgs& a, int splits, hipStream_t st) {
  hipLaunchKernelGGL(attn_rows_kernel<DF>, dim3(splits, (a.R + 15) / 16, B), dim3(AR_THREADS), 0, st, a);
  BUCTD_CHECK_LAUNCH("buctd_attn_rows");
  return BUCTD_OK;
}

extern "C" int buctd_attn_rows(const buctd_attn_rows_args* g, void* stream) {
  BUCTD_CHECK_ARG(g, "buctd_attn_rows: null descriptor");
  BUCTD_CHECK_ARG(g->q && g->k && g->out, "buctd_attn_rows: null q, k or out");
  BUCTD_CHECK_ARG(g->B >= 1 && g->B <= 65535, "buctd_attn_rows: batch %d outside 1 .. 65535", g->B);
  BUCTD_CHECK_ARG(buctd_attn_rows_supported(g->T, g->h, g->dh),
                  "buctd_attn_rows: unsupported shape T%d h%d dh%d (T >= 1, h >= 1, dh %% 4 == 0, dh <= 128)", g->T, g->h, g->dh);
  BUCTD_CHECK_ARG(g->R >= 1 && g->R <= 16 * 65535, "buctd_attn_rows: R = %d rows outside 1 .. %d", g->R, 16 * 65535);
  BUCTD_CHECK_ARG(g->rows || g->R == g->T, "buctd_attn_rows: rows == NULL is the full map and needs R == T (R %d, T %d)", g->R,
                  g->T);
  const int hd = g->h * g->dh;
  BUCTD_CHECK_ARG(g->ldq >= hd && g->ldk >= hd && g->ldq % 4 == 0 && g->ldk % 4 == 0,
                  "buctd_attn_rows: row strides must be >= h * dh and multiples of 4 floats");
  BUCTD_CHECK_ARG(((uintptr_t)g->q | (uintptr_t)g->k | (uintptr_t)g->out | (uintptr_t)g->out_heads) % 16 == 0,
                  "buctd_attn_rows: q, k, out, out_heads must be 16-byte aligned");
  BUCTD_CHECK_ARG((uintptr_t)g->rows % 4 == 0, "buctd_attn_rows: rows must be 4-byte aligned");
  AttnRowsArgs a;
  a.q = g->q; a.k = g->k; a.rows = g->rows; a.out = g->out; a.out_heads = g->out_heads;
  a.T = g->T; a.R = g->R; a.h = g->h; a.dh = g->dh; a.ldq = g->ldq; a.ldk = g->ldk;
  a.scale = g->scale; a.inv_h = 1.0f / (float)g->h;
  // With fewer than 128 row tiles the keys of pass 2 are split along grid.x until there are about 256 workgroups (one per
  // CU), each with at least one 16-key block per wavefront; from 128 tiles on the tiles alone occupy the machine.
  const int nkb = (g->T + 15) / 16;
  const long tiles = (long)g->B * ((g->R + 15) / 16);
  int splits = 1;
  if (tiles < 128) splits = (int)min((long)(nkb + AR_WAVES - 1) / AR_WAVES, (256 + tiles - 1) / tiles);
  a.kb_per_split = ((nkb + splits - 1) / splits + AR_WAVES - 1) / AR_WAVES * AR_WAVES;
  splits = (nkb + a.kb_per_split - 1) / a.kb_per_split;
  hipStream_t st = (hipStream_t)stream;
  switch ((g->dh + 15) / 16) {
#define AR_CASE(n) case n: return attn_rows_launch<n>(g->B, a, splits, st);
    AR_CASE(1) AR_CASE(2) AR_CASE(3) AR_CASE(4) AR_CASE(5) AR_CASE(6) AR_CASE(7) AR_CASE(8)
#undef AR_CASE
  }
  buctd_set_error("buctd_attn_rows: no kernel for dh=%d", g->dh);
  return BUCTD_EINVAL;
}
