// Split-fp32 operands for v_mfma_f32_16x16x32_bf16 (x = hi + mid + lo in bf16 pieces, fp32 accumulate): the pieces,
// the LDS row layout and the MFMA sequence shared by the fused attention kernels (attn_smallqk.hip, attn_mha.hip).
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// Two fp32 values -> NP packed bf16 pairs (exact residual chain): one v_cvt_pk_bf16_f32 per piece delivers the packed
// word that is stored, the two residuals come from its halves (shift / mask) - same roundings as the element-wise form,
// 5 instead of 8-9 VALU instructions per value and piece pair.
typedef float a_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 a_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned a_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned a_u32x4 __attribute__((ext_vector_type(4)));
template <int NP>
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned (&w)[NP]) {
  a_f32x2 r = {x0, x1};
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    w[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, a_bf16x2));
    if (q + 1 < NP) r -= (a_f32x2){__uint_as_float(w[q] << 16), __uint_as_float(w[q] & 0xffff0000u)};
  }
}
// channels c..c+3 of one LDS row -> NP bf16 pieces, piece q at byte q * LO + 2c
template <int LO, int NP>
__device__ __forceinline__ void split_store4(unsigned char* row, int c, f32x4 v) {
  unsigned lo[NP], hi[NP];
  split_pair<NP>(v[0], v[1], lo);
  split_pair<NP>(v[2], v[3], hi);
#pragma unroll
  for (int q = 0; q < NP; ++q) *reinterpret_cast<a_u32x2*>(row + q * LO + 2 * c) = (a_u32x2){lo[q], hi[q]};
}
// gfx950 transpose read: the 16 lanes of a group address 4 rows x 16 bf16; lane c receives the 4 rows of column c.
// Two of them (rows +0..3 at p, rows +0..3 at q) give the 8 reduction slots of one MFMA operand.
__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* p, const unsigned char* q) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p);
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)q);
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <int NP>
__device__ __forceinline__ void split8(const float (&x)[8], bf16x8 (&pc)[NP]) {
  unsigned w[4][NP];
#pragma unroll
  for (int e = 0; e < 4; ++e) split_pair<NP>(x[2 * e], x[2 * e + 1], w[e]);
#pragma unroll
  for (int q = 0; q < NP; ++q) pc[q] = __builtin_bit_cast(bf16x8, (a_u32x4){w[0][q], w[1][q], w[2][q], w[3][q]});
}
// acc += a . b on split operands, smallest terms first.  NP = 2: the three terms of weight >= 2^-8 (bf16x3, product
// error ~2^-16); NP = 3: the six terms of weight >= 2^-16 (bf16x6, fp32 class - see conv3x3.hip)
template <int NP>
__device__ __forceinline__ void mfma_split(f32x4& acc, const bf16x8 (&a)[NP], const bf16x8 (&b)[NP]) {
  if constexpr (NP == 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], acc, 0, 0, 0);
  }
}
// LDS tile row of C channels in NP bf16 pieces, padded to 32 mod 64 bytes (conflict-free 16-byte row reads)
constexpr int split_row_bytes(int c, int np) { return c * 2 * np + (((c * 2 * np) % 64 == 32) ? 0 : 32); }
template <int C, int NP>
struct SplitRow {
  static constexpr int LO = C * 2;
  static constexpr int RS = split_row_bytes(C, NP);
};
