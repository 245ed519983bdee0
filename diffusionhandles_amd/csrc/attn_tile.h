// Tile products of the attention kernels (attention.hip) that the cross-attention epilogue of k_gemm_dma (gemm.hip) runs as well:
// the padded LDS tile layout, S^T = K Q^T from row fragments, the transposed A operand of O^T = V^T P^T, and the accumulator ->
// B-operand packing of P.  See the head of attention.hip for the product shapes.
#pragma once
#include "gemm_k.h"

namespace dh {

typedef short v4s __attribute__((ext_vector_type(4)));

template <class T> using Mma = Mfma<T>;      // (gemm_k.h: v_mfma_f32_32x32x16 on 16-bit operands)

constexpr int HD = 64;        // head dim
constexpr int TLD = 72;       // LDS row stride in halves (144 B: conflict-free b128 and tr_b16 reads)
constexpr int TILE = 64 * TLD;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float SCALE = 0.125f;               // 1/sqrt(64)
constexpr float CEXP = SCALE * LOG2E;         // scores are exponentiated as exp2(s * CEXP - m * CEXP)

__device__ __forceinline__ v16f zero16() {
  v16f z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// acc = sum_kk mfma(A = rows (rowbase + lane&31) of an LDS row-major tile, B = register fragments)
template <class T>
__device__ __forceinline__ v16f tile_times_frags(const unsigned short* tile, int rowbase, int ln, int hi, const uint4 (&f)[4]) {
  v16f acc = zero16();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const uint4 a = *reinterpret_cast<const uint4*>(&tile[(rowbase + ln) * TLD + 16 * kk + 8 * hi]);
    acc = Mma<T>::run(a, f[kk], acc);
  }
  return acc;
}

// A operand = TRANSPOSE of a row-major tile: fragment row = tile column (cbase + lane&31), reduction slots =
// tile rows r0.., in the accumulator order (rows r0 + 4 hi + 0..3 and r0 + 8 + 4 hi + 0..3).
// `tptr` = &tile[(4 hi + (t >> 2)) * TLD + 16 * ((lane >> 4) & 1) + 4 * (t & 3)], t = lane & 15 (per lane, hoisted)
__device__ __forceinline__ uint4 tr_frag(const unsigned short* tptr, int cbase, int r0) {
  typedef __attribute__((address_space(3))) v4s* lp;
  const unsigned short* a = tptr + r0 * TLD + cbase;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a));
  const v4s up = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a + 8 * TLD));
  const uint2 l2 = __builtin_bit_cast(uint2, lo), u2 = __builtin_bit_cast(uint2, up);
  return make_uint4(l2.x, l2.y, u2.x, u2.y);
}

// registers 8s..8s+7 of an accumulator -> B operand (16-bit), rounded to NEAREST in both types.  fp16 used v_cvt_pkrtz_f16_f32
// (toward zero) until tests/test_attention_range_gpu.py: the forward's o = sum(P16 v) / sum(P) then came out low by up to 2^-11 of
// itself -- the row maximum's own P, exp2 of an fma residue a hair under zero, became 1 - 2^-11 -- and delta = rowsum(dO o) carried
// that bias times |delta| into dS, where a common component of k (dq) or a sum over many alike rows (dk) adds it up coherently: dq,
// dk 1.1 to 2.2 tolerances off where the once-rounded o gives 0.4.  gfx950's v_cvt_pk_f16_f32 rounds to nearest, one instruction too.
typedef float pk2f __attribute__((ext_vector_type(2)));
typedef _Float16 pk2h __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack2_f16(float a, float b) {
  const pk2f x = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(x, pk2h));
}
template <class T>
__device__ __forceinline__ uint4 pack8(const v16f& p, int s);
template <>
__device__ __forceinline__ uint4 pack8<f16>(const v16f& p, int s) {
  uint4 o;
  o.x = pack2_f16(p[8 * s + 0], p[8 * s + 1]);
  o.y = pack2_f16(p[8 * s + 2], p[8 * s + 3]);
  o.z = pack2_f16(p[8 * s + 4], p[8 * s + 5]);
  o.w = pack2_f16(p[8 * s + 6], p[8 * s + 7]);
  return o;
}
template <>
__device__ __forceinline__ uint4 pack8<bf16>(const v16f& p, int s) {
  bf16 o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (bf16)p[8 * s + j];
  return *reinterpret_cast<uint4*>(o);
}

__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }


}  // namespace dh
