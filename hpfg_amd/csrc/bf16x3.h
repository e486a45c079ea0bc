// The split-bf16 ("bf16x3") arithmetic of the default math mode, ONE definition of each piece for every kernel family that multiplies on
// v_mfma_f32_16x16x32_bf16 -- the four convolution families through stage.h, the three attention families through attn_frag.h, the token
// GEMMs of gemm.hip:
//   * the vector types of a fragment and of its staging;
//   * the split x = hi + lo, hi = bf16(x) (round to nearest even), lo = bf16(x - hi), of a pair (split2) and its packings for 4 and 8
//     values (split4, split8, split8v): loops over split2 plus a bit cast, the rounding is stated in split2 alone;
//   * the transposing LDS read pair that hands a lane 8 contraction values of an image stored contraction-index-slow (tr_read8);
//   * the product a b ~ ah bh + al bh + ah bl as three MFMA issues into one fp32 accumulator, the lo lo term dropped (2^-16 relative)
//     (HPFG_MFMA3).  Each issue rounds into the accumulator, so the order of the two lo issues is part of a kernel's bits: it is the
//     macro's compile-time argument and every call site passes the order it has always had.
// oracle/bf16x3_ref.py and the float64 tolerances of the suite restate this contract; tests/golden/conv_bits.json, attn_bits.json and
// dense_bits.json pin its bits per family.  A change to the contract is an edit here and new golden files, nowhere else.
// Deliberate exceptions (a site stays its own text where the shared form would change its bits or its machine code): none.
#pragma once
#include "common.h"

namespace hpfg_bf16x3 {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// (x0, x1) -> the packed hi word and the packed lo word: the pair goes through v_cvt_pk_bf16_f32, and the packed hi word is widened back
// with one shift / one mask.  (hw is assigned last: assigned first and read back for the widening, the chunked, fused and weight-gradient
// kernels of the BNACT and CAT sources came out with another schedule.)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& hw, uint32_t& lw) {
  const bf16x2 h = __builtin_convertvector(f32x2{x0, x1}, bf16x2);
  const uint32_t w = __builtin_bit_cast(uint32_t, h);
  const f32x2 hf = {__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)};
  const bf16x2 l = __builtin_convertvector(f32x2{x0, x1} - hf, bf16x2);
  hw = w;
  lw = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ void split4(const f32x4& v, bf16x4& hi, bf16x4& lo) {
  uint32_t h[2], l[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) split2(v[2 * k], v[2 * k + 1], h[k], l[k]);
  const bf16x2 h0 = __builtin_bit_cast(bf16x2, h[0]), h1 = __builtin_bit_cast(bf16x2, h[1]);
  const bf16x2 l0 = __builtin_bit_cast(bf16x2, l[0]), l1 = __builtin_bit_cast(bf16x2, l[1]);
  hi = bf16x4{h0[0], h0[1], h1[0], h1[1]};
  lo = bf16x4{l0[0], l0[1], l1[0], l1[1]};
}
__device__ __forceinline__ void split8v(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) split2(v[2 * k], v[2 * k + 1], h[k], l[k]);
  hi = __builtin_bit_cast(bf16x8, (u32x4{h[0], h[1], h[2], h[3]}));
  lo = __builtin_bit_cast(bf16x8, (u32x4{l[0], l[1], l[2], l[3]}));
}
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) split2(k < 2 ? a[2 * k] : b[2 * k - 4], k < 2 ? a[2 * k + 1] : b[2 * k - 3], h[k], l[k]);
  hi = __builtin_bit_cast(bf16x8, (u32x4{h[0], h[1], h[2], h[3]}));
  lo = __builtin_bit_cast(bf16x8, (u32x4{l[0], l[1], l[2], l[3]}));
}

// ds_read_b64_tr_b16 twice: p0 / p1 are this lane's addresses inside two 4-row blocks of an LDS image whose rows run along the
// contraction index ([pixel][16 ch] in wgrad_bf16_kernel.h, [k][row] and [token][n] in gemm.hip); the result is the 8 contraction values
// of this lane's column
__device__ __forceinline__ bf16x8 tr_read8(const unsigned char* p0, const unsigned char* p1) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p0));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p1));
  return __builtin_bit_cast(bf16x8, (s16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}));
}

}  // namespace hpfg_bf16x3

// ACC += a b in three issues, a the builtin's first operand and b its second: (AH, BH), then the two lo terms in the order ORDER names.
//   LO_OF_FIRST_THEN_SECOND   (AL, BH) then (AH, BL): chunked, whole-tile and fused dgrad convolutions, GEMM, attention
//   LO_OF_SECOND_THEN_FIRST   (AH, BL) then (AL, BH): the weight gradients (wgrad_bf16_kernel.h, the wgrad part of fused_bwd_kernel.h)
// A macro, not an inline function: through a function's reference parameter the same three issues came out of the compiler with other
// registers and another schedule in attn_mfma_dkv_kernel<32> and three SPLIT16 instantiations of the weight gradient.
#define HPFG_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, ACC, 0, 0, 0);
#define HPFG_MFMA3_LO_OF_FIRST_THEN_SECOND(ACC, AH, AL, BH, BL) HPFG_MFMA(ACC, AH, BH) HPFG_MFMA(ACC, AL, BH) HPFG_MFMA(ACC, AH, BL)
#define HPFG_MFMA3_LO_OF_SECOND_THEN_FIRST(ACC, AH, AL, BH, BL) HPFG_MFMA(ACC, AH, BH) HPFG_MFMA(ACC, AH, BL) HPFG_MFMA(ACC, AL, BH)
#define HPFG_MFMA3(ORDER, ACC, AH, AL, BH, BL) HPFG_MFMA3_##ORDER(ACC, AH, AL, BH, BL)
