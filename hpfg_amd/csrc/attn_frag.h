// Fragment helpers of the attention kernels on the matrix cores: the LDS image geometry and the fragment loaders.  The arithmetic -- the
// vector types, the hi / lo split (split8v) and the three-issue product (HPFG_MFMA3, the first operand's lo first) -- is bf16x3.h's, shared with
// the convolutions and the GEMMs.  attn_core.h builds the kernels' phases on them and documents the lane layouts at its top.
#pragma once
#include "bf16x3.h"

namespace {

using namespace hpfg_bf16x3;

constexpr int MK = 64;                         // keys of one LDS image (attn.hip, attn_window.hip: the maximum; attn_keys.hip: one key block)
constexpr int TROW = 144;                      // bytes per row of a [D d][64 keys] bf16 image (128 B + 16 B pad)
constexpr int QROW = 80;                       // bytes per row of a per-wave [D d][32 q] bf16 image (64 B + 16 B pad)
template <int D> struct Geo {
  static_assert(D == 32 || D == 64, "head dim 32 or 64");
  static constexpr int KS = D / 32, DT = D / 16;          // MFMA k-steps over the head dim, 16-row d-tiles
  static constexpr int KROW = 2 * D + 16;                  // bytes per row of a [64 keys][D d] bf16 image (+ 16 B pad)
  static constexpr int KPLANE = MK * KROW, TPL = D * TROW, QPL = D * QROW;
};
constexpr float NEG = -3.0e38f;

// (stage_win of attn_window.hip is this text with the window's token table; why the two are not one function: top of attn_core.h)
// rows [key][D d] of k or v (which = 0 / 1) of one (image, head) -> natural image [64][D] (hi, lo) and / or transposed image [D][64].
// The image holds keys key0 .. key0 + 63 of the M keys (key0 = 0 in attn.hip); rows of keys >= M are zeros and are never loaded.
template <int D>
__device__ __forceinline__ void stage_kv(const float* __restrict__ kv, int b, int h, int M, int C, int which, unsigned char* nat, unsigned char* trn, int tid,
                                         int key0 = 0) {
  constexpr int KROW = Geo<D>::KROW, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
#pragma unroll
  for (int chunk = tid; chunk < MK * D / 8; chunk += 256) {      // 8 head-dim values per thread and pass: one pass at D = 32, two at 64
    const int key = chunk / (D / 8), d0 = (chunk % (D / 8)) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (key0 + key < M) {
      const float* p = kv + (((long)b * M + key0 + key) * 2 + which) * C + h * D + d0;
      const f32x4 a = *reinterpret_cast<const f32x4*>(p), c = *reinterpret_cast<const f32x4*>(p + 4);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = c[0]; v[5] = c[1]; v[6] = c[2]; v[7] = c[3];
    }
    bf16x8 hi, lo;
    split8v(v, hi, lo);
    if (nat) {
      *reinterpret_cast<bf16x8*>(nat + key * KROW + d0 * 2) = hi;
      *reinterpret_cast<bf16x8*>(nat + key * KROW + d0 * 2 + KPLANE) = lo;
    }
    if (trn) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        *reinterpret_cast<__bf16*>(trn + (d0 + j) * TROW + key * 2) = hi[j];
        *reinterpret_cast<__bf16*>(trn + (d0 + j) * TROW + key * 2 + TPL) = lo[j];
      }
    }
  }
}

// fragment of a natural [rows][D d] image for k-step ks: row = row0 + (lane & 15), 8 consecutive d of k-group lane >> 4 (d = 32 ks + 8 g ..)
template <int D>
__device__ __forceinline__ bf16x8 nat_frag(const unsigned char* plane, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(plane + (row0 + (lane & 15)) * Geo<D>::KROW + ks * 64 + (lane >> 4) * 16);
}
// fragment of a transposed [D d][64 pos] image for contraction step s over 32 positions, in the accumulator-operand order: this lane's
// positions are 32 s + 4 g + {0..3} and 32 s + 16 + 4 g + {0..3} (g = lane >> 4), row = d0 + (lane & 15)
__device__ __forceinline__ bf16x8 trn_frag(const unsigned char* plane, int rowbytes, int d0, int s, int lane) {
  const unsigned char* p = plane + (d0 + (lane & 15)) * rowbytes + (32 * s + 4 * (lane >> 4)) * 2;
  const bf16x4 a = *reinterpret_cast<const bf16x4*>(p), b = *reinterpret_cast<const bf16x4*>(p + 32);
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// this lane's 8 head-dim values of k-step ks (k-group lane >> 4) of row `row` of a [.., heads, D] tensor, times `mul`; zeros beyond `nrows`
template <int D>
__device__ __forceinline__ void load_row8(const float* __restrict__ base, long row, long nrows, int C, int h, int ks, int lane, float mul, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (row < nrows) {
    const float* p = base + row * C + h * D + ks * 32 + (lane >> 4) * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), c = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0] * mul; v[1] = a[1] * mul; v[2] = a[2] * mul; v[3] = a[3] * mul;
    v[4] = c[0] * mul; v[5] = c[1] * mul; v[6] = c[2] * mul; v[7] = c[3] * mul;
  }
}

// one row's D values as the split-bf16 fragments of its KS k-steps
template <int D>
__device__ __forceinline__ void load_row_frags(const float* __restrict__ base, long row, long nrows, int C, int h, int lane, float mul,
                                               bf16x8 (&hi)[Geo<D>::KS], bf16x8 (&lo)[Geo<D>::KS]) {
#pragma unroll
  for (int ks = 0; ks < Geo<D>::KS; ++ks) {
    float v[8];
    load_row8<D>(base, row, nrows, C, h, ks, lane, mul, v);
    split8v(v, hi[ks], lo[ks]);
  }
}

// accumulator tiles (2 s, 2 s + 1) -> split-bf16 B operand of contraction step s
__device__ __forceinline__ void acc_operand(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& lo) {
  split8(a, b, hi, lo);
}

}  // namespace
