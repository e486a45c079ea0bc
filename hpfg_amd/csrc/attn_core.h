// The phases of the forward and dQ attention kernels on the matrix cores, written once: csrc/attn.hip (at most 64 keys), csrc/attn_keys.hip
// (up to 256 keys in blocks of 64) and csrc/attn_window.hip (shifted windows with bias and mask) are their own addressing and key walk around
// them.  The three families must give the same bits where their operations coincide, so a phase is edited here or nowhere.
// NOT here: the dK / dV kernels of the three files and attn_keys_dq_kernel, which are still three / two edited copies of one text.  Built
// from shared phases they gave the same bits from the same instruction counts but another schedule, and ran slower (the <= 64-key dK / dV
// kernel 5 to 10 % at head dim 64, the 65 .. 256-key backward 0.2 to 1.3 %: appendix (A) of profiles/attn_core_timing.txt), so they keep the parent's text;
// staging is two copies as well (stage_kv of attn_frag.h, stage_win of attn_window.hip): with one function and the row's pointer as a
// functor, kernels that were otherwise the parent's text still measured 0.2 to 2.4 % slower (appendix (B) there).  tests/test_gpu_attn_bits.py fails if the
// copies drift apart in a bit that the cases reach.
//
// Every product is split-bf16 ("bf16x3": hi*hi + hi*lo + lo*hi, fp32 accumulate) on v_mfma_f32_16x16x32_bf16, like the convolutions.
// Head dim 32 is exactly one MFMA k-step, so a 16 x 16 score tile costs three MFMAs; head dim 64 (MiT-B1 and wider) is two k-steps, six
// MFMAs, and P V / dS K / dV / dK produce four 16-row d-tiles instead of two.  Two facts keep the kernels free of LDS transposes of the
// probabilities:
//   * Q, K, V and dO fragments all have the same lane layout (row or column = lane & 15, 8 consecutive head-dim elements of k-group
//     lane >> 4), so the SAME registers give S^T = K Q^T (keys on the accumulator rows, the query on the lane) or S = Q K^T (queries on
//     the rows, the key on the lane) just by swapping the MFMA arguments.
//   * An accumulator tile feeds the next MFMA as its B operand directly (MI355X guide, "accumulator tile as the next MFMA's operand"):
//     the 8 contraction positions of a lane are its 4 accumulator rows of tile 2s and its 4 rows of tile 2s + 1; the OTHER operand (V^T,
//     K^T, dO^T, Q^T from LDS) is gathered in that same permuted order, which costs two 8-byte LDS reads instead of one 16-byte read.
// Forward and dQ use the S^T orientation (softmax statistics are then a 16-value reduction in registers plus two cross-lane steps);
// dK / dV use the S orientation and accumulate over the queries of a workgroup in registers, 32 queries per wave and step, and the waves
// are added in a fixed order through LDS (deterministic, no atomics).
// LDS rows: a natural [64 keys][D d] bf16 image has rows of 2 D + 16 bytes (80 / 144), a transposed [D d][64 keys] image rows of 144 bytes.
// Both strides are 4 (mod 16) dwords -- 20 and 36 -- so the 16 rows of a 16-byte fragment read start at 16 distinct multiples of 4 dwords
// and cover the 64 banks once; the 8-byte reads of the transposed images (row stride 36 dwords, + 2 dwords per k-group) are conflict-free
// within each half wave if the hardware serves them half wave by half wave.  This is bank arithmetic, not a measurement: no LDS conflict
// counter was read for these kernels.  Not analysed at all: the 2-byte scalar stores that write a transposed image in stage_kv (stride
// TROW between a thread's 8 stores; one pass at D = 32, two at D = 64) -- staging runs once per workgroup.  The 16-byte pad stays at D = 64
// on that reasoning; what was measured is the kernels' time against equal-work D = 32 launches.
//
// What varies between the families goes in by value: the logit term of the lane's query, (score, key position) -> logit: NoTerm, or the
// window's bias + mask.  Keys beyond the key count are excluded here, in one place: NEG before the maximum, an exact 0 after the expf.
//
// Bits: the files are built with fp contraction on, so whether an `x += a * b` (ds_t's `delta`, the sums inside expf) becomes one fma is
// the compiler's choice, and the result's last bit depends on it.  None of them is spelled out as fmaf: they compile as they did in the
// text this header replaced, and only tests/test_gpu_attn_bits.py (SHA-256 of every result against tests/golden/attn_bits.json) says so.
// Run it after any edit to this header, a compiler change included.  (The dK / dV row statistics did change when they were moved into a
// function here -- their `delta` sum came out unfused -- one more reason why those kernels were left as they are.)
#pragma once
#include "attn_frag.h"

namespace {

constexpr int Q_PER_BLOCK = 512;                 // queries per dK / dV workgroup of attn.hip / attn_keys.hip (a multiple of 128: four waves x 32)

struct NoTerm {
  __device__ __forceinline__ float operator()(float sc, int) const { return sc; }
};

template <int N>
__device__ __forceinline__ void zero_tiles(f32x4 (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- S^T orientation (forward, dQ): keys on the accumulator rows, one query per lane (lane & 15) -----------------------------------------
// tile t of a natural image times the row whose fragments this lane holds: S^T = K q (bh / bl = the scaled query) or dP^T = V dO
template <int D>
__device__ __forceinline__ void tile_t(const unsigned char* img, int t, const bf16x8 (&bh)[Geo<D>::KS], const bf16x8 (&bl)[Geo<D>::KS], int lane,
                                       f32x4& acc) {
  acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < Geo<D>::KS; ++ks) {
    const bf16x8 ah = nat_frag<D>(img, 16 * t, ks, lane), al = nat_frag<D>(img + Geo<D>::KPLANE, 16 * t, ks, lane);
    { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, acc, ah, al, bh[ks], bl[ks]) }
  }
}

// the four score tiles p[0..3] of one K image (keys key0 ..): p[t][r] = logit of key key0 + 16 t + 4 g + r for the query on this lane; mx = running maximum
template <int D, class Term>
__device__ __forceinline__ void scores_t(const unsigned char* ldsK, const bf16x8 (&qh)[Geo<D>::KS], const bf16x8 (&ql)[Geo<D>::KS], int key0, int M,
                                         int lane, Term term, f32x4* p, float& mx) {
  const int g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f32x4& s = p[t];
    tile_t<D>(ldsK, t, qh, ql, lane, s);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = key0 + 16 * t + 4 * g + r;
      s[r] = key < M ? term(s[r], key) : NEG;
      mx = fmaxf(mx, s[r]);
    }
  }
}

// logits of T tiles -> probabilities: the exact two-pass softmax (max, exp, sum, one reciprocal); leaves the row maximum and sum in mx / den
template <int T>
__device__ __forceinline__ void softmax_finish_t(f32x4* p, int M, int lane, float& mx, float& den) {
  const int g = lane >> 4;
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  den = 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = 16 * t + 4 * g + r < M ? expf(p[t][r] - mx) : 0.f;
      den += p[t][r];
    }
  den += __shfl_xor(den, 16);
  den += __shfl_xor(den, 32);
  const float inv = 1.f / den;
#pragma unroll
  for (int t = 0; t < T; ++t) p[t] *= inv;
}

// one image of at most 64 keys: probabilities p[t][r] of key 16 t + 4 g + r for the query on this lane
template <int D, class Term>
__device__ __forceinline__ void softmax_t(const unsigned char* ldsK, const bf16x8 (&qh)[Geo<D>::KS], const bf16x8 (&ql)[Geo<D>::KS], int M,
                                          int lane, Term term, f32x4 (&p)[4]) {
  float mx = NEG, den;
  scores_t<D>(ldsK, qh, ql, 0, M, lane, term, p, mx);
  softmax_finish_t<4>(p, M, lane, mx, den);
}

// dp = dS^T = P .* (dP^T - rowsum(P .* dP)) with dP^T = V dO
template <int D>
__device__ __forceinline__ void ds_t(const unsigned char* ldsV, const bf16x8 (&dh)[Geo<D>::KS], const bf16x8 (&dl)[Geo<D>::KS], int lane,
                                     const f32x4 (&p)[4], f32x4 (&dp)[4]) {
  float delta = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tile_t<D>(ldsV, t, dh, dl, lane, dp[t]);
#pragma unroll
    for (int r = 0; r < 4; ++r) delta += p[t][r] * dp[t][r];
  }
  delta += __shfl_xor(delta, 16);
  delta += __shfl_xor(delta, 32);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dp[t][r] = p[t][r] * (dp[t][r] - delta);
}

// o[dt] += (transposed image [D][64 keys]) x (the four accumulator tiles a[0..3] of those keys): O^T = V^T P or dQ^T / scale = K^T dS^T
template <int D>
__device__ __forceinline__ void mul_trn(const f32x4* a, const unsigned char* trn, int lane, f32x4 (&o)[Geo<D>::DT]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 ah, al;
    acc_operand(a[2 * s], a[2 * s + 1], ah, al);
#pragma unroll
    for (int dt = 0; dt < Geo<D>::DT; ++dt) {
      const bf16x8 fh = trn_frag(trn, TROW, 16 * dt, s, lane), fl = trn_frag(trn + Geo<D>::TPL, TROW, 16 * dt, s, lane);
      { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, o[dt], fh, fl, ah, al) }
    }
  }
}

// this lane's part of its query's row: op = the row's head + 4 (lane >> 4)
template <int D>
__device__ __forceinline__ void store_o(float* op, const f32x4 (&o)[Geo<D>::DT]) {
#pragma unroll
  for (int dt = 0; dt < Geo<D>::DT; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt];
}
template <int D>
__device__ __forceinline__ void store_o(float* op, const f32x4 (&o)[Geo<D>::DT], float mul) {
#pragma unroll
  for (int dt = 0; dt < Geo<D>::DT; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt] * mul;
}

}  // namespace
