// Attention core of the SegFormer branch on the matrix cores (reference model/segformer.py:92-128, Attention.forward after the q / kv
// projections and the spatial reduction):   out = softmax(scale * q k^T) v   per (image, head), head dim D = 32 or 64 (every kernel is a template over D), at most 64 keys.
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
// dK / dV use the S orientation and accumulate over all queries of a workgroup in registers; per-workgroup partials are summed in a fixed
// order by attn_dkv_sum_kernel (deterministic, no atomics).
//   q [B,N,heads,D], kv [B,M,2,heads,D] (the kv Linear's output layout), out / dq like q, dkv like kv.
// LDS rows: a natural [64 keys][D d] bf16 image has rows of 2 D + 16 bytes (80 / 144), a transposed [D d][64 keys] image rows of 144 bytes.
// Both strides are 4 (mod 16) dwords -- 20 and 36 -- so the 16 rows of a 16-byte fragment read start at 16 distinct multiples of 4 dwords
// and cover the 64 banks once; the 8-byte reads of the transposed images (row stride 36 dwords, + 2 dwords per k-group) are conflict-free
// within each half wave if the hardware serves them half wave by half wave.  This is bank arithmetic, not a measurement: no LDS conflict
// counter was read for these kernels.  Not analysed at all: the 2-byte scalar stores that write a transposed image in stage_kv (stride
// TROW between a thread's 8 stores; one pass at D = 32, two at D = 64) -- staging runs once per workgroup.  The 16-byte pad stays at D = 64
// on that reasoning; what was measured is the kernels' time against equal-work D = 32 launches.
#include "common.h"

namespace {

typedef __bf16 a_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 a_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 a_bf16x2 __attribute__((ext_vector_type(2)));
typedef float a_f32x2 __attribute__((ext_vector_type(2)));

constexpr int MK = 64;                         // maximum keys
constexpr int TROW = 144;                      // bytes per row of a [D d][64 keys] bf16 image (128 B + 16 B pad)
constexpr int QROW = 80;                       // bytes per row of a per-wave [D d][32 q] bf16 image (64 B + 16 B pad)
template <int D> struct Geo {
  static_assert(D == 32 || D == 64, "head dim 32 or 64");
  static constexpr int KS = D / 32, DT = D / 16;          // MFMA k-steps over the head dim, 16-row d-tiles
  static constexpr int KROW = 2 * D + 16;                  // bytes per row of a [64 keys][D d] bf16 image (+ 16 B pad)
  static constexpr int KPLANE = MK * KROW, TPL = D * TROW, QPL = D * QROW;
};
constexpr float NEG = -3.0e38f;

__device__ __forceinline__ void split2(float x0, float x1, uint32_t& hw, uint32_t& lw) {
  const a_bf16x2 h = __builtin_convertvector(a_f32x2{x0, x1}, a_bf16x2);
  hw = __builtin_bit_cast(uint32_t, h);
  const a_f32x2 hf = {__builtin_bit_cast(float, hw << 16), __builtin_bit_cast(float, hw & 0xFFFF0000u)};
  lw = __builtin_bit_cast(uint32_t, __builtin_convertvector(a_f32x2{x0, x1} - hf, a_bf16x2));
}
__device__ __forceinline__ void split8v(const float (&v)[8], a_bf16x8& hi, a_bf16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) split2(v[2 * k], v[2 * k + 1], h[k], l[k]);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  hi = __builtin_bit_cast(a_bf16x8, (u32x4{h[0], h[1], h[2], h[3]}));
  lo = __builtin_bit_cast(a_bf16x8, (u32x4{l[0], l[1], l[2], l[3]}));
}

#define ATT_MFMA3(ACC, AH, AL, BH, BL)                                \
  ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, BH, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AL, BH, ACC, 0, 0, 0); \
  ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AH, BL, ACC, 0, 0, 0);

// rows [key][D d] of k or v (which = 0 / 1) of one (image, head) -> natural image [64][D] (hi, lo) and / or transposed image [D][64]
template <int D>
__device__ __forceinline__ void stage_kv(const float* __restrict__ kv, int b, int h, int M, int C, int which, unsigned char* nat, unsigned char* trn, int tid) {
  constexpr int KROW = Geo<D>::KROW, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
#pragma unroll
  for (int chunk = tid; chunk < MK * D / 8; chunk += 256) {      // 8 head-dim values per thread and pass: one pass at D = 32, two at 64
    const int key = chunk / (D / 8), d0 = (chunk % (D / 8)) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (key < M) {
      const float* p = kv + (((long)b * M + key) * 2 + which) * C + h * D + d0;
      const f32x4 a = *reinterpret_cast<const f32x4*>(p), c = *reinterpret_cast<const f32x4*>(p + 4);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = c[0]; v[5] = c[1]; v[6] = c[2]; v[7] = c[3];
    }
    a_bf16x8 hi, lo;
    split8v(v, hi, lo);
    if (nat) {
      *reinterpret_cast<a_bf16x8*>(nat + key * KROW + d0 * 2) = hi;
      *reinterpret_cast<a_bf16x8*>(nat + key * KROW + d0 * 2 + KPLANE) = lo;
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
__device__ __forceinline__ a_bf16x8 nat_frag(const unsigned char* plane, int row0, int ks, int lane) {
  return *reinterpret_cast<const a_bf16x8*>(plane + (row0 + (lane & 15)) * Geo<D>::KROW + ks * 64 + (lane >> 4) * 16);
}
// fragment of a transposed [D d][64 pos] image for contraction step s over 32 positions, in the accumulator-operand order: this lane's
// positions are 32 s + 4 g + {0..3} and 32 s + 16 + 4 g + {0..3} (g = lane >> 4), row = d0 + (lane & 15)
__device__ __forceinline__ a_bf16x8 trn_frag(const unsigned char* plane, int rowbytes, int d0, int s, int lane) {
  const unsigned char* p = plane + (d0 + (lane & 15)) * rowbytes + (32 * s + 4 * (lane >> 4)) * 2;
  const a_bf16x4 a = *reinterpret_cast<const a_bf16x4*>(p), b = *reinterpret_cast<const a_bf16x4*>(p + 32);
  return a_bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
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
                                               a_bf16x8 (&hi)[Geo<D>::KS], a_bf16x8 (&lo)[Geo<D>::KS]) {
#pragma unroll
  for (int ks = 0; ks < Geo<D>::KS; ++ks) {
    float v[8];
    load_row8<D>(base, row, nrows, C, h, ks, lane, mul, v);
    split8v(v, hi[ks], lo[ks]);
  }
}

// S^T tiles (keys on rows) of 16 queries -> probabilities p[t][r] of key 16 t + 4 g + r for the query on this lane (lane & 15)
template <int D>
__device__ __forceinline__ void softmax_t(const unsigned char* ldsK, const a_bf16x8 (&qh)[Geo<D>::KS], const a_bf16x8 (&ql)[Geo<D>::KS], int M, int lane,
                                          f32x4 (&p)[4]) {
  const int g = lane >> 4;
  float mx = NEG;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    p[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < Geo<D>::KS; ++ks) {
      const a_bf16x8 kh = nat_frag<D>(ldsK, 16 * t, ks, lane), kl = nat_frag<D>(ldsK + Geo<D>::KPLANE, 16 * t, ks, lane);
      ATT_MFMA3(p[t], kh, kl, qh[ks], ql[ks])
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (16 * t + 4 * g + r >= M) p[t][r] = NEG;
      mx = fmaxf(mx, p[t][r]);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[t][r] = 16 * t + 4 * g + r < M ? expf(p[t][r] - mx) : 0.f;
      den += p[t][r];
    }
  den += __shfl_xor(den, 16);
  den += __shfl_xor(den, 32);
  const float inv = 1.f / den;
#pragma unroll
  for (int t = 0; t < 4; ++t) p[t] *= inv;
}

// accumulator tiles (2 s, 2 s + 1) -> split-bf16 B operand of contraction step s
__device__ __forceinline__ void acc_operand(const f32x4& a, const f32x4& b, a_bf16x8& hi, a_bf16x8& lo) {
  const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  split8v(v, hi, lo);
}

template <int D>
__global__ __launch_bounds__(256) void attn_mfma_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out, int N, int M,
                                                            int heads, float scale) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KPLANE + 2 * TPL];      // K hi | K lo | V^T hi | V^T lo  (20 KB / 36 KB)
  unsigned char* ldsK = lds;
  unsigned char* ldsVT = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  stage_kv<D>(kv, b, h, M, C, 0, ldsK, nullptr, tid);
  stage_kv<D>(kv, b, h, M, C, 1, nullptr, ldsVT, tid);
  __syncthreads();
  const long qi = (long)blockIdx.x * 64 + wave * 16 + (lane & 15);
  a_bf16x8 qh[KS], ql[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  f32x4 p[4];
  softmax_t<D>(ldsK, qh, ql, M, lane, p);
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    a_bf16x8 ph, pl;
    acc_operand(p[2 * s], p[2 * s + 1], ph, pl);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const a_bf16x8 vh = trn_frag(ldsVT, TROW, 16 * dt, s, lane), vl = trn_frag(ldsVT + TPL, TROW, 16 * dt, s, lane);
      ATT_MFMA3(o[dt], vh, vl, ph, pl)          // O^T[d][q]
    }
  }
  if (qi < N) {
    float* op = out + ((long)b * N + qi) * C + h * D + (lane >> 4) * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt];
  }
}

// dq = scale * dS K with dS = P .* (dP - rowsum(P .* dP)), dP = dO V^T   (S^T orientation, one query per lane)
template <int D>
__global__ __launch_bounds__(256) void attn_mfma_dq_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ dout,
                                                           float* __restrict__ dq, int N, int M, int heads, float scale) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * TPL];      // K hi|lo, V hi|lo (natural), K^T hi|lo  (29 KB / 54 KB)
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  unsigned char* ldsKT = lds + 4 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  stage_kv<D>(kv, b, h, M, C, 0, ldsK, ldsKT, tid);
  stage_kv<D>(kv, b, h, M, C, 1, ldsV, nullptr, tid);
  __syncthreads();
  const long qi = (long)blockIdx.x * 64 + wave * 16 + (lane & 15);
  a_bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  load_row_frags<D>(dout + (long)b * N * C, qi, N, C, h, lane, 1.f, dh, dl);
  f32x4 p[4], dp[4];
  softmax_t<D>(ldsK, qh, ql, M, lane, p);
  float delta = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const a_bf16x8 vh = nat_frag<D>(ldsV, 16 * t, ks, lane), vl = nat_frag<D>(ldsV + KPLANE, 16 * t, ks, lane);
      ATT_MFMA3(dp[t], vh, vl, dh[ks], dl[ks])  // dP^T[key][q]
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) delta += p[t][r] * dp[t][r];
  }
  delta += __shfl_xor(delta, 16);
  delta += __shfl_xor(delta, 32);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dp[t][r] = p[t][r] * (dp[t][r] - delta);          // dS^T
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    a_bf16x8 sh, sl;
    acc_operand(dp[2 * s], dp[2 * s + 1], sh, sl);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const a_bf16x8 kh = trn_frag(ldsKT, TROW, 16 * dt, s, lane), kl = trn_frag(ldsKT + TPL, TROW, 16 * dt, s, lane);
      ATT_MFMA3(o[dt], kh, kl, sh, sl)          // dQ^T[d][q] / scale
    }
  }
  if (qi < N) {
    float* op = dq + ((long)b * N + qi) * C + h * D + g * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt] * scale;
  }
}

// dV = P^T dO, dK = scale * dS^T Q over the queries [q0, q1) of this workgroup (S orientation: 4 queries per lane, the key on the lane).
// Each wave takes 32 queries per step; the transposed images dO^T / Q^T [D d][32 q] of those queries live in a per-wave LDS slot.
// The K / V fragments with the key on the lane are constant over the loop: at D = 32 they stay in registers (64 VGPRs); at D = 64 they
// would take 128 next to 128 accumulator registers, so they are re-read from LDS at every step instead (HOLD = false).
template <int D>
__global__ __launch_bounds__(256) void attn_mfma_dkv_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ dout,
                                                            float* __restrict__ part, int N, int M, int heads, float scale, int q_per_block) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, QPL = Geo<D>::QPL;
  constexpr bool HOLD = D == 32;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 4 * 4 * QPL];      // K, V natural (hi|lo each); per wave: dO^T hi|lo, Q^T hi|lo
  static_assert(2 * MK * D * 4 <= 4 * KPLANE, "the wave reduction reuses the K / V images");
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  unsigned char* myDO = lds + 4 * KPLANE + wave * 4 * QPL;
  unsigned char* myQ = myDO + 2 * QPL;
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  stage_kv<D>(kv, b, h, M, C, 0, ldsK, nullptr, tid);
  stage_kv<D>(kv, b, h, M, C, 1, ldsV, nullptr, tid);
  __syncthreads();
  f32x4 accV[DT][4], accK[DT][4];               // dV^T / dK^T [d tile][key tile]: rows d, column = key on the lane
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      accV[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      accK[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  // K / V fragments with the key on the lane (column operand)
  a_bf16x8 kh[HOLD ? 4 : 1][KS], kl[HOLD ? 4 : 1][KS], vh[HOLD ? 4 : 1][KS], vl[HOLD ? 4 : 1][KS];
  if constexpr (HOLD) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        kh[t][ks] = nat_frag<D>(ldsK, 16 * t, ks, lane);
        kl[t][ks] = nat_frag<D>(ldsK + KPLANE, 16 * t, ks, lane);
        vh[t][ks] = nat_frag<D>(ldsV, 16 * t, ks, lane);
        vl[t][ks] = nat_frag<D>(ldsV + KPLANE, 16 * t, ks, lane);
      }
  }
  const long q0 = (long)blockIdx.x * q_per_block, q1 = q0 + q_per_block < N ? q0 + q_per_block : N;
  const float* qb = q + (long)b * N * C;
  const float* db = dout + (long)b * N * C;
  for (long base = q0 + wave * 32; base < q1; base += 128) {
    f32x4 s[2][4], dp[2][4];
    a_bf16x8 qh[2][KS], ql[2][KS], dh[2][KS], dl[2][KS];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long qi = base + 16 * u + (lane & 15);
      load_row_frags<D>(qb, qi, q1, C, h, lane, scale, qh[u], ql[u]);
      load_row_frags<D>(db, qi, q1, C, h, lane, 1.f, dh[u], dl[u]);
      // transposed per-wave images for the dV / dK products: element (d = 32 ks + 8 g + j, query position 16 u + (lane & 15))
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int off = (32 * ks + 8 * g + j) * QROW + (16 * u + (lane & 15)) * 2;
          *reinterpret_cast<__bf16*>(myDO + off) = dh[u][ks][j];
          *reinterpret_cast<__bf16*>(myDO + off + QPL) = dl[u][ks][j];
          *reinterpret_cast<__bf16*>(myQ + off) = qh[u][ks][j];
          *reinterpret_cast<__bf16*>(myQ + off + QPL) = ql[u][ks][j];
        }
    }
    // S[q][key] and dP[q][key]: queries 16 u + 4 g + r on the rows, key 16 t + (lane & 15) on the lane
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a_bf16x8 fkh[KS], fkl[KS], fvh[KS], fvl[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (HOLD) {
          fkh[ks] = kh[t][ks]; fkl[ks] = kl[t][ks]; fvh[ks] = vh[t][ks]; fvl[ks] = vl[t][ks];
        } else {
          fkh[ks] = nat_frag<D>(ldsK, 16 * t, ks, lane);
          fkl[ks] = nat_frag<D>(ldsK + KPLANE, 16 * t, ks, lane);
          fvh[ks] = nat_frag<D>(ldsV, 16 * t, ks, lane);
          fvl[ks] = nat_frag<D>(ldsV + KPLANE, 16 * t, ks, lane);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { ATT_MFMA3(s[u][t], qh[u][ks], ql[u][ks], fkh[ks], fkl[ks]) }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { ATT_MFMA3(dp[u][t], dh[u][ks], dl[u][ks], fvh[ks], fvl[ks]) }
      }
    }
    // softmax statistics per query row: 4 tiles x 16 lanes hold a row's 64 scores
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = NEG;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (16 * t + (lane & 15) >= M) s[u][t][r] = NEG;
          mx = fmaxf(mx, s[u][t][r]);
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          s[u][t][r] = 16 * t + (lane & 15) < M ? expf(s[u][t][r] - mx) : 0.f;
          den += s[u][t][r];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) den += __shfl_xor(den, o);
        const float inv = 1.f / den;
        float delta = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          s[u][t][r] *= inv;                                 // P
          delta += s[u][t][r] * dp[u][t][r];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) delta += __shfl_xor(delta, o);
        const bool live = base + 16 * u + 4 * g + r < q1;      // rows beyond the range contribute nothing (their q / dO were zeroed; P is not zero)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          dp[u][t][r] = live ? s[u][t][r] * (dp[u][t][r] - delta) : 0.f;      // dS
          if (!live) s[u][t][r] = 0.f;
        }
      }
    // dV^T[d][key] += dO^T[d][q] P[q][key],  dK^T[d][key] += Q^T[d][q] dS[q][key]   (one contraction step over the wave's 32 queries)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a_bf16x8 ph, pl, sh, sl;
      acc_operand(s[0][t], s[1][t], ph, pl);
      acc_operand(dp[0][t], dp[1][t], sh, sl);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const a_bf16x8 oh = trn_frag(myDO, QROW, 16 * dt, 0, lane), ol = trn_frag(myDO + QPL, QROW, 16 * dt, 0, lane);
        const a_bf16x8 th = trn_frag(myQ, QROW, 16 * dt, 0, lane), tl = trn_frag(myQ + QPL, QROW, 16 * dt, 0, lane);
        ATT_MFMA3(accV[dt][t], oh, ol, ph, pl)
        ATT_MFMA3(accK[dt][t], th, tl, sh, sl)
      }
    }
  }
  // reduce the four waves in a fixed order (wave 0 stores, waves 1..3 add in turn) and write this workgroup's partial [2][64 keys][D d];
  // accumulator rows = d (4 g + r), column = key.  The K / V images are dead by now.
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);                       // [2][64][D] floats = 16 KB / 32 KB
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = 16 * t + (lane & 15), d = 16 * dt + 4 * g + r;
            float* pk = red + (0 * MK + key) * D + d;
            float* pv = red + (1 * MK + key) * D + d;
            *pk = w == 0 ? accK[dt][t][r] : *pk + accK[dt][t][r];
            *pv = w == 0 ? accV[dt][t][r] : *pv + accV[dt][t][r];
          }
    }
    __syncthreads();
  }
  float* o = part + (((long)(b * heads + h) * gridDim.x + blockIdx.x) * 2) * MK * D;
  for (int e = tid; e < 2 * MK * D; e += 256) o[e] = red[e];
}

// dkv[b][key][which][h][d] = sum over the query blocks of part[b][h][blk][which][key][d]  (dK already carries the scale through the scaled q)
template <int D>
__global__ __launch_bounds__(256) void attn_dkv_sum_kernel(const float* __restrict__ part, float* __restrict__ dkv, int nblk, int M, int heads) {
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  for (int e = threadIdx.x; e < 2 * M * D; e += 256) {
    const int which = e / (M * D), key = (e / D) % M, d = e % D;
    const float* p = part + (((long)(b * heads + h) * nblk) * 2 + which) * MK * D + key * D + d;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += p[(long)k * 2 * MK * D];
    dkv[(((long)b * M + key) * 2 + which) * C + h * D + d] = s;
  }
}

constexpr int Q_PER_BLOCK = 512;                 // queries per dK / dV workgroup (a multiple of 128: four waves x 32)

template <int D>
int launch_fwd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, float scale, hipStream_t st) {
  hipLaunchKernelGGL(attn_mfma_fwd_kernel<D>, dim3((N + 63) / 64, heads, B), dim3(256), 0, st, q, kv, out, N, M, heads, scale);
  return hpfg_launch_status("attn_mfma_fwd_kernel");
}

template <int D>
int launch_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, float* scratch, int B, int N, int M, int heads, float scale,
               hipStream_t st) {
  hipLaunchKernelGGL(attn_mfma_dq_kernel<D>, dim3((N + 63) / 64, heads, B), dim3(256), 0, st, q, kv, dout, dq, N, M, heads, scale);
  const int nblk = hpfg_attn_mfma_blocks(N);
  hipLaunchKernelGGL(attn_mfma_dkv_kernel<D>, dim3(nblk, heads, B), dim3(256), 0, st, q, kv, dout, scratch, N, M, heads, scale, Q_PER_BLOCK);
  hipLaunchKernelGGL(attn_dkv_sum_kernel<D>, dim3(1, heads, B), dim3(256), 0, st, scratch, dkv, nblk, M, heads);
  return hpfg_launch_status("attn_mfma_bwd");
}

}  // namespace

extern "C" int hpfg_attn_mfma_blocks(int N) { return (N + Q_PER_BLOCK - 1) / Q_PER_BLOCK; }

extern "C" long hpfg_attn_mfma_scratch_floats(int B, int N, int heads, int head_dim) {
  if (B <= 0 || N <= 0 || heads <= 0 || (head_dim != 32 && head_dim != 64)) return -1;
  return (long)B * heads * hpfg_attn_mfma_blocks(N) * 2 * MK * head_dim;
}

extern "C" int hpfg_attn_mfma_fwd_hd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, int head_dim, float scale, void* stream) {
  HPFG_ARG_CHECK(q && kv && out && B > 0 && N > 0 && M > 0 && M <= MK && heads > 0 && (head_dim == 32 || head_dim == 64),
                 "attn_mfma_fwd: bad args (at most %d keys, head dim 32 or 64, got %d keys, head dim %d)", MK, M, head_dim);
  return head_dim == 32 ? launch_fwd<32>(q, kv, out, B, N, M, heads, scale, (hipStream_t)stream)
                        : launch_fwd<64>(q, kv, out, B, N, M, heads, scale, (hipStream_t)stream);
}

/* dq [B,N,heads,D], dkv [B,M,2,heads,D]; scratch: hpfg_attn_mfma_scratch_floats(B, N, heads, head_dim) floats */
extern "C" int hpfg_attn_mfma_bwd_hd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, float* scratch, int B, int N, int M, int heads,
                                     int head_dim, float scale, void* stream) {
  HPFG_ARG_CHECK(q && kv && dout && dq && dkv && scratch && B > 0 && N > 0 && M > 0 && M <= MK && heads > 0 && (head_dim == 32 || head_dim == 64),
                 "attn_mfma_bwd: bad args (at most %d keys, head dim 32 or 64, got %d keys, head dim %d)", MK, M, head_dim);
  return head_dim == 32 ? launch_bwd<32>(q, kv, dout, dq, dkv, scratch, B, N, M, heads, scale, (hipStream_t)stream)
                        : launch_bwd<64>(q, kv, dout, dq, dkv, scratch, B, N, M, heads, scale, (hipStream_t)stream);
}

/* head dim 32: the entry points older callers bind */
extern "C" int hpfg_attn_mfma_fwd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, float scale, void* stream) {
  return hpfg_attn_mfma_fwd_hd(q, kv, out, B, N, M, heads, 32, scale, stream);
}

extern "C" int hpfg_attn_mfma_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, float* scratch, int B, int N, int M, int heads,
                                  float scale, void* stream) {
  return hpfg_attn_mfma_bwd_hd(q, kv, dout, dq, dkv, scratch, B, N, M, heads, 32, scale, stream);
}
