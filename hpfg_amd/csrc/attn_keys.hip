// Attention core over 1 .. 256 keys (reference model/segformer.py:92-128, Attention.forward after the q / kv projections and the spatial
// reduction):   out = softmax(scale * q k^T) v   per (image, head), head dim D = 32 or 64.  A MiT stage has (H / 32) (W / 32) keys, so the
// one-image kernels of attn.hip (at most 64 keys) stop at 256 x 256 inputs; these serve up to 512 x 512.
//
// The arithmetic, lane layouts, LDS images and phases are those of attn_core.h.  This file's own is the walk over the keys in blocks of 64,
// one LDS image at a time:
//   * forward: all NB = ceil(M / 64) <= 4 blocks' score tiles of a query stay in registers (16 NB values per lane), so the softmax is the
//     exact two-pass one (max, exp, sum, one reciprocal) -- no online rescaling; then P V accumulates block by block in key order.  Masked
//     positions are exact zeros, so for M <= 64 (NB = 1) the operation sequence, hence every bit of `out`, is that of attn_mfma_fwd_kernel.
//     It also writes the row log-sum-exp lse = max + log(sum) for the backward.
//   * backward: P = exp(S - lse) per block (no second softmax), delta = rowsum(dO . O) from the saved output (the dQ kernel computes it in
//     its prologue and leaves it in the scratch for the dK / dV kernel), dS = P . (dP - delta).  dQ accumulates over the blocks in key order
//     in registers; dK / dV run one workgroup per (query block, key block) like attn_mfma_dkv_kernel and their partials are summed in a
//     fixed order by attn_keys_dkv_sum_kernel.  No atomics anywhere: results are bit-identical from run to run.
// LDS: the images of attn.hip, one key block at a time -- forward 20 / 36 KB, dQ 29 / 54 KB, dK / dV 60 / 116 KB at D = 32 / 64.
// HPFG_MATH=f32: thread-per-query fp32 kernels over the same key blocks (scores are recomputed in a second pass instead of being kept:
// 256 of them would not fit a thread's registers); dK / dV through hpfg_gemm_f32 like the <= 64-key path.
#include "attn_core.h"

namespace {

constexpr int KEYS_MAX = 256;

// NB x 64 keys; lse may be null (inference)
template <int D, int NB>
__global__ __launch_bounds__(256) void attn_keys_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out,
                                                            float* __restrict__ lse, int N, int M, int heads, float scale) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KPLANE + 2 * TPL];      // K hi | K lo | V^T hi | V^T lo of ONE key block
  unsigned char* ldsK = lds;
  unsigned char* ldsVT = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  const long qi = (long)blockIdx.x * 64 + wave * 16 + (lane & 15);
  bf16x8 qh[KS], ql[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  // S^T tiles of every key block: p[4 kb + t][r] = score of key 64 kb + 16 t + 4 g + r for the query on this lane
  f32x4 p[4 * NB], o[DT];
  float mx = NEG, den;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (kb) __syncthreads();                    // every wave is done with the previous K image
    stage_kv<D>(kv, b, h, M, C, 0, ldsK, nullptr, tid, 64 * kb);
    if (kb == 0) stage_kv<D>(kv, b, h, M, C, 1, nullptr, ldsVT, tid, 0);
    __syncthreads();
    scores_t<D>(ldsK, qh, ql, 64 * kb, M, lane, NoTerm{}, p + 4 * kb, mx);
  }
  softmax_finish_t<4 * NB>(p, M, lane, mx, den);
  zero_tiles(o);
  // block 0, whose V^T image was staged beside its K image, then blocks 1 .. NB - 1.  Not one loop over all blocks with `if (kb)` around
  // the restaging: built on the shared phases that form cost <32, 1> a wave per SIMD (profiles/attn_core_resources.txt)
  mul_trn<D>(p, ldsVT, lane, o);                 // O^T[d][q]
#pragma unroll
  for (int kb = 1; kb < NB; ++kb) {
    __syncthreads();                            // every wave is done with the previous V^T image
    stage_kv<D>(kv, b, h, M, C, 1, nullptr, ldsVT, tid, 64 * kb);
    __syncthreads();
    mul_trn<D>(p + 4 * kb, ldsVT, lane, o);
  }
  if (qi < N) {
    store_o<D>(out + ((long)b * N + qi) * C + h * D + g * 4, o);
    if (lse && g == 0) lse[((long)b * heads + h) * N + qi] = mx + logf(den);
  }
}

// dq = scale * dS K with dS = P .* (dP - delta), P = exp(S - lse), dP = dO V^T, delta = rowsum(dO .* O)   (S^T orientation, one query per
// lane).  Also leaves delta [B,heads,N] for the dK / dV kernel.
template <int D>
__global__ __launch_bounds__(256) void attn_keys_dq_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ out,
                                                           const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dq,
                                                           float* __restrict__ delta_out, int N, int M, int heads, float scale) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * TPL];      // K hi|lo, V hi|lo (natural), K^T hi|lo of ONE key block
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  unsigned char* ldsKT = lds + 4 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, C = heads * D;
  const long qi = (long)blockIdx.x * 64 + wave * 16 + (lane & 15);
  bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  load_row_frags<D>(dout + (long)b * N * C, qi, N, C, h, lane, 1.f, dh, dl);
  float delta = 0.f;                             // fp32 on the unsplit values: this lane's 8 KS head-dim positions, then the four k-groups
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float a[8], c[8];
    load_row8<D>(dout + (long)b * N * C, qi, N, C, h, ks, lane, 1.f, a);
    load_row8<D>(out + (long)b * N * C, qi, N, C, h, ks, lane, 1.f, c);
#pragma unroll
    for (int j = 0; j < 8; ++j) delta += a[j] * c[j];
  }
  delta += __shfl_xor(delta, 16);
  delta += __shfl_xor(delta, 32);
  const long row = ((long)b * heads + h) * N + qi;
  const float l = qi < N ? lse[row] : 0.f;
  if (qi < N && g == 0) delta_out[row] = delta;
  f32x4 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nb = (M + MK - 1) / MK;
  for (int kb = 0; kb < nb; ++kb) {
    if (kb) __syncthreads();                    // every wave is done with the previous block's images
    stage_kv<D>(kv, b, h, M, C, 0, ldsK, ldsKT, tid, 64 * kb);
    stage_kv<D>(kv, b, h, M, C, 1, ldsV, nullptr, tid, 64 * kb);
    __syncthreads();
    f32x4 ds[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 kh = nat_frag<D>(ldsK, 16 * t, ks, lane), kl = nat_frag<D>(ldsK + KPLANE, 16 * t, ks, lane);
        { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, s, kh, kl, qh[ks], ql[ks]) }     // S^T[key][q]
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 vh = nat_frag<D>(ldsV, 16 * t, ks, lane), vl = nat_frag<D>(ldsV + KPLANE, 16 * t, ks, lane);
        { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, dp, vh, vl, dh[ks], dl[ks]) }    // dP^T[key][q]
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = 64 * kb + 16 * t + 4 * g + r < M ? expf(s[r] - l) : 0.f;
        ds[t][r] = pr * (dp[r] - delta);          // dS^T
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 sh, sl;
      acc_operand(ds[2 * s], ds[2 * s + 1], sh, sl);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 kh = trn_frag(ldsKT, TROW, 16 * dt, s, lane), kl = trn_frag(ldsKT + TPL, TROW, 16 * dt, s, lane);
        { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, o[dt], kh, kl, sh, sl) }          // dQ^T[d][q] / scale
      }
    }
  }
  if (qi < N) {
    float* op = dq + ((long)b * N + qi) * C + h * D + g * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(op + 16 * dt) = o[dt] * scale;
  }
}

// dV = P^T dO, dK = scale * dS^T Q of key block blockIdx.y % nb over the queries [q0, q1) of this workgroup (S orientation: 4 queries per
// lane, the key on the lane), as attn_mfma_dkv_kernel with P = exp(S - lse) and the delta the dQ kernel left.  The K / V fragments are
// re-read from LDS at every step at both head dims (the lse / delta loads take the registers the D = 32 hold of attn.hip used).
template <int D>
__global__ __launch_bounds__(256) void attn_keys_dkv_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ lse,
                                                            const float* __restrict__ delta, const float* __restrict__ dout, float* __restrict__ part,
                                                            int N, int M, int heads, int nb, float scale, int q_per_block) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, QPL = Geo<D>::QPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 4 * 4 * QPL];      // K, V natural (hi|lo each); per wave: dO^T hi|lo, Q^T hi|lo
  static_assert(2 * MK * D * 4 <= 4 * KPLANE, "the wave reduction reuses the K / V images");
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  unsigned char* myDO = lds + 4 * KPLANE + wave * 4 * QPL;
  unsigned char* myQ = myDO + 2 * QPL;
  const int b = blockIdx.z, h = blockIdx.y / nb, kb = blockIdx.y % nb, C = heads * D;
  stage_kv<D>(kv, b, h, M, C, 0, ldsK, nullptr, tid, 64 * kb);
  stage_kv<D>(kv, b, h, M, C, 1, ldsV, nullptr, tid, 64 * kb);
  __syncthreads();
  f32x4 accV[DT][4], accK[DT][4];               // dV^T / dK^T [d tile][key tile]: rows d, column = key on the lane
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      accV[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      accK[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const long q0 = (long)blockIdx.x * q_per_block, q1 = q0 + q_per_block < N ? q0 + q_per_block : N;
  const float* qb = q + (long)b * N * C;
  const float* db = dout + (long)b * N * C;
  const float* lb = lse + ((long)b * heads + h) * N;
  const float* eb = delta + ((long)b * heads + h) * N;
  for (long base = q0 + wave * 32; base < q1; base += 128) {
    f32x4 s[2][4], dp[2][4];
    bf16x8 qh[2][KS], ql[2][KS], dh[2][KS], dl[2][KS];
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
    // S[q][key] and dP[q][key]: queries 16 u + 4 g + r on the rows, key 64 kb + 16 t + (lane & 15) on the lane
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8 fkh[KS], fkl[KS], fvh[KS], fvl[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        fkh[ks] = nat_frag<D>(ldsK, 16 * t, ks, lane);
        fkl[ks] = nat_frag<D>(ldsK + KPLANE, 16 * t, ks, lane);
        fvh[ks] = nat_frag<D>(ldsV, 16 * t, ks, lane);
        fvl[ks] = nat_frag<D>(ldsV + KPLANE, 16 * t, ks, lane);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, s[u][t], qh[u][ks], ql[u][ks], fkh[ks], fkl[ks]) }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, dp[u][t], dh[u][ks], dl[u][ks], fvh[ks], fvl[ks]) }
      }
    }
    // P = exp(S - lse), dS = P (dP - delta); rows beyond the range and keys beyond M contribute exact zeros
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long qrow = base + 16 * u + 4 * g + r;
        const bool live = qrow < q1;
        const float l = live ? lb[qrow] : 0.f, dlt = live ? eb[qrow] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float pr = live && 64 * kb + 16 * t + (lane & 15) < M ? expf(s[u][t][r] - l) : 0.f;
          dp[u][t][r] = pr * (dp[u][t][r] - dlt);      // dS
          s[u][t][r] = pr;                              // P
        }
      }
    // dV^T[d][key] += dO^T[d][q] P[q][key],  dK^T[d][key] += Q^T[d][q] dS[q][key]   (one contraction step over the wave's 32 queries)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8 ph, pl, sh, sl;
      acc_operand(s[0][t], s[1][t], ph, pl);
      acc_operand(dp[0][t], dp[1][t], sh, sl);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 oh = trn_frag(myDO, QROW, 16 * dt, 0, lane), ol = trn_frag(myDO + QPL, QROW, 16 * dt, 0, lane);
        const bf16x8 th = trn_frag(myQ, QROW, 16 * dt, 0, lane), tl = trn_frag(myQ + QPL, QROW, 16 * dt, 0, lane);
        { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, accV[dt][t], oh, ol, ph, pl) }
        { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, accK[dt][t], th, tl, sh, sl) }
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
  float* o = part + ((((long)(b * heads + h) * nb + kb) * gridDim.x + blockIdx.x) * 2) * MK * D;
  for (int e = tid; e < 2 * MK * D; e += 256) o[e] = red[e];
}

// dkv[b][64 kb + key][which][h][d] = sum over the query blocks of part[b][h][kb][blk][which][key][d]   (grid: key block, head, image)
template <int D>
__global__ __launch_bounds__(256) void attn_keys_dkv_sum_kernel(const float* __restrict__ part, float* __restrict__ dkv, int nblk, int M, int heads) {
  const int kb = blockIdx.x, nb = gridDim.x, b = blockIdx.z, h = blockIdx.y, C = heads * D;
  const float* base = part + (((long)(b * heads + h) * nb + kb) * nblk) * 2 * MK * D;
  for (int e = threadIdx.x; e < 2 * MK * D; e += 256) {
    const int which = e / (MK * D), key = (e / D) % MK, d = e % D;
    if (64 * kb + key >= M) continue;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += base[(long)k * 2 * MK * D + e];
    dkv[(((long)b * M + 64 * kb + key) * 2 + which) * C + h * D + d] = s;
  }
}

// ---- exact fp32 (HPFG_MATH=f32): thread per query, one 64-key block of K / V in LDS at a time ------------------------------------------------
template <int AD>
__device__ __forceinline__ void stage_kv_f32(const float* __restrict__ kv, int b, int h, int M, int C, int key0, float (*ks)[AD], float (*vs)[AD]) {
  const int n = (M - key0 < MK ? M - key0 : MK) * AD;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int j = e / AD, c = e % AD;
    ks[j][c] = kv[(((long)b * M + key0 + j) * 2 + 0) * C + h * AD + c];
    vs[j][c] = kv[(((long)b * M + key0 + j) * 2 + 1) * C + h * AD + c];
  }
}

template <int AD>
__global__ __launch_bounds__(256) void attn_keys_f32_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out,
                                                                float* __restrict__ lse, int N, int M, int heads, float scale) {
  __shared__ float ks[MK][AD], vs[MK][AD];
  const int b = blockIdx.z, h = blockIdx.y, C = heads * AD;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N;                       // (no early return: every thread stages and meets the barriers)
  float qv[AD];
#pragma unroll
  for (int c = 0; c < AD; ++c) qv[c] = 0.f;
  if (live) {
    const float* qp = q + ((long)b * N + i) * C + h * AD;
#pragma unroll
    for (int c = 0; c < AD; c += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + c);
      qv[c] = t[0]; qv[c + 1] = t[1]; qv[c + 2] = t[2]; qv[c + 3] = t[3];
    }
  }
  float mx = NEG;
  for (int key0 = 0; key0 < M; key0 += MK) {    // pass 1: the row maximum
    __syncthreads();
    stage_kv_f32<AD>(kv, b, h, M, C, key0, ks, vs);
    __syncthreads();
    const int jn = M - key0 < MK ? M - key0 : MK;
    for (int j = 0; j < jn; ++j) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < AD; ++c) d += qv[c] * ks[j][c];
      mx = fmaxf(mx, d * scale);
    }
  }
  float den = 0.f, o[AD];
#pragma unroll
  for (int c = 0; c < AD; ++c) o[c] = 0.f;
  for (int key0 = 0; key0 < M; key0 += MK) {    // pass 2: the same scores again -> exp, sum, unnormalised P V
    __syncthreads();
    stage_kv_f32<AD>(kv, b, h, M, C, key0, ks, vs);
    __syncthreads();
    const int jn = M - key0 < MK ? M - key0 : MK;
    for (int j = 0; j < jn; ++j) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < AD; ++c) d += qv[c] * ks[j][c];
      const float e = expf(d * scale - mx);
      den += e;
#pragma unroll
      for (int c = 0; c < AD; ++c) o[c] += e * vs[j][c];
    }
  }
  if (!live) return;
  const float inv = 1.f / den;
  float* op = out + ((long)b * N + i) * C + h * AD;
#pragma unroll
  for (int c = 0; c < AD; c += 4) *reinterpret_cast<f32x4*>(op + c) = f32x4{o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv};
  if (lse) lse[((long)b * heads + h) * N + i] = mx + logf(den);
}

// backward per query: dq, and the two [B,h,N,M] matrices P and scale * dS from which dV = P^T dO and dK = (scale dS)^T Q follow (GEMMs)
template <int AD>
__global__ __launch_bounds__(256) void attn_keys_f32_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ out,
                                                                const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dq,
                                                                float* __restrict__ P, float* __restrict__ dS, int N, int M, int heads, float scale) {
  __shared__ float ks[MK][AD], vs[MK][AD];
  const int b = blockIdx.z, h = blockIdx.y, C = heads * AD;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < N;
  float qv[AD], dov[AD], dqv[AD], delta = 0.f, l = 0.f;
#pragma unroll
  for (int c = 0; c < AD; ++c) qv[c] = dov[c] = dqv[c] = 0.f;
  if (live) {
    const long off = ((long)b * N + i) * C + h * AD;
#pragma unroll
    for (int c = 0; c < AD; c += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(q + off + c), u = *reinterpret_cast<const f32x4*>(dout + off + c),
                  w = *reinterpret_cast<const f32x4*>(out + off + c);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        qv[c + k] = t[k];
        dov[c + k] = u[k];
        delta += u[k] * w[k];
      }
    }
    l = lse[((long)b * heads + h) * N + i];
  }
  const long prow = live ? (((long)b * heads + h) * N + i) * M : 0;
  for (int key0 = 0; key0 < M; key0 += MK) {
    __syncthreads();
    stage_kv_f32<AD>(kv, b, h, M, C, key0, ks, vs);
    __syncthreads();
    const int jn = live ? (M - key0 < MK ? M - key0 : MK) : 0;
    for (int j = 0; j < jn; ++j) {
      float d = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < AD; ++c) {
        d += qv[c] * ks[j][c];
        dp += dov[c] * vs[j][c];
      }
      const float pr = expf(d * scale - l), ds = pr * (dp - delta);
      P[prow + key0 + j] = pr;
      dS[prow + key0 + j] = ds * scale;
#pragma unroll
      for (int c = 0; c < AD; ++c) dqv[c] += ds * ks[j][c];
    }
  }
  if (!live) return;
  float* qo = dq + ((long)b * N + i) * C + h * AD;
#pragma unroll
  for (int c = 0; c < AD; c += 4) *reinterpret_cast<f32x4*>(qo + c) = f32x4{dqv[c] * scale, dqv[c + 1] * scale, dqv[c + 2] * scale, dqv[c + 3] * scale};
}

int blocks_of(int N) { return (N + Q_PER_BLOCK - 1) / Q_PER_BLOCK; }
long delta_floats(int B, int N, int heads) { return ((long)B * heads * N + 3) / 4 * 4; }      // the partials after it stay 16-byte aligned

template <int D>
int launch_fwd(const float* q, const float* kv, float* out, float* lse, int B, int N, int M, int heads, float scale, hipStream_t st) {
  const dim3 grid((N + 63) / 64, heads, B);
  switch ((M + MK - 1) / MK) {
    case 1: hipLaunchKernelGGL((attn_keys_fwd_kernel<D, 1>), grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale); break;
    case 2: hipLaunchKernelGGL((attn_keys_fwd_kernel<D, 2>), grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale); break;
    case 3: hipLaunchKernelGGL((attn_keys_fwd_kernel<D, 3>), grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale); break;
    default: hipLaunchKernelGGL((attn_keys_fwd_kernel<D, 4>), grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale); break;
  }
  return hpfg_launch_status("attn_keys_fwd_kernel");
}

template <int D>
int launch_bwd(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv, float* scratch, int B, int N,
               int M, int heads, float scale, hipStream_t st) {
  float* delta = scratch;
  float* part = scratch + delta_floats(B, N, heads);
  const int nb = (M + MK - 1) / MK, nblk = blocks_of(N);
  hipLaunchKernelGGL(attn_keys_dq_kernel<D>, dim3((N + 63) / 64, heads, B), dim3(256), 0, st, q, kv, out, lse, dout, dq, delta, N, M, heads, scale);
  hipLaunchKernelGGL(attn_keys_dkv_kernel<D>, dim3(nblk, heads * nb, B), dim3(256), 0, st, q, kv, lse, delta, dout, part, N, M, heads, nb, scale,
                     Q_PER_BLOCK);
  hipLaunchKernelGGL(attn_keys_dkv_sum_kernel<D>, dim3(nb, heads, B), dim3(256), 0, st, part, dkv, nblk, M, heads);
  return hpfg_launch_status("attn_keys_bwd");
}

template <int D>
int launch_bwd_f32(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv, float* scratch, int B,
                   int N, int M, int heads, float scale, void* stream) {
  const long C = (long)heads * D;
  float* P = scratch;
  float* dS = scratch + (long)B * heads * N * M;
  hipLaunchKernelGGL(attn_keys_f32_bwd_kernel<D>, dim3((N + 255) / 256, heads, B), dim3(256), 0, (hipStream_t)stream, q, kv, out, lse, dout, dq, P, dS, N, M,
                     heads, scale);
  if (int rc = hpfg_launch_status("attn_keys_f32_bwd_kernel")) return rc;
  // dV = P^T dO, dK = (scale dS)^T Q per (image, head), written straight into the [B,M,2,heads,D] layout: A(m = key, k = query) = X[k][m]
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < heads; ++h) {
      const long x = ((long)b * heads + h) * N * M, t = (long)b * N * C + h * D, o = (long)b * M * 2 * C + h * D;
      if (int rc = hpfg_gemm_f32(P + x, 1, M, dout + t, C, 1, dkv + o + C, 2 * C, M, D, N, nullptr, 0, 0, stream)) return rc;
      if (int rc = hpfg_gemm_f32(dS + x, 1, M, q + t, C, 1, dkv + o, 2 * C, M, D, N, nullptr, 0, 0, stream)) return rc;
    }
  return 0;
}

bool shape_ok(int B, int N, int M, int heads, int head_dim, int math) {
  return B > 0 && B <= 65535 && N > 0 && M > 0 && M <= KEYS_MAX && heads > 0 && heads <= 16384 && (head_dim == 32 || head_dim == 64) &&
         (math == HPFG_MATH_F32 || math == HPFG_MATH_BF16X3);
}

}  // namespace

#define ATTN_KEYS_SHAPE_MSG "%s: bad args (1 to %d keys, head dim 32 or 64, math 0 or 1; got B %d, N %d, %d keys, %d heads, head dim %d, math %d, or a null pointer)"

extern "C" int hpfg_attn_keys_max(void) { return KEYS_MAX; }

extern "C" long hpfg_attn_keys_scratch_floats(int B, int N, int M, int heads, int head_dim, int math) {
  if (!shape_ok(B, N, M, heads, head_dim, math)) {
    hpfg_set_error(ATTN_KEYS_SHAPE_MSG, "attn_keys_scratch_floats", KEYS_MAX, B, N, M, heads, head_dim, math);
    return -1;
  }
  if (math == HPFG_MATH_F32) return 2L * B * heads * N * M;                                                          // P and scale * dS
  return delta_floats(B, N, heads) + (long)B * heads * ((M + MK - 1) / MK) * blocks_of(N) * 2 * MK * head_dim;      // delta, dK / dV partials
}

extern "C" int hpfg_attn_keys_fwd(const float* q, const float* kv, float* out, float* lse, int B, int N, int M, int heads, int head_dim, float scale,
                                  int math, void* stream) {
  HPFG_ARG_CHECK(q && kv && out && shape_ok(B, N, M, heads, head_dim, math), ATTN_KEYS_SHAPE_MSG, "attn_keys_fwd", KEYS_MAX, B, N, M, heads, head_dim, math);
  const hipStream_t st = (hipStream_t)stream;
  if (math == HPFG_MATH_BF16X3)
    return head_dim == 32 ? launch_fwd<32>(q, kv, out, lse, B, N, M, heads, scale, st) : launch_fwd<64>(q, kv, out, lse, B, N, M, heads, scale, st);
  const dim3 grid((N + 255) / 256, heads, B);
  if (head_dim == 32) hipLaunchKernelGGL(attn_keys_f32_fwd_kernel<32>, grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale);
  else hipLaunchKernelGGL(attn_keys_f32_fwd_kernel<64>, grid, dim3(256), 0, st, q, kv, out, lse, N, M, heads, scale);
  return hpfg_launch_status("attn_keys_f32_fwd_kernel");
}

extern "C" int hpfg_attn_keys_bwd(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv,
                                  float* scratch, int B, int N, int M, int heads, int head_dim, float scale, int math, void* stream) {
  HPFG_ARG_CHECK(q && kv && out && lse && dout && dq && dkv && scratch && shape_ok(B, N, M, heads, head_dim, math), ATTN_KEYS_SHAPE_MSG, "attn_keys_bwd",
                 KEYS_MAX, B, N, M, heads, head_dim, math);
  const hipStream_t st = (hipStream_t)stream;
  if (math == HPFG_MATH_BF16X3)
    return head_dim == 32 ? launch_bwd<32>(q, kv, out, lse, dout, dq, dkv, scratch, B, N, M, heads, scale, st)
                          : launch_bwd<64>(q, kv, out, lse, dout, dq, dkv, scratch, B, N, M, heads, scale, st);
  return head_dim == 32 ? launch_bwd_f32<32>(q, kv, out, lse, dout, dq, dkv, scratch, B, N, M, heads, scale, stream)
                        : launch_bwd_f32<64>(q, kv, out, lse, dout, dq, dkv, scratch, B, N, M, heads, scale, stream);
}
