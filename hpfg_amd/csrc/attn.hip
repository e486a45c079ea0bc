// Attention core of the SegFormer branch on the matrix cores (reference model/segformer.py:92-128, Attention.forward after the q / kv
// projections and the spatial reduction):   out = softmax(scale * q k^T) v   per (image, head), head dim D = 32 or 64 (every kernel is a template over D), at most 64 keys.
//
// The arithmetic, lane layouts, LDS images and every phase of the kernels are in attn_core.h, shared with attn_keys.hip (65 .. 256 keys --
// inputs above 256 x 256) and attn_window.hip.  This file's own: one LDS image of all keys staged once per workgroup, no logit term,
// the dK / dV kernel (its whole text: dK / dV are not among the shared phases) with its fragments held in registers at D = 32, and
// per-workgroup dK / dV partials summed in a fixed order by attn_dkv_sum_kernel.
//   q [B,N,heads,D], kv [B,M,2,heads,D] (the kv Linear's output layout), out / dq like q, dkv like kv.
#include "attn_core.h"

namespace {

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
  bf16x8 qh[KS], ql[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  f32x4 p[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, M, lane, NoTerm{}, p);
  zero_tiles(o);
  mul_trn<D>(p, ldsVT, lane, o);               // O^T[d][q]
  if (qi < N) store_o<D>(out + ((long)b * N + qi) * C + h * D + (lane >> 4) * 4, o);
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
  bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  load_row_frags<D>(q + (long)b * N * C, qi, N, C, h, lane, scale, qh, ql);
  load_row_frags<D>(dout + (long)b * N * C, qi, N, C, h, lane, 1.f, dh, dl);
  f32x4 p[4], dp[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, M, lane, NoTerm{}, p);
  ds_t<D>(ldsV, dh, dl, lane, p, dp);              // dS^T
  zero_tiles(o);
  mul_trn<D>(dp, ldsKT, lane, o);              // dQ^T[d][q] / scale
  if (qi < N) store_o<D>(dq + ((long)b * N + qi) * C + h * D + g * 4, o, scale);
}

// dV = P^T dO, dK = scale * dS^T Q over the queries [q0, q1) of this workgroup (S orientation: 4 queries per lane, the key on the lane).
// Each wave takes 32 queries per step; the transposed images dO^T / Q^T [D d][32 q] of those queries live in a per-wave LDS slot.
// The K / V fragments with the key on the lane are constant over the loop: at D = 32 they stay in registers (64 VGPRs); at D = 64 they
// would take 128 next to 128 accumulator registers, so they are re-read from LDS at every step instead (HOLD = false).
// The loop body and the wave reduction exist again, edited, in attn_keys_dkv_kernel and attn_window_dkv_kernel (see the top of attn_core.h
// for why they are not shared phases): an edit here is made there too.
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
  bf16x8 kh[HOLD ? 4 : 1][KS], kl[HOLD ? 4 : 1][KS], vh[HOLD ? 4 : 1][KS], vl[HOLD ? 4 : 1][KS];
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
    // S[q][key] and dP[q][key]: queries 16 u + 4 g + r on the rows, key 16 t + (lane & 15) on the lane
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8 fkh[KS], fkl[KS], fvh[KS], fvl[KS];
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
        for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, s[u][t], qh[u][ks], ql[u][ks], fkh[ks], fkl[ks]) }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, dp[u][t], dh[u][ks], dl[u][ks], fvh[ks], fvl[ks]) }
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
