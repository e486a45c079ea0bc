// Shifted-window attention of the Swin blocks (reference model/swinunet.py:207-248, WindowAttention.forward between the qkv and the proj
// Linear):   out = softmax(scale * q k^T + bias + mask) v   per (image, window, head), head dim D = 32 or 64, windows of w x w tokens with
// w^2 <= 64 keys (49 at w = 7) -- the ranges attn.hip was built for, so the arithmetic, lane layouts, LDS images and phases are those of
// attn_core.h; this file's own is the window addressing (token table), the logit term (bias + mask) and the bias gradient.
//
// One workgroup per (window, head, image).  What the reference does as four tensor copies per block -- roll by -s, window partition,
// window reverse, roll by +s -- is addressing here: position l = i w + j of window (wy, wx) is the rolled coordinate (y', x') =
// (wy w + i, wx w + j), i.e. the token ((y' + s) mod H, (x' + s) mod W) of the [B,H,W,3C] qkv map (channel = t C + h D + p, t = q, k, v),
// and the output row of a query is written at the token the query came from.  A 64-entry LDS table holds the token of every position.
//   logits  S[l1][l2] = scale q[l1].k[l2] + table[idx(l1,l2)][h] + mask(l1,l2)
//   idx     = (i1 - i2 + w - 1)(2w - 1) + (j1 - j2 + w - 1) = a[l1] - a[l2] + 2w(w - 1)  with  a[l] = i (2w - 1) + j  (one LDS word per position)
//   mask    = -100 (the reference's literal, not -inf) where the regions 3 r(y') + r(x') of query and key differ, r(y') = 0 below H - w,
//             1 below H - s, else 2 (create_mask :182-205); no mask at s = 0.  Padding keys (w^2 .. 63) are excluded exactly (-3e38 -> p = 0).
// With s = 0 and a zero table the added terms are exact zeros and the operation sequence is that of attn_mfma_fwd_kernel.
// Backward: dQ as attn_mfma_dq_kernel; dK / dV need no partial sums -- all queries of a key sit in its own window -- so the 2-wave dK / dV
// kernel (32 queries per wave = one contraction step) writes them straight into dqkv: with dQ every element of dqkv is written exactly
// once.  d table[idx][h] = sum of dS over images, windows and the (l1, l2) pairs of that idx: the dQ kernel leaves its 64 x 64 dS tile in
// LDS, one thread per idx adds the <= w^2 pairs in a fixed order into a per-workgroup partial, and attn_window_dbias_sum_kernel adds the
// partials in a fixed order (four contiguous slices, then ((0 + 1) + 2) + 3).  No atomics: two runs give the same bits.
// HPFG_MATH_F32: one thread per query / per key in plain fp32 (scores kept in LDS rows), same addressing, same partial scheme.
// LDS rows as in attn_core.h (strides of 4 mod 16 dwords); the dS tile has rows of 65 floats (a lane's row starts one bank after its neighbour's).
// The window geometry, the logit term, stage_win, the dropout rule and the partial sum are in attn_window.h, shared with attn_window_packed.hip.
#include "attn_window.h"

namespace {

// tok[l]: token (y W + x) of position l of window `win`, -1 for the padding positions; rel[l] = a[l] | region << 16
__device__ __forceinline__ void win_tables(const Win& g, int win, int tid, int* tok, int* rel) {
  if (tid < MK) {
    int t = -1, a = 0;
    if (tid < g.L()) {
      const int nwx = g.W / g.w, wy = win / nwx, wx = win % nwx, i = tid / g.w, j = tid % g.w;
      const int yp = wy * g.w + i, xp = wx * g.w + j;
      const int ry = g.s == 0 ? 0 : (yp < g.H - g.w ? 0 : (yp < g.H - g.s ? 1 : 2));
      const int rx = g.s == 0 ? 0 : (xp < g.W - g.w ? 0 : (xp < g.W - g.s ? 1 : 2));
      const int y = yp + g.s < g.H ? yp + g.s : yp + g.s - g.H, x = xp + g.s < g.W ? xp + g.s : xp + g.s - g.W;
      t = y * g.W + x;
      a = (i * (2 * g.w - 1) + j) | ((3 * ry + rx) << 16);
    }
    tok[tid] = t;
    rel[tid] = a;
  }
}

// the logit term of attn_core.h for the one query of a lane, whose word rq was loaded once: bias + mask of the logit against key position kp
struct WinTerm {
  int rq;
  const int* rel;
  const float* bias;
  int c0;
  __device__ __forceinline__ float operator()(float sc, int kp) const { return logit_add(sc, rq, rel[kp], c0, bias); }
};

// the factors of the lane's query l1 in the S^T orientation: f[t][r] for key 16 t + 4 g + r (1 outside the window's positions: p is 0 or unused there)
__device__ __forceinline__ void drop_factors_t(const Drop& dr, uint32_t sd, uint32_t base, int l1, int L, int lane, f32x4 (&f)[4]) {
  const int g = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 16 * t + 4 * g + r;
      f[t][r] = l1 < L && key < L ? dr(sd, base + (uint32_t)(l1 * L + key)) : 1.f;
    }
}

template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_window_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table, float* __restrict__ out, Win gm,
                                                              float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KPLANE + 2 * TPL];      // K hi | K lo | V^T hi | V^T lo
  __shared__ int tok[MK], rel[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsVT = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int win = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C;
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  win_tables(gm, win, tid, tok, rel);
  load_bias<256>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win<D, 256>(img, tok, C3, C + h * D, ldsK, nullptr, tid);
  stage_win<D, 256>(img, tok, C3, 2 * C + h * D, nullptr, ldsVT, tid);
  __syncthreads();
  const int l1 = wave * 16 + (lane & 15), t1 = tok[l1];
  bf16x8 qh[KS], ql[KS];
  load_row_frags<D>(img, t1 >= 0 ? t1 : HW, HW, C3, h, lane, scale, qh, ql);
  f32x4 p[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, gm.L(), lane, WinTerm{rel[l1], rel, bias, gm.c0()}, p);
  if constexpr (DROP) {
    f32x4 f[4];
    drop_factors_t(dr, dr.word(), drop_base(gm, b, gridDim.x, win, h), l1, gm.L(), lane, f);
#pragma unroll
    for (int t = 0; t < 4; ++t) p[t] *= f[t];
  }
  zero_tiles(o);
  mul_trn<D>(p, ldsVT, lane, o);                  // O^T[d][q]
  if (t1 >= 0) store_o<D>(out + ((long)b * HW + t1) * C + h * D + (lane >> 4) * 4, o);
}

// this workgroup's part[idx] = sum of ds[l1][l2] over the pairs of the window with bias index idx, in a fixed order (l2 ascending)
template <int NT>
__device__ __forceinline__ void bias_partial(const float* ds, const Win& g, float* __restrict__ part, int tid) {
  const int w = g.w, n = 2 * w - 1;
  for (int e = tid; e < g.T(); e += NT) {
    const int di = e / n - (w - 1), dj = e % n - (w - 1);      // i1 - i2, j1 - j2
    const int i0 = di < 0 ? -di : 0, i1 = di > 0 ? w - di : w, j0 = dj < 0 ? -dj : 0, j1 = dj > 0 ? w - dj : w;
    float s = 0.f;
    for (int i2 = i0; i2 < i1; ++i2)
      for (int j2 = j0; j2 < j1; ++j2) s += ds[((i2 + di) * w + j2 + dj) * DSROW + i2 * w + j2];
    part[e] = s;
  }
}

// dq = scale * dS K with dS = P .* (dP - rowsum(P .* dP)), dP = dO V^T (S^T orientation, one query per lane); the dS tile -> the bias partial
template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_window_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ table, const float* __restrict__ dout,
                                                             float* __restrict__ dqkv, float* __restrict__ part, Win gm, float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * TPL];      // K hi|lo, V hi|lo (natural), K^T hi|lo
  __shared__ float dsl[MK * DSROW];
  __shared__ int tok[MK], rel[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  unsigned char* ldsKT = lds + 4 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int win = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C;
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  win_tables(gm, win, tid, tok, rel);
  load_bias<256>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win<D, 256>(img, tok, C3, C + h * D, ldsK, ldsKT, tid);
  stage_win<D, 256>(img, tok, C3, 2 * C + h * D, ldsV, nullptr, tid);
  __syncthreads();
  const int l1 = wave * 16 + (lane & 15), t1 = tok[l1];
  bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  load_row_frags<D>(img, t1 >= 0 ? t1 : HW, HW, C3, h, lane, scale, qh, ql);
  load_row_frags<D>(dout + (long)b * HW * C, t1 >= 0 ? t1 : HW, HW, C, h, lane, 1.f, dh, dl);
  f32x4 p[4], dp[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, gm.L(), lane, WinTerm{rel[l1], rel, bias, gm.c0()}, p);
  if constexpr (DROP) {
    f32x4 f[4];
    drop_factors_t(dr, dr.word(), drop_base(gm, b, gridDim.x, win, h), l1, gm.L(), lane, f);
    ds_drop_t<D>(ldsV, dh, dl, lane, p, f, dp);
  } else {
    ds_t<D>(ldsV, dh, dl, lane, p, dp);            // dS^T: zero at the padding keys (p = 0) and padding queries (dO = 0)
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dsl[l1 * DSROW + 16 * t + 4 * g + r] = dp[t][r];
  zero_tiles(o);
  mul_trn<D>(dp, ldsKT, lane, o);                 // dQ^T[d][q] / scale
  if (t1 >= 0) store_o<D>(dqkv + ((long)b * HW + t1) * C3 + h * D + g * 4, o, scale);
  __syncthreads();
  bias_partial<256>(dsl, gm, part + (((long)b * gridDim.x + win) * gm.heads + h) * gm.T(), tid);
}

// dV = P^T dO, dK = scale * dS^T Q over the window's 64 query positions (S orientation: 4 queries per lane, the key on the lane), as
// attn_mfma_dkv_kernel with two waves of 32 queries each; the sum of the two waves IS dK / dV of the window's keys.
template <int D, bool DROP>
__global__ __launch_bounds__(128) void attn_window_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ table, const float* __restrict__ dout,
                                                              float* __restrict__ dqkv, Win gm, float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, QPL = Geo<D>::QPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * 4 * QPL];      // K, V natural (hi|lo each); per wave: dO^T hi|lo, Q^T hi|lo
  static_assert(2 * MK * D * 4 <= 4 * KPLANE, "the wave reduction reuses the K / V images");
  __shared__ int tok[MK], rel[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  unsigned char* myDO = lds + 4 * KPLANE + wave * 4 * QPL;
  unsigned char* myQ = myDO + 2 * QPL;
  const int win = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C, L = gm.L(), c0 = gm.c0();
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  const float* db = dout + (long)b * HW * C;
  const uint32_t drop_seed = DROP ? dr.word() : 0u, drop_e0 = drop_base(gm, b, gridDim.x, win, h);
  win_tables(gm, win, tid, tok, rel);
  load_bias<128>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win<D, 128>(img, tok, C3, C + h * D, ldsK, nullptr, tid);
  stage_win<D, 128>(img, tok, C3, 2 * C + h * D, ldsV, nullptr, tid);
  __syncthreads();
  f32x4 accV[DT][4], accK[DT][4];               // dV^T / dK^T [d tile][key tile]: rows d, column = key on the lane
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      accV[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      accK[dt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const int base = wave * 32;
  f32x4 s[2][4], dp[2][4];
  bf16x8 qh[2][KS], ql[2][KS], dh[2][KS], dl[2][KS];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int tq = tok[base + 16 * u + (lane & 15)];
    load_row_frags<D>(img, tq >= 0 ? tq : HW, HW, C3, h, lane, scale, qh[u], ql[u]);
    load_row_frags<D>(db, tq >= 0 ? tq : HW, HW, C, h, lane, 1.f, dh[u], dl[u]);
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
  // S[q][key] and dP[q][key]: queries base + 16 u + 4 g + r on the rows, key 16 t + (lane & 15) on the lane
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
    const int key = 16 * t + (lane & 15), rk = rel[key];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      s[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, s[u][t], qh[u][ks], ql[u][ks], fkh[ks], fkl[ks]) }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, dp[u][t], dh[u][ks], dl[u][ks], fvh[ks], fvl[ks]) }
#pragma unroll
      for (int r = 0; r < 4; ++r) s[u][t][r] = key < L ? logit_add(s[u][t][r], rel[base + 16 * u + 4 * g + r], rk, c0, bias) : NEG;
    }
  }
  // softmax statistics per query row: 4 tiles x 16 lanes hold a row's 64 scores
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = NEG;
#pragma unroll
      for (int t = 0; t < 4; ++t) mx = fmaxf(mx, s[u][t][r]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float den = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[u][t][r] = 16 * t + (lane & 15) < L ? expf(s[u][t][r] - mx) : 0.f;
        den += s[u][t][r];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) den += __shfl_xor(den, o);
      const float inv = 1.f / den;
      float delta = 0.f;
      const bool live = base + 16 * u + 4 * g + r < L;      // padding queries contribute nothing (their q / dO were zeroed; P is not zero)
      float fm[4];                                          // DROP: M / (1 - p) of (this query, the lane's key of tile t)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[u][t][r] *= inv;                                 // P
        if constexpr (DROP) {
          const int key = 16 * t + (lane & 15);
          fm[t] = live && key < L ? dr(drop_seed, drop_e0 + (uint32_t)((base + 16 * u + 4 * g + r) * L + key)) : 1.f;
          dp[u][t][r] *= fm[t];
        }
        delta += s[u][t][r] * dp[u][t][r];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) delta += __shfl_xor(delta, o);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        dp[u][t][r] = live ? s[u][t][r] * (dp[u][t][r] - delta) : 0.f;      // dS
        if (!live) s[u][t][r] = 0.f;
        if constexpr (DROP) s[u][t][r] *= fm[t];           // dV takes the dropped probabilities
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
  // add the two waves in a fixed order (wave 0 stores, wave 1 adds): [2][64 keys][D d]; accumulator rows = d (4 g + r), column = key.
  // The K / V images are dead by now.
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);                       // [2][64][D] floats = 16 KB / 32 KB
  for (int w = 0; w < 2; ++w) {
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
  // dqkv[token of the key][1 + which][h][d]   (dK already carries the scale through the scaled q)
  for (int e = tid; e < 2 * MK * D / 4; e += 128) {
    const int which = e / (MK * D / 4), key = (e / (D / 4)) % MK, d = (e % (D / 4)) * 4;
    const int t = tok[key];
    if (t >= 0) *reinterpret_cast<f32x4*>(dqkv + ((long)b * HW + t) * C3 + (1 + which) * C + h * D + d) = *reinterpret_cast<const f32x4*>(red + 4 * e);
  }
}

// ---- exact fp32 (HPFG_MATH_F32): one workgroup of 64 threads per (window, head, image) ---------------------------------------------------
template <int AD>
__device__ __forceinline__ void stage_win_f32(const float* __restrict__ img, const int* tok, int L, int C3, int coff, float (*dst)[AD + 1], float mul) {
  for (int e = threadIdx.x; e < L * AD; e += 64) {
    const int j = e / AD, c = e % AD;
    dst[j][c] = img[(long)tok[j] * C3 + coff + c] * mul;
  }
}

template <int AD, bool DROP>
__global__ __launch_bounds__(64) void attn_window_f32_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table, float* __restrict__ out,
                                                                 Win gm, float scale, Drop dr) {
  __shared__ float ks[MK][AD + 1], vs[MK][AD + 1], sc[MK * DSROW];
  __shared__ int tok[MK], rel[MK];
  __shared__ float bias[TMAX];
  const int tid = threadIdx.x, win = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * AD, C3 = 3 * C, L = gm.L(), c0 = gm.c0();
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  win_tables(gm, win, tid, tok, rel);
  load_bias<64>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win_f32<AD>(img, tok, L, C3, C + h * AD, ks, 1.f);
  stage_win_f32<AD>(img, tok, L, C3, 2 * C + h * AD, vs, 1.f);
  __syncthreads();
  if (tid >= L) return;                          // (no barrier below)
  const int t1 = tok[tid], rq = rel[tid];
  float qv[AD], o[AD];
#pragma unroll
  for (int c = 0; c < AD; c += 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(img + (long)t1 * C3 + h * AD + c);
    qv[c] = t[0] * scale; qv[c + 1] = t[1] * scale; qv[c + 2] = t[2] * scale; qv[c + 3] = t[3] * scale;
    o[c] = o[c + 1] = o[c + 2] = o[c + 3] = 0.f;
  }
  float* row = sc + tid * DSROW;
  float mx = NEG;
  for (int j = 0; j < L; ++j) {
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < AD; ++c) d += qv[c] * ks[j][c];
    row[j] = logit_add(d, rq, rel[j], c0, bias);
    mx = fmaxf(mx, row[j]);
  }
  float den = 0.f;
  const uint32_t drop_seed = DROP ? dr.word() : 0u, drop_e0 = drop_base(gm, b, gridDim.x, win, h) + (uint32_t)(tid * L);
  for (int j = 0; j < L; ++j) {
    float e = expf(row[j] - mx);
    den += e;
    if constexpr (DROP) e *= dr(drop_seed, drop_e0 + j);
#pragma unroll
    for (int c = 0; c < AD; ++c) o[c] += e * vs[j][c];
  }
  const float inv = 1.f / den;
  float* op = out + ((long)b * HW + t1) * C + h * AD;
#pragma unroll
  for (int c = 0; c < AD; c += 4) *reinterpret_cast<f32x4*>(op + c) = f32x4{o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv};
}

// phase 1, thread = query: P and dS rows into LDS, dq; phase 2, thread = key: dK = dS^T (scale q), dV = P^T dO; then the bias partial
template <int AD, bool DROP>
__global__ __launch_bounds__(64) void attn_window_f32_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                 const float* __restrict__ dout, float* __restrict__ dqkv, float* __restrict__ part, Win gm,
                                                                 float scale, Drop dr) {
  __shared__ float ks[MK][AD + 1], vs[MK][AD + 1], qs[MK][AD + 1], dos[MK][AD + 1], P[MK * DSROW], dS[MK * DSROW];
  __shared__ int tok[MK], rel[MK];
  __shared__ float bias[TMAX];
  const int tid = threadIdx.x, win = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * AD, C3 = 3 * C, L = gm.L(), c0 = gm.c0();
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  win_tables(gm, win, tid, tok, rel);
  load_bias<64>(table, gm, h, tid, bias);
  for (int e = tid; e < MK * DSROW; e += 64) dS[e] = 0.f;      // the bias partial reads rows and columns of valid positions only; keep the rest defined
  __syncthreads();
  stage_win_f32<AD>(img, tok, L, C3, h * AD, qs, scale);
  stage_win_f32<AD>(img, tok, L, C3, C + h * AD, ks, 1.f);
  stage_win_f32<AD>(img, tok, L, C3, 2 * C + h * AD, vs, 1.f);
  stage_win_f32<AD>(dout + (long)b * HW * C, tok, L, C, h * AD, dos, 1.f);
  __syncthreads();
  const bool live = tid < L;
  const int t1 = live ? tok[tid] : 0;
  const uint32_t drop_seed = DROP ? dr.word() : 0u, drop_e0 = drop_base(gm, b, gridDim.x, win, h) + (uint32_t)(tid * L);
  if (live) {
    const int rq = rel[tid];
    float* prow = P + tid * DSROW;
    float* srow = dS + tid * DSROW;
    float mx = NEG;
    for (int j = 0; j < L; ++j) {
      float d = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < AD; ++c) {
        d += qs[tid][c] * ks[j][c];
        dp += dos[tid][c] * vs[j][c];
      }
      prow[j] = logit_add(d, rq, rel[j], c0, bias);
      if constexpr (DROP) dp *= dr(drop_seed, drop_e0 + j);
      srow[j] = dp;
      mx = fmaxf(mx, prow[j]);
    }
    float den = 0.f, delta = 0.f;
    for (int j = 0; j < L; ++j) {
      const float e = expf(prow[j] - mx);
      prow[j] = e;
      den += e;
      delta += e * srow[j];
    }
    const float inv = 1.f / den;
    delta *= inv;
    float dqv[AD];
#pragma unroll
    for (int c = 0; c < AD; ++c) dqv[c] = 0.f;
    for (int j = 0; j < L; ++j) {
      const float pr = prow[j] * inv, ds = pr * (srow[j] - delta);
      if constexpr (DROP) prow[j] = pr * dr(drop_seed, drop_e0 + j);      // dV takes the dropped probabilities
      else prow[j] = pr;
      srow[j] = ds;
#pragma unroll
      for (int c = 0; c < AD; ++c) dqv[c] += ds * ks[j][c];
    }
    float* qo = dqkv + ((long)b * HW + t1) * C3 + h * AD;
#pragma unroll
    for (int c = 0; c < AD; c += 4) *reinterpret_cast<f32x4*>(qo + c) = f32x4{dqv[c] * scale, dqv[c + 1] * scale, dqv[c + 2] * scale, dqv[c + 3] * scale};
  }
  __syncthreads();
  if (live) {
    float dk[AD], dv[AD];
#pragma unroll
    for (int c = 0; c < AD; ++c) dk[c] = dv[c] = 0.f;
    for (int q = 0; q < L; ++q) {
      const float pr = P[q * DSROW + tid], ds = dS[q * DSROW + tid];
#pragma unroll
      for (int c = 0; c < AD; ++c) {
        dk[c] += ds * qs[q][c];
        dv[c] += pr * dos[q][c];
      }
    }
    float* ko = dqkv + ((long)b * HW + t1) * C3 + C + h * AD;
#pragma unroll
    for (int c = 0; c < AD; c += 4) {
      *reinterpret_cast<f32x4*>(ko + c) = f32x4{dk[c], dk[c + 1], dk[c + 2], dk[c + 3]};
      *reinterpret_cast<f32x4*>(ko + C + c) = f32x4{dv[c], dv[c + 1], dv[c + 2], dv[c + 3]};
    }
  }
  bias_partial<64>(dS, gm, part + (((long)b * gridDim.x + win) * gm.heads + h) * gm.T(), tid);
}

bool shape_ok(int B, int H, int W, int heads, int head_dim, int window, int shift, int math) {
  return B > 0 && B <= 65535 && H > 0 && W > 0 && heads > 0 && heads <= 65535 && (head_dim == 32 || head_dim == 64) && window > 0 &&
         window * window <= MK && H % window == 0 && W % window == 0 && shift >= 0 && shift < window && (long)H * W <= (1L << 30) &&
         (math == HPFG_MATH_F32 || math == HPFG_MATH_BF16X3);
}

template <int D, bool DROP>
void launch_fwd(const float* qkv, const float* table, float* out, int B, const Win& g, float scale, int math, const Drop& dr, hipStream_t st) {
  const dim3 grid(g.nwin(), g.heads, B);
  if (math == HPFG_MATH_BF16X3) hipLaunchKernelGGL((attn_window_fwd_kernel<D, DROP>), grid, dim3(256), 0, st, qkv, table, out, g, scale, dr);
  else hipLaunchKernelGGL((attn_window_f32_fwd_kernel<D, DROP>), grid, dim3(64), 0, st, qkv, table, out, g, scale, dr);
}

template <int D, bool DROP>
void launch_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dbias, float* part, int B, const Win& g, float scale, int math,
                const Drop& dr, hipStream_t st) {
  const dim3 grid(g.nwin(), g.heads, B);
  if (math == HPFG_MATH_BF16X3) {
    hipLaunchKernelGGL((attn_window_dq_kernel<D, DROP>), grid, dim3(256), 0, st, qkv, table, dout, dqkv, part, g, scale, dr);
    hipLaunchKernelGGL((attn_window_dkv_kernel<D, DROP>), grid, dim3(128), 0, st, qkv, table, dout, dqkv, g, scale, dr);
  } else {
    hipLaunchKernelGGL((attn_window_f32_bwd_kernel<D, DROP>), grid, dim3(64), 0, st, qkv, table, dout, dqkv, part, g, scale, dr);
  }
  hipLaunchKernelGGL(attn_window_dbias_sum_kernel, dim3((g.heads * g.T() + 63) / 64), dim3(256), 0, st, part, dbias, B * g.nwin(), g.heads, g.T());
}

}  // namespace

#define ATTN_WINDOW_SHAPE_MSG                                                                                                                        \
  "%s: bad args (window^2 <= %d keys, H and W multiples of the window, 0 <= shift < window, head dim 32 or 64, heads >= 1, math 0 or 1; got B %d, " \
  "map %d x %d, %d heads, head dim %d, window %d, shift %d, math %d, or a null pointer)"

extern "C" long hpfg_attn_window_scratch_floats(int B, int H, int W, int heads, int head_dim, int window, int math) {
  if (!shape_ok(B, H, W, heads, head_dim, window, 0, math)) {
    hpfg_set_error(ATTN_WINDOW_SHAPE_MSG, "attn_window_scratch_floats", MK, B, H, W, heads, head_dim, window, 0, math);
    return -1;
  }
  const Win g{H, W, window, 0, heads};
  return (long)B * g.nwin() * heads * g.T();
}

extern "C" int hpfg_attn_window_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window,
                                    int shift, float scale, int math, void* stream) {
  HPFG_ARG_CHECK(qkv && bias_table && out && shape_ok(B, H, W, heads, head_dim, window, shift, math), ATTN_WINDOW_SHAPE_MSG, "attn_window_fwd", MK, B, H, W,
                 heads, head_dim, window, shift, math);
  const Win g{H, W, window, shift, heads};
  if (head_dim == 32) launch_fwd<32, false>(qkv, bias_table, out, B, g, scale, math, Drop{}, (hipStream_t)stream);
  else launch_fwd<64, false>(qkv, bias_table, out, B, g, scale, math, Drop{}, (hipStream_t)stream);
  return hpfg_launch_status("attn_window_fwd");
}

extern "C" int hpfg_attn_window_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B, int H,
                                    int W, int heads, int head_dim, int window, int shift, float scale, int math, void* stream) {
  HPFG_ARG_CHECK(qkv && bias_table && dout && dqkv && dbias && scratch && shape_ok(B, H, W, heads, head_dim, window, shift, math), ATTN_WINDOW_SHAPE_MSG,
                 "attn_window_bwd", MK, B, H, W, heads, head_dim, window, shift, math);
  const Win g{H, W, window, shift, heads};
  if (head_dim == 32) launch_bwd<32, false>(qkv, bias_table, dout, dqkv, dbias, scratch, B, g, scale, math, Drop{}, (hipStream_t)stream);
  else launch_bwd<64, false>(qkv, bias_table, dout, dqkv, dbias, scratch, B, g, scale, math, Drop{}, (hipStream_t)stream);
  return hpfg_launch_status("attn_window_bwd");
}

#define ATTN_WINDOW_DROP_MSG "%s: bad dropout args (0 <= p < 1, B nW heads L^2 < 2^32 mask elements; got p %g)"

extern "C" int hpfg_attn_window_drop_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window,
                                         int shift, float scale, int math, float p, uint32_t seed, const uint32_t* seed_dev, const uint8_t* mask,
                                         void* stream) {
  HPFG_ARG_CHECK(qkv && bias_table && out && shape_ok(B, H, W, heads, head_dim, window, shift, math), ATTN_WINDOW_SHAPE_MSG, "attn_window_drop_fwd", MK, B, H,
                 W, heads, head_dim, window, shift, math);
  const Win g{H, W, window, shift, heads};
  HPFG_ARG_CHECK(p >= 0.f && p < 1.f && drop_elems(B, g) < (1L << 32), ATTN_WINDOW_DROP_MSG, "attn_window_drop_fwd", (double)p);
  if (p == 0.f && !mask) return hpfg_attn_window_fwd(qkv, bias_table, out, B, H, W, heads, head_dim, window, shift, scale, math, stream);
  const Drop dr{mask, seed_dev, seed, hpfg_drop_threshold(p), 1.f / (1.f - p)};
  if (head_dim == 32) launch_fwd<32, true>(qkv, bias_table, out, B, g, scale, math, dr, (hipStream_t)stream);
  else launch_fwd<64, true>(qkv, bias_table, out, B, g, scale, math, dr, (hipStream_t)stream);
  return hpfg_launch_status("attn_window_drop_fwd");
}

extern "C" int hpfg_attn_window_drop_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B, int H,
                                         int W, int heads, int head_dim, int window, int shift, float scale, int math, float p, uint32_t seed,
                                         const uint32_t* seed_dev, const uint8_t* mask, void* stream) {
  HPFG_ARG_CHECK(qkv && bias_table && dout && dqkv && dbias && scratch && shape_ok(B, H, W, heads, head_dim, window, shift, math), ATTN_WINDOW_SHAPE_MSG,
                 "attn_window_drop_bwd", MK, B, H, W, heads, head_dim, window, shift, math);
  const Win g{H, W, window, shift, heads};
  HPFG_ARG_CHECK(p >= 0.f && p < 1.f && drop_elems(B, g) < (1L << 32), ATTN_WINDOW_DROP_MSG, "attn_window_drop_bwd", (double)p);
  if (p == 0.f && !mask)
    return hpfg_attn_window_bwd(qkv, bias_table, dout, dqkv, dbias, scratch, B, H, W, heads, head_dim, window, shift, scale, math, stream);
  const Drop dr{mask, seed_dev, seed, hpfg_drop_threshold(p), 1.f / (1.f - p)};
  if (head_dim == 32) launch_bwd<32, true>(qkv, bias_table, dout, dqkv, dbias, scratch, B, g, scale, math, dr, (hipStream_t)stream);
  else launch_bwd<64, true>(qkv, bias_table, dout, dqkv, dbias, scratch, B, g, scale, math, dr, (hipStream_t)stream);
  return hpfg_launch_status("attn_window_drop_bwd");
}

extern "C" long hpfg_attn_window_drop_elems(int B, int H, int W, int heads, int window) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || window <= 0 || window * window > MK || H % window || W % window) {
    hpfg_set_error("attn_window_drop_elems: bad args (B %d, map %d x %d, %d heads, window %d)", B, H, W, heads, window);
    return -1;
  }
  return drop_elems(B, Win{H, W, window, 0, heads});
}

extern "C" int hpfg_attn_window_drop_mask(uint8_t* out, int B, int H, int W, int heads, int window, float p, uint32_t seed, const uint32_t* seed_dev,
                                          void* stream) {
  const long n = hpfg_attn_window_drop_elems(B, H, W, heads, window);
  if (n < 0) return -1;
  return hpfg_dropout_mask(out, n, p, seed, seed_dev, stream);          // the hash rule over the flat element index IS the mask
}
