// Shifted-window attention for windows of at most 16 tokens (window 2, 3, 4: the LIDC Swin-UNet of the reference, model/swinunet_LIDC.py,
// window 3 at 96 x 96 and 4 at 64 x 64), the operation of csrc/attn_window.hip (reference model/swinunet.py:207-248) with several windows in
// one 64-row tile.  attn_window.hip gives every window a workgroup with a 64-key LDS image: at w = 3 nine of the 64 rows are real.  Here
// P = 64 / w^2 windows (16, 7, 4) of one (image, head), taken in raster order, share the tile: one workgroup per (tile, head, image) with
// tiles = ceil(nW / P).  Tile row p = slot L + l is position l of window tile P + slot; rows of the slots the last tile of an image does not
// fill, and rows P L .. 63, are padding as rows 49 .. 63 are at w = 7.
//   logits  S[p1][p2] = scale q[p1].k[p2] + table[idx(l1, l2)][h] + mask   between positions of one window (the term of attn_window.h);
//           between positions of different windows of the tile the key is excluded exactly, as padding keys are: NEG before the maximum, an
//           exact 0 after the expf (expf(NEG - mx) is 0 for every finite mx, and a live row's maximum is finite: it holds its own window).
//           The per-position word carries the slot beside the region: a[l] | region << 16 | slot << 20; padding rows carry PAD_SLOT.
// Forward and dQ are the S^T phases of attn_core.h with that term.  All queries of a key sit in the key's own tile, so dK / dV need no
// partial sums (the two-wave kernel of attn_window.hip with the packed term) and with dQ every element of dqkv is written exactly once.
// d table: the dS tile stays in LDS, one thread per table index adds the pairs of the tile's windows in a fixed order (slot, then l2
// ascending) into a per-workgroup partial, attn_window_dbias_sum_kernel adds the partials in a fixed order.  No atomics.
// Dropout: the keep decision of element (((b nW + win) heads + h) L + l1) L + l2 with win the window's index in the IMAGE, not its slot, so
// hpfg_attn_window_drop_mask / _drop_elems and a mask recorded from the reference serve both families.
// HPFG_MATH_F32 runs the one-thread-per-query kernels of attn_window.hip through hpfg_attn_window_drop_fwd / _bwd: exact mode is not the
// fast path, and the bits are theirs.
#include "attn_window.h"

namespace {

constexpr int PACK_MAX_WINDOW = 4;             // w^2 <= 16: at least four windows per tile
constexpr int PAD_SLOT = 31;                   // slot field of a padding row (slots are 0 .. 15)

struct Pack {
  Win g;
  int P, tiles;                                // windows per tile, tiles per (image, head)
  __device__ __host__ int live(int tile) const {          // real rows of a tile
    const int n = g.nwin() - tile * P;
    return (n < P ? n : P) * g.L();
  }
};

// tables of tile `tile`: tok[p] token (y W + x) or -1, rel[p] = a | region << 16 | slot << 20, dbase[p] = first dropout element of the
// row's [L] keys for head h (the element of key position l2 is dbase[p1] + pos[p2]), pos[p] = l
__device__ __forceinline__ void pack_tables(const Pack& pk, int tile, int b, int h, int tid, int* tok, int* rel, uint32_t* dbase, int* pos) {
  if (tid < MK) {
    const Win& g = pk.g;
    const int L = g.L(), slot = tid / L, l = tid % L, win = tile * pk.P + slot;
    int t = -1, a = PAD_SLOT << 20;
    uint32_t e = 0;
    if (slot < pk.P && win < g.nwin()) {
      const int nwx = g.W / g.w, wy = win / nwx, wx = win % nwx, i = l / g.w, j = l % g.w;
      const int yp = wy * g.w + i, xp = wx * g.w + j;
      const int ry = g.s == 0 ? 0 : (yp < g.H - g.w ? 0 : (yp < g.H - g.s ? 1 : 2));
      const int rx = g.s == 0 ? 0 : (xp < g.W - g.w ? 0 : (xp < g.W - g.s ? 1 : 2));
      const int y = yp + g.s < g.H ? yp + g.s : yp + g.s - g.H, x = xp + g.s < g.W ? xp + g.s : xp + g.s - g.W;
      t = y * g.W + x;
      a = (i * (2 * g.w - 1) + j) | ((3 * ry + rx) << 16) | (slot << 20);
      e = drop_base(g, b, g.nwin(), win, h) + (uint32_t)(l * L);
    }
    tok[tid] = t;
    rel[tid] = a;
    dbase[tid] = e;
    pos[tid] = l;
  }
}

// the window's bias + mask inside a window, exclusion between windows (query word rq, key word rk)
__device__ __forceinline__ float pack_logit(float sc, int rq, int rk, int c0, const float* bias) {
  return ((rq ^ rk) >> 20) != 0 ? NEG : logit_add(sc, rq, rk, c0, bias);
}

// the logit term of attn_core.h for the one query of a lane
struct PackTerm {
  int rq;
  const int* rel;
  const float* bias;
  int c0;
  __device__ __forceinline__ float operator()(float sc, int kp) const { return pack_logit(sc, rq, rel[kp], c0, bias); }
};

// the dropout factors of the lane's query p1 in the S^T orientation: f[t][r] for key row 16 t + 4 g + r (1 outside the query's window: p is 0 there)
__device__ __forceinline__ void pack_drop_factors_t(const Drop& dr, uint32_t sd, int p1, int M, const int* rel, const uint32_t* dbase, const int* pos, int lane,
                                                    f32x4 (&f)[4]) {
  const int g = lane >> 4, rq = rel[p1];
  const uint32_t e0 = dbase[p1];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 16 * t + 4 * g + r;
      f[t][r] = p1 < M && key < M && ((rq ^ rel[key]) >> 20) == 0 ? dr(sd, e0 + (uint32_t)pos[key]) : 1.f;
    }
}

template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_window_packed_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table, float* __restrict__ out,
                                                                     Pack pk, float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * KPLANE + 2 * TPL];      // K hi | K lo | V^T hi | V^T lo
  __shared__ int tok[MK], rel[MK], pos[MK];
  __shared__ uint32_t dbase[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsVT = lds + 2 * KPLANE;
  const Win& gm = pk.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C, M = pk.live(tile);
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  pack_tables(pk, tile, b, h, tid, tok, rel, dbase, pos);
  load_bias<256>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win<D, 256>(img, tok, C3, C + h * D, ldsK, nullptr, tid);
  stage_win<D, 256>(img, tok, C3, 2 * C + h * D, nullptr, ldsVT, tid);
  __syncthreads();
  const int p1 = wave * 16 + (lane & 15), t1 = tok[p1];
  bf16x8 qh[KS], ql[KS];
  load_row_frags<D>(img, t1 >= 0 ? t1 : HW, HW, C3, h, lane, scale, qh, ql);
  f32x4 p[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, M, lane, PackTerm{rel[p1], rel, bias, gm.c0()}, p);
  if constexpr (DROP) {
    f32x4 f[4];
    pack_drop_factors_t(dr, dr.word(), p1, M, rel, dbase, pos, lane, f);
#pragma unroll
    for (int t = 0; t < 4; ++t) p[t] *= f[t];
  }
  zero_tiles(o);
  mul_trn<D>(p, ldsVT, lane, o);                  // O^T[d][q]
  if (t1 >= 0) store_o<D>(out + ((long)b * HW + t1) * C + h * D + (lane >> 4) * 4, o);
}

// this workgroup's part[idx] = sum of ds[p1][p2] over the pairs with bias index idx of the tile's nw windows, in a fixed order (slot, then l2 ascending)
__device__ __forceinline__ void pack_bias_partial(const float* ds, const Win& g, int nw, float* __restrict__ part, int tid) {
  const int w = g.w, n = 2 * w - 1, L = g.L();
  for (int e = tid; e < g.T(); e += 256) {
    const int di = e / n - (w - 1), dj = e % n - (w - 1);      // i1 - i2, j1 - j2
    const int i0 = di < 0 ? -di : 0, i1 = di > 0 ? w - di : w, j0 = dj < 0 ? -dj : 0, j1 = dj > 0 ? w - dj : w;
    float s = 0.f;
    for (int slot = 0; slot < nw; ++slot)
      for (int i2 = i0; i2 < i1; ++i2)
        for (int j2 = j0; j2 < j1; ++j2) s += ds[(slot * L + (i2 + di) * w + j2 + dj) * DSROW + slot * L + i2 * w + j2];
    part[e] = s;
  }
}

// dq = scale * dS K (S^T orientation, one query per lane); the dS tile -> the bias partial
template <int D, bool DROP>
__global__ __launch_bounds__(256) void attn_window_packed_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                    const float* __restrict__ dout, float* __restrict__ dqkv, float* __restrict__ part, Pack pk,
                                                                    float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * TPL];      // K hi|lo, V hi|lo (natural), K^T hi|lo
  __shared__ float dsl[MK * DSROW];
  __shared__ int tok[MK], rel[MK], pos[MK];
  __shared__ uint32_t dbase[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  unsigned char* ldsKT = lds + 4 * KPLANE;
  const Win& gm = pk.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C, M = pk.live(tile);
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  pack_tables(pk, tile, b, h, tid, tok, rel, dbase, pos);
  load_bias<256>(table, gm, h, tid, bias);
  __syncthreads();
  stage_win<D, 256>(img, tok, C3, C + h * D, ldsK, ldsKT, tid);
  stage_win<D, 256>(img, tok, C3, 2 * C + h * D, ldsV, nullptr, tid);
  __syncthreads();
  const int p1 = wave * 16 + (lane & 15), t1 = tok[p1];
  bf16x8 qh[KS], ql[KS], dh[KS], dl[KS];
  load_row_frags<D>(img, t1 >= 0 ? t1 : HW, HW, C3, h, lane, scale, qh, ql);
  load_row_frags<D>(dout + (long)b * HW * C, t1 >= 0 ? t1 : HW, HW, C, h, lane, 1.f, dh, dl);
  f32x4 p[4], dp[4], o[DT];
  softmax_t<D>(ldsK, qh, ql, M, lane, PackTerm{rel[p1], rel, bias, gm.c0()}, p);
  if constexpr (DROP) {
    f32x4 f[4];
    pack_drop_factors_t(dr, dr.word(), p1, M, rel, dbase, pos, lane, f);
    ds_drop_t<D>(ldsV, dh, dl, lane, p, f, dp);
  } else {
    ds_t<D>(ldsV, dh, dl, lane, p, dp);            // dS^T: zero at the excluded keys (p = 0) and the padding queries (dO = 0)
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dsl[p1 * DSROW + 16 * t + 4 * g + r] = dp[t][r];
  zero_tiles(o);
  mul_trn<D>(dp, ldsKT, lane, o);                 // dQ^T[d][q] / scale
  if (t1 >= 0) store_o<D>(dqkv + ((long)b * HW + t1) * C3 + h * D + g * 4, o, scale);
  __syncthreads();
  pack_bias_partial(dsl, gm, M / gm.L(), part + (((long)b * gridDim.x + tile) * gm.heads + h) * gm.T(), tid);
}

// dV = P^T dO, dK = scale * dS^T Q over the tile's 64 query rows (S orientation: 4 queries per lane, the key on the lane): the text of
// attn_window_dkv_kernel with the packed term; the sum of the two waves IS dK / dV of the tile's keys.
template <int D, bool DROP>
__global__ __launch_bounds__(128) void attn_window_packed_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                     const float* __restrict__ dout, float* __restrict__ dqkv, Pack pk, float scale, Drop dr) {
  constexpr int KS = Geo<D>::KS, DT = Geo<D>::DT, KPLANE = Geo<D>::KPLANE, QPL = Geo<D>::QPL;
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * KPLANE + 2 * 4 * QPL];      // K, V natural (hi|lo each); per wave: dO^T hi|lo, Q^T hi|lo
  static_assert(2 * MK * D * 4 <= 4 * KPLANE, "the wave reduction reuses the K / V images");
  __shared__ int tok[MK], rel[MK], pos[MK];
  __shared__ uint32_t dbase[MK];
  __shared__ float bias[TMAX];
  unsigned char* ldsK = lds;
  unsigned char* ldsV = lds + 2 * KPLANE;
  const Win& gm = pk.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  unsigned char* myDO = lds + 4 * KPLANE + wave * 4 * QPL;
  unsigned char* myQ = myDO + 2 * QPL;
  const int tile = blockIdx.x, h = blockIdx.y, b = blockIdx.z, C = gm.heads * D, C3 = 3 * C, M = pk.live(tile), c0 = gm.c0();
  const long HW = (long)gm.H * gm.W;
  const float* img = qkv + (long)b * HW * C3;
  const float* db = dout + (long)b * HW * C;
  const uint32_t drop_seed = DROP ? dr.word() : 0u;
  pack_tables(pk, tile, b, h, tid, tok, rel, dbase, pos);
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
    // transposed per-wave images for the dV / dK products: element (d = 32 ks + 8 g + j, query row 16 u + (lane & 15))
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
  // S[q][key] and dP[q][key]: query rows base + 16 u + 4 g + r on the rows, key row 16 t + (lane & 15) on the lane
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
      for (int r = 0; r < 4; ++r) s[u][t][r] = key < M ? pack_logit(s[u][t][r], rel[base + 16 * u + 4 * g + r], rk, c0, bias) : NEG;
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
        s[u][t][r] = 16 * t + (lane & 15) < M ? expf(s[u][t][r] - mx) : 0.f;
        den += s[u][t][r];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) den += __shfl_xor(den, o);
      const float inv = 1.f / den;
      float delta = 0.f;
      const int q = base + 16 * u + 4 * g + r;
      const bool live = q < M;                              // padding queries contribute nothing (their q / dO were zeroed; P is not zero)
      const int rq = rel[q];
      const uint32_t e0 = dbase[q];
      float fm[4];                                          // DROP: M / (1 - p) of (this query, the lane's key of tile t)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        s[u][t][r] *= inv;                                 // P
        if constexpr (DROP) {
          const int key = 16 * t + (lane & 15);
          fm[t] = live && key < M && ((rq ^ rel[key]) >> 20) == 0 ? dr(drop_seed, e0 + (uint32_t)pos[key]) : 1.f;
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
  // add the two waves in a fixed order (wave 0 stores, wave 1 adds): [2][64 keys][D d]; the K / V images are dead by now
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
            float* pk_ = red + (0 * MK + key) * D + d;
            float* pv = red + (1 * MK + key) * D + d;
            *pk_ = w == 0 ? accK[dt][t][r] : *pk_ + accK[dt][t][r];
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

// the rule an argument breaks, or null
const char* broken_rule(int B, int H, int W, int heads, int head_dim, int window, int shift, int math) {
  if (window < 2 || window > PACK_MAX_WINDOW) return "window must be 2, 3 or 4 (at most 16 tokens per window; larger windows: hpfg_attn_window_*)";
  if (H <= 0 || W <= 0 || H % window || W % window) return "map sides must be positive multiples of the window";
  if (shift != 0 && shift != window / 2) return "shift must be 0 or window / 2";
  if (head_dim != 32 && head_dim != 64) return "head dim must be 32 or 64";
  if (B <= 0 || B > 65535 || heads <= 0 || heads > 65535 || (long)H * W > (1L << 30)) return "1 <= B, heads <= 65535 and H W <= 2^30";
  if (math != HPFG_MATH_F32 && math != HPFG_MATH_BF16X3) return "math must be 0 (f32) or 1 (bf16x3)";
  return nullptr;
}

#define PACKED_MSG "%s: %s (got B %d, map %d x %d, %d heads, head dim %d, window %d, shift %d, math %d)"
#define PACKED_CHECK(who, ptrs)                                                                    \
  do {                                                                                             \
    const char* rule = (ptrs) ? broken_rule(B, H, W, heads, head_dim, window, shift, math) : "null pointer"; \
    HPFG_ARG_CHECK(!rule, PACKED_MSG, who, rule, B, H, W, heads, head_dim, window, shift, math); \
  } while (0)

Pack make_pack(int H, int W, int heads, int window, int shift) {
  Pack pk{Win{H, W, window, shift, heads}, MK / (window * window), 0};
  pk.tiles = (pk.g.nwin() + pk.P - 1) / pk.P;
  return pk;
}

template <int D, bool DROP>
void launch_fwd(const float* qkv, const float* table, float* out, int B, const Pack& pk, float scale, const Drop& dr, hipStream_t st) {
  hipLaunchKernelGGL((attn_window_packed_fwd_kernel<D, DROP>), dim3(pk.tiles, pk.g.heads, B), dim3(256), 0, st, qkv, table, out, pk, scale, dr);
}

template <int D, bool DROP>
void launch_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dbias, float* part, int B, const Pack& pk, float scale,
                const Drop& dr, hipStream_t st) {
  const dim3 grid(pk.tiles, pk.g.heads, B);
  hipLaunchKernelGGL((attn_window_packed_dq_kernel<D, DROP>), grid, dim3(256), 0, st, qkv, table, dout, dqkv, part, pk, scale, dr);
  hipLaunchKernelGGL((attn_window_packed_dkv_kernel<D, DROP>), grid, dim3(128), 0, st, qkv, table, dout, dqkv, pk, scale, dr);
  hipLaunchKernelGGL(attn_window_dbias_sum_kernel, dim3((pk.g.heads * pk.g.T() + 63) / 64), dim3(256), 0, st, part, dbias, B * pk.tiles, pk.g.heads,
                     pk.g.T());
}

}  // namespace

#define PACKED_DROP_MSG "%s: bad dropout args (0 <= p < 1, B nW heads L^2 < 2^32 mask elements; got p %g)"

// per-workgroup bias partials: one [heads][T] slab per (image, tile); HPFG_MATH_F32: the scratch of hpfg_attn_window_bwd
extern "C" long hpfg_attn_window_packed_scratch_floats(int B, int H, int W, int heads, int head_dim, int window, int math) {
  const int shift = 0;
  if (const char* rule = broken_rule(B, H, W, heads, head_dim, window, shift, math)) {
    hpfg_set_error(PACKED_MSG, "attn_window_packed_scratch_floats", rule, B, H, W, heads, head_dim, window, shift, math);
    return -1;
  }
  if (math == HPFG_MATH_F32) return hpfg_attn_window_scratch_floats(B, H, W, heads, head_dim, window, math);
  const Pack pk = make_pack(H, W, heads, window, 0);
  return (long)B * pk.tiles * heads * pk.g.T();
}

// replaces reference model/swinunet.py:219-241 (the attention of WindowAttention.forward between qkv and proj, attn_drop included) together
// with :263-276's roll / window_partition / window_reverse / roll back, for window <= 4
extern "C" int hpfg_attn_window_packed_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window,
                                           int shift, float scale, int math, float p, uint32_t seed, const uint32_t* seed_dev, const uint8_t* mask,
                                           void* stream) {
  PACKED_CHECK("attn_window_packed_fwd", qkv && bias_table && out);
  const Pack pk = make_pack(H, W, heads, window, shift);
  HPFG_ARG_CHECK(p >= 0.f && p < 1.f && drop_elems(B, pk.g) < (1L << 32), PACKED_DROP_MSG, "attn_window_packed_fwd", (double)p);
  if (math == HPFG_MATH_F32)
    return hpfg_attn_window_drop_fwd(qkv, bias_table, out, B, H, W, heads, head_dim, window, shift, scale, math, p, seed, seed_dev, mask, stream);
  const hipStream_t st = (hipStream_t)stream;
  if (p == 0.f && !mask) {
    if (head_dim == 32) launch_fwd<32, false>(qkv, bias_table, out, B, pk, scale, Drop{}, st);
    else launch_fwd<64, false>(qkv, bias_table, out, B, pk, scale, Drop{}, st);
  } else {
    const Drop dr{mask, seed_dev, seed, hpfg_drop_threshold(p), 1.f / (1.f - p)};
    if (head_dim == 32) launch_fwd<32, true>(qkv, bias_table, out, B, pk, scale, dr, st);
    else launch_fwd<64, true>(qkv, bias_table, out, B, pk, scale, dr, st);
  }
  return hpfg_launch_status("attn_window_packed_fwd");
}

// replaces the autograd backward of the same lines: dqkv (every element written once) and the gradient of the bias table
extern "C" int hpfg_attn_window_packed_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B,
                                           int H, int W, int heads, int head_dim, int window, int shift, float scale, int math, float p, uint32_t seed,
                                           const uint32_t* seed_dev, const uint8_t* mask, void* stream) {
  PACKED_CHECK("attn_window_packed_bwd", qkv && bias_table && dout && dqkv && dbias && scratch);
  const Pack pk = make_pack(H, W, heads, window, shift);
  HPFG_ARG_CHECK(p >= 0.f && p < 1.f && drop_elems(B, pk.g) < (1L << 32), PACKED_DROP_MSG, "attn_window_packed_bwd", (double)p);
  if (math == HPFG_MATH_F32)
    return hpfg_attn_window_drop_bwd(qkv, bias_table, dout, dqkv, dbias, scratch, B, H, W, heads, head_dim, window, shift, scale, math, p, seed, seed_dev,
                                     mask, stream);
  const hipStream_t st = (hipStream_t)stream;
  if (p == 0.f && !mask) {
    if (head_dim == 32) launch_bwd<32, false>(qkv, bias_table, dout, dqkv, dbias, scratch, B, pk, scale, Drop{}, st);
    else launch_bwd<64, false>(qkv, bias_table, dout, dqkv, dbias, scratch, B, pk, scale, Drop{}, st);
  } else {
    const Drop dr{mask, seed_dev, seed, hpfg_drop_threshold(p), 1.f / (1.f - p)};
    if (head_dim == 32) launch_bwd<32, true>(qkv, bias_table, dout, dqkv, dbias, scratch, B, pk, scale, dr, st);
    else launch_bwd<64, true>(qkv, bias_table, dout, dqkv, dbias, scratch, B, pk, scale, dr, st);
  }
  return hpfg_launch_status("attn_window_packed_bwd");
}
