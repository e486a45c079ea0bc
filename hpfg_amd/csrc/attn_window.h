// What the two window-attention kernel families share: csrc/attn_window.hip (one window per workgroup, window^2 <= 64 keys) and
// csrc/attn_window_packed.hip (64 / window^2 windows of at most 16 tokens per workgroup).  The window geometry, the logit term (bias + mask),
// the staging through a token table, the dropout rule of the probabilities and the fixed-order sum of the bias partials are one text here;
// each file's own is its position table (which token and which window a tile row is) and its kernels.
#pragma once
#include "attn_core.h"

namespace {

constexpr int TMAX = 225;                      // (2 w - 1)^2 at w = 8
constexpr int DSROW = 65;                      // floats per row of the [64 l1][64 l2] dS tile
constexpr float MASKED = -100.0f;              // reference model/swinunet.py:204

struct Win {
  int H, W, w, s, heads;
  __device__ __host__ int L() const { return w * w; }
  __device__ __host__ int T() const { return (2 * w - 1) * (2 * w - 1); }
  __device__ __host__ int c0() const { return 2 * w * (w - 1); }
  __device__ __host__ int nwin() const { return (H / w) * (W / w); }
};

template <int NT>
__device__ __forceinline__ void load_bias(const float* __restrict__ table, const Win& g, int h, int tid, float* bias) {
  for (int e = tid; e < g.T(); e += NT) bias[e] = table[(long)e * g.heads + h];
}

// bias + mask of the logit (query word rq, key word rk)
__device__ __forceinline__ float logit_add(float sc, int rq, int rk, int c0, const float* bias) {
  const float m = (rq >> 16) != (rk >> 16) ? MASKED : 0.f;
  return (sc + bias[(rq & 0xFFFF) - (rk & 0xFFFF) + c0]) + m;
}

// stage_kv of attn_core.h with the window's token table: channels [coff, coff + D) of the tokens tok[0..63] of image base `img` ([HW][C3])
template <int D, int NT>
__device__ __forceinline__ void stage_win(const float* __restrict__ img, const int* tok, int C3, int coff, unsigned char* nat, unsigned char* trn, int tid) {
  constexpr int KROW = Geo<D>::KROW, KPLANE = Geo<D>::KPLANE, TPL = Geo<D>::TPL;
#pragma unroll
  for (int chunk = tid; chunk < MK * D / 8; chunk += NT) {
    const int key = chunk / (D / 8), d0 = (chunk % (D / 8)) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int t = tok[key];
    if (t >= 0) {
      const float* p = img + (long)t * C3 + coff + d0;
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

// ---- dropout of the probabilities (WindowAttention.attn_drop, reference model/swinunet.py:237): the DROP instantiations of the kernels ------
//   out = (P .* M / (1 - p)) V,   dP = (dO V^T) .* M / (1 - p),   dS = P .* (dP - rowsum(P .* dP)),   dV = (P .* M / (1 - p))^T dO
// Element e = (((b nW + win) heads + h) L + l1) L + l2 with L = w^2 unpadded: the flat index of the reference's attn tensor [B nW, heads, L, L]
// in its rolled, window-partitioned order.  keep(e) is a byte of an explicit mask in that layout or hpfg_keep(e, seed + *seed_dev, threshold) of
// common.h, the rule of the HpfgAct dropout.  Only pairs of valid positions are looked up: the padding keys keep their exact zeros and the
// padding queries contribute nothing, as without dropout.  DROP = false compiles to the kernels as they were.
struct Drop {
  const uint8_t* mask;
  const uint32_t* seed_dev;
  uint32_t seed, thresh;
  float inv_keep;
  __device__ __forceinline__ uint32_t word() const { return seed + (seed_dev ? *seed_dev : 0u); }
  __device__ __forceinline__ float operator()(uint32_t sd, uint32_t e) const {
    const bool keep = mask ? mask[e] != 0 : hpfg_keep(e, sd, thresh);
    return keep ? inv_keep : 0.f;
  }
};

// first element of the [L][L] tile of (image b, window win, head h)
__device__ __forceinline__ uint32_t drop_base(const Win& g, int b, int nwin, int win, int h) {
  return (uint32_t)((b * nwin + win) * g.heads + h) * (uint32_t)(g.L() * g.L());
}

// ds_t of attn_core.h with dP masked before the row sum.  The masked dP is a rounded product of its own (contraction off): fused into the
// `dp - delta` below, dS would take the unrounded dP .* f while delta summed the rounded one, and a row whose probability sits on one kept
// key (dS = 0: every other key behind the mask's -100) came out at the product's rounding error, 1e-7 |dP|, instead of 0.
template <int D>
__device__ __forceinline__ void ds_drop_t(const unsigned char* ldsV, const bf16x8 (&dh)[Geo<D>::KS], const bf16x8 (&dl)[Geo<D>::KS], int lane,
                                          const f32x4 (&p)[4], const f32x4 (&f)[4], f32x4 (&dp)[4]) {
  float delta = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tile_t<D>(ldsV, t, dh, dl, lane, dp[t]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      {
#pragma clang fp contract(off)
        dp[t][r] = dp[t][r] * f[t][r];
      }
      delta += p[t][r] * dp[t][r];
    }
  }
  delta += __shfl_xor(delta, 16);
  delta += __shfl_xor(delta, 32);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dp[t][r] = p[t][r] * (dp[t][r] - delta);
}

// dbias[idx][h] = sum over the workgroups of part[wg][h][idx]: four contiguous slices of the workgroups, each added in order, then
// ((0 + 1) + 2) + 3
__global__ __launch_bounds__(256) void attn_window_dbias_sum_kernel(const float* __restrict__ part, float* __restrict__ dbias, int nwg, int heads, int T) {
  __shared__ float red[4][64];
  const int tid = threadIdx.x, col = tid & 63, sl = tid >> 6, n = heads * T, e = blockIdx.x * 64 + col;
  const int per = (nwg + 3) / 4, k0 = sl * per, k1 = k0 + per < nwg ? k0 + per : nwg;
  float s = 0.f;
  if (e < n)
    for (int k = k0; k < k1; ++k) s += part[(long)k * n + e];
  red[sl][col] = s;
  __syncthreads();
  if (sl == 0 && e < n) dbias[(long)(e % T) * heads + e / T] = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
}

// elements of the [B nW, heads, L, L] probability tensor the dropout draws over; they are indexed with 32 bits
inline long drop_elems(int B, const Win& g) { return (long)B * g.nwin() * g.heads * g.L() * g.L(); }

}  // namespace
