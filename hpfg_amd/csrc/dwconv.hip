// Depthwise k x k convolution (k = 3, 5; pad k / 2, stride 1) WITHOUT an activation on NHWC tokens [B, H, W, C], forward and backward
// (reference model/uniformer.py: pos_embed of CBlock / SABlock, x + dwconv3x3(x), :91,102 and :125,135; CBlock.attn, the depthwise 5 x 5, :96,103).
//   forward   y  = (res ? res : 0) + dw_k(x) + bias
//   backward  dx = dw_k^T(dy) (+ dy), dwk[t][c] = sum_p dy[p][c] x[p + off(t)][c], dbias[c] = sum_p dy[p][c]
// One pass over the map each: a workgroup stages a DWT x DWT pixel tile plus its halo of DWQ channel quads in LDS ONCE (16-byte accesses along
// C; halo pixels are another workgroup's interior, so they reach HBM once and L2 otherwise) and every output takes its k^2 taps from there.
// Thread t <-> channel quad t % DWQ of the slice (blockIdx.y) and pixel lane t / DWQ: the quad is fixed, so the k^2 weights (forward, dx) or
// the k^2 + 1 gradient sums (dwk, dbias) stay in registers while the workgroup walks its tiles (blockIdx.x, grid-stride over B x tiles).
// dx is the forward kernel on dy with the taps mirrored.  The gradient sums leave the workgroup as one row of partials; a fixed-order
// reduction in double finishes them: no atomics, the same bits every run.
#include "common.h"

namespace {

constexpr int DWT = 16;          // tile edge in pixels
constexpr int DWQ = 8;           // channel quads per workgroup: 128 contiguous bytes of a pixel
constexpr int DWPL = 256 / DWQ;  // pixel lanes
constexpr int DW_MAX_BLOCKS = 512;

struct DwGeo {
  int B, H, W, C, Q, tiles_x, tiles_y;
  long items;      // B * tiles_y * tiles_x
};

__host__ __device__ inline DwGeo dw_geo(int B, int H, int W, int C) {
  DwGeo g;
  g.B = B, g.H = H, g.W = W, g.C = C, g.Q = C >> 2;
  g.tiles_x = (W + DWT - 1) / DWT;
  g.tiles_y = (H + DWT - 1) / DWT;
  g.items = (long)B * g.tiles_y * g.tiles_x;
  return g;
}

struct DwTile {
  int b, y0, x0, th, tw, ew;      // image, origin, interior extent, staged row pitch (tw + K - 1) in pixels
};

template <int K>
__device__ __forceinline__ DwTile dw_tile_of(const DwGeo& g, long item) {
  DwTile t;
  const int tx = (int)(item % g.tiles_x);
  const long r = item / g.tiles_x;
  t.b = (int)(r / g.tiles_y);
  t.y0 = (int)(r % g.tiles_y) * DWT;
  t.x0 = tx * DWT;
  t.th = g.H - t.y0 < DWT ? g.H - t.y0 : DWT;
  t.tw = g.W - t.x0 < DWT ? g.W - t.x0 : DWT;
  t.ew = t.tw + K - 1;
  return t;
}

// the tile's (th + K - 1) x (tw + K - 1) pixels of channel quads [q0, q0 + DWQ) -> LDS, zeros outside the map and past the last quad
template <int K>
__device__ __forceinline__ void dw_stage(const float* __restrict__ src, f32x4* tile, const DwGeo& g, const DwTile& t, int q0) {
  constexpr int P = K / 2;
  const int n = (t.th + K - 1) * t.ew * DWQ;
#pragma unroll 4
  for (int i = threadIdx.x; i < n; i += 256) {
    const int ql = i % DWQ, pix = i / DWQ;
    const int yy = t.y0 + pix / t.ew - P, xx = t.x0 + pix % t.ew - P;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (yy >= 0 && yy < g.H && xx >= 0 && xx < g.W && q0 + ql < g.Q)
      v = *reinterpret_cast<const f32x4*>(src + (((long)t.b * g.H + yy) * g.W + xx) * g.C + (q0 + ql) * 4);
    tile[i] = v;
  }
}

// out = (res ? res : 0) + sum_t wk[FLIP ? K^2 - 1 - t : t] * src[p + off(t)] + (bias ? bias : 0)
template <int K, bool FLIP>
__global__ __launch_bounds__(256) void dwconv_kernel(const float* __restrict__ src, const float* __restrict__ wk, const float* __restrict__ bias,
                                                     const float* res, float* __restrict__ out, int B, int H, int W, int C) {
  constexpr int KK = K * K, P = K / 2, E = DWT + K - 1;
  __shared__ f32x4 tile[E * E * DWQ];
  const DwGeo g = dw_geo(B, H, W, C);
  const int q0 = blockIdx.y * DWQ, ql = threadIdx.x % DWQ, pl = threadIdx.x / DWQ;
  const bool live = q0 + ql < g.Q;
  const int c = (live ? q0 + ql : q0) * 4;
  f32x4 wr[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) wr[t] = *reinterpret_cast<const f32x4*>(wk + (FLIP ? KK - 1 - t : t) * C + c);
  f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (bias) b4 = *reinterpret_cast<const f32x4*>(bias + c);
  const bool res_in_tile = res == src;      // x + dw(x), dy + dw^T(dy): the addend is the tile's own centre
  for (long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const DwTile t = dw_tile_of<K>(g, item);
    __syncthreads();      // (the previous tile's readers are done)
    dw_stage<K>(src, tile, g, t, q0);
    __syncthreads();
    if (!live) continue;
    for (int p = pl; p < t.th * t.tw; p += DWPL) {
      const int py = p / t.tw, px = p % t.tw;
      const f32x4* row = tile + (py * t.ew + px) * DWQ + ql;
      f32x4 a = b4;
#pragma unroll
      for (int dy = 0; dy < K; ++dy)
#pragma unroll
        for (int dx = 0; dx < K; ++dx) a += row[(dy * t.ew + dx) * DWQ] * wr[dy * K + dx];
      const long o = (((long)t.b * H + t.y0 + py) * W + t.x0 + px) * C + c;
      if (res) a += res_in_tile ? row[(P * t.ew + P) * DWQ] : *reinterpret_cast<const f32x4*>(res + o);
      *reinterpret_cast<f32x4*>(out + o) = a;
    }
  }
}

// part[blockIdx.x][t][c] = sum over the workgroup's pixels of dy[p][c] * x[p + off(t)][c] (t < K^2), and of dy[p][c] (t = K^2)
template <int K>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part, int B,
                                                           int H, int W, int C) {
  constexpr int KK = K * K, E = DWT + K - 1, NS = KK + 1;
  __shared__ f32x4 tile[E * E * DWQ];
  static_assert(E * E * DWQ * 4 >= 4 * NS * DWQ * 4, "the reduction reuses the tile's LDS");
  const DwGeo g = dw_geo(B, H, W, C);
  const int q0 = blockIdx.y * DWQ, ql = threadIdx.x % DWQ, pl = threadIdx.x / DWQ;
  const bool live = q0 + ql < g.Q;
  const int c = (live ? q0 + ql : q0) * 4;
  f32x4 acc[NS];
#pragma unroll
  for (int t = 0; t < NS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long item = blockIdx.x; item < g.items; item += gridDim.x) {
    const DwTile t = dw_tile_of<K>(g, item);
    __syncthreads();
    dw_stage<K>(x, tile, g, t, q0);
    __syncthreads();
    if (!live) continue;
    for (int p = pl; p < t.th * t.tw; p += DWPL) {
      const int py = p / t.tw, px = p % t.tw;
      const f32x4* row = tile + (py * t.ew + px) * DWQ + ql;
      const f32x4 d = *reinterpret_cast<const f32x4*>(dy + (((long)t.b * H + t.y0 + py) * W + t.x0 + px) * C + c);
      acc[KK] += d;
#pragma unroll
      for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[i * K + j] += d * row[(i * t.ew + j) * DWQ];
    }
  }
  // the 8 pixel lanes of a wave (lane bits 3..5) by shuffles, the 4 waves through LDS: one fixed order
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = acc[t][j];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      acc[t][j] = v;
    }
  __syncthreads();      // every tile reader is done: the LDS is free
  float* red = reinterpret_cast<float*>(tile);      // [4 waves][NS][DWQ * 4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < DWQ) {
#pragma unroll
    for (int t = 0; t < NS; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[(wave * NS + t) * (DWQ * 4) + lane * 4 + j] = acc[t][j];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < NS * DWQ * 4; o += 256) {
    const int t = o / (DWQ * 4), cc = o % (DWQ * 4);
    if (q0 * 4 + cc < C)
      part[((long)blockIdx.x * NS + t) * C + q0 * 4 + cc] = (red[(0 * NS + t) * (DWQ * 4) + cc] + red[(1 * NS + t) * (DWQ * 4) + cc]) +
                                                            (red[(2 * NS + t) * (DWQ * 4) + cc] + red[(3 * NS + t) * (DWQ * 4) + cc]);
  }
}

// dwk[o] (o < nw) / dbias[o - nw] = sum_i part[i][o], in double, fixed order (the col_reduce_kernel of tokens.hip with two destinations)
__global__ __launch_bounds__(64) void dwconv_reduce_kernel(const float* __restrict__ part, int nblk, int stride, int nw, float* __restrict__ dwk,
                                                           float* __restrict__ dbias) {
  const int o = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) a += (double)part[(long)i * stride + o];
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) a += __shfl_xor(a, s);
  if (threadIdx.x == 0) {
    if (o < nw) dwk[o] = (float)a;
    else dbias[o - nw] = (float)a;
  }
}

bool dw_shape_ok(int B, int H, int W, int C, int k) {
  return B > 0 && H > 0 && W > 0 && C >= 4 && C % 4 == 0 && (k == 3 || k == 5) && (long)B * H * W * C < (1L << 40);
}

}  // namespace

extern "C" int hpfg_dwconv_bwd_blocks(int B, int H, int W, int k) {
  if (B <= 0 || H <= 0 || W <= 0 || (k != 3 && k != 5)) return 0;
  const long items = dw_geo(B, H, W, 4).items;
  return (int)(items < DW_MAX_BLOCKS ? items : DW_MAX_BLOCKS);
}

extern "C" int hpfg_dwconv_fwd(const float* x, const float* wk, const float* bias, const float* res, float* y, int B, int H, int W, int C, int k,
                               void* stream) {
  HPFG_ARG_CHECK(x && wk && bias && y && y != x && y != res && dw_shape_ok(B, H, W, C, k),
                 "dwconv_fwd: bad args (k = 3 or 5, C %% 4 == 0, y apart from its inputs; got B %d H %d W %d C %d k %d)", B, H, W, C, k);
  const dim3 grid(hpfg_dwconv_bwd_blocks(B, H, W, k), (C / 4 + DWQ - 1) / DWQ);
  if (k == 3) hipLaunchKernelGGL((dwconv_kernel<3, false>), grid, dim3(256), 0, (hipStream_t)stream, x, wk, bias, res, y, B, H, W, C);
  else hipLaunchKernelGGL((dwconv_kernel<5, false>), grid, dim3(256), 0, (hipStream_t)stream, x, wk, bias, res, y, B, H, W, C);
  return hpfg_launch_status("dwconv_kernel");
}

extern "C" int hpfg_dwconv_bwd(const float* x, const float* wk, const float* dy, float* dx, int add_dy, float* dwk, float* dbias, float* partials, int B,
                               int H, int W, int C, int k, void* stream) {
  HPFG_ARG_CHECK(x && wk && dy && dx && dx != dy && dx != x && dwk && dbias && partials && dw_shape_ok(B, H, W, C, k),
                 "dwconv_bwd: bad args (k = 3 or 5, C %% 4 == 0, dx apart from its inputs; got B %d H %d W %d C %d k %d)", B, H, W, C, k);
  const int nblk = hpfg_dwconv_bwd_blocks(B, H, W, k), ns = k * k + 1;
  const dim3 grid(nblk, (C / 4 + DWQ - 1) / DWQ);
  const float* none = nullptr;
  const float* res = add_dy ? dy : none;
  if (k == 3) {
    hipLaunchKernelGGL((dwconv_kernel<3, true>), grid, dim3(256), 0, (hipStream_t)stream, dy, wk, none, res, dx, B, H, W, C);
    hipLaunchKernelGGL(dwconv_wgrad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, x, dy, partials, B, H, W, C);
  } else {
    hipLaunchKernelGGL((dwconv_kernel<5, true>), grid, dim3(256), 0, (hipStream_t)stream, dy, wk, none, res, dx, B, H, W, C);
    hipLaunchKernelGGL(dwconv_wgrad_kernel<5>, grid, dim3(256), 0, (hipStream_t)stream, x, dy, partials, B, H, W, C);
  }
  hipLaunchKernelGGL(dwconv_reduce_kernel, dim3(ns * C), dim3(64), 0, (hipStream_t)stream, partials, nblk, ns * C, (ns - 1) * C, dwk, dbias);
  return hpfg_launch_status("dwconv_bwd_kernel");
}
