// Cubic B-spline resize of a volume's slices on the device: scipy.ndimage.zoom(slice, (H/h, W/w), order=3) of the reference's Synapse
// evaluation (val.py:243), [S,h,w] -> [S,H,W] fp32, every slice in one call.
//
// Spline prefilter (pole z = sqrt(3) - 2, mirror boundaries) and 4-tap interpolation are both linear and separable, so one output sample of
// one axis is a fixed linear form of its input line.  The prefilter's impulse response decays as |z|^k (below 1e-9 at k = 16), so that form
// has HPFG_RESIZE_TAPS = 4 + 2 * 16 coefficients worth keeping, around the sample's position; the caller derives them per axis on the host
// (fp64: closed-form mirror start, both recursions, B-spline weights, scipy's own validity of the last coordinate) and ships them as the
// axis' tap table.  The device work is then two banded passes without any dependent chain along a line:
//   rows:  tmp[s][O][x] = sum_t wy[O][t] * src[s][first_y[O] + t][x]      adjacent lanes = adjacent x (16-byte loads / stores), wave-uniform O
//   cols:  dst[s][O][X] = sum_t wx[X][t] * tmp[s][O][first_x[X] + t]      rows staged in LDS by coalesced loads; a lane owns one X
// The axis-0 pass runs first: the axis-1 pass then works on the (usually smaller) [S,H,w] intermediate, which lives in the caller's scratch.
#include "common.h"

#define TAPS HPFG_RESIZE_TAPS
constexpr int RESIZE_RY = 8;          // output rows per wave of the row pass: 8 neighbouring windows share most of their input rows
constexpr int RESIZE_UJ = 4;          // input rows of the row pass requested before the first is used
constexpr int RESIZE_XT = 256;        // output columns per workgroup of the column pass (one per lane)
constexpr int RESIZE_MAX_ROWS = 16;   // rows per workgroup of the column pass (LDS: rows x staged span)
constexpr int RESIZE_LDS_BYTES = 48 * 1024;
constexpr int RESIZE_MAX_AXIS = 8192;

template <int VEC>
struct ResizeVec;
template <>
struct ResizeVec<1> {
  typedef float T;
};
template <>
struct ResizeVec<4> {
  typedef f32x4 T;
};

// first[o] of a tap table, forced into the range the kernels may touch whatever the table holds: -1 (output is 0) or [0, n_in - teff]
__device__ __forceinline__ int resize_first(const float* __restrict__ taps, int n_out, int o, int n_in, int teff) {
  const int s = reinterpret_cast<const int*>(taps + (long)TAPS * n_out)[o];
  return s < 0 ? -1 : (s > n_in - teff ? n_in - teff : s);
}

// grid (column tiles of 64 * VEC, groups of RESIZE_RY output rows, slices), one wave per workgroup
template <int VEC>
__global__ __launch_bounds__(64) HPFG_NO_PK_F32 void resize_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                                        int h, int w, int H) {
  typedef typename ResizeVec<VEC>::T V;
  const int col = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const int o0 = blockIdx.y * RESIZE_RY;
  const int teff = TAPS < h ? TAPS : h;
  int st[RESIZE_RY], lo = h, hi = 0;
#pragma unroll
  for (int r = 0; r < RESIZE_RY; ++r) {
    st[r] = o0 + r < H ? resize_first(taps, H, o0 + r, h, teff) : -1;
    if (st[r] >= 0) {
      lo = st[r] < lo ? st[r] : lo;
      hi = st[r] + teff > hi ? st[r] + teff : hi;
    }
  }
  if (col >= w) return;
  const float* p = src + (long)blockIdx.z * h * w + col;
  V acc[RESIZE_RY];
#pragma unroll
  for (int r = 0; r < RESIZE_RY; ++r) acc[r] = V(0.f);
  for (int j = lo; j < hi; j += RESIZE_UJ) {          // the union of the group's windows: each input row is loaded once
    V a[RESIZE_UJ];
#pragma unroll
    for (int u = 0; u < RESIZE_UJ; ++u) a[u] = *reinterpret_cast<const V*>(p + (long)(j + u < hi ? j + u : hi - 1) * w);      // all in flight together
#pragma unroll
    for (int u = 0; u < RESIZE_UJ; ++u) {
#pragma unroll
      for (int r = 0; r < RESIZE_RY; ++r) {          // wave-uniform weight, 0 outside row r's window: no branch between the multiply-adds
        const int t = j + u - st[r];
        const bool in = st[r] >= 0 && (unsigned)t < (unsigned)teff && j + u < hi;
        const float wgt = taps[(long)(o0 + r < H ? o0 + r : 0) * TAPS + (in ? t : 0)];
        acc[r] += (in ? wgt : 0.f) * a[u];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RESIZE_RY; ++r)
    if (o0 + r < H) *reinterpret_cast<V*>(dst + ((long)blockIdx.z * H + o0 + r) * w + col) = st[r] >= 0 ? acc[r] : V(0.f);
}

// grid (groups of `rows_pb` rows of the [rows_total = S * H][w] intermediate, tiles of RESIZE_XT output columns); dynamic LDS rows_pb * stride floats
template <int VEC>
__global__ __launch_bounds__(RESIZE_XT) HPFG_NO_PK_F32 void resize_cols_kernel(const float* __restrict__ tmp, float* __restrict__ dst, const float* __restrict__ taps,
                                                                               long rows_total, int w, int W, int stride, int rows_pb) {
  typedef typename ResizeVec<VEC>::T V;
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int span[2];
  const int tid = threadIdx.x, X = blockIdx.y * RESIZE_XT + tid;
  const int teff = TAPS < w ? TAPS : w;
  const int s = X < W ? resize_first(taps, W, X, w, teff) : -1;
  if (tid == 0) {
    span[0] = w;
    span[1] = 0;
  }
  __syncthreads();
  if (s >= 0) {
    atomicMin(&span[0], s);
    atomicMax(&span[1], s + teff);
  }
  __syncthreads();
  const long row0 = (long)blockIdx.x * rows_pb;
  const int nrows = rows_total - row0 < rows_pb ? (int)(rows_total - row0) : rows_pb;
  if (span[1] == 0) {          // no valid output column in this tile
    if (X < W)
      for (int r = 0; r < nrows; ++r) dst[(row0 + r) * W + X] = 0.f;
    return;
  }
  const int c0 = span[0] / VEC * VEC;          // first staged column (16-byte aligned in the VEC = 4 form: w % 4 == 0)
  int c1 = (span[1] + VEC - 1) / VEC * VEC;    // <= w, a multiple of VEC
  if (c1 - c0 > stride) c1 = c0 + stride;      // (only a table that breaks the caller's span bound gets here)
  const int nq = (c1 - c0) / VEC;
  for (int i = tid; i < nrows * nq; i += RESIZE_XT) {
    const int r = i / nq, q = i - r * nq;
    *reinterpret_cast<V*>(tile + r * stride + q * VEC) = *reinterpret_cast<const V*>(tmp + (row0 + r) * w + c0 + q * VEC);
  }
  float wt[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; t += 4) {
    const f32x4 v = s >= 0 ? *reinterpret_cast<const f32x4*>(taps + (long)X * TAPS + t) : f32x4(0.f);
    wt[t] = v[0], wt[t + 1] = v[1], wt[t + 2] = v[2], wt[t + 3] = v[3];
  }
  __syncthreads();
  if (X >= W) return;
  int base = s >= 0 ? s - c0 : 0;
  if (base > c1 - c0 - teff) base = c1 - c0 - teff;
  if (teff == TAPS) {
    for (int r = 0; r < nrows; ++r) {
      const float* line = tile + r * stride + base;
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < TAPS; ++t) acc += wt[t] * line[t];
      dst[(row0 + r) * W + X] = s >= 0 ? acc : 0.f;
    }
  } else {          // rows shorter than the window (w < HPFG_RESIZE_TAPS): nothing is staged beyond them
    for (int r = 0; r < nrows; ++r) {
      const float* line = tile + r * stride + base;
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < TAPS; ++t)
        if (t < teff) acc += wt[t] * line[t];
      dst[(row0 + r) * W + X] = s >= 0 ? acc : 0.f;
    }
  }
}

// floats per staged row of the column pass: the widest span of input columns that RESIZE_XT neighbouring outputs can tap (their first taps
// lie within (RESIZE_XT - 1) * (w - 1) / (W - 1) + 1 of each other), never more than the row, plus the alignment slack; a multiple of 4
static int resize_stride(int w, int W) {
  long span = ((long)(RESIZE_XT - 1) * (w - 1) + (W - 2)) / (W - 1) + 1 + TAPS;
  if (span > w) span = w;
  if (span < TAPS) span = TAPS;
  return (int)((span + 3 + 3) / 4 * 4);
}

static bool resize_dims_ok(int S, int h, int w, int H, int W) {
  return S >= 1 && S <= 65535 && h >= 2 && w >= 2 && H >= 2 && W >= 2 && h <= RESIZE_MAX_AXIS && w <= RESIZE_MAX_AXIS && H <= RESIZE_MAX_AXIS &&
         W <= RESIZE_MAX_AXIS;
}

extern "C" long hpfg_resize_cubic_scratch_bytes(int S, int h, int w, int H, int W) {
  if (!resize_dims_ok(S, h, w, H, W)) return -1;
  return ((long)S * H * w * (long)sizeof(float) + 15) / 16 * 16;
}

extern "C" int hpfg_resize_cubic(const float* src, int S, int h, int w, float* dst, int H, int W, const float* taps_y, const float* taps_x,
                                 void* scratch, long scratch_bytes, void* stream) {
  HPFG_ARG_CHECK(src && dst && taps_y && taps_x && scratch, "resize_cubic: null pointer");
  HPFG_ARG_CHECK(resize_dims_ok(S, h, w, H, W), "resize_cubic: [%d,%d,%d] -> [%d,%d]: every axis needs 2 .. %d samples, S 1 .. 65535", S, h, w, H, W,
                 RESIZE_MAX_AXIS);
  HPFG_ARG_CHECK(scratch_bytes >= hpfg_resize_cubic_scratch_bytes(S, h, w, H, W), "resize_cubic: scratch of %ld bytes, %ld needed", scratch_bytes,
                 hpfg_resize_cubic_scratch_bytes(S, h, w, H, W));
  HPFG_ARG_CHECK((uintptr_t)taps_x % 16 == 0 && (uintptr_t)taps_y % 4 == 0 && (uintptr_t)scratch % 4 == 0, "resize_cubic: misaligned table or scratch");
  float* tmp = (float*)scratch;
  const bool vec = w % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)tmp % 16 == 0;
  const int stride = resize_stride(w, W);
  int rows_pb = RESIZE_LDS_BYTES / (stride * (int)sizeof(float));
  rows_pb = rows_pb > RESIZE_MAX_ROWS ? RESIZE_MAX_ROWS : rows_pb;
  HPFG_ARG_CHECK(rows_pb >= 1, "resize_cubic: a staged row of %d floats does not fit the LDS", stride);
  const long rows_total = (long)S * H;
  const dim3 grid_r((w + 64 * (vec ? 4 : 1) - 1) / (64 * (vec ? 4 : 1)), (H + RESIZE_RY - 1) / RESIZE_RY, S);
  const dim3 grid_c((unsigned)((rows_total + rows_pb - 1) / rows_pb), (W + RESIZE_XT - 1) / RESIZE_XT);
  const size_t lds = (size_t)rows_pb * stride * sizeof(float);
  if (vec) {
    hipLaunchKernelGGL(resize_rows_kernel<4>, grid_r, dim3(64), 0, (hipStream_t)stream, src, tmp, taps_y, h, w, H);
    hipLaunchKernelGGL(resize_cols_kernel<4>, grid_c, dim3(RESIZE_XT), lds, (hipStream_t)stream, tmp, dst, taps_x, rows_total, w, W, stride, rows_pb);
  } else {
    hipLaunchKernelGGL(resize_rows_kernel<1>, grid_r, dim3(64), 0, (hipStream_t)stream, src, tmp, taps_y, h, w, H);
    hipLaunchKernelGGL(resize_cols_kernel<1>, grid_c, dim3(RESIZE_XT), lds, (hipStream_t)stream, tmp, dst, taps_x, rows_total, w, W, stride, rows_pb);
  }
  return hpfg_launch_status("resize_cubic");
}
