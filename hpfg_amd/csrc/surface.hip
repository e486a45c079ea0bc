// HD95 of the evaluation on the device (val.py:376-387: medpy.metric.binary.hd95(pred == c, gt == c) per foreground class): the surface
// voxels of every class mask of both label volumes, and for every surface voxel the squared distance to the nearest surface voxel of the
// same class in the other volume.  With unit voxel spacing those squares are integers below 2^28, so the search below is exact: it gives
// the values scipy's distance_transform_edt holds at the same voxels (the square roots are taken on the host in fp64).
//
//   surface_scan_kernel<false>   counts the surface voxels per segment (seg = (c - 1) * 2 + side; side 0 = pred, 1 = gt)
//   surface_scan_kernel<true>    the same scan again, now writing the linear voxel index of every surface voxel into its segment of `points`
//                                (offsets = running sum of the host's counts; an atomic cursor per segment, so the order inside a segment
//                                is arbitrary -- nothing downstream depends on it)
//   surface_nearest_kernel       one thread owns one query point, the workgroup streams the partner segment through LDS in tiles of 256
//                                points (every lane reads the same 16-byte slot: a broadcast), integer d^2 = dz^2 + dy^2 + dx^2 from 24-bit
//                                multiplies, minimum by integer atomicMin (order independent).  All classes and both directions are one
//                                launch: a block looks its (segment, query block, target split) up in a table passed by value.
//   surface_sums_kernel          the exact sum of sqrt(d^2) over every searched segment, for ASD (val.py:109-122): integer atomics only
// A voxel of a mask is on its surface when one of its 2 * ndim face neighbours is outside the mask or outside the volume
// (mask ^ binary_erosion(mask, generate_binary_structure(ndim, 1)), border_value = 0).
#include "common.h"

#define SEGS HPFG_SURFACE_SEGS
constexpr int SURF_MAX_AXIS = 8192;          // 3 * 8191^2 < 2^28: d^2 and a 4-bit class tag share one 32-bit key
constexpr int SURF_TILE = 256;               // target points per LDS tile = query points per workgroup
constexpr int SURF_MIN_BLOCKS = 2048;        // a segment with fewer query blocks splits its targets over several workgroups
constexpr unsigned SURF_KEY_BIAS = 0x80000000u;

struct SurfCounts {
  unsigned n[SEGS];
};
struct SurfTable {
  unsigned off[SEGS + 1];          // first point of every segment (running sum of the counts)
  unsigned first[SEGS + 1];        // first workgroup of every segment's search
  unsigned tps[SEGS];              // target tiles per workgroup
  int nseg;
};

// segment of voxel i = (z, y, x) of `v` if it is a surface voxel of a foreground class, else -1
__device__ __forceinline__ int surface_seg(const uint8_t* __restrict__ v, long i, int z, int y, int x, int S, int h, int w, int C, int ndim, int side) {
  const int l = v[i];
  if (l == 0 || l >= C) return -1;
  const long hw = (long)h * w;
  bool s = x == 0 || v[i - 1] != l || x == w - 1 || v[i + 1] != l || y == 0 || v[i - w] != l || y == h - 1 || v[i + w] != l;
  if (!s && ndim == 3) s = z == 0 || v[i - hw] != l || z == S - 1 || v[i + hw] != l;
  return s ? (l - 1) * 2 + side : -1;
}

// grid: one thread per voxel.  COMPACT = false: counts[seg] += surface voxels.  COMPACT = true: points[off[seg] + k] = voxel index, k from
// the segment's cursor (one global atomic per workgroup and segment: ranks inside the workgroup come from LDS atomics); a segment never
// receives more than keep.n[seg] points, whatever the volumes hold.
template <bool COMPACT>
__global__ __launch_bounds__(256) void surface_scan_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, long n, int S, int h, int w,
                                                           int C, int ndim, unsigned* __restrict__ counts, SurfCounts keep, int* __restrict__ points) {
  __shared__ unsigned lcnt[SEGS], lbase[SEGS];
  const int tid = threadIdx.x;
  if (tid < SEGS) lcnt[tid] = 0;
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + tid;
  int sp = -1, sg = -1;
  unsigned rp = 0, rg = 0;
  if (i < n) {
    const int x = (int)(i % w), y = (int)((i / w) % h), z = (int)(i / ((long)h * w));
    sp = surface_seg(pred, i, z, y, x, S, h, w, C, ndim, 0);
    sg = surface_seg(gt, i, z, y, x, S, h, w, C, ndim, 1);
    if (sp >= 0) rp = atomicAdd(&lcnt[sp], 1u);
    if (sg >= 0) rg = atomicAdd(&lcnt[sg], 1u);
  }
  __syncthreads();
  if (tid < SEGS && lcnt[tid]) lbase[tid] = atomicAdd(&counts[tid], lcnt[tid]);
  if (!COMPACT) return;
  __syncthreads();
  unsigned off = 0;
  for (int s = 0; s < SEGS; ++s) {          // (uniform: the running sum of the kept counts up to this thread's two segments)
    if (s == sp && lbase[s] + rp < keep.n[s]) points[(long)off + lbase[s] + rp] = (int)i;
    if (s == sg && lbase[s] + rg < keep.n[s]) points[(long)off + lbase[s] + rg] = (int)i;
    off += keep.n[s];
  }
}

// grid: t.first[t.nseg] workgroups.  Segment s queries its partner s ^ 1; workgroup `local` of the segment owns query block local / splits and
// the target tiles [split * tps, (split + 1) * tps).  keys[off[s] + q] = min(keys, ((s >> 1) << 28 | d^2) ^ 2^31) as a signed integer: the
// caller filled keys with 0x7F bytes (above every key), and a signed sort of all keys is a sort by (class, d^2).
__global__ __launch_bounds__(SURF_TILE) void surface_nearest_kernel(const int* __restrict__ points, int* __restrict__ keys, SurfTable t, int h, int w) {
  __shared__ __attribute__((aligned(16))) int4 tile[SURF_TILE];
  const int tid = threadIdx.x;
  int s = 0;
  while (s + 1 < t.nseg && blockIdx.x >= t.first[s + 1]) ++s;
  const unsigned nq = t.off[s + 1] - t.off[s], t0 = t.off[s ^ 1], nt = t.off[(s ^ 1) + 1] - t0;
  const unsigned ntiles = (nt + SURF_TILE - 1) / SURF_TILE, tps = t.tps[s], splits = (ntiles + tps - 1) / tps;
  const unsigned local = blockIdx.x - t.first[s], qb = local / splits, split = local - qb * splits;
  const unsigned q = qb * SURF_TILE + tid;
  const unsigned tile0 = split * tps, tile1 = tile0 + tps < ntiles ? tile0 + tps : ntiles;
  const int hw = h * w;
  int qz = 0, qy = 0, qx = 0;
  if (q < nq) {
    const int p = points[(long)t.off[s] + q];
    qz = p / hw, qy = (p - qz * hw) / w, qx = p - qz * hw - qy * w;
  }
  unsigned best = 0x0FFFFFFFu;
  unsigned j = tile0 * SURF_TILE + tid;
  int nxt = j < nt ? points[(long)t0 + j] : 0;          // the next tile's point is requested before this tile is searched
  for (unsigned tl = tile0; tl < tile1; ++tl) {
    const int tz = nxt / hw, ty = (nxt - tz * hw) / w;
    tile[tid] = make_int4(tz, ty, nxt - tz * hw - ty * w, 0);
    __syncthreads();
    j += SURF_TILE;
    nxt = (tl + 1 < tile1 && j < nt) ? points[(long)t0 + j] : 0;
    const unsigned left = nt - tl * SURF_TILE;
    if (left >= SURF_TILE) {
#pragma unroll 8
      for (int k = 0; k < SURF_TILE; ++k) {
        const int4 c = tile[k];
        const int dz = qz - c.x, dy = qy - c.y, dx = qx - c.z;
        const unsigned d = (unsigned)(__mul24(dz, dz) + __mul24(dy, dy) + __mul24(dx, dx));
        best = d < best ? d : best;
      }
    } else {          // the ragged last tile of the segment
      for (int k = 0; k < (int)left; ++k) {
        const int4 c = tile[k];
        const int dz = qz - c.x, dy = qy - c.y, dx = qx - c.z;
        const unsigned d = (unsigned)(__mul24(dz, dz) + __mul24(dy, dy) + __mul24(dx, dx));
        best = d < best ? d : best;
      }
    }
    __syncthreads();
  }
  if (q < nq) atomicMin(&keys[(long)t.off[s] + q], (int)((((unsigned)(s >> 1) << 28) | best) ^ SURF_KEY_BIAS));
}

// ASD of the evaluation (val.py:109-122: medpy.metric.binary.asd = the mean of one direction's surface distances): the sum of sqrt(d^2) over
// every segment's keys, exactly.  The order of the points inside a segment is arbitrary (the compaction's atomic cursor), so nothing that
// rounds may be added up: x = sqrt((double)d^2) is 0 or in [1, 2^14), hence a multiple of 2^-52, and splits without loss into
// hi = rint(x * 2^19) <= 2^33 and lo = (x - hi * 2^-19) * 2^52, an integer with |lo| <= 2^32.  Both are added with integer atomics (LDS per
// workgroup, then one global atomic per workgroup and touched word): associative, so the totals are the same bits in any order, and
// 2^31 - 1 points overflow neither word.  sum = hi * 2^-19 + lo * 2^-52; the host divides by the count in rational arithmetic.
constexpr double SURF_SUM_HI = 524288.0;                    // 2^19
constexpr double SURF_SUM_LO = 4503599627370496.0;          // 2^52

struct SurfSumTable {
  unsigned off[SEGS + 1];          // first key of every segment (running sum of the counts)
  unsigned live;                   // bit s: segment s is summed (searched: neither it nor its partner is empty)
};

// grid: one thread per key.  sums[2 s] += hi, sums[2 s + 1] += lo (two's complement) over the keys of every live segment s.
__global__ __launch_bounds__(256) void surface_sums_kernel(const int* __restrict__ keys, SurfSumTable t, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long lsum[2 * SEGS];
  const int tid = threadIdx.x;
  if (tid < 2 * SEGS) lsum[tid] = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256u + tid;          // (below 2^31 + 256)
  if (i < t.off[SEGS]) {
    int s = 0;          // off is non-decreasing: the segment of key i is the number of boundaries off[1 .. SEGS-1] at or below i
#pragma unroll
    for (int k = 1; k < SEGS; ++k) s += i >= t.off[k] ? 1 : 0;
    if ((t.live >> s) & 1u) {
#pragma clang fp contract(off)
      const unsigned d2 = ((unsigned)keys[i] ^ SURF_KEY_BIAS) & 0x0FFFFFFFu;
      const double x = sqrt((double)d2);
      const double hi = rint(x * SURF_SUM_HI);
      const double lo = (x - hi * (1.0 / SURF_SUM_HI)) * SURF_SUM_LO;
      atomicAdd(&lsum[2 * s], (unsigned long long)hi);
      atomicAdd(&lsum[2 * s + 1], (unsigned long long)(long long)lo);
    }
  }
  __syncthreads();
  if (tid < 2 * SEGS && lsum[tid]) atomicAdd(&sums[tid], lsum[tid]);
}

static int surface_dims_check(const char* who, int S, int h, int w, int C, int ndim) {
  HPFG_ARG_CHECK(ndim == 2 || ndim == 3, "%s: ndim %d (2 or 3)", who, ndim);
  HPFG_ARG_CHECK(C >= 2 && C <= 16, "%s: %d classes (2 .. 16)", who, C);
  HPFG_ARG_CHECK(S >= 1 && h >= 1 && w >= 1 && S <= SURF_MAX_AXIS && h <= SURF_MAX_AXIS && w <= SURF_MAX_AXIS, "%s: [%d,%d,%d]: every axis needs 1 .. %d voxels",
                 who, S, h, w, SURF_MAX_AXIS);
  HPFG_ARG_CHECK(ndim == 3 || S == 1, "%s: a 2-D volume has S = 1, not %d", who, S);
  HPFG_ARG_CHECK((long)S * h * w < (1L << 31), "%s: [%d,%d,%d] has 2^31 voxels or more", who, S, h, w);
  return 0;
}

// total points of the segments of C classes, or -1 (a count in a segment no class owns, 2^31 points or more)
static long surface_total(const unsigned* counts_host, int C) {
  long n = 0;
  for (int s = 0; s < SEGS; ++s) {
    if (s >= 2 * (C - 1) && counts_host[s]) return -1;
    n += counts_host[s];
  }
  return n < (1L << 31) ? n : -1;
}

static long surface_pad(long bytes) { return (bytes + 255) / 256 * 256; }

extern "C" long hpfg_surface_workspace_bytes(int C, long n_points) {
  if (C < 2 || C > 16 || n_points < 0 || n_points >= (1L << 31)) return -1;
  return 256 + 2 * surface_pad(n_points * 4);
}

extern "C" int hpfg_surface_counts(const uint8_t* pred, const uint8_t* gt, int S, int h, int w, int C, int ndim, unsigned int* counts, void* stream) {
  HPFG_ARG_CHECK(pred && gt && counts, "surface_counts: null pointer");
  if (surface_dims_check("surface_counts", S, h, w, C, ndim)) return -1;
  const long n = (long)S * h * w;
  hipError_t e = hipMemsetAsync(counts, 0, SEGS * sizeof(unsigned), (hipStream_t)stream);
  HPFG_ARG_CHECK(e == hipSuccess, "surface_counts: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(surface_scan_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, gt, n, S, h, w, C, ndim, counts,
                     SurfCounts(), (int*)nullptr);
  return hpfg_launch_status("surface_counts");
}

extern "C" int hpfg_surface_distances(const uint8_t* pred, const uint8_t* gt, int S, int h, int w, int C, int ndim, const unsigned int* counts_host,
                                      void* workspace, long workspace_bytes, void* stream) {
  HPFG_ARG_CHECK(pred && gt && counts_host && workspace, "surface_distances: null pointer");
  if (surface_dims_check("surface_distances", S, h, w, C, ndim)) return -1;
  const long total = surface_total(counts_host, C), n = (long)S * h * w;
  HPFG_ARG_CHECK(total >= 0, "surface_distances: counts beyond the %d segments of %d classes, or 2^31 points or more", 2 * (C - 1), C);
  HPFG_ARG_CHECK(workspace_bytes >= hpfg_surface_workspace_bytes(C, total), "surface_distances: workspace of %ld bytes, %ld needed", workspace_bytes,
                 hpfg_surface_workspace_bytes(C, total));
  HPFG_ARG_CHECK((uintptr_t)workspace % 16 == 0, "surface_distances: misaligned workspace");
  SurfCounts keep;
  SurfTable t;
  t.nseg = 2 * (C - 1);
  t.off[0] = t.first[0] = 0;
  long blocks = 0;
  for (int s = 0; s < SEGS; ++s) {
    HPFG_ARG_CHECK(counts_host[s] <= (unsigned long)n, "surface_distances: segment %d holds %u points, the volume %ld voxels", s, counts_host[s], n);
    keep.n[s] = counts_host[s];
    t.off[s + 1] = t.off[s] + counts_host[s];
  }
  for (int s = 0; s < SEGS; ++s) {          // nothing is launched for a segment that is empty or whose partner is
    const long nq = counts_host[s], nt = counts_host[s ^ 1];
    t.tps[s] = 1;
    if (s < t.nseg && nq > 0 && nt > 0) {
      const long qblocks = (nq + SURF_TILE - 1) / SURF_TILE, ntiles = (nt + SURF_TILE - 1) / SURF_TILE;
      long splits = (SURF_MIN_BLOCKS + qblocks - 1) / qblocks;
      splits = splits > ntiles ? ntiles : splits;
      const long tps = (ntiles + splits - 1) / splits;
      t.tps[s] = (unsigned)tps;
      blocks += qblocks * ((ntiles + tps - 1) / tps);
    }
    HPFG_ARG_CHECK(blocks < (1L << 31), "surface_distances: %ld workgroups", blocks);
    t.first[s + 1] = (unsigned)blocks;
  }
  unsigned* cursors = (unsigned*)workspace;
  int* keys = (int*)((char*)workspace + 256);
  int* points = (int*)((char*)workspace + 256 + surface_pad(total * 4));
  if (total == 0) return 0;
  hipError_t e = hipMemsetAsync(cursors, 0, SEGS * sizeof(unsigned), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(keys, 0x7F, (size_t)total * 4, (hipStream_t)stream);
  HPFG_ARG_CHECK(e == hipSuccess, "surface_distances: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(surface_scan_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred, gt, n, S, h, w, C, ndim, cursors, keep,
                     points);
  if (blocks > 0)
    hipLaunchKernelGGL(surface_nearest_kernel, dim3((unsigned)blocks), dim3(SURF_TILE), 0, (hipStream_t)stream, (const int*)points, keys, t, h, w);
  return hpfg_launch_status("surface_distances");
}

extern "C" int hpfg_surface_sums(const void* workspace, long workspace_bytes, int C, const unsigned int* counts_host, long long* sums, void* stream) {
  HPFG_ARG_CHECK(workspace && counts_host && sums, "surface_sums: null pointer");
  HPFG_ARG_CHECK(C >= 2 && C <= 16, "surface_sums: %d classes (2 .. 16)", C);
  const long total = surface_total(counts_host, C);
  HPFG_ARG_CHECK(total >= 0, "surface_sums: counts beyond the %d segments of %d classes, or 2^31 points or more", 2 * (C - 1), C);
  HPFG_ARG_CHECK(workspace_bytes >= hpfg_surface_workspace_bytes(C, total), "surface_sums: workspace of %ld bytes, %ld needed", workspace_bytes,
                 hpfg_surface_workspace_bytes(C, total));
  HPFG_ARG_CHECK((uintptr_t)workspace % 16 == 0 && (uintptr_t)sums % 8 == 0, "surface_sums: misaligned workspace or sums");
  SurfSumTable t;
  t.off[0] = 0;
  t.live = 0;
  for (int s = 0; s < SEGS; ++s) {
    t.off[s + 1] = t.off[s] + counts_host[s];
    if (s < 2 * (C - 1) && counts_host[s] > 0 && counts_host[s ^ 1] > 0) t.live |= 1u << s;          // the segments hpfg_surface_distances searched
  }
  hipError_t e = hipMemsetAsync(sums, 0, 2 * SEGS * sizeof(long long), (hipStream_t)stream);
  HPFG_ARG_CHECK(e == hipSuccess, "surface_sums: %s", hipGetErrorString(e));
  if (t.live)
    hipLaunchKernelGGL(surface_sums_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const int*)((const char*)workspace + 256), t, (unsigned long long*)sums);
  return hpfg_launch_status("surface_sums");
}
