// Staging code shared by the four split-bf16 kernel families -- the chunked 3x3 / 1x1 kernels (conv_bf16_kernel.h), the whole-tile forward
// kernel (conv_thin_kernel.h), the fused dgrad + wgrad kernel (fused_bwd_kernel.h) and the weight gradient (wgrad_bf16_kernel.h).  Each phase
// below has ONE definition; the kernels differ in the template constants and arguments they pass, never by a branch in here.  The arithmetic
// underneath -- the vector types, the hi / lo split (split8), the transposing LDS read of the kernels that contract over pixels (tr_read8:
// fused, weight gradient) and the three-issue product (HPFG_MFMA3) -- is bf16x3.h's, shared with the GEMM and attention kernels:
//   * per piece: raw loads of an 8-channel piece of a virtual activation (issue_piece), the producer chain (finish_piece), its hi / lo
//     fragments (split_piece) -- all four families;
//   * per-channel source tables: LDS rows filled once per launch (fill_tables_lds; row stride and row length are the caller's) and read
//     back into a Tab (load_tables_lds<KIND, STRIDE>) -- all four families;
//   * the upsampled half of a concat source through an LDS patch: geometry (UpPatch), first source row / column (up_base), the patch
//     piece of a thread (up_patch_issue), parking it (up_patch_park), the blend expression (bilerp: what finish_piece<CAT> computes) --
//     all four families; the blend of an output piece's four taps from the patch (up_blend) -- chunked, weight gradient.  Patch channel
//     stride and width are template constants, the halo and the validity mask are the caller's arguments;
//   * the XCD-contiguous tile walk (tile_walk) -- all four families; the number of XCD groups is the caller's (see there);
//   * the in-kernel time stamps of the diagnostics build (HPFG_TR, HPFG_TR_REAL) -- chunked, fused, weight gradient.
// The whole-tile layout that the thin and the fused kernel share on top of this is tile16.h.
// Deliberate exceptions (a phase stays a family's own text where the shared form would need a branch on its caller, or changes a result):
//   * thin and fused kernel, the blend of an output piece: the text of up_blend around the shared expression (bilerp), not a call.  Built
//     from the call, the compiler contracts the blend's first row the other way round (wx1 * a01 fused, wx0 * a00 multiplied) in these two
//     families: one ulp on the staged values, and the digests of tests/golden/conv_bits.json change for every concat case of the two;
//   * weight gradient, tables of the layer input: load_tables (registers, straight from the table, once per workgroup: its 16 NI channels
//     do not change with the work item), not the LDS rows;
//   * weight gradient, SPLIT16 operands: their issue is an address select and their staging a copy (wgrad_bf16_kernel.h), no piece chain.
#pragma once
#include "bf16x3.h"

namespace hpfg_stage {

using namespace hpfg_bf16x3;

__device__ __forceinline__ f32x4 ld4(const float* base, int off) { return *reinterpret_cast<const f32x4*>(base + off); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }   // v_med3_i32

// Diagnostics build only (make TRACE=1 -> libhpfg_hip_trace.so, tools/trace_conv.py, tools/trace_fused.py): with math bit 0x2000 one thread
// of every workgroup writes (id << 56 | s_memtime) stamps to the kernel's own u64 buffer tr_buf (256 per workgroup; the kernel says where).
#ifdef HPFG_TRACE
#define HPFG_TR(ID)                                                                                        \
  if (tr_on && tr_i < 255) {                                                                               \
    tr_buf[tr_i++] = ((unsigned long long)(ID) << 56) | (__builtin_amdgcn_s_memtime() & 0xffffffffffffffull); \
  }
#define HPFG_TR_REAL(ID)                                                                                   \
  if (tr_on && tr_i < 255) {                                                                               \
    tr_buf[tr_i++] = ((unsigned long long)(ID) << 56) | (__builtin_amdgcn_s_memrealtime() & 0xffffffffffffffull); \
  }
#else
#define HPFG_TR(ID)
#define HPFG_TR_REAL(ID)
#endif

// XCD-aware work mapping of the persistent kernels: workgroups are dealt round-robin over the 8 XCDs (b % 8 names the XCD group), each XCD
// has its own L2.  Give every XCD group a CONTIGUOUS range of tiles (row-major inside an image) so that tiles sharing a halo are read
// through the same L2; inside a group, workgroup j takes tiles j, j + step, j + 2 step, ... of the range.  (Speed only: any mapping is
// correct.)  nx = 8 where blockIdx.x % 8 names the XCD, else 1 -- the caller's to say: a 1-D or (x, slice) grid with at least 8 workgroups
// in x, or the weight gradient's (x, ci, co) grid, whose linear workgroup id is x + gridDim.x * (...) and needs gridDim.x % 8 == 0.
struct TileWalk {
  int w, wend, step;      // first work item of this workgroup, end of its group's range, workgroups of the group = stride
};
__device__ __forceinline__ TileWalk tile_walk(int nwork, int nx) {
  const int xg = (int)blockIdx.x % nx, xj = (int)blockIdx.x / nx;
  const int per_x = (nwork + nx - 1) / nx;                 // tiles per XCD group
  TileWalk t;
  t.wend = (xg + 1) * per_x < nwork ? (xg + 1) * per_x : nwork;
  t.step = ((int)gridDim.x - xg + nx - 1) / nx;
  t.w = xg * per_x + xj;
  return t;
}

// ---- per-kind staging: issue_piece() puts the raw global loads of one 8-channel piece in flight, finish_piece() applies the
// ---- producer chain.  Raw loads per piece: PLAIN/BNACT 2, DZ 4 (z + dA), POOL 8 (2x2 pixels), CAT 8 (4 bilinear taps).
template <int KIND>
struct RawCount { static constexpr int N = KIND == HPFG_KIND_POOL || KIND == HPFG_KIND_CAT ? 8 : (KIND == HPFG_KIND_DZ ? 4 : 2); };

// Raw (in-flight) data of one staging piece: the float4 loads plus, for the kinds that apply Dropout, the two words of an
// explicit keep mask (HpfgAct.drop_mask, tests only).  The mask words are requested WITH the data loads: a load inside
// finish_piece() would sit behind every younger prefetch in the in-order vmcnt queue and drain the whole ring.
template <int KIND>
struct RawPiece {
  f32x4 v[RawCount<KIND>::N];
  uint32_t dm[2];
};

struct Tab {   // per-chunk per-channel tables of this thread's 8 channels
  f32x4 sc[2], sh[2], k1[2], k2[2], k3[2];
};

template <int KIND>
__device__ __forceinline__ void load_tables(Tab& t, const HpfgAct& a0, int c0, bool chvalid) {
  if (KIND == HPFG_KIND_PLAIN || KIND == HPFG_KIND_SPLIT || !chvalid) return;
  if (KIND == HPFG_KIND_CAT && c0 >= a0.C) return;
  const float* b = a0.bn + a0.bn_coff + c0;
  const int st = a0.bn_stride;
  t.sc[0] = ld4(b, HPFG_BN_SCALE * st);
  t.sc[1] = ld4(b, HPFG_BN_SCALE * st + 4);
  t.sh[0] = ld4(b, HPFG_BN_SHIFT * st);
  t.sh[1] = ld4(b, HPFG_BN_SHIFT * st + 4);
  if (KIND == HPFG_KIND_DZ) {
    t.k1[0] = ld4(b, HPFG_BN_K1 * st);
    t.k1[1] = ld4(b, HPFG_BN_K1 * st + 4);
    t.k2[0] = ld4(b, HPFG_BN_K2 * st);
    t.k2[1] = ld4(b, HPFG_BN_K2 * st + 4);
    t.k3[0] = ld4(b, HPFG_BN_K3 * st);
    t.k3[1] = ld4(b, HPFG_BN_K3 * st + 4);
  }
}

// The kinds with a producer chain (BNACT / POOL / concat skip half: scale, shift; DZ: scale, shift, k1, k2, k3) read the rows of the whole
// source from LDS rows [row][STRIDE] the kernel prologue filled (from the table, or derived from the sum accumulators: common.h).  STRIDE is
// HPFG_BN_CMAX in the chunked kernels, which serve any source, and the channel count of the instantiation in the others.
constexpr int HPFG_BN_CMAX = 256;      // channels of a BatchNorm'd source whose coefficients a consumer keeps in LDS
template <int KIND>
constexpr bool tab_in_lds() { return KIND == HPFG_KIND_BNACT || KIND == HPFG_KIND_POOL || KIND == HPFG_KIND_CAT || KIND == HPFG_KIND_DZ; }
template <int KIND>
constexpr int tab_rows() { return KIND == HPFG_KIND_DZ ? 5 : 2; }      // scale, shift [, k1, k2, k3]
template <int KIND, int STRIDE = HPFG_BN_CMAX>
__device__ __forceinline__ void load_tables_lds(Tab& t, const float* ldsT, const HpfgAct& a0, int c0) {
  if (!tab_in_lds<KIND>() || (KIND == HPFG_KIND_CAT && c0 >= a0.C)) return;
  t.sc[0] = ld4(ldsT, c0);
  t.sc[1] = ld4(ldsT, c0 + 4);
  t.sh[0] = ld4(ldsT, STRIDE + c0);
  t.sh[1] = ld4(ldsT, STRIDE + c0 + 4);
  if (KIND == HPFG_KIND_DZ) {
    t.k1[0] = ld4(ldsT, 2 * STRIDE + c0);
    t.k1[1] = ld4(ldsT, 2 * STRIDE + c0 + 4);
    t.k2[0] = ld4(ldsT, 3 * STRIDE + c0);
    t.k2[1] = ld4(ldsT, 3 * STRIDE + c0 + 4);
    t.k3[0] = ld4(ldsT, 4 * STRIDE + c0);
    t.k3[1] = ld4(ldsT, 4 * STRIDE + c0 + 4);
  }
}
// the kernel prologue's fill of those rows: channels [0, nch) of every row, zeros at and past a0.C (all threads call, the caller syncs).
// ACC = false: scale / shift from the table rows even where a0.bn_acc is set (common.h)
template <int KIND, int STRIDE = HPFG_BN_CMAX, bool ACC = true>
__device__ __forceinline__ void fill_tables_lds(const HpfgAct& a0, float* ldsT, int nch, int tid, int nthr) {
  if (KIND == HPFG_KIND_DZ) hpfg_dz_rows_to_lds(a0, ldsT, STRIDE, nch, tid, nthr);
  else if (tab_in_lds<KIND>()) hpfg_bn_rows_to_lds<ACC>(a0, ldsT, STRIDE, nch, tid, nthr);
}

// bilinear x2 (align_corners=True) source taps of output coordinate o for a low-res extent L
__device__ __forceinline__ void up_coord(int o, int L, int& i0, int& i1, float& w1) {
  const float r = L > 1 ? (float)(L - 1) / (float)(2 * L - 1) : 0.f;
  const float f = r * (float)o;
  i0 = (int)f;
  i1 = i0 + (i0 < L - 1 ? 1 : 0);
  w1 = f - (float)i0;
}

// the blend of the four taps (a00 a01 / a10 a11) of one output value: THE expression of the upsampled half, on float4 values; the compiler is
// free to contract it into FMAs
__device__ __forceinline__ f32x4 bilerp(float wy0, float wy1, float wx0, float wx1, const f32x4& a00, const f32x4& a01, const f32x4& a10,
                                        const f32x4& a11) {
  return wy0 * (wx0 * a00 + wx1 * a01) + wy1 * (wx0 * a10 + wx1 * a11);
}

// ---- Concat loader, upsampled half through an LDS patch: the bilinear x2 taps of a TH x TW tile (with or without a halo pixel) come from a
// (TH/2+3) x (TW/2+3) patch of the low-resolution 1x1-conv output.  That patch is fetched ONCE per tile and chunk of CW channels (a thread
// requests one 8-channel piece, two float4, prefetched like the cheap loaders), parked in LDS as fp32 [pixel][CW channels], and every output
// piece interpolates its four taps from LDS -- instead of 8 float4 global loads per output piece (24 per thread and chunk in the chunked
// kernel), whose registers forced a two-k-step pipeline that exposed one memory latency per piece.
template <int TH, int TW>
struct UpPatch {
  static constexpr int SH = TH / 2 + 3, SW = TW / 2 + 3;
};
// first low-res row / column a tile touches: source index of output coordinate max(o0, 0) (o0 = the tile's first row / column, halo included)
__device__ __forceinline__ int up_base(int o0, int L) {
  const float r = L > 1 ? (float)(L - 1) / (float)(2 * L - 1) : 0.f;
  return (int)(r * (float)(o0 < 0 ? 0 : o0));
}
// this thread's piece of the patch of image n at (sy_base, sx_base): patch pixel `pix`, channels cu .. cu + 7 of the upsampled tensor
template <int SW>
__device__ __forceinline__ void up_patch_issue(f32x4 (&rawU)[2], const HpfgAct& u, int n, int sy_base, int sx_base, int pix, int cu) {
  const int sy = clampi(sy_base + pix / SW, 0, u.Hs - 1), sx = clampi(sx_base + pix % SW, 0, u.Ws - 1);
  const int off = ((n * u.Hs + sy) * u.Ws + sx) * u.pstride + cu;
  rawU[0] = ld4(u.z, off);
  rawU[1] = ld4(u.z, off + 4);
}
template <int CW>
__device__ __forceinline__ void up_patch_park(float* ldsU, const f32x4 (&rawU)[2], int pix, int cg) {
  float* d = ldsU + pix * CW + cg;
  *reinterpret_cast<f32x4*>(d) = rawU[0];
  *reinterpret_cast<f32x4*>(d + 4) = rawU[1];
}
// (v0, v1) = channels cg .. cg + 7 of output pixel (gy, gx) (clamped into the image by the caller) from the parked patch; zeros unless ok.
// The expression tree is finish_piece<CAT>'s -- the kernels agree to the bit with the per-piece loader (tests/test_gpu_conv_thin.py, the
// float64 bound of tests/helpers.py states it with the u * f term) up to how one compilation contracts it into FMAs.
template <int CW, int SW>
__device__ __forceinline__ void up_blend(f32x4& v0, f32x4& v1, const float* ldsU, const HpfgAct& u, int gy, int gx, int sy_base, int sx_base,
                                         int cg, bool ok) {
  int y0, y1, x0, x1;
  float wy1, wx1;
  up_coord(gy, u.Hs, y0, y1, wy1);
  up_coord(gx, u.Ws, x0, x1, wx1);
  const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
  const float* r0 = ldsU + ((y0 - sy_base) * SW) * CW + cg;
  const float* r1 = ldsU + ((y1 - sy_base) * SW) * CW + cg;
  const int o0 = (x0 - sx_base) * CW, o1 = (x1 - sx_base) * CW;
  const f32x4 a00 = *reinterpret_cast<const f32x4*>(r0 + o0), b00 = *reinterpret_cast<const f32x4*>(r0 + o0 + 4);
  const f32x4 a01 = *reinterpret_cast<const f32x4*>(r0 + o1), b01 = *reinterpret_cast<const f32x4*>(r0 + o1 + 4);
  const f32x4 a10 = *reinterpret_cast<const f32x4*>(r1 + o0), b10 = *reinterpret_cast<const f32x4*>(r1 + o0 + 4);
  const f32x4 a11 = *reinterpret_cast<const f32x4*>(r1 + o1), b11 = *reinterpret_cast<const f32x4*>(r1 + o1 + 4);
  v0 = bilerp(wy0, wy1, wx0, wx1, a00, a01, a10, a11);
  v1 = bilerp(wy0, wy1, wx0, wx1, b00, b01, b10, b11);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v0[j] = ok ? v0[j] : 0.f;
    v1[j] = ok ? v1[j] : 0.f;
  }
}

template <int KIND>
__device__ __forceinline__ void issue_piece(RawPiece<KIND>& rp, const HpfgAct& a, const HpfgAct& u, const ActCtx& cx0, int n, int gy,
                                            int gx, int c0, bool ok) {
  f32x4 (&raw)[RawCount<KIND>::N] = rp.v;
  if ((KIND == HPFG_KIND_BNACT || KIND == HPFG_KIND_DZ) && a.drop_mask && a.drop_p > 0.f) {
    const uint32_t e = (uint32_t)(((n * a.Hs + gy) * a.Ws + gx) * a.C + c0);
    rp.dm[0] = *reinterpret_cast<const uint32_t*>(a.drop_mask + e);
    rp.dm[1] = *reinterpret_cast<const uint32_t*>(a.drop_mask + e + 4);
  }
  // Branch-free on the pixel predicate: an out-of-image (halo) pixel is clamped into the image and loaded anyway, finish_piece()
  // selects zero for it.  Keeps the conv k-loop a single basic block so the compiler can software-pipeline LDS reads and MFMAs.
  if (KIND == HPFG_KIND_CAT) {      // two sources behind a per-thread branch anyway: keep the predicated form
#pragma unroll
    for (int i = 0; i < RawCount<KIND>::N; ++i) raw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!ok) return;
  }
  if (KIND == HPFG_KIND_SPLIT) {      // 8 channels of the stored (hi | lo) pair: two 16-byte words, carried as bit patterns
    const int off = ((n * a.Hs + gy) * a.Ws + gx) * a.pstride + c0;      // fp32 words == (hi, lo) pairs: 32 contiguous bytes per 8 channels
    raw[0] = ld4(a.z, off);
    raw[1] = ld4(a.z, off + 4);
  } else if (KIND == HPFG_KIND_PLAIN) {
    if (a.mode == HPFG_ACT_STRIDED) {
      raw[0] = act_load4_mode<HPFG_ACT_STRIDED>(a, cx0, n, gy, gx, c0);
      raw[1] = act_load4_mode<HPFG_ACT_STRIDED>(a, cx0, n, gy, gx, c0 + 4);
    } else {      // whole quads: C % 4 == 0 here -- a PLAIN source that ends inside a quad arrives as STRIDED (common.h hpfg_plain_by_lane)
      const int off = ((n * a.Hs + gy) * a.Ws + gx) * a.pstride + c0;
      raw[0] = ld4(a.z, off);
      raw[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c0 + 4 < a.C) raw[1] = ld4(a.z, off + 4);
    }
  } else if (KIND == HPFG_KIND_BNACT || (KIND == HPFG_KIND_CAT && c0 < a.C)) {
    const int off = ((n * a.Hs + gy) * a.Ws + gx) * a.pstride + c0;
    raw[0] = ld4(a.z, off);
    raw[1] = ld4(a.z, off + 4);
  } else if (KIND == HPFG_KIND_POOL) {
    const int off = ((n * a.Hs + 2 * gy) * a.Ws + 2 * gx) * a.pstride + c0;
    const int ro = a.Ws * a.pstride;
    raw[0] = ld4(a.z, off);
    raw[1] = ld4(a.z, off + 4);
    raw[2] = ld4(a.z, off + a.pstride);
    raw[3] = ld4(a.z, off + a.pstride + 4);
    raw[4] = ld4(a.z, off + ro);
    raw[5] = ld4(a.z, off + ro + 4);
    raw[6] = ld4(a.z, off + ro + a.pstride);
    raw[7] = ld4(a.z, off + ro + a.pstride + 4);
  } else if (KIND == HPFG_KIND_CAT) {   // upsampled half
    int y0, y1, x0, x1;
    float wy, wx;
    up_coord(gy, u.Hs, y0, y1, wy);
    up_coord(gx, u.Ws, x0, x1, wx);
    const int cb = n * u.Hs * u.Ws * u.pstride + (c0 - a.C);
    const int o00 = cb + (y0 * u.Ws + x0) * u.pstride, o01 = cb + (y0 * u.Ws + x1) * u.pstride;
    const int o10 = cb + (y1 * u.Ws + x0) * u.pstride, o11 = cb + (y1 * u.Ws + x1) * u.pstride;
    raw[0] = ld4(u.z, o00);
    raw[1] = ld4(u.z, o00 + 4);
    raw[2] = ld4(u.z, o01);
    raw[3] = ld4(u.z, o01 + 4);
    raw[4] = ld4(u.z, o10);
    raw[5] = ld4(u.z, o10 + 4);
    raw[6] = ld4(u.z, o11);
    raw[7] = ld4(u.z, o11 + 4);
  } else {   // DZ
    const int pix = (n * a.Hs + gy) * a.Ws + gx;
    raw[0] = ld4(a.z, pix * a.pstride + c0);
    raw[1] = ld4(a.z, pix * a.pstride + c0 + 4);
    raw[2] = ld4(a.aux, pix * a.aux_pstride + c0);
    raw[3] = ld4(a.aux, pix * a.aux_pstride + c0 + 4);
  }
}

// keep test of the four 8-bit draws (or mask bytes) in h against thr: v[j] = keep_j ? v[j] : 0
__device__ __forceinline__ void keep_select4(f32x4& v, uint32_t h, uint32_t thr) {
  v[0] = (h & 0xFFu) >= thr ? v[0] : 0.f;
  v[1] = ((h >> 8) & 0xFFu) >= thr ? v[1] : 0.f;
  v[2] = ((h >> 16) & 0xFFu) >= thr ? v[2] : 0.f;
  v[3] = (h >> 24) >= thr ? v[3] : 0.f;
}
__device__ __forceinline__ f32x4 lrelu4(const f32x4& y) { return __builtin_elementwise_max(y, y * HPFG_LEAKY); }

// The producer chain on the raw data of one piece.  Written on float4 values so that the multiplies / FMAs pair up into
// v_pk_fma_f32 / v_pk_mul_f32 (the loaders are VALU-issue bound: instruction count is what matters here).  `ok` = the piece is
// inside the image and its channel group exists; a piece that is not yields zeros (its loads were clamped to valid addresses).
template <int KIND>
__device__ __forceinline__ void finish_piece(f32x4& v0, f32x4& v1, const RawPiece<KIND>& rp, const Tab& t, const HpfgAct& a,
                                             const HpfgAct& u, const ActCtx& cx0, int n, int gy, int gx, int c0, bool ok) {
  const f32x4 (&raw)[RawCount<KIND>::N] = rp.v;
  bool need_ok = true;
  v0 = f32x4{0.f, 0.f, 0.f, 0.f};
  v1 = v0;
  if (KIND == HPFG_KIND_PLAIN || KIND == HPFG_KIND_SPLIT) {      // (SPLIT: v0 / v1 carry the hi / lo words; zero bits are bf16 zeros)
    v0 = raw[0];
    v1 = raw[1];
  } else if (KIND == HPFG_KIND_BNACT || (KIND == HPFG_KIND_CAT && c0 < a.C)) {
    v0 = lrelu4(raw[0] * t.sc[0] + t.sh[0]);
    v1 = lrelu4(raw[1] * t.sc[1] + t.sh[1]);
    if (KIND == HPFG_KIND_BNACT && a.drop_p > 0.f) {
      const uint32_t e = (uint32_t)(((n * a.Hs + gy) * a.Ws + gx) * a.C + c0);
      const uint32_t thr = drop_thresh(a, cx0);
      uint32_t h0 = a.drop_mask ? rp.dm[0] : hpfg_hash32(e >> 2, cx0.seed);
      uint32_t h1 = a.drop_mask ? rp.dm[1] : hpfg_hash32((e + 4) >> 2, cx0.seed);
      if (thr >= 1u) {       // a zero draw is always dropped: fold the in-image predicate into the draws
        h0 = ok ? h0 : 0u;
        h1 = ok ? h1 : 0u;
        need_ok = false;
      }
      v0 = v0 * cx0.inv_keep;
      v1 = v1 * cx0.inv_keep;
      keep_select4(v0, h0, thr);
      keep_select4(v1, h1, thr);
    }
  } else if (KIND == HPFG_KIND_POOL) {
    f32x4 m0 = lrelu4(raw[0] * t.sc[0] + t.sh[0]), m1 = lrelu4(raw[1] * t.sc[1] + t.sh[1]);
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      m0 = __builtin_elementwise_max(m0, lrelu4(raw[2 * q] * t.sc[0] + t.sh[0]));
      m1 = __builtin_elementwise_max(m1, lrelu4(raw[2 * q + 1] * t.sc[1] + t.sh[1]));
    }
    v0 = m0;
    v1 = m1;
  } else if (KIND == HPFG_KIND_CAT) {
    int i0, i1;
    float wy1, wx1;
    up_coord(gy, u.Hs, i0, i1, wy1);
    up_coord(gx, u.Ws, i0, i1, wx1);
    const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    v0 = bilerp(wy0, wy1, wx0, wx1, raw[0], raw[2], raw[4], raw[6]);
    v1 = bilerp(wy0, wy1, wx0, wx1, raw[1], raw[3], raw[5], raw[7]);
  } else {   // DZ: k1*g + k2*z + k3, g = dA * dropmask/(1-p) * lrelu'(scale*z+shift)
    f32x4 ga = raw[2], gb = raw[3];
    if (a.drop_p > 0.f) {
      const uint32_t e = (uint32_t)(((n * a.Hs + gy) * a.Ws + gx) * a.C + c0);
      const uint32_t thr = drop_thresh(a, cx0);
      ga = ga * cx0.inv_keep;
      gb = gb * cx0.inv_keep;
      keep_select4(ga, a.drop_mask ? rp.dm[0] : hpfg_hash32(e >> 2, cx0.seed), thr);
      keep_select4(gb, a.drop_mask ? rp.dm[1] : hpfg_hash32((e + 4) >> 2, cx0.seed), thr);
    }
    const f32x4 ya = raw[0] * t.sc[0] + t.sh[0], yb = raw[1] * t.sc[1] + t.sh[1];
    const f32x4 la = ga * HPFG_LEAKY, lb = gb * HPFG_LEAKY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ga[j] = ya[j] > 0.f ? ga[j] : la[j];
      gb[j] = yb[j] > 0.f ? gb[j] : lb[j];
    }
    v0 = t.k1[0] * ga + (t.k2[0] * raw[0] + t.k3[0]);
    v1 = t.k1[1] * gb + (t.k2[1] * raw[1] + t.k3[1]);
  }
  if (need_ok) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {     // select, not branch: the raw values of a clamped (out-of-image / padding) piece are discarded
      v0[j] = ok ? v0[j] : 0.f;
      v1[j] = ok ? v1[j] : 0.f;
    }
  }
}

// (v0, v1) of finish_piece() -> the hi / lo bf16 fragments a staging store writes
template <int KIND>
__device__ __forceinline__ void split_piece(const f32x4& v0, const f32x4& v1, bf16x8& hi, bf16x8& lo) {
  if (KIND == HPFG_KIND_SPLIT) {      // stored already split (HPFG_ACT_SPLIT16): a copy
    hi = __builtin_bit_cast(bf16x8, v0);
    lo = __builtin_bit_cast(bf16x8, v1);
  } else {
    split8(v0, v1, hi, lo);
  }
}

}  // namespace hpfg_stage
