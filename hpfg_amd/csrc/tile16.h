// The whole-tile layout shared by the thin forward kernel (conv_thin_kernel.h) and the fused backward kernel (fused_bwd_kernel.h): a 16 x 16
// pixel tile with its 1-pixel halo -- all channels of the (virtual) source at once -- staged as [16-channel chunk][hi|lo][pixel slot][16 ch],
// 32 bytes per pixel and plane, so that a pixel-major ds_read_b128 fragment (conv) and a transposing ds_read_b64_tr_b16 (weight gradient)
// are both conflict-free (fused_bwd_kernel.h says why).  Every load of a tile is in flight in registers (issue_halo) while the previous
// tile computes, and is converted and written to LDS afterwards (stage_halo): one exposed memory round trip per tile.
#pragma once
#include "conv_bf16_kernel.h"

namespace hpfg_tile16 {

using namespace hpfg_stage;

constexpr int T = 16, HP = 18, RS = 18;                 // tile edge, halo tile edge, row stride in pixel slots
constexpr int NSLOT = (HP * HP + 15) / 16 * 16;         // 336
constexpr int PL = NSLOT * 32;                          // bytes per hi / lo plane of one 16-channel chunk of a halo tile
constexpr int CH = 2 * PL;                              // one 16-channel chunk = (hi, lo)
using UP = UpPatch<T, T>;                               // low-resolution source patch of an upsampled chunk
constexpr int UBYTES = UP::SH * UP::SW * 16 * 4;        // fp32, [pixel][16 ch]

// CI 16-channel chunks of a layer input of loader kind AK: a concat is CI / 2 chunks of the skip half (BN + LeakyReLU pieces, read through
// a0) and CI / 2 upsampled chunks (LDS patch, read through a1)
template <int CI, int AK>
struct Halves {
  static constexpr bool CATK = AK == HPFG_KIND_CAT;
  static constexpr int AK0 = CATK ? HPFG_KIND_BNACT : AK;
  static constexpr int NA0 = CATK ? CI / 2 : CI, NA1 = CATK ? CI / 2 : 0;
};
template <bool CATK>
__device__ __forceinline__ HpfgAct skip_source(const HpfgAct& a) {
  HpfgAct s = a;
  if (CATK) s.drop_p = 0.f;      // (the skip half of a concat carries no dropout: model/unet.py:57 concatenates block outputs)
  return s;
}

// Weight fragments of the conv do not depend on the tile: the PB k-steps x NT channel tiles stay in registers for the whole kernel when they
// are few, otherwise (TOLDS) all nfrag of them are copied to LDS once -- streamed from L2 per tile they stalled every other k-step (8 waves x
// 40 KB per tile, each k-step pair shorter than the L2 latency).  The caller's barrier covers the LDS copy.
template <class C, int PB, bool TOLDS>
__device__ __forceinline__ void resident_weights(bf16x8 (&pbh)[PB > 0 ? PB : 1][C::NI], bf16x8 (&pbl)[PB > 0 ? PB : 1][C::NI], const bf16x8* wpk,
                                                 int ntn, bf16x8* ldsB, int nfrag, int tid, int nth) {
#pragma unroll
  for (int k = 0; k < PB; ++k) hpfg_conv16::load_b<C>(pbh[k], pbl[k], wpk, k, ntn, 0, tid & 63);
  if (TOLDS)
    for (int i = tid; i < nfrag; i += nth) ldsB[i] = wpk[i];
}

// conv fragment offsets inside a chunk (conv_bf16_kernel.h): pixel tile m of this wave; k-group = (tap parity, 8-channel half)
template <int MI>
__device__ __forceinline__ void frag_offsets(int (&aoff)[MI], int (&toff)[5], int wave, int lane) {
  const int kg = lane >> 4, gl = kg & 1;
#pragma unroll
  for (int m = 0; m < MI; ++m) {
    const int pxl = (wave * MI + m) * 16 + (lane & 15);
    aoff[m] = ((pxl / T) * RS + (pxl % T)) * 32 + gl * 16;
  }
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    int tap = 2 * s + (kg >> 1);
    tap = tap > 8 ? 8 : tap;                             // tap 9 re-reads tap 8 against zero weights
    toff[s] = ((tap / 3) * RS + (tap % 3)) * 32;
  }
}

// the ND halo-tile pieces of a thread in one 16-channel chunk: piece idx = tid + i * NTH is 8-channel group idx & 1 of pixel idx >> 1
template <int NTH>
constexpr int halo_pieces() { return (HP * HP * 2 + NTH - 1) / NTH; }

// every load of one chunk of the halo tile at (n, ty0, tx0); live == false: no further tile -- all lanes read pixel (0, 0, 0), one cache
// line, and nothing is made of it
template <int KIND, int NTH>
__device__ __forceinline__ void issue_halo(RawPiece<KIND> (&raw)[halo_pieces<NTH>()], const HpfgAct& a, const ActCtx& cx, int n, int ty0, int tx0,
                                           int H, int W, int tid, int c0, bool chv, bool live) {
  const HpfgAct none = {};
#pragma unroll
  for (int i = 0; i < halo_pieces<NTH>(); ++i) {
    const int idx = tid + i * NTH, pix = idx >> 1;
    const int gy = ty0 + pix / HP - 1, gx = tx0 + pix % HP - 1;
    const bool ok = live && idx < HP * HP * 2 && chv && gy >= 0 && gy < H && gx >= 0 && gx < W;
    issue_piece<KIND>(raw[i], a, none, cx, n, live ? clampi(gy, 0, H - 1) : 0, live ? clampi(gx, 0, W - 1) : 0, chv ? c0 : 0, ok);
  }
}
// the store of a halo piece: hi | lo at [pixel slot] of the chunk
__device__ __forceinline__ void store_halo(unsigned char* chunk, int idx, const f32x4& v0, const f32x4& v1) {
  if (idx < HP * HP * 2) {
    const int pix = idx >> 1;
    bf16x8 hi, lo;
    split8(v0, v1, hi, lo);
    unsigned char* o = chunk + ((pix / HP) * RS + pix % HP) * 32 + (idx & 1) * 16;
    *reinterpret_cast<bf16x8*>(o) = hi;
    *reinterpret_cast<bf16x8*>(o + PL) = lo;
  }
}
// prefetched raw data of that chunk -> producer chain -> bf16 hi / lo -> LDS
template <int KIND, int NTH>
__device__ __forceinline__ void stage_halo(unsigned char* chunk, const RawPiece<KIND> (&raw)[halo_pieces<NTH>()], const Tab& t, const HpfgAct& a,
                                           const ActCtx& cx, int n, int ty0, int tx0, int H, int W, int tid, int c0, bool chv) {
  const HpfgAct none = {};
#pragma unroll
  for (int i = 0; i < halo_pieces<NTH>(); ++i) {
    const int idx = tid + i * NTH, pix = idx >> 1;
    const int gy = ty0 + pix / HP - 1, gx = tx0 + pix % HP - 1;
    const bool ok = idx < HP * HP * 2 && chv && gy >= 0 && gy < H && gx >= 0 && gx < W;
    f32x4 v0, v1;
    finish_piece<KIND>(v0, v1, raw[i], t, a, none, cx, n, clampi(gy, 0, H - 1), clampi(gx, 0, W - 1), chv ? c0 : 0, ok);
    store_halo(chunk, idx, v0, v1);
  }
}

}  // namespace hpfg_tile16
