// 3x3 convolution of the thin layers -- forward, and the dgrad of a 32-channel layer into a 64-channel input (dZ source) -- (16 / 32 input channels, or a 32-channel concat; 16 / 32 output channels; H and W multiples
// of 16) on the bf16 matrix cores with split-precision operands -- the forward twin of fused_bwd_kernel.h, built on what that kernel's
// timelines and counters showed:
//   * the WHOLE 18 x 18 halo tile of the (virtual) input -- all input channels -- is staged at once as [chunk][hi|lo][pixel slot][16 ch]
//     (32 bytes per pixel and plane: conflict-free ds_read_b128 fragments), not chunk by chunk through a double buffer;
//   * every load of the next tile is in flight (in registers) during the MFMAs and the epilogue of the current one, so a tile costs one
//     exposed memory round trip;
//   * nothing in the MFMA phase touches global memory: the weight fragments do not depend on the tile and stay in registers for the whole
//     kernel (<= 80 VGPRs) or in LDS, the BatchNorm tables of the loader live in LDS;
//   * the concat loader's upsampled half reads its low-resolution source patch once per tile (one piece per thread) into LDS and blends
//     the four bilinear taps from there (stage.h);
//   * a workgroup walks a contiguous range of its XCD's tiles; the BatchNorm partial sums stay in registers across tiles, one row per
//     workgroup.
// Values and MFMA order are those of conv_bf16x3_kernel, so the raw output is bit-identical to it; only the partition of the BatchNorm
// partial sums (rows = workgroups) differs.
#pragma once
#include <type_traits>
#include "tile16.h"

namespace hpfg_thin {

using namespace hpfg_tile16;
using hpfg_conv16::Cfg;

template <int CI, int CO, int AK, int NW>
struct Geo : Halves<CI, AK> {
  using Halves<CI, AK>::NA0;
  using Halves<CI, AK>::NA1;
  static constexpr int NTH = 64 * NW;
  static constexpr int ND = halo_pieces<NTH>();                    // staging pieces (8 channels of one pixel) per thread and chunk
  static constexpr int MI = 16 / NW;                               // 16-pixel MFMA tiles per wave
  static constexpr int KS = 5 * CI;                                // k-steps: 2 taps x 16 channels each
  static constexpr bool BREG = KS * CO * 8 <= 80;                  // weight fragments: registers or LDS
  static constexpr int TAB = tab_rows<AK>() * 16 * NA0 * 4;        // table rows of the loader: scale, shift [, k1, k2, k3 of a dZ source]
  static constexpr int STAT = 2 * NW * 16 * CO * 4;
  static constexpr int BFR = BREG ? 0 : KS * CO * 2 * 1024;
  static constexpr int OFF_TAB = CI * CH, OFF_STAT = OFF_TAB + TAB, OFF_U = OFF_STAT + STAT, OFF_B = OFF_U + NA1 * UBYTES;
  static constexpr int LDS = OFF_B + BFR;
  static_assert(NW == 4 || NW == 8, "4 or 8 waves");
  static_assert(UP::SH * UP::SW * 2 <= NTH, "one source piece per thread");
};

template <int CI, int CO, int AK, int NW, int WGS>
__global__ __launch_bounds__(64 * NW, WGS) void conv_thin_kernel(HpfgConvArgs p, int tiles_x, int tiles_y) {
  using C = Cfg<16, 16, 4, 1, CO, 9, 16>;               // (weight-fragment indexing: CO output-channel tiles)
  using G = Geo<CI, CO, AK, NW>;
  constexpr int AK0 = G::AK0, NA0 = G::NA0, NA1 = G::NA1, NTH = G::NTH, ND = G::ND, MI = G::MI, KS = G::KS;
  __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS];
  float* tabA = reinterpret_cast<float*>(lds + G::OFF_TAB);
  float* ldsf = reinterpret_cast<float*>(lds + G::OFF_STAT);
  float* ldsU = reinterpret_cast<float*>(lds + G::OFF_U);
  const bf16x8* ldsB = reinterpret_cast<const bf16x8*>(lds + G::OFF_B);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, W = p.W;
  const int ntiles = tiles_x * tiles_y, nwork = ntiles * p.N;
  const HpfgAct aS = skip_source<G::CATK>(p.a0);
  const ActCtx cxa = make_ctx(aS);
  const int gsel = tid & 1;                              // this thread's 8-channel group inside a 16-channel chunk

  const int ntn = p.CoutPad / 16;
  const bf16x8* wpk = reinterpret_cast<const bf16x8*>(p.wpk);
  constexpr int PB = G::BREG ? KS : 0;
  bf16x8 pbh[PB > 0 ? PB : 1][CO], pbl[PB > 0 ? PB : 1][CO];
  resident_weights<C, PB, !G::BREG>(pbh, pbl, wpk, ntn, reinterpret_cast<bf16x8*>(lds + G::OFF_B), KS * CO * 2 * 64, tid, NTH);

  int aoff[MI], toff[5];
  frag_offsets<MI>(aoff, toff, wave, lane);
  f32x4 s1[CO], s2[CO], bias[CO];
#pragma unroll
  for (int j = 0; j < CO; ++j) {
    s1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    s2[j] = s1[j];
    bias[j] = s1[j];
    const int co = j * 16 + (lane >> 4) * 4;
    if (p.bias && co < p.CoutPad) bias[j] = ld4(p.bias, co);
  }

  const TileWalk tw = tile_walk(nwork, gridDim.x >= 8 ? 8 : 1);      // every XCD group walks a contiguous range of tiles
  const int wend = tw.wend, GS = tw.step;

  RawPiece<AK0> raw[NA0][ND];
  f32x4 rawU[NA1 > 0 ? NA1 : 1][2];

  // every load of one tile; live == false: no further tile (then n = ty0 = tx0 = 0: issue_halo)
  auto issue = [&](int n, int ty0, int tx0, bool live) {
#pragma unroll
    for (int c = 0; c < NA0; ++c) {
      const int c0 = c * 16 + gsel * 8;
      issue_halo<AK0, NTH>(raw[c], aS, cxa, n, ty0, tx0, H, W, tid, c0, c0 < aS.C, live);
    }
    if (NA1 > 0) {
      const int sy_base = up_base(ty0 - 1, p.a1.Hs), sx_base = up_base(tx0 - 1, p.a1.Ws);
#pragma unroll
      for (int c = 0; c < NA1; ++c) {
        const int cu = c * 16 + gsel * 8;
        up_patch_issue<UP::SW>(rawU[c], p.a1, n, sy_base, sx_base, live ? tid >> 1 : 0, cu < p.a1.C ? cu : 0);
      }
    }
  };

  int w = tw.w;
  if (w < wend) issue(w / ntiles, ((w % ntiles) / tiles_x) * T, ((w % ntiles) % tiles_x) * T, true);
  // BatchNorm coefficients of the source -> LDS, behind the first tile's loads (one exposed round trip for both): the table rows, or --
  // forward kinds with HpfgAct.bn_acc -- scale / shift derived here from the producer's sum accumulators (no finalize launch in between)
  // (a dZ source: rows scale, shift, k1, k2, k3 -- the table, or k1 .. k3 derived from the backward sum accumulators); zeros at and past C
  fill_tables_lds<AK0, 16 * NA0>(aS, tabA, 16 * NA0, tid, NTH);
  __syncthreads();                                       // tables, weight fragments

  for (; w < wend; w += GS) {
    const int n = w / ntiles, ty0 = ((w % ntiles) / tiles_x) * T, tx0 = ((w % ntiles) % tiles_x) * T;
    // ---- prefetched raw data -> producer chain -> bf16 hi / lo -> LDS
#pragma unroll
    for (int c = 0; c < NA0; ++c) {
      const int c0 = c * 16 + gsel * 8;
      Tab ta;
      load_tables_lds<AK0, 16 * NA0>(ta, tabA, aS, c0);
      stage_halo<AK0, NTH>(lds + c * CH, raw[c], ta, aS, cxa, n, ty0, tx0, H, W, tid, c0, c0 < aS.C);
    }
    if (NA1 > 0) {
      // park the low-res patches (fp32, [pixel][16 channels]), then every output piece blends its four taps from LDS
      if (tid < UP::SH * UP::SW * 2) {
#pragma unroll
        for (int c = 0; c < NA1; ++c) up_patch_park<16>(ldsU + c * (UBYTES / 4), rawU[c], tid >> 1, gsel * 8);
      }
      __syncthreads();
      const int sy_base = up_base(ty0 - 1, p.a1.Hs), sx_base = up_base(tx0 - 1, p.a1.Ws);
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const int idx = tid + i * NTH, pix = idx >> 1;
        const int gy = ty0 + pix / HP - 1, gx = tx0 + pix % HP - 1;
        const bool inimg = idx < HP * HP * 2 && gy >= 0 && gy < H && gx >= 0 && gx < W;
        // (the text of up_blend, not a call: stage.h says why)
        int y0, y1, x0, x1;
        float wy1, wx1;
        up_coord(clampi(gy, 0, H - 1), p.a1.Hs, y0, y1, wy1);
        up_coord(clampi(gx, 0, W - 1), p.a1.Ws, x0, x1, wx1);
        const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
        const int o0 = (x0 - sx_base) * 16, o1 = (x1 - sx_base) * 16;
#pragma unroll
        for (int c = 0; c < NA1; ++c) {
          const bool ok = inimg && c * 16 + gsel * 8 < p.a1.C;
          const float* r0 = ldsU + c * (UBYTES / 4) + ((y0 - sy_base) * UP::SW) * 16 + gsel * 8;
          const float* r1 = ldsU + c * (UBYTES / 4) + ((y1 - sy_base) * UP::SW) * 16 + gsel * 8;
          const f32x4 a00 = *reinterpret_cast<const f32x4*>(r0 + o0), b00 = *reinterpret_cast<const f32x4*>(r0 + o0 + 4);
          const f32x4 a01 = *reinterpret_cast<const f32x4*>(r0 + o1), b01 = *reinterpret_cast<const f32x4*>(r0 + o1 + 4);
          const f32x4 a10 = *reinterpret_cast<const f32x4*>(r1 + o0), b10 = *reinterpret_cast<const f32x4*>(r1 + o0 + 4);
          const f32x4 a11 = *reinterpret_cast<const f32x4*>(r1 + o1), b11 = *reinterpret_cast<const f32x4*>(r1 + o1 + 4);
          f32x4 v0 = bilerp(wy0, wy1, wx0, wx1, a00, a01, a10, a11);
          f32x4 v1 = bilerp(wy0, wy1, wx0, wx1, b00, b01, b10, b11);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v0[j] = ok ? v0[j] : 0.f;
            v1[j] = ok ? v1[j] : 0.f;
          }
          store_halo(lds + (NA0 + c) * CH, idx, v0, v1);
        }
      }
    }
    __syncthreads();
    // ---- every load of the next tile goes in flight
    {
      const int w2 = w + GS;
      const bool live = w2 < wend;
      const int ws = live ? w2 : 0;
      issue(ws / ntiles, ((ws % ntiles) / tiles_x) * T, ((ws % ntiles) % tiles_x) * T, live);
    }
    // ---- z tile = A (*) W, K = (tap pair, 16 channels) per MFMA
    f32x4 acc[MI][CO];
#pragma unroll
    for (int m = 0; m < MI; ++m)
#pragma unroll
      for (int j = 0; j < CO; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int c = ks / 5, s = ks % 5;
      const unsigned char* cur = lds + c * CH;
      bf16x8 ah[MI], al[MI], bh[CO], bl[CO];
      if (!G::BREG) {
#pragma unroll
        for (int j = 0; j < CO; ++j) {
          bh[j] = ldsB[((ks * CO + j) * 2) * 64 + lane];
          bl[j] = ldsB[((ks * CO + j) * 2 + 1) * 64 + lane];
        }
      }
#pragma unroll
      for (int m = 0; m < MI; ++m) {
        ah[m] = *reinterpret_cast<const bf16x8*>(cur + aoff[m] + toff[s]);
        al[m] = *reinterpret_cast<const bf16x8*>(cur + aoff[m] + toff[s] + PL);
      }
#pragma unroll
      for (int m = 0; m < MI; ++m)
#pragma unroll
        for (int j = 0; j < CO; ++j) {
          if (G::BREG) { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, acc[m][j], pbh[G::BREG ? ks : 0][j], pbl[G::BREG ? ks : 0][j], ah[m], al[m]) }
          else { HPFG_MFMA3(LO_OF_FIRST_THEN_SECOND, acc[m][j], bh[j], bl[j], ah[m], al[m]) }
        }
    }
    // ---- epilogue: acc holds D[channel = 4 (lane >> 4) + r][pixel = lane & 15] -> one 16-byte store per lane and tile; BatchNorm sums
#pragma unroll
    for (int j = 0; j < CO; ++j) {
      const int co = j * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int m = 0; m < MI; ++m) {
        const int pxl = (wave * MI + m) * 16 + (lane & 15);
        const int pix = (n * H + ty0 + pxl / T) * W + tx0 + pxl % T;
        if (co < p.Cout) {
          const f32x4 v = acc[m][j] + bias[j];
          *reinterpret_cast<f32x4*>(p.out + pix * p.out_pstride + co) = v;
          s1[j] += v;
          s2[j] += v * v;
        }
      }
    }
    __syncthreads();                                     // this tile's LDS reads are done: the next one may be written
  }
  if (p.stat_partials || p.stat_acc) {
    // per-lane sums -> over the 16 pixel lanes -> over the waves; row blockIdx.x of stat_partials ([rows][2][CoutPad]): sum(z), sum(z^2)
    // (or, stat_acc: integer atomics into the layer accumulator)
#pragma unroll
    for (int j = 0; j < CO; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float a = s1[j][r], b = s2[j][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          a += __shfl_xor(a, o);
          b += __shfl_xor(b, o);
        }
        s1[j][r] = a;
        s2[j][r] = b;
      }
    constexpr int BN = 16 * CO;
    if ((lane & 15) == 0) {
#pragma unroll
      for (int j = 0; j < CO; ++j) {
        const int cl = j * 16 + (lane >> 4) * 4;
        *reinterpret_cast<f32x4*>(ldsf + (0 * NW + wave) * BN + cl) = s1[j];
        *reinterpret_cast<f32x4*>(ldsf + (1 * NW + wave) * BN + cl) = s2[j];
      }
    }
    __syncthreads();
    if (tid < 2 * BN) {
      const int which = tid / BN, cl = tid % BN;
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < NW; ++k) t += ldsf[(which * NW + k) * BN + cl];
      if (p.stat_acc && cl < p.Cout) hpfg_acc_add(p.stat_acc, p.CoutPad, (int)blockIdx.x & (p.stat_shards - 1), which, cl, t);
      if (p.stat_partials && cl < p.CoutPad) p.stat_partials[((long)blockIdx.x * 2 + which) * p.CoutPad + cl] = t;
    }
  }
}

// workgroups of the launch = rows of stat_partials
template <int CI, int CO, int AK, int NW, int WGS>
inline int thin_grid(const HpfgConvArgs& a) {
  const long nwork = (long)a.N * (a.H / T) * (a.W / T);
  int per_cu = 160 * 1024 / Geo<CI, CO, AK, NW>::LDS;
  if (per_cu > WGS) per_cu = WGS;
  if (per_cu < 1) per_cu = 1;
  const long cap = 256L * per_cu;
  const long rounds = (nwork + cap - 1) / cap;           // equal work per workgroup, all of them resident
  long grid = (nwork + rounds - 1) / rounds;
  grid = (grid + 7) / 8 * 8;                             // the same number of workgroups on every XCD
  return (int)(grid < cap ? grid : cap);
}

}  // namespace hpfg_thin
