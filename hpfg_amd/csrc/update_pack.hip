// SGD (+ EMA teacher) update over the flat buffers that also writes the split-bf16 MFMA weight fragments of every packed conv layer, so that
// the next forward of the student (and of the teacher) starts without a pack_weights launch.  The update arithmetic is sgd_kernel's /
// sgd_ema_kernel's (misc.hip), the fragment values and positions are those of pack_weights_kernel's bf16x3 section: both bit for bit.
#include "common.h"

namespace {

constexpr int UP_ROW = 16 * 9 + 1;      // LDS row of one output channel: 16 input channels x 9 taps (+1: the dgrad reads walk down a column)
constexpr int UP_MAX_LAYERS = 32, UP_MAX_GAPS = 64;      // (the U-Net: 22 packed layers, 23 gaps)
constexpr int UP_CHUNK = 1024;      // elements of a gap one workgroup updates

struct UpArgs {
  float* p;
  const float* g;
  float* mom;
  float* t;      // or NULL
  long n, n_ema;
  const float* lr_dev;
  const float* alpha_dev;      // or NULL (no teacher)
  float momentum, wd, gscale;
  const HpfgUpdatePackDesc* table;
  int nlayers;
  const long* gaps;      // [ngaps][2]: the ranges [lo, hi) of the flat buffer no descriptor owns
  int ngaps;
  // the 1-D grid: workgroups [wg0[y], wg0[y + 1]) own the blocks of layer y, [gwg0[k], gwg0[k + 1]) the UP_CHUNK-element pieces of gap k
  // (by value, read with constant indices only: they stay in scalar registers)
  int wg0[UP_MAX_LAYERS + 1];
  int gwg0[UP_MAX_GAPS + 1];
};

// the expressions of sgd_kernel / sgd_ema_kernel (misc.hip) in their order: new momentum *b, new weight *s, new teacher value *tn
__device__ __forceinline__ void update_math(const UpArgs& a, float w, float g, float m, float tv, float lr, float al, float* b, float* s, float* tn) {
#pragma clang fp contract(off)      // separately rounded products, as in misc.hip: the fused and the separate launches agree bit for bit
  float d = g * a.gscale + a.wd * w;
  *b = a.momentum * m + d;
  *s = w - lr * *b;
  *tn = tv * al + *s * (1.f - al);
}

// one flat element.  Returns the new weight, *tn the new teacher value (0 without a teacher).
__device__ __forceinline__ float update_elem(const UpArgs& a, long i, float lr, float al, float* tn) {
  const bool has_t = a.t && i < a.n_ema;
  float b, s, tv;
  update_math(a, a.p[i], a.g[i], a.mom[i], has_t ? a.t[i] : 0.f, lr, al, &b, &s, &tv);
  a.mom[i] = b;
  a.p[i] = s;
  if (has_t) a.t[i] = tv;
  *tn = has_t ? tv : 0.f;
  return s;
}

// the 16 co x 16 ci x TAPS block at (co0, ci0) of layer d: every load of the thread's elements is issued before the first store (the
// buffers do not overlap; an element-by-element loop would wait for memory PER times in a row), new weights into sw, new teacher values into st
template <int TAPS>
__device__ __forceinline__ void update_block(const UpArgs& a, const HpfgUpdatePackDesc& d, int co0, int ci0, float lr, float al, float* sw, float* st) {
  constexpr int ROW = 16 * TAPS, PER = 16 * ROW / 256;
  float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  float* __restrict__ mom = a.mom;
  float* __restrict__ t = a.t;
  long idx[PER];
  float w[PER], gv[PER], mv[PER], tv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = threadIdx.x + 256 * k, r = e / ROW, q = e % ROW;      // q = ci_local * TAPS + tap: contiguous in the OIHW row
    idx[k] = (co0 + r < d.Cout && ci0 + q / TAPS < d.Cin) ? d.w_off + ((long)(co0 + r) * d.Cin + ci0) * TAPS + q : -1;
    w[k] = gv[k] = mv[k] = tv[k] = 0.f;
    if (idx[k] >= 0) {
      w[k] = p[idx[k]];
      gv[k] = g[idx[k]];
      mv[k] = mom[idx[k]];
      if (t && idx[k] < a.n_ema) tv[k] = t[idx[k]];
    }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int e = threadIdx.x + 256 * k, r = e / ROW, q = e % ROW;
    float b, s = 0.f, tn = 0.f;
    if (idx[k] >= 0) {
      update_math(a, w[k], gv[k], mv[k], tv[k], lr, al, &b, &s, &tn);
      mom[idx[k]] = b;
      p[idx[k]] = s;
      if (t && idx[k] < a.n_ema) t[idx[k]] = tn;
      else tn = 0.f;
    }
    sw[r * UP_ROW + q] = s;
    st[r * UP_ROW + q] = tn;
  }
}

// the piece [lo, hi) of a gap, hi - lo <= UP_CHUNK: loads first, then stores, as in update_block
__device__ __forceinline__ void update_chunk(const UpArgs& a, long lo, long hi, float lr, float al) {
  constexpr int PER = UP_CHUNK / 256;
  float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  float* __restrict__ mom = a.mom;
  float* __restrict__ t = a.t;
  float w[PER], gv[PER], mv[PER], tv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const long i = lo + threadIdx.x + 256 * k;
    w[k] = gv[k] = mv[k] = tv[k] = 0.f;
    if (i < hi) {
      w[k] = p[i];
      gv[k] = g[i];
      mv[k] = mom[i];
      if (t && i < a.n_ema) tv[k] = t[i];
    }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const long i = lo + threadIdx.x + 256 * k;
    if (i < hi) {
      float b, s, tn;
      update_math(a, w[k], gv[k], mv[k], tv[k], lr, al, &b, &s, &tn);
      mom[i] = b;
      p[i] = s;
      if (t && i < a.n_ema) t[i] = tn;
    }
  }
}

struct bf16x8 {
  __bf16 v[8];
} __attribute__((aligned(16)));

// hi / lo planes of eight consecutive contraction channels: the split of pack_weights_kernel
__device__ __forceinline__ void store_split8(__bf16* out, long base, int lane, const float* w8) {
  bf16x8 hi, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)w8[j];
    hi.v[j] = h;
    lo.v[j] = (__bf16)(w8[j] - (float)h);
  }
  *reinterpret_cast<bf16x8*>(out + (base + 0) * 512 + lane * 8) = hi;
  *reinterpret_cast<bf16x8*>(out + (base + 1) * 512 + lane * 8) = lo;
}

// k-step and lane quarter of the eight contraction channels k0 + 8 g .. + 7 (k0 a multiple of 16) at `tap` (pack_weights_kernel inverted):
// taps == 1: one k-step per 32 channels; kc == 32: nine, one per tap; kc == 16: five, two taps x 16 channels each (tap 9 is padding)
__device__ __forceinline__ void frag_pos(int taps, int kc, int k0, int g, int tap, int* ks, int* lq) {
  if (taps == 1) {
    *ks = k0 / 32;
    *lq = (k0 % 32) / 8 + g;
  } else if (kc == 32) {
    *ks = (k0 / 32) * 9 + tap;
    *lq = (k0 % 32) / 8 + g;
  } else {
    *ks = (k0 / 16) * 5 + tap / 2;
    *lq = (tap & 1) * 2 + g;
  }
}

// fwd fragments of the 16 x 16 x taps block in `sw`: contraction = input channel, column = output channel
__device__ __forceinline__ void emit_fwd(__bf16* out, const float* sw, int taps, int kc, int co0, int ci0, int CoutPad) {
  const int ntn = CoutPad / 16;
  for (int it = threadIdx.x; it < 32 * taps; it += 256) {
    const int r = it & 15, g = (it >> 4) & 1, tap = it >> 5;
    float w8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w8[j] = sw[r * UP_ROW + (g * 8 + j) * taps + tap];
    int ks, lq;
    frag_pos(taps, kc, ci0, g, tap, &ks, &lq);
    store_split8(out, ((long)ks * ntn + co0 / 16) * 2, lq * 16 + r, w8);
  }
}

// dgrad fragments: contraction = output channel, column = input channel, taps flipped
__device__ __forceinline__ void emit_dgrad(__bf16* out, const float* sw, int taps, int kc, int co0, int ci0, int CinPad) {
  const int ntn = CinPad / 16;
  for (int it = threadIdx.x; it < 32 * taps; it += 256) {
    const int c = it & 15, g = (it >> 4) & 1, tap = it >> 5;
    float w8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w8[j] = sw[(g * 8 + j) * UP_ROW + c * taps + (taps - 1 - tap)];
    int ks, lq;
    frag_pos(taps, kc, co0, g, tap, &ks, &lq);
    store_split8(out, ((long)ks * ntn + ci0 / 16) * 2, lq * 16 + c, w8);
  }
}

// One workgroup per 16 co x 16 ci x taps block of a layer's conv weight (the first of a layer also takes its bias), then one per gap piece.
__global__ __launch_bounds__(256) HPFG_NO_PK_F32 void sgd_ema_pack_kernel(UpArgs a) {
  __shared__ float sw[16 * UP_ROW], st[16 * UP_ROW];
  const float lr = *a.lr_dev, al = a.alpha_dev ? *a.alpha_dev : 0.f;
  const int b = blockIdx.x;
  if (b >= a.wg0[UP_MAX_LAYERS]) {
    const int c = b - a.wg0[UP_MAX_LAYERS];
    int k = 0, base = 0;
#pragma unroll
    for (int i = 1; i < UP_MAX_GAPS; ++i)
      if (i < a.ngaps && c >= a.gwg0[i]) {
        k = i;
        base = a.gwg0[i];
      }
    const long lo = a.gaps[2 * k] + (long)(c - base) * UP_CHUNK, end = a.gaps[2 * k + 1];
    update_chunk(a, lo, lo + UP_CHUNK < end ? lo + UP_CHUNK : end, lr, al);
    return;
  }
  int y = 0, first = 0;
#pragma unroll
  for (int i = 1; i < UP_MAX_LAYERS; ++i)
    if (i < a.nlayers && b >= a.wg0[i]) {
      y = i;
      first = a.wg0[i];
    }
  const HpfgUpdatePackDesc d = a.table[y];
  const int taps = d.taps, blk = b - first;
  const int nib = (d.Cin + 15) / 16;
  if (blk == 0) {      // the bias: updated, and copied into the padded rows the conv kernels read
    for (int i = threadIdx.x; i < d.CoutPad; i += 256) {
      float tn = 0.f, s = 0.f;
      if (i < d.Cout) s = update_elem(a, d.b_off + i, lr, al, &tn);
      d.bias_pad[i] = s;
      if (d.t_bias_pad) d.t_bias_pad[i] = tn;
    }
  }
  const int co0 = (blk / nib) * 16, ci0 = (blk % nib) * 16;
  if (taps == 9) update_block<9>(a, d, co0, ci0, lr, al, sw, st);
  else update_block<1>(a, d, co0, ci0, lr, al, sw, st);
  __syncthreads();
  if (d.wpk16_fwd) emit_fwd(reinterpret_cast<__bf16*>(d.wpk16_fwd), sw, taps, d.kc, co0, ci0, d.CoutPad);
  if (d.wpk16_dgrad) emit_dgrad(reinterpret_cast<__bf16*>(d.wpk16_dgrad), sw, taps, d.kc, co0, ci0, d.CinPad);
  if (d.t_wpk16_fwd) emit_fwd(reinterpret_cast<__bf16*>(d.t_wpk16_fwd), st, taps, d.kc_t, co0, ci0, d.CoutPad);
}

}  // namespace

extern "C" int hpfg_sgd_ema_pack_step(float* p, const float* g, float* mom, long n, const float* lr_dev, float momentum, float weight_decay,
                                      float grad_scale, float* t, long n_ema, const float* alpha_dev, const HpfgUpdatePackDesc* table_dev,
                                      const HpfgUpdatePackDesc* table_host, int nlayers, const long* gaps_dev, const long* gaps_host, int ngaps,
                                      void* stream) {
  HPFG_ARG_CHECK(p && g && mom && lr_dev && n > 0, "sgd_ema_pack_step: bad args");
  HPFG_ARG_CHECK((t == nullptr) == (alpha_dev == nullptr) && t != p && n_ema >= 0 && n_ema <= n && (t || n_ema == 0), "sgd_ema_pack_step: bad teacher args");
  HPFG_ARG_CHECK(table_dev && table_host && nlayers > 0 && nlayers <= UP_MAX_LAYERS && gaps_dev && gaps_host && ngaps >= 0 && ngaps <= UP_MAX_GAPS,
                 "sgd_ema_pack_step: bad tables (at most %d layers, %d gaps)", UP_MAX_LAYERS, UP_MAX_GAPS);
  UpArgs a = {p, g, mom, t, n, n_ema, lr_dev, alpha_dev, momentum, weight_decay, grad_scale, table_dev, nlayers, gaps_dev, ngaps, {0}, {0}};
  // the descriptors (ascending, weight then bias of a layer) and the gaps between them must tile [0, n) exactly: every element is updated once
  long at = 0, wgs = 0;
  int k = 0;
  auto gap_to = [&](long lo) {
    if (at == lo) return true;
    if (k >= ngaps || gaps_host[2 * k] != at || gaps_host[2 * k + 1] != lo) return false;
    ++k;
    at = lo;
    return true;
  };
  for (int i = 0; i < nlayers; ++i) {
    const HpfgUpdatePackDesc& d = table_host[i];
    HPFG_ARG_CHECK(d.Cout > 0 && d.Cin > 0 && d.CinPad % 16 == 0 && d.CoutPad % 16 == 0 && d.Cin <= d.CinPad && d.Cout <= d.CoutPad && (d.taps == 1 || d.taps == 9),
                   "sgd_ema_pack_step: bad descriptor %d", i);
    HPFG_ARG_CHECK(d.bias_pad && (d.kc == 32 || (d.kc == 16 && d.taps == 9)) && (!d.t_wpk16_fwd || d.kc_t == 32 || (d.kc_t == 16 && d.taps == 9)),
                   "sgd_ema_pack_step: bad kc or bias row in descriptor %d", i);
    HPFG_ARG_CHECK((!d.t_wpk16_fwd && !d.t_bias_pad) || t, "sgd_ema_pack_step: descriptor %d has teacher fragments but there is no teacher", i);
    const long wn = (long)d.Cout * d.Cin * d.taps;
    HPFG_ARG_CHECK(d.w_off >= at && gap_to(d.w_off), "sgd_ema_pack_step: weight of descriptor %d is out of order or the gaps do not match", i);
    at += wn;
    HPFG_ARG_CHECK(d.b_off >= at && gap_to(d.b_off), "sgd_ema_pack_step: bias of descriptor %d is out of order or the gaps do not match", i);
    at += d.Cout;
    HPFG_ARG_CHECK(at <= n && (!(d.t_wpk16_fwd || d.t_bias_pad) || at <= n_ema), "sgd_ema_pack_step: descriptor %d ends behind the updated range", i);
    a.wg0[i] = (int)wgs;
    wgs += (long)((d.Cout + 15) / 16) * ((d.Cin + 15) / 16);
  }
  HPFG_ARG_CHECK(gap_to(n) && k == ngaps, "sgd_ema_pack_step: descriptors and gaps do not tile the %ld elements", n);
  for (int i = nlayers; i <= UP_MAX_LAYERS; ++i) a.wg0[i] = (int)wgs;      // (wg0[UP_MAX_LAYERS]: the first gap workgroup)
  long gw = 0;
  for (int i = 0; i <= UP_MAX_GAPS; ++i) {
    a.gwg0[i] = (int)gw;
    if (i < ngaps) gw += (gaps_host[2 * i + 1] - gaps_host[2 * i] + UP_CHUNK - 1) / UP_CHUNK;
  }
  HPFG_ARG_CHECK(wgs + gw < (1L << 30), "sgd_ema_pack_step: too many workgroups");
  hipLaunchKernelGGL(sgd_ema_pack_kernel, dim3((unsigned)(wgs + gw)), dim3(256), 0, (hipStream_t)stream, a);
  return hpfg_launch_status("sgd_ema_pack_kernel");
}
