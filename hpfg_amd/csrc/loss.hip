// Fused per-pixel segmentation losses on NHWC logits: softmax + cross-entropy(ignore 255) + Dice + MSE consistency, 2 <= C <= 16 classes
// (up to four: the ACDC-shaped configs; above: multi-organ labels, the reference's Synapse configs, num_classes 9).
//
// Reference arithmetic:
//   CE    nn.CrossEntropyLoss(ignore_index=255): mean over non-ignored pixels of -log softmax[target]
//         (main.py:92,164,167; utils/loss/medloss.py:49)
//   Dice  utils/loss/diceloss.py:155-191: one-hot by equality (ignored pixels match no class but still count in sum p^2),
//         per class 1 - (2*sum(p*t)+1e-5)/(sum(p*p)+sum(t*t)+1e-5) with sums over the whole batch, mean over classes
//   MSE   mean((softmax(student) - softmax(teacher))^2) over the unlabelled images (main.py:191, Mean-Teacher :104)
//   total = ce0*CE0 + dice0*Dice0 + ce1*CE1 + dice1*Dice1 + mse_w*MSE, two label groups: images [0,n_lab) with labels0,
//           images [n_lab,N) with labels1 (pseudo-labels; CPS :108-110, HPFG main.py:176-180).
// Dice is a ratio of batch-wide sums, so the op is two-phase: (1) partial sums -> sums (all-reduce them across ranks for
// data parallel), finalize -> scalars; (2) backward re-reads the logits and writes dlogits from the global sums.
// Nothing here synchronises with the host; the reference's per-class dice.item() (diceloss.py:189) has no counterpart.
//
// One kernel family, instantiated for every C:
//   - sums layout, hpfg_loss_nsum(C) = 8 + 6 * S floats with class stride S = 4 for C <= 4 and 16 above (32 or 104 floats): 0 nll0, 1 cnt0,
//     2 nll1, 3 cnt1, 4 mse (masked: sum mask*d^2), 5 sum mask, 6..7 unused, then 8 + g * 3 * S + k * S + c for label group g and
//     k = 0 / 1 / 2 = I (sum p t) / Z (sum p p) / Y (sum t t);
//   - the partial-sum kernel holds the Dice sums of ONE label group at a time: the group of a pixel is a property of its image (n < n_lab), so
//     a block's 1024 pixels fall into at most two contiguous segments, [p0, boundary) and [boundary, p1); each non-empty segment is
//     accumulated and reduced on its own (3 * C accumulators per thread instead of 6 * C: no scratch at C = 16);
//   - the backward kernel keeps the per-class Dice derivative coefficients in LDS (2 * 2 * 16 floats) instead of registers;
//   - C % 4 == 0: 16-byte loads / stores of logits, teacher logits and dlogits; other C: scalar accesses.
// Up to four classes the partial sums once came from a kernel of their own (all 6 * C accumulators in registers, pixels assigned to threads from
// the block start).  Against that kernel the sums of C <= 4 moved in the last bits, for exactly two reasons (tests/test_gpu_loss_bits.py):
//   1. Z adds p * p as one fma where that kernel added the rounded product (`on ? p * p : 0.f`); every other entry kept its bits;
//   2. a workgroup that straddles the label-group boundary at (n_lab * H * W - p0) % 256 != 0 assigns the second segment's pixels to threads
//      from the boundary, so the summation order inside that one workgroup differs (H * W a multiple of 1024: no workgroup straddles).
// Finalize and backward are pure functions of their inputs and kept every bit for every C.
#include <string.h>
#include "common.h"
#include "peer.h"

namespace {

constexpr int PIX_PER_BLOCK = 1024;
constexpr float SMOOTH = 1e-5f;
constexpr int OFF_I0 = 8;
constexpr int stride_of(int C) { return C <= 4 ? 4 : 16; }          // class slots per block of the layout
constexpr int nsum_of(int C) { return OFF_I0 + 6 * stride_of(C); }
static_assert(nsum_of(4) == HPFG_LOSS_NSUM && nsum_of(5) == HPFG_LOSS_NSUM_WIDE && nsum_of(16) == HPFG_LOSS_NSUM_WIDE, "sums layout");

// All per-pixel arrays are statically indexed (runtime-indexed register arrays would spill to scratch).
template <int C>
__device__ inline void load_px(const float* base, long pix, float* l) {
  if (C % 4 == 0) {
    const f32x4* b = reinterpret_cast<const f32x4*>(base + pix * C);
#pragma unroll
    for (int j = 0; j < C / 4; ++j) {
      f32x4 v = b[j];
      l[4 * j] = v[0]; l[4 * j + 1] = v[1]; l[4 * j + 2] = v[2]; l[4 * j + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = base[pix * C + c];
  }
}

template <int C>
__device__ inline void store_px(float* base, long pix, const float* g) {
  if (C % 4 == 0) {
    f32x4* b = reinterpret_cast<f32x4*>(base + pix * C);
#pragma unroll
    for (int j = 0; j < C / 4; ++j) b[j] = f32x4{g[4 * j], g[4 * j + 1], g[4 * j + 2], g[4 * j + 3]};
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) base[pix * C + c] = g[c];
  }
}

// softmax of l -> p; m = max, se = sum exp(l - m) (the cross-entropy reuses them)
template <int C>
__device__ inline void softmax_w(const float* l, float* p, float& m, float& se) {
  m = l[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, l[c]);
  se = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = expf(l[c] - m);
    se += p[c];
  }
  const float inv = 1.f / se;
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] *= inv;
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int C>
__global__ __launch_bounds__(256) void loss_partials_kernel(HpfgLossArgs a, long npix_img) {
  constexpr int S = stride_of(C), NS = nsum_of(C);
  __shared__ float red[4][NS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * NS; i += 256) (&red[0][0])[i] = 0.f;
  const long total = (long)a.N * npix_img;
  const long p0 = (long)blockIdx.x * PIX_PER_BLOCK;
  const long p1 = p0 + PIX_PER_BLOCK < total ? p0 + PIX_PER_BLOCK : total;
  const long pb = (long)a.n_lab * npix_img;          // first pixel of group 1
  __syncthreads();
#pragma nounroll
  for (int grp = 0; grp < 2; ++grp) {
    const long lo = grp == 0 ? p0 : (p0 > pb ? p0 : pb);
    const long hi = grp == 0 ? (p1 < pb ? p1 : pb) : p1;
    if (lo >= hi) continue;          // (uniform over the block)
    const uint8_t* lab = grp == 0 ? a.labels0 : a.labels1;
    const long lab_off = grp == 0 ? 0 : pb;
    const bool cons = grp == 1 && a.t_logits;
    float nll = 0.f, cnt = 0.f, mse = 0.f, msk = 0.f;
    float I[C], Z[C], Y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) I[c] = Z[c] = Y[c] = 0.f;
    for (long pix = lo + tid; pix < hi; pix += 256) {
      float l[C], p[C], m, se;
      load_px<C>(a.logits, pix, l);
      softmax_w<C>(l, p, m, se);          // (always: the cross-entropy term takes m and se from it, whatever p becomes)
      if (a.input_is_prob) {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = l[c];
      }
      if (lab) {
        const int t = lab[pix - lab_off];
        float lt = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) lt = (t == c) ? l[c] : lt;
        const bool valid = t != 255 && t < C;
        nll += valid ? (m + logf(se)) - lt : 0.f;
        cnt += valid ? 1.f : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float tc = (t == c) ? 1.f : 0.f;
          I[c] += p[c] * tc;
          Z[c] += p[c] * p[c];
          Y[c] += tc;
        }
      }
      if (cons) {
        float q[C], tl[C], tm, ts;
        const long upix = pix - pb;
        load_px<C>(a.t_logits, a.t_unlab_only ? upix : pix, tl);
        if (a.teacher_is_prob) {
#pragma unroll
          for (int c = 0; c < C; ++c) q[c] = tl[c];
        } else {
          softmax_w<C>(tl, q, tm, ts);
        }
        const float w = a.cons_mask ? a.cons_mask[upix] : 1.f;
        float dd = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float d = p[c] - q[c];
          dd += d * d;
        }
        mse += w * dd;
        msk += w;
      }
    }
    float* r = red[wave];
    const int base = OFF_I0 + grp * 3 * S;
    nll = wave_sum(nll);
    cnt = wave_sum(cnt);
    if (lane == 0) {
      r[2 * grp] = nll;
      r[2 * grp + 1] = cnt;
    }
    if (cons) {
      mse = wave_sum(mse);
      msk = wave_sum(msk);
      if (lane == 0) {
        r[4] = mse;
        r[5] = msk;
      }
    }
    if (lab) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float vi = wave_sum(I[c]), vz = wave_sum(Z[c]), vy = wave_sum(Y[c]);
        if (lane == 0) {
          r[base + c] = vi;
          r[base + S + c] = vz;
          r[base + 2 * S + c] = vy;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NS; i += 256) a.partials[(long)blockIdx.x * NS + i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}

// one block per sum index, fp64, fixed order, on rows of ns floats
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ partials, int nblk, int ns, float* __restrict__ sums, HpfgPeerX px) {
  __shared__ double sh[4];
  const int i = blockIdx.x;
  double v = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) v += (double)partials[(long)b * ns + i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[1] = {sh[0] + sh[1] + sh[2] + sh[3]};
    if (px.world > 1) {          // data parallel, global-batch mode: the ranks' sums of this term (peer mailbox, rank order)
      const int idx[1] = {i};
      hpfg_peer_allreduce<1>(px, idx, t);
    }
    sums[i] = (float)t[0];
  }
}

__device__ inline float dice_of(const float* s, int base, int S, int C) {
  float d = 0.f;
  for (int c = 0; c < C; ++c) d += 1.f - (2.f * s[base + c] + SMOOTH) / (s[base + S + c] + s[base + 2 * S + c] + SMOOTH);
  return d / (float)C;
}

__global__ void loss_finalize_kernel(HpfgLossArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float* s = a.sums;
  const int C = a.C, S = stride_of(C);
  float ce0 = s[1] > 0.f ? s[0] / s[1] : 0.f;
  float ce1 = s[3] > 0.f ? s[2] / s[3] : 0.f;
  float d0 = a.labels0 && a.n_lab > 0 ? dice_of(s, OFF_I0, S, C) : 0.f;
  float d1 = a.labels1 && a.n_lab < a.N ? dice_of(s, OFF_I0 + 3 * S, S, C) : 0.f;
  float cnt = (float)((double)(a.N - a.n_lab) * a.H * a.W * C * a.world);
  float mse = (a.t_logits && cnt > 0.f) ? (a.cons_mask ? s[4] / (2.f * s[5] + 1e-16f) : s[4] / cnt) : 0.f;
  const float* k = a.coef;
  a.out[0] = k[0] * ce0 + k[1] * d0 + k[2] * ce1 + k[3] * d1 + k[4] * mse;
  a.out[1] = ce0;
  a.out[2] = d0;
  a.out[3] = ce1;
  a.out[4] = d1;
  a.out[5] = mse;
  a.out[6] = 0.f;
  a.out[7] = 0.f;
}

template <int C>
__global__ __launch_bounds__(256) void loss_bwd_kernel(HpfgLossArgs a, long npix_img, const float* __restrict__ gscale_dev) {
  constexpr int S = stride_of(C), CW = 16;          // CW: class slots of the LDS tables, whatever S
  // per-group, per-class Dice derivative coefficients: dDice/dp_c = A_c * t_c + B_c * p_c
  __shared__ float cA[2][CW], cB[2][CW];
  const float gscale = gscale_dev ? *gscale_dev : 1.f;
  const float* s = a.sums;
  const float* k = a.coef;
  const long total = (long)a.N * npix_img;
  const long pb = (long)a.n_lab * npix_img;
  const float cnt_mse = (float)((double)(a.N - a.n_lab) * a.H * a.W * C * a.world);
  if (threadIdx.x < 2 * CW) {
    const int g = threadIdx.x / CW, c = threadIdx.x % CW;
    float ca = 0.f, cb = 0.f;
    if (c < C) {
      const int base = OFF_I0 + g * 3 * S;
      const float wd = k[2 * g + 1] / (float)C;
      const float den = s[base + S + c] + s[base + 2 * S + c] + SMOOTH;
      const float num = 2.f * s[base + c] + SMOOTH;
      ca = -2.f * wd / den;
      cb = 2.f * wd * num / (den * den);
    }
    cA[g][c] = ca;
    cB[g][c] = cb;
  }
  __syncthreads();
  const float wm = cnt_mse > 0.f ? k[4] * 2.f / (a.cons_mask ? 2.f * s[5] + 1e-16f : cnt_mse) : 0.f;
  for (long pix = blockIdx.x * 256L + threadIdx.x; pix < total; pix += (long)gridDim.x * 256) {
    const int grp = pix < pb ? 0 : 1;
    float l[C], p[C], dp[C], m, se;
    load_px<C>(a.logits, pix, l);
    if (a.input_is_prob) {
#pragma unroll
      for (int c = 0; c < C; ++c) p[c] = l[c];
    } else {
      softmax_w<C>(l, p, m, se);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dp[c] = 0.f;
    const uint8_t* lab = grp == 0 ? a.labels0 : a.labels1;
    int t = 255;
    if (lab) {
      t = grp == 0 ? lab[pix] : lab[pix - pb];
      const float* ga = cA[grp];
      const float* gb = cB[grp];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float tc = (t == c) ? 1.f : 0.f;
        dp[c] += ga[c] * tc + gb[c] * p[c];
      }
    }
    if (grp == 1 && a.t_logits) {
      float q[C], tl[C], tm, ts;
      const long upix = pix - pb;
      load_px<C>(a.t_logits, a.t_unlab_only ? upix : pix, tl);
      if (a.teacher_is_prob) {
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = tl[c];
      } else {
        softmax_w<C>(tl, q, tm, ts);
      }
      const float w = a.cons_mask ? wm * a.cons_mask[upix] : wm;
#pragma unroll
      for (int c = 0; c < C; ++c) dp[c] += w * (p[c] - q[c]);
    }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) dot += p[c] * dp[c];
    const float cn = s[2 * grp + 1];
    const float wc = k[2 * grp];
    const bool ce_on = lab && t != 255 && t < C && cn > 0.f;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      g[c] = a.input_is_prob ? dp[c] : p[c] * (dp[c] - dot);
      if (ce_on && !a.input_is_prob) g[c] += wc * (p[c] - (t == c ? 1.f : 0.f)) / cn;
      g[c] *= gscale;
    }
    store_px<C>(a.dlogits, pix, g);
  }
}

// C -> instantiation (2..16; check_loss has refused every other C)
#define HPFG_LOSS_CASE(N_, ...) case N_: { constexpr int C = N_; __VA_ARGS__; } break;
#define HPFG_LOSS_DISPATCH(C_, ...) \
  switch (C_) {                      \
    HPFG_LOSS_CASE(2, __VA_ARGS__) HPFG_LOSS_CASE(3, __VA_ARGS__) HPFG_LOSS_CASE(4, __VA_ARGS__) HPFG_LOSS_CASE(5, __VA_ARGS__) HPFG_LOSS_CASE(6, __VA_ARGS__)      \
    HPFG_LOSS_CASE(7, __VA_ARGS__) HPFG_LOSS_CASE(8, __VA_ARGS__) HPFG_LOSS_CASE(9, __VA_ARGS__) HPFG_LOSS_CASE(10, __VA_ARGS__) HPFG_LOSS_CASE(11, __VA_ARGS__)    \
    HPFG_LOSS_CASE(12, __VA_ARGS__) HPFG_LOSS_CASE(13, __VA_ARGS__) HPFG_LOSS_CASE(14, __VA_ARGS__) HPFG_LOSS_CASE(15, __VA_ARGS__) HPFG_LOSS_CASE(16, __VA_ARGS__) \
    default: HPFG_ARG_CHECK(false, "seg_loss: C must be 2..16 (got %d)", C_); \
  }

}  // namespace

extern "C" int hpfg_loss_blocks(int N, int H, int W) { return (int)(((long)N * H * W + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK); }

// floats of one row of `partials` and of `sums` (the layout above)
extern "C" int hpfg_loss_nsum(int C) { return nsum_of(C); }

static int check_loss(const HpfgLossArgs* a) {
  HPFG_ARG_CHECK(a && a->logits && a->coef && a->sums, "seg_loss: null pointer");
  HPFG_ARG_CHECK(a->C >= 2 && a->C <= 16, "seg_loss: C must be 2..16 (got %d)", a->C);
  HPFG_ARG_CHECK(a->N > 0 && a->n_lab >= 0 && a->n_lab <= a->N && a->H > 0 && a->W > 0 && a->world >= 1, "seg_loss: bad sizes");
  HPFG_ARG_CHECK(a->n_lab == 0 || a->labels0, "seg_loss: labels0 missing");
  return 0;
}

static int loss_partials_impl(const HpfgLossArgs* a, const HpfgPeerX* px, void* stream) {
  if (int rc = check_loss(a)) return rc;
  HPFG_ARG_CHECK(a->partials, "seg_loss_partials: workspace missing");
  const int nblk = hpfg_loss_blocks(a->N, a->H, a->W), ns = nsum_of(a->C);
  const long npix = (long)a->H * a->W;
  HPFG_LOSS_DISPATCH(a->C, hipLaunchKernelGGL(loss_partials_kernel<C>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, *a, npix));
  HpfgPeerX none;
  memset(&none, 0, sizeof(none));
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(ns), dim3(256), 0, (hipStream_t)stream, a->partials, nblk, ns, a->sums, px ? *px : none);
  return hpfg_launch_status("loss_partials_kernel");
}

extern "C" int hpfg_seg_loss_partials(const HpfgLossArgs* a, void* stream) { return loss_partials_impl(a, nullptr, stream); }

extern "C" int hpfg_seg_loss_partials_x(const HpfgLossArgs* a, const HpfgPeerX* px, void* stream) {
  HPFG_ARG_CHECK(px, "seg_loss_partials_x: null exchange descriptor");
  if (int rc = check_loss(a)) return rc;
  if (px->world > 1) {
    HPFG_ARG_CHECK(px->world <= HPFG_PEER_MAX_RANKS && px->rank >= 0 && px->rank < px->world && px->epoch && px->slot >= 0 &&
                       hpfg_loss_nsum(a->C) <= px->cap && px->slot_bytes == hpfg_peer_slot_bytes(px->world, px->cap),
                   "seg_loss_partials_x: bad exchange descriptor");
    for (int r = 0; r < px->world; ++r) HPFG_ARG_CHECK(px->mbox[r], "seg_loss_partials_x: mailbox of rank %d not mapped", r);
  }
  return loss_partials_impl(a, px, stream);
}

extern "C" int hpfg_seg_loss_finalize(const HpfgLossArgs* a, void* stream) {
  if (int rc = check_loss(a)) return rc;
  HPFG_ARG_CHECK(a->out, "seg_loss_finalize: out missing");
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a);
  return hpfg_launch_status("loss_finalize_kernel");
}

extern "C" int hpfg_seg_loss_bwd(const HpfgLossArgs* a, const float* grad_scale_dev, void* stream) {
  if (int rc = check_loss(a)) return rc;
  HPFG_ARG_CHECK(a->dlogits, "seg_loss_bwd: dlogits missing");
  const long npix = (long)a->H * a->W, total = a->N * npix;
  long b = (total + 255) / 256;
  if (b > 4096) b = 4096;
  HPFG_LOSS_DISPATCH(a->C, hipLaunchKernelGGL(loss_bwd_kernel<C>, dim3((int)b), dim3(256), 0, (hipStream_t)stream, *a, npix, grad_scale_dev));
  return hpfg_launch_status("loss_bwd_kernel");
}
