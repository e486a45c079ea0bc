// Swin-MAE pretraining pieces (reference model/swin_mae.py:649-710 window_masking, :621-633 patchify, :775-791 forward_loss; the driver's loss
// 2022_12_CVPR_Swin-MAE.py:112) as kernels: the window mask from a noise tensor, the mask-token substitution with its backward, and the masked
// reconstruction loss with its gradient.  Everything the reference does on the host here (np.setdiff1d, .cpu().numpy(), per-image loops) is
// device work on the caller's stream, so a step that uses them can be captured into a hipGraph.  Reductions: per-workgroup partials written to
// scratch, then one finishing kernel that adds them in index order -- no float atomics, equal bits from run to run.
#include "common.h"

#define MAE_NT 256
#define MAE_MAX_GROUPS 1024

static inline unsigned mae_grid_cap(long work, long cap) {
  long b = (work + MAE_NT - 1) / MAE_NT;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- window mask -------------------------------------------------------------------------------------------------------------------------
// One workgroup per image.  rank(g) = #{j : (noise[j], j) < (noise[g], g)}, counted against the image's noise row held in LDS: a total order,
// so the ranks are a permutation of 0 .. n-1 whatever the values are; group g is kept iff rank(g) < n_keep (argsort(noise)[:n_keep]).
__global__ __launch_bounds__(MAE_NT) void mae_window_mask_kernel(const float* __restrict__ noise, uint8_t* __restrict__ mask, int S, int r, int d,
                                                                 int n_keep) {
  __shared__ float v[MAE_MAX_GROUPS];
  __shared__ uint8_t removed[MAE_MAX_GROUPS];
  const int n = d * d, b = blockIdx.x, tid = threadIdx.x;
  for (int g = tid; g < n; g += MAE_NT) v[g] = noise[(long)b * n + g];
  __syncthreads();
  for (int g = tid; g < n; g += MAE_NT) {
    const float mine = v[g];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float o = v[j];
      rank += (o < mine || (o == mine && j < g)) ? 1 : 0;
    }
    removed[g] = rank < n_keep ? 0 : 1;
  }
  __syncthreads();
  uint8_t* m = mask + (long)b * S * S;
  if (r % 4 == 0) {          // four neighbouring tokens of a row lie in one group: one 32-bit store (S % 4 == 0 follows from S % r == 0)
    const int S4 = S / 4;
    for (int t = tid; t < S * S4; t += MAE_NT) {
      const int y = t / S4, x = (t - y * S4) * 4;
      const uint32_t one = removed[(y / r) * d + x / r];
      reinterpret_cast<uint32_t*>(m)[t] = one * 0x01010101u;
    }
  } else {
    for (int t = tid; t < S * S; t += MAE_NT) {
      const int y = t / S, x = t - y * S;
      m[t] = removed[(y / r) * d + x / r];
    }
  }
}

extern "C" int hpfg_mae_window_mask(const float* noise, uint8_t* mask, int B, int S, int r, int n_keep, void* stream) {
  HPFG_ARG_CHECK(noise && mask && B > 0 && S > 0 && r > 0 && S % r == 0, "mae_window_mask: bad args (null pointer, B %d, token side %d, group side %d: S %% r == 0)",
                 B, S, r);
  const int d = S / r;
  HPFG_ARG_CHECK(d * d <= MAE_MAX_GROUPS, "mae_window_mask: %d x %d groups; one workgroup ranks at most %d", d, d, MAE_MAX_GROUPS);
  HPFG_ARG_CHECK(n_keep >= 0 && n_keep <= d * d, "mae_window_mask: n_keep %d outside 0 .. %d", n_keep, d * d);
  hipLaunchKernelGGL(mae_window_mask_kernel, dim3(B), dim3(MAE_NT), 0, (hipStream_t)stream, noise, mask, S, r, d, n_keep);
  return hpfg_launch_status("mae_window_mask_kernel");
}

// ---- mask-token substitution ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAE_NT) void mae_mask_tokens_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ token, float* __restrict__ y, int C4, long total4) {
  for (long i = (long)blockIdx.x * MAE_NT + threadIdx.x; i < total4; i += (long)gridDim.x * MAE_NT) {
    const long row = i / C4;
    const int c4 = (int)(i - row * C4);
    const f32x4 v = mask[row] ? reinterpret_cast<const f32x4*>(token)[c4] : reinterpret_cast<const f32x4*>(x)[i];      // a masked row of x is not read
    reinterpret_cast<f32x4*>(y)[i] = v;
  }
}

extern "C" int hpfg_mae_mask_tokens_fwd(const float* x, const uint8_t* mask, const float* token, float* y, long rows, int C, void* stream) {
  HPFG_ARG_CHECK(x && mask && token && y && rows > 0 && C % 4 == 0 && C >= 4 && C <= 1536,
                 "mae_mask_tokens_fwd: bad args (null pointer, rows %ld, C %d: C %% 4 == 0, 4 <= C <= 1536)", rows, C);
  const long total4 = rows * (C / 4);
  hipLaunchKernelGGL(mae_mask_tokens_fwd_kernel, dim3(mae_grid_cap(total4, 8192)), dim3(MAE_NT), 0, (hipStream_t)stream, x, mask, token, y, C / 4, total4);
  return hpfg_launch_status("mae_mask_tokens_fwd_kernel");
}

extern "C" int hpfg_mae_mask_tokens_bwd_blocks(long rows) {
  long b = (rows + 63) / 64;
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

// Workgroup k owns rows [k per, (k + 1) per).  C / 4 <= 256: the threads form 256 / (C / 4) row lanes x C / 4 column quads, a row lane walks its
// rows in order, lane 0 then adds the lanes' sums in lane order; wider rows: one lane, the quads in passes of 256.  part[k][C] = the
// workgroup's sum of dy over its masked rows (zeros for a workgroup without rows).
__global__ __launch_bounds__(MAE_NT) HPFG_NO_PK_F32 void mae_mask_tokens_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ mask,
                                                                                    float* __restrict__ dx, float* __restrict__ part, long rows, int C4,
                                                                                    int per) {
  __shared__ f32x4 lane_sum[MAE_NT];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * per;
  const long r1 = r0 + per < rows ? r0 + per : rows;
  const bool narrow = C4 <= MAE_NT;
  const int lanes = narrow ? MAE_NT / C4 : 1;
  for (int cb = 0; cb < C4; cb += MAE_NT) {          // (one pass when narrow)
    const int lane = narrow ? tid / C4 : 0;
    const int c4 = narrow ? tid - lane * C4 : cb + tid;
    const bool active = narrow ? lane < lanes : c4 < C4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      for (long row = r0 + lane; row < r1; row += lanes) {
        const f32x4 g = reinterpret_cast<const f32x4*>(dy)[row * C4 + c4];
        const bool m = mask[row] != 0;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f32x4*>(dx)[row * C4 + c4] = m ? zero : g;
        if (m) {
          acc[0] += g[0];
          acc[1] += g[1];
          acc[2] += g[2];
          acc[3] += g[3];
        }
      }
    }
    if (lanes > 1) {
      lane_sum[tid] = acc;
      __syncthreads();
      if (active && lane == 0) {
        for (int k = 1; k < lanes; ++k) {
          const f32x4 o = lane_sum[k * C4 + c4];
          acc[0] += o[0];
          acc[1] += o[1];
          acc[2] += o[2];
          acc[3] += o[3];
        }
      }
      __syncthreads();
    }
    if (active && lane == 0) reinterpret_cast<f32x4*>(part)[(long)blockIdx.x * C4 + c4] = acc;
  }
}

// out[c] = sum over k of part[k][c], the finishing pass of the reduction above, in a fixed order: a workgroup owns 32 channels, its 8 lanes per
// channel add part[j], part[j + 8], ... (ascending; the loads of a lane do not depend on each other, so they are in flight together -- one thread
// walking all 512 partials is one L2 round trip per partial), lane 0 then adds the 8 lane sums in lane order
#define MAE_FIN_C 32
#define MAE_FIN_LANES (MAE_NT / MAE_FIN_C)
__global__ __launch_bounds__(MAE_NT) void mae_col_finish_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ out) {
  __shared__ float lane_sum[MAE_FIN_LANES][MAE_FIN_C];
  const int cl = threadIdx.x % MAE_FIN_C, lane = threadIdx.x / MAE_FIN_C;
  const int c = blockIdx.x * MAE_FIN_C + cl;
  float s = 0.f;
  if (c < C) {
#pragma unroll 8
    for (int k = lane; k < nblk; k += MAE_FIN_LANES) s += part[(long)k * C + c];
  }
  lane_sum[lane][cl] = s;
  __syncthreads();
  if (lane == 0 && c < C) {
    float t = lane_sum[0][cl];
    for (int j = 1; j < MAE_FIN_LANES; ++j) t += lane_sum[j][cl];
    out[c] = t;
  }
}

extern "C" int hpfg_mae_mask_tokens_bwd(const float* dy, const uint8_t* mask, float* dx, float* dtoken, float* partials, long rows, int C, void* stream) {
  HPFG_ARG_CHECK(dy && mask && dx && dtoken && partials && rows > 0 && C % 4 == 0 && C >= 4 && C <= 1536,
                 "mae_mask_tokens_bwd: bad args (null pointer, rows %ld, C %d: C %% 4 == 0, 4 <= C <= 1536)", rows, C);
  const int nblk = hpfg_mae_mask_tokens_bwd_blocks(rows);
  const int per = (int)((rows + nblk - 1) / nblk);
  hipLaunchKernelGGL(mae_mask_tokens_bwd_kernel, dim3(nblk), dim3(MAE_NT), 0, (hipStream_t)stream, dy, mask, dx, partials, rows, C / 4, per);
  int rc = hpfg_launch_status("mae_mask_tokens_bwd_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mae_col_finish_kernel, dim3((C + MAE_FIN_C - 1) / MAE_FIN_C), dim3(MAE_NT), 0, (hipStream_t)stream, partials, nblk, C, dtoken);
  return hpfg_launch_status("mae_col_finish_kernel");
}

// ---- masked reconstruction loss ------------------------------------------------------------------------------------------------------------
// the workgroup's sum of s[0 .. 256) by halving: the same tree whatever the values, thread 0 returns it
__device__ __forceinline__ float mae_block_sum(float* s, int tid) {
  __syncthreads();
  for (int w = MAE_NT / 2; w > 0; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w];
    __syncthreads();
  }
  return s[0];
}

// One thread per token (b, h, w).  A kept token writes D zeros of dpred and reads nothing else.  A masked one gathers its patch
// target[(p 4 + q) CIN + c] = img[b][c][4 h + p][4 w + q] (patchify's 'nchpwq->nhwpqc') with one 16-byte load per (c, p), optionally normalises it
// (mean and unbiased variance over the D values, eps 1e-6, forward_loss :782-785), then walks its pred row once: the squared differences into its
// sum (j ascending), g (pred - target) into dpred.  part[workgroup] = the tree sum of the 256 token sums.
template <int CIN>
__global__ __launch_bounds__(MAE_NT) HPFG_NO_PK_F32 void mae_loss_kernel(const float* __restrict__ pred, const float* __restrict__ img,
                                                                         const uint8_t* __restrict__ mask, float* __restrict__ dpred,
                                                                         float* __restrict__ part, long tokens, int Hp, int Wp, float g, int norm_pix) {
  constexpr int D = 16 * CIN;
  __shared__ float sums[MAE_NT];
  const int tid = threadIdx.x;
  const long tok = (long)blockIdx.x * MAE_NT + tid;
  float mine = 0.f;
  if (tok < tokens) {
    f32x4* dp = reinterpret_cast<f32x4*>(dpred + tok * D);
    if (!mask[tok]) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < D / 4; ++j) dp[j] = zero;
    } else {
      const int w = (int)(tok % Wp), h = (int)((tok / Wp) % Hp);
      const long b = tok / ((long)Wp * Hp);
      const long W = 4L * Wp, H = 4L * Hp;
      float t[D];
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(img + ((b * CIN + c) * H + 4 * h + p) * W + 4 * w);
#pragma unroll
          for (int q = 0; q < 4; ++q) t[(p * 4 + q) * CIN + c] = v[q];
        }
      }
      if (norm_pix) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) s += t[j];
        const float mean = s / (float)D;
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          t[j] -= mean;
          ss = fmaf(t[j], t[j], ss);
        }
        const float sd = sqrtf(ss / (float)(D - 1) + 1e-6f);
#pragma unroll
        for (int j = 0; j < D; ++j) t[j] /= sd;
      }
      const f32x4* pp = reinterpret_cast<const f32x4*>(pred + tok * D);
#pragma unroll
      for (int j = 0; j < D / 4; ++j) {
        const f32x4 pv = pp[j];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float diff = pv[k] - t[4 * j + k];
          mine = fmaf(diff, diff, mine);
          o[k] = g * diff;
        }
        dp[j] = o;
      }
    }
  }
  sums[tid] = mine;
  const float total = mae_block_sum(sums, tid);
  if (tid == 0) part[blockIdx.x] = total;
}

// loss = scale * sum_k part[k]: thread t adds part[t], part[t + 256], ... in order, then the tree
__global__ __launch_bounds__(MAE_NT) void mae_loss_finish_kernel(const float* __restrict__ part, int nblk, float scale, float* __restrict__ loss) {
  __shared__ float sums[MAE_NT];
  const int tid = threadIdx.x;
  float s = 0.f;
  for (int k = tid; k < nblk; k += MAE_NT) s += part[k];
  sums[tid] = s;
  const float total = mae_block_sum(sums, tid);
  if (tid == 0) *loss = scale * total;
}

extern "C" long hpfg_mae_loss_blocks(int B, int H, int W, int patch) {
  if (B <= 0 || H <= 0 || W <= 0 || patch != 4 || H % 4 || W % 4) {
    hpfg_set_error("mae_loss_blocks: bad args (B %d, image %d x %d, patch %d: patch 4, sides divisible by it)", B, H, W, patch);
    return -1;
  }
  return ((long)B * (H / 4) * (W / 4) + MAE_NT - 1) / MAE_NT;
}

extern "C" int hpfg_mae_loss(const float* pred, const float* img, const uint8_t* mask, float scale, int norm_pix, float* loss, float* dpred,
                             float* partials, int B, int Cin, int H, int W, int patch, void* stream) {
  HPFG_ARG_CHECK(pred && img && mask && loss && dpred && partials, "mae_loss: null pointer");
  HPFG_ARG_CHECK(patch == 4 && Cin >= 1 && Cin <= 4, "mae_loss: patch %d with %d channels is not built (patch 4, 1 to 4 channels)", patch, Cin);
  const long nblk = hpfg_mae_loss_blocks(B, H, W, patch);
  if (nblk < 0) return -1;
  HPFG_ARG_CHECK(nblk <= 0x7fffffffL, "mae_loss: %ld workgroups", nblk);
  const long tokens = (long)B * (H / 4) * (W / 4);
  const float g = 2.f * scale;
#define MAE_LOSS(CC)                                                                                                                              \
  hipLaunchKernelGGL(mae_loss_kernel<CC>, dim3((unsigned)nblk), dim3(MAE_NT), 0, (hipStream_t)stream, pred, img, mask, dpred, partials, tokens, H / 4, \
                     W / 4, g, norm_pix)
  switch (Cin) {
    case 1: MAE_LOSS(1); break;
    case 2: MAE_LOSS(2); break;
    case 3: MAE_LOSS(3); break;
    default: MAE_LOSS(4); break;
  }
#undef MAE_LOSS
  int rc = hpfg_launch_status("mae_loss_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mae_loss_finish_kernel, dim3(1), dim3(MAE_NT), 0, (hipStream_t)stream, partials, (int)nblk, scale, loss);
  return hpfg_launch_status("mae_loss_finish_kernel");
}
