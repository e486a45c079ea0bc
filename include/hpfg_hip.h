/*
 * hpfg_hip.h -- C ABI of libhpfg_hip.so: the MI355X (gfx950) kernels behind HPFG's training hot path.
 *
 * The reference (fakerlove1/HPFG) is pure Python/PyTorch: its "FFI" for this path is the set of torch ops its
 * U-Net and losses issue.  Each entry point below replaces one fused family of those ops
 * and cites the reference lines whose arithmetic it reproduces.  Conventions:
 *   - activations are fp32 NHWC on the device; all pointers are device pointers unless marked host;
 *   - every function only enqueues work on `stream` (a hipStream_t passed as void*): no allocation, no
 *     synchronisation, no host<->device copies, safe to capture into a hipGraph;
 *   - return value 0 = ok, <0 = argument error (see hpfg_last_error()), >0 = hipError_t from the launch.
 *
 * "Virtual activations": train-mode BatchNorm makes conv -> BN -> LeakyReLU -> Dropout -> (MaxPool | Upsample+concat)
 * a chain of per-element maps once the batch statistics are known, so consumers apply that chain while they load
 * the producer's raw (pre-BN) conv output instead of reading a materialised activation.  HpfgAct describes such a
 * source; the same descriptor describes the backward-side virtual tensor dZ (gradient w.r.t. a raw conv output).
 */
#ifndef HPFG_HIP_H
#define HPFG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPFG_VERSION 144
enum { HPFG_MATH_F32 = 0, HPFG_MATH_BF16X3 = 1 };

/* rows of a per-layer BatchNorm table `bn` ([HPFG_BN_ROWS][C] floats) */
enum { HPFG_BN_MEAN = 0, HPFG_BN_RSTD = 1, HPFG_BN_SCALE = 2, HPFG_BN_SHIFT = 3,
       HPFG_BN_K1 = 4, HPFG_BN_K2 = 5, HPFG_BN_K3 = 6, HPFG_BN_SPARE = 7, HPFG_BN_ROWS = 8 };

enum {
  HPFG_ACT_NONE = 0,       /* contributes no channels */
  HPFG_ACT_PLAIN = 1,      /* v = z[n,y,x,c]                       (NHWC, float4 path, C%4==0)               */
  HPFG_ACT_STRIDED = 2,    /* v = z[n*sn + c*sc + y*sy + x*sx]     (any layout, scalar path; network input)  */
  HPFG_ACT_BNACT = 3,      /* v = drop(lrelu(z*scale+shift))       unet.py:19-21,23-24 (BN train, LeakyReLU .01, Dropout) */
  HPFG_ACT_BNACT_POOL = 4, /* v = max 2x2 of lrelu(z*scale+shift)  unet.py:37 (MaxPool2d(2)) fused on load   */
  HPFG_ACT_UP2X = 5,       /* v = bilinear x2, align_corners=True  unet.py:51,56 fused on load               */
  HPFG_ACT_DZ = 6,         /* v = k1*g + k2*z + k3, g = aux*dropmask*lrelu'(z*scale+shift): BN/LeakyReLU/Dropout backward */
  HPFG_ACT_SPLIT16 = 7,    /* a side tensor stored by HpfgConvArgs.stage_out (round 5): the value ALREADY split for the bf16x3 matrix-core
                              products, v = hi + lo with hi = bf16(v), lo = bf16(v - hi): z = bf16 [N][Hs][Ws][pstride / 8][hi 8 | lo 8]
                              (pstride = channels per pixel, C % 8 == 0: 32 contiguous bytes per 8 channels, the size of the fp32 tensor).
                              Read by hpfg_wgrad only: its loader becomes a copy into LDS. */
  HPFG_ACT_UPBWD = 8       /* (round 5, 1x1 dgrad only) the gradient w.r.t. a tensor BEFORE nn.Upsample(x2, bilinear, align_corners=True) (unet.py:51),
                              gathered on load from the gradient w.r.t. the upsampled tensor: z = that gradient [N][2*Hs][2*Ws] with pstride
                              floats per pixel, C channels; the value at (n, y, x) is the transposed interpolation -- what
                              hpfg_upsample2x_bwd writes into a tensor of its own */
};

typedef struct HpfgAct {
  const float* z;      /* raw tensor */
  const float* bn;     /* BN table [HPFG_BN_ROWS][bn_stride] for BNACT/BNACT_POOL/DZ, else NULL */
  const float* aux;    /* DZ: upstream gradient w.r.t. the activated output (dA) */
  int32_t mode;
  int32_t C;           /* channels this source provides (virtual channels >= C read as 0) */
  int32_t Hs, Ws;      /* spatial size of z (POOL: 2x the virtual size, UP2X: half of it) */
  int32_t pstride;     /* floats between pixels of z (PLAIN/BNACT/POOL/UP2X/DZ) */
  int32_t aux_pstride; /* floats between pixels of aux (DZ) */
  int32_t bn_stride;   /* row length of bn (= channel count of the producing layer) */
  int32_t bn_coff;     /* first channel of this source inside the bn rows (normally 0) */
  int32_t sn, sc, sy, sx; /* STRIDED element strides */
  float drop_p;        /* dropout probability applied to this activation (BNACT, DZ); 0 = none */
  uint32_t drop_seed;  /* counter-based RNG key; keep(i) = hash(i, seed) >= p*2^32, i = NHWC element index */
  const uint8_t* drop_mask; /* optional explicit keep-mask (bytes, NHWC element order) used instead of the RNG: lets parity
                               tests replay the masks torch drew in the reference run */
  const uint32_t* seed_dev; /* optional device word added to drop_seed at run time (lets a captured hipGraph draw new masks per replay) */
  /* BatchNorm statistics straight from the producer's sum accumulators (round 4; BNACT / BNACT_POOL sources of the bf16x3 forward kernels):
     with bn_acc != NULL the consumer derives scale / shift of its input channels itself in its prologue -- mean = S1 / count,
     var = S2 / count - mean^2, rstd = 1 / sqrt(var + eps), scale = gamma * rstd, shift = beta - mean * scale (fp64, the arithmetic of
     hpfg_bn_fwd_finalize) -- instead of reading the rows of `bn`, so that no finalize launch sits between a conv and its consumer
     (unet.py:18-24: conv -> BatchNorm -> LeakyReLU).  `bn` is then written once per forward by hpfg_bn_acc_finalize for the backward kernels. */
  const long long* bn_acc;  /* accumulators of the producing layer, see HpfgConvArgs.stat_acc; NULL = read the table rows */
  const float* bn_gamma;    /* BatchNorm weight / bias of the producing layer ([bn_stride]) */
  const float* bn_beta;
  float bn_count;           /* N * H * W of the producing layer (elements per channel) */
  float bn_eps;
  int32_t bn_shards;        /* shards of bn_acc (the producer's stat_shards) */
  int32_t reserved1;
} HpfgAct;

typedef struct HpfgConvArgs {
  HpfgAct a0, a1;       /* input = channel concat [a0 | a1]  (torch.cat([skip, up]), unet.py:57); (a0.C+a1.C) padded to 16 */
  const float* wpk;     /* weights in MFMA fragment order, see hpfg_pack_weights */
  const float* bias;    /* [CoutPad] or NULL */
  float* out;           /* raw output, NHWC, out_pstride floats per pixel */
  float* stat_partials; /* NULL or [hpfg_conv_stat_blocks()][2][CoutPad]: per-block sum(z), sum(z*z) for BN (unet.py:19,23) */
  int32_t out_pstride, Cout, CoutPad;
  int32_t N, H, W;      /* output (= virtual input) size */
  int32_t taps;         /* 9 (3x3, pad 1) or 1 (1x1) */
  int32_t math;         /* HPFG_MATH_F32: exact fp32 MFMA, wpk = fp32 fragments; HPFG_MATH_BF16X3: split-bf16 MFMA (hi*hi+hi*lo+lo*hi,
                           fp32 accumulate), wpk = the wpk16_* buffer of hpfg_pack_weights */
  int32_t bwd_stats;    /* dgrad only (BF16X3, DZ or PLAIN source).  2 (3x3): `out` would be the gradient w.r.t. MaxPool2d(2) of bwd_of's activated
                           output (bwd_of at 2H x 2W, its gradient so far in bwd_of.aux, no dropout behind it): the epilogue adds the tile at the
                           arg-max of each 2 x 2 window into bwd_of.aux IN PLACE (unet.py:37 backward), accumulates the backward sums of the
                           completed gradient as below, and does not write `out` -- hpfg_bn_bwd_reduce_pool without its launch.
                           1 = `out` is the COMPLETE gradient w.r.t. the activated output of the
                           BatchNorm layer described by `bwd_of`; stat_partials then receives that layer's backward sums
                           sum(g), sum(g*xhat)  (g = out * LeakyReLU' * dropout) instead of sum(z), sum(z*z) -- what hpfg_bn_bwd_reduce
                           would compute in a pass of its own; feed the rows to hpfg_bn_bwd_finalize */
  HpfgAct bwd_of;       /* that layer: z, its table (mean, rstd, scale, shift rows), dropout fields; C == Cout, Hs x Ws == H x W */
  float* out2;          /* optional second destination: output channels >= out_split go to out2[pixel * out2_pstride + (co - out_split)]
                           instead of `out`.  The dgrad of a decoder block's first conv writes d(skip) and d(upsampled) -- the two halves of the
                           concat gradient, unet.py:57 -- into buffers of their own, so that neither is read through a half-used pixel stride */
  int32_t out_split;    /* multiple of 16; 0 = everything to `out` */
  int32_t out2_pstride;
  long long* stat_acc;  /* optional (bf16x3 kernels), instead of stat_partials: the per-channel sums are ADDED to this layer accumulator,
                           long long [HPFG_ACC_SHARDS][2 (sum z | sum z^2)][CoutPad][2 (limb)], by integer atomics.  A partial sum t is split
                           exactly as t = hi + lo * 2^-52 (hi = rint(t), lo = (t - hi) * 2^52): integer addition is associative, so the
                           totals are bit-reproducible whatever order the workgroups finish in.  Shard = workgroup id % stat_shards: more
                           shards = less same-address contention among the producer's workgroups (1 shard of a 768-workgroup launch: +40 us),
                           fewer = less to read in every consumer workgroup's prologue (32 bytes per channel and shard).
                           The accumulator must be zero when the launch starts (hpfg_pack_weights_bump zeroes a region).  A launch of
                           more than 2048 workgroups is refused: the readers add the low limbs of all shards in 64 bits. */
  int32_t stat_shards;  /* power of two, 1 .. HPFG_ACC_MAX_SHARDS */
  int32_t reserved2;
  float* stage_out;     /* optional, 3x3 layers on the bf16x3 kernels with a non-PLAIN source of (a0.C + a1.C) % 8 == 0 channels at sizes that are
                           not multiples of 16 (the channel-rich 56 / 28 / 14-pixel levels; the aligned ones have fused kernels): the staging
                           derives the virtual input of every pixel anyway (BatchNorm + LeakyReLU + Dropout [+ max-pool | + bilinear upsample and
                           concat] in a forward conv; dZ = k1*g + k2*z + k3 in a dgrad) -- the workgroups of output-channel slice 0 also store
                           it -- as the (hi | lo) bf16 pair the staging has in registers anyway (conv_bf16_kernel.h store_piece):
                           bf16 [N][H][W][(a0.C + a1.C) / 8][hi 8 | lo 8], the same 4 bytes per element an fp32 tensor takes.  The layer's weight
                           gradient reads them as HPFG_ACT_SPLIT16 sources (its input from the forward conv, its dZ from the dgrad): no
                           BatchNorm / LeakyReLU / Dropout chain, no fp32 -> bf16 split, in any of its (input-channel slice x output-channel
                           slice) workgroups -- its loader is a copy (autograd's saved tensors of nn.Conv2d, model/unet.py:18,22).
                           With an HPFG_ACT_UPBWD source (1x1 dgrad): fp32 [N][H][W][a0.C], the gathered gradient itself -- the dZ of the 1x1
                           conv's weight gradient -- stored by the workgroups of output-channel slice 0 */
  float* side_sums;     /* optional, HPFG_ACT_UPBWD source only: [hpfg_conv_stat_rows()][a0.C] per-workgroup channel sums of the gathered
                           gradient (slice 0), the rows of the 1x1 conv's bias gradient (summed in a fixed order by hpfg_slab_reduce_multi) */
} HpfgConvArgs;
#define HPFG_ACC_MAX_SHARDS 8
#define HPFG_ACC_WORDS(C, shards) ((shards) * 2 * 2 * (C))   /* long long words of one layer accumulator */

typedef struct HpfgWgradArgs {
  HpfgAct a0, a1;       /* conv input (as in forward) */
  HpfgAct g;            /* dZ: gradient w.r.t. the conv's raw output (DZ or PLAIN) */
  float* slab;          /* workspace [S][taps][CinPad][CoutPad] */
  float* dw_oihw;       /* result, PyTorch layout [Cout][Cin][k][k] (written, not accumulated) */
  int32_t Cin, CinPad, Cout, CoutPad;
  int32_t N, H, W, taps;
  int32_t S;            /* number of pixel splits (slabs), from hpfg_wgrad_splits() */
  int32_t math;         /* HPFG_MATH_F32 or HPFG_MATH_BF16X3 (3x3 only; 1x1 always runs the exact fp32 kernel) */
  int32_t defer_reduce; /* 1: leave the slabs in `slab`; the caller sums them later with hpfg_slab_reduce_multi (one launch per backward) */
} HpfgWgradArgs;

typedef struct HpfgFusedBwdArgs {   /* hpfg_fused_bwd: both gradients of a thin 3x3 layer from ONE staging of dZ (see below) */
  HpfgConvArgs d;       /* the dgrad side exactly as hpfg_conv_fwd takes it: a0 = dZ (DZ or PLAIN), wpk = wpk16_dgrad, out / out2 = dX,
                           Cout / CoutPad = the layer's Cin / CinPad, bwd_stats / bwd_of / stat_partials; math = HPFG_MATH_BF16X3 */
  HpfgAct xa0, xa1;     /* the layer's input as in forward (BNACT | BNACT_POOL | [BNACT | UP2X]) */
  float* slab;          /* [hpfg_fused_bwd_grid()][9][CinPad][CoutPad]: per-workgroup weight-gradient sums (hpfg_slab_reduce_multi) */
  int32_t Cin, CinPad, Cout, CoutPad;   /* of the layer: dW is [Cout][Cin][3][3] */
} HpfgFusedBwdArgs;

typedef struct HpfgSlabDesc {   /* one layer of hpfg_slab_reduce_multi: dw_oihw[co][ci][tap] = sum_s slab[s][tap][ci][co] */
  const float* slab;
  float* dw_oihw;
  int32_t S, taps, Cin, CinPad, Cout, CoutPad;
} HpfgSlabDesc;

typedef struct HpfgPackDesc {   /* one conv layer for hpfg_pack_weights (device array of these) */
  const float* w_oihw;  /* [Cout][Cin][k][k] (nn.Conv2d.weight, unet.py:18,22,50,99) */
  const float* b;       /* [Cout] */
  float* wpk_fwd;       /* [taps][CinPad/16][CoutPad/16][64][4]: B fragments of mfma_f32_16x16x4f32, k = input channel; may be NULL */
  float* wpk_dgrad;     /* [taps][CoutPad/16][CinPad/16][64][4]: transposed + tap-flipped weights for dgrad; may be NULL */
  float* bias_pad;      /* [CoutPad] */
  void* wpk16_fwd;      /* bf16x3 B fragments [k-step][CoutPad/16][hi|lo][64][8] (hpfg_wpk16_elems() bf16 values), or NULL */
  void* wpk16_dgrad;    /* same for dgrad (k = output channel, taps flipped), or NULL */
  int32_t Cout, Cin, CoutPad, CinPad, taps;
  int32_t kc;           /* K packing of the bf16 buffers: 32 = one tap x 32 channels, 16 = two taps x 16 channels (3x3 on 16x16 tiles);
                           use hpfg_conv_kc(H, W, taps) */
} HpfgPackDesc;

int hpfg_version(void);
const char* hpfg_last_error(void);
/* Kernel-form switches for tests and A/B tools (the launch paths read no environment variables): returns the previous value (>= 0) or < 0.
 * HPFG_OPT_CONV_THIN: 0 = the thin forward layers on the chunked conv kernel instead of the whole-tile kernel;
 * HPFG_OPT_FIRST_MFMA: 0 = the 1- / 3-channel first layer as a VALU loop instead of the MFMA form (bit-identical outputs);
 * HPFG_OPT_FIRST_WGRAD: 0 = the first layer's weight gradient on the tile kernel of hpfg_fused_bwd instead of the streaming kernel;
 * HPFG_OPT_NARROW_DEEP: the workgroup count up to which a 3x3 launch on 4 x 16-pixel tiles takes 32-wide instead of 64-wide output-channel slices
 *   (default 128: launches that would leave half of the CUs idle; 0 = never);
 * HPFG_OPT_UPDATE_PACK: 0 = the optimizers never write weight fragments (hpfg_sgd_ema_pack_step is not used): every forward packs its own. */
enum { HPFG_OPT_CONV_THIN = 0, HPFG_OPT_FIRST_MFMA = 1, HPFG_OPT_FIRST_WGRAD = 2, HPFG_OPT_NARROW_DEEP = 3, HPFG_OPT_UPDATE_PACK = 4, HPFG_OPT_COUNT = 5 };
int hpfg_get_option(int which);
int hpfg_set_option(int which, int value);

/* ---- forward ------------------------------------------------------------------------------------------- */
/* nn.Conv2d(Cin<=4 -> 16, k3, p1) on the network input + BN partial sums (encoder.in_conv, unet.py:18-19,72). */
int hpfg_conv3x3_first_fwd(const HpfgAct* x, const float* w_oihw, const float* bias, float* out, float* stat_partials,
                           int N, int H, int W, int Cin, int Cout, void* stream);
int hpfg_conv_first_rows(int N, int H, int W);            /* rows of stat_partials hpfg_conv3x3_first_fwd writes (persistent grid) */
/* the same layer with its BatchNorm sums added to a layer accumulator (HpfgConvArgs.stat_acc / stat_shards) as well as / instead of rows of partial sums */
int hpfg_conv3x3_first_fwd_acc(const HpfgAct* x, const float* w_oihw, const float* bias, float* out, float* stat_partials, long long* stat_acc,
                               int stat_shards, int N, int H, int W, int Cin, int Cout, void* stream);
/* nn.Conv2d k3/k1 (+ fused producer BN/LeakyReLU/Dropout/MaxPool/Upsample/cat on load) + BN partial sums.
 * Also serves dgrad: a0 = dZ (mode DZ/PLAIN), wpk = wpk_dgrad. */
int hpfg_conv_fwd(const HpfgConvArgs* args, void* stream);
int hpfg_conv_stat_blocks(int N, int H, int W);          /* rows written by the fp32 kernels / upper bound for workspace sizing */
int hpfg_conv_stat_rows(const HpfgConvArgs* args);         /* rows hpfg_conv_fwd(args) writes (depends on args->math) */
/* BatchNorm2d train-mode statistics -> table rows mean/rstd/scale/shift, running stats (momentum .1, unbiased var)
 * (unet.py:19,23).  Either partials (float [nblk][2][C]) or pre-reduced sums (double [2][C], e.g. after an all-reduce). */
int hpfg_bn_fwd_finalize(const float* partials, int nblk, const double* sums, double count, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, float* bn, int C, void* stream);
/* The same for EVERY BatchNorm layer of a forward pass in one launch, from the layers' sum accumulators (HpfgConvArgs.stat_acc): the forward
 * consumers derive scale / shift themselves (HpfgAct.bn_acc), so this call follows the LAST conv of the forward and writes the table rows
 * the backward kernels read, plus running_mean / running_var (momentum, unbiased variance).  Device array of descriptors + host copy. */
typedef struct HpfgBnAccDesc {
  const long long* acc;     /* [HPFG_ACC_WORDS(C, shards)]: read, then ZEROED for the next forward (every consumer has run by then) */
  const float* gamma;
  const float* beta;
  float* running_mean;      /* both or neither */
  float* running_var;
  float* bn;                /* table [HPFG_BN_ROWS][C]: rows mean, rstd, scale, shift are written */
  int32_t C;
  float count;              /* N * H * W */
  int32_t shards;
  int32_t reserved;
} HpfgBnAccDesc;
int hpfg_bn_acc_finalize(const HpfgBnAccDesc* table_dev, const HpfgBnAccDesc* table_host, int nlayers, float momentum, float eps, void* stream);
/* Backward counterpart.  With HpfgAct.bn_acc on a DZ source every dZ consumer (dgrad, fused dgrad + wgrad, wgrad) derives k1, k2, k3 from the
 * layer's BACKWARD accumulator -- sum(g), sum(g * xhat), added there by the dgrad epilogue that completed the layer's gradient
 * (HpfgConvArgs.bwd_stats + stat_acc) or by hpfg_bn_bwd_reduce[_pool]_acc -- so no hpfg_bn_bwd_finalize launch sits on the chain of backward.
 * This call follows the last dZ consumer of the listed layers: dgamma / dbeta (native_batch_norm_backward), the k1 .. k3 table rows, and the
 * accumulators are zeroed for the next pass. */
typedef struct HpfgBnAccBwdDesc {
  long long* acc;           /* [HPFG_ACC_WORDS(C, shards)]: read, then zeroed */
  const float* gamma;
  float* bn;                /* table: rows mean, rstd are read, k1, k2, k3 written */
  float* dgamma;            /* or NULL */
  float* dbeta;             /* or NULL */
  int32_t C;
  float count;
  int32_t shards;
  int32_t reserved;
} HpfgBnAccBwdDesc;
int hpfg_bn_acc_bwd_finalize(const HpfgBnAccBwdDesc* table_dev, const HpfgBnAccBwdDesc* table_host, int nlayers, void* stream);
int hpfg_bn_bwd_reduce_acc(const HpfgAct* g, int N, int H, int W, long long* acc, int shards, void* stream);
int hpfg_bn_bwd_reduce_pool_acc(const HpfgAct* g, const float* dP, int dp_pstride, int N, int Hp, int Wp, long long* acc, int shards, void* stream);
int hpfg_reduce_partials(const float* partials, int nblk, int C, double* sums, void* stream);
/* eval-mode BatchNorm (model.eval(), val.py:268-287): table rows from the running statistics */
int hpfg_bn_eval_table(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                       float* bn, int C, void* stream);
/* hpfg_conv3x3_first_fwd[_acc] that also advances the two per-forward device counters of hpfg_pack_weights_bump (workgroup 0, before anything
 * else): for a forward whose weight fragments are current, so that it starts without a pack launch.  stat_acc may be NULL (plain partial rows). */
int hpfg_conv3x3_first_fwd_bump(const HpfgAct* x, const float* w_oihw, const float* bias, float* out, float* stat_partials, long long* stat_acc,
                                int stat_shards, long long* counters, int n_counters, int32_t* seed_word, int seed_add, int N, int H, int W, int Cin,
                                int Cout, void* stream);
int hpfg_conv_kc(int H, int W, int taps);
long hpfg_wpk16_elems(int Kchannels, int NchannelsPad, int taps, int kc);   /* bf16 elements of one wpk16 buffer */
int hpfg_pack_weights(const HpfgPackDesc* table_dev, const HpfgPackDesc* table_host, int nlayers, void* stream);
/* The same launch also advances two per-forward device counters (nn.BatchNorm2d's num_batches_tracked += 1 of a train-mode forward,
 * model/unet.py:14-27 via torch; and the engine's dropout seed word, so that a replayed hipGraph draws fresh nn.Dropout masks):
 * counters[0..n_counters) += 1 (int64), *seed_word = (*seed_word + seed_add) & 0x7fffffff.  Either may be absent (0 / NULL).
 * zero_words[0..n_zero) = 0: the BatchNorm sum accumulators (HpfgConvArgs.stat_acc) of the pass this launch precedes. */
int hpfg_pack_weights_bump(const HpfgPackDesc* table_dev, const HpfgPackDesc* table_host, int nlayers, long long* counters, int n_counters,
                           int32_t* seed_word, int seed_add, long long* zero_words, long n_zero, void* stream);
/* evaluate a virtual activation into memory (tests, projection-neck inputs): out [N,H,W,a0.C+a1.C] */
int hpfg_act_materialize(const HpfgAct* a0, const HpfgAct* a1, int N, int H, int W, float* out, void* stream);
/* the dropout keep-mask the loaders use, as bytes [n_elems] (tests feed it to the oracle) */
int hpfg_dropout_mask(uint8_t* out, long n_elems, float p, uint32_t seed, const uint32_t* seed_dev, void* stream);

/* ---- backward ------------------------------------------------------------------------------------------ */
/* per-channel sum(g), sum(g*xhat) with g = dA*dropmask*lrelu'(y): partials [hpfg_bn_bwd_blocks][2][C] */
int hpfg_bn_bwd_reduce(const HpfgAct* g /* mode DZ; k rows unused */, int N, int H, int W, float* partials, void* stream);
int hpfg_bn_bwd_blocks(int N, int H, int W, int C);
/* finalize: dgamma, dbeta (BatchNorm backward) and table rows k1,k2,k3 so that dz = k1*g + k2*z + k3 */
/* the same for a layer whose output also went through MaxPool2d(2) (model/unet.py:37): first dA += maxpool_backward(dP) in place
 * (arg-max recomputed from the raw output), then the sums -- replaces hpfg_pool_scatter_add + hpfg_bn_bwd_reduce in one pass */
int hpfg_bn_bwd_reduce_pool(const HpfgAct* g /* DZ source at the un-pooled size */, const float* dP, int dp_pstride, int N, int Hp, int Wp,
                            float* partials /* [hpfg_bn_bwd_pool_blocks()][2][C] */, void* stream);
int hpfg_bn_bwd_pool_blocks(int N, int Hp, int Wp, int C);
/* param_grad_scale multiplies dgamma / dbeta only: with all-reduced `sums` (data parallel, R ranks) every rank holds the GLOBAL
 * sums, so it writes global/R and the SUM all-reduce of the gradient buffer restores the global value; 1 otherwise */
int hpfg_bn_bwd_finalize(const float* partials, int nblk, const double* sums, double count, const float* gamma,
                         float* bn, float* dgamma, float* dbeta, int C, float param_grad_scale, void* stream);
int hpfg_wgrad(const HpfgWgradArgs* args, void* stream);
/* Fused backward of a thin 3x3 layer (bf16x3; H, W multiples of 16; CinPad <= 64, CoutPad <= 32): dX (as hpfg_conv_fwd with a dZ source,
 * including the bwd_stats epilogue and out2) AND the weight-gradient slabs (as hpfg_wgrad with defer_reduce) from one read of (dA, z) and
 * one read of the layer input -- replaces reference loss.backward()'s separate conv-transpose and weight-gradient kernels of one Conv2d
 * (model/unet.py:18,22).  hpfg_fused_bwd_grid: workgroups of the launch = slabs = rows of d.stat_partials; 0 = shape not instantiated
 * (the caller then uses hpfg_wgrad + hpfg_conv_fwd). */
int hpfg_fused_bwd(const HpfgFusedBwdArgs* args, void* stream);
int hpfg_fused_bwd_grid(const HpfgFusedBwdArgs* args);
int hpfg_slab_reduce_multi(const HpfgSlabDesc* table_dev, const HpfgSlabDesc* table_host, int nlayers, void* stream);
int hpfg_wgrad_splits(int N, int H, int W, int CinPad, int CoutPad, int taps);
long hpfg_wgrad_slab_floats(int N, int H, int W, int CinPad, int CoutPad, int taps);
/* first-layer wgrad: dW[co][ci][tap] for Cin<=4 from the strided input */
/* bias gradient of a conv without BN: db[c] = sum over pixels of g[p][c] (conv1x1 / out_conv) */
int hpfg_channel_sum(const float* g, int pstride, long npix, int C, float* out, float* scratch, void* stream);
/* first stage only: partials [hpfg_channel_sum_blocks(npix, C)][C]; the caller sums the rows later, e.g. as one more "layer"
 * {slab = partials, S = blocks, taps = 1, Cin = CinPad = 1, Cout = CoutPad = C, dw_oihw = db} of hpfg_slab_reduce_multi */
int hpfg_channel_sum_partials(const float* g, int pstride, long npix, int C, float* partials, void* stream);
int hpfg_channel_sum_blocks(long npix, int C);
/* MaxPool2d(2) backward: dA[argmax position] += dP, recomputing the arg-max from the producer's raw output */
int hpfg_pool_scatter_add(const HpfgAct* src /* BNACT view of the pooled tensor's producer */, const float* dP, int dp_pstride,
                          float* dA, int da_pstride, int N, int Hp, int Wp, void* stream);
/* bilinear x2 (align_corners) backward: dU[low res] = sum of taps of dUp (dUp has dup_pstride floats per pixel) */
int hpfg_upsample2x_bwd(const float* dUp, int dup_pstride, float* dU, int N, int Hl, int Wl, int C, void* stream);
/* same, and csum_partials[hpfg_upsample2x_bwd_blocks()][C] receives per-workgroup channel sums of dU (the bias gradient of the
 * 1x1 conv in front of the upsample, model/unet.py:50; rows are summed by hpfg_slab_reduce_multi like hpfg_channel_sum_partials') */
int hpfg_upsample2x_bwd_sums(const float* dUp, int dup_pstride, float* dU, int N, int Hl, int Wl, int C, float* csum_partials, void* stream);
int hpfg_upsample2x_bwd_blocks(int N, int Hl, int Wl, int C);

/* ---- data parallel: peer mailbox exchange (csrc/peer.h) ------------------------------------------------------------------------
 * The reference is single-device (main.py:44); under data parallel in the global-batch mode every BatchNorm layer's sums and the loss sums
 * must be added over the ranks between two kernels of the step.  Instead of ~90 latency-bound collectives per step, the kernel that
 * produces a sum exchanges it itself: it stores the value into every peer's mailbox (IPC-mapped fine-grained memory: xGMI between the
 * GPUs of a node), then reads the peers' values from its own mailbox and adds them in rank order.  No host code between the kernels,
 * so the step stays capturable into a hipGraph. */
#define HPFG_PEER_MAX_RANKS 8
#define HPFG_PEER_HANDLE_BYTES 64
#define HPFG_PEER_MAX_SPINS (1L << 22)      /* bounded poll (a few seconds): on expiry *err = 1 and the kernel carries on */
typedef struct HpfgPeerX {
  void* mbox[HPFG_PEER_MAX_RANKS];   /* mbox[r] = rank r's mailbox as mapped in this process (mbox[rank] = its own); unused entries NULL */
  const int32_t* epoch;              /* device word: the use count of `slot` (consecutive integers >= 1, the same on every rank) */
  int32_t* err;                      /* device word set to 1 when a poll expires (or NULL) */
  int32_t world, rank;               /* world <= 1: no exchange (the struct may be all zero) */
  int32_t slot, cap;                 /* slot index; cap = payload values per rank and parity in a slot */
  int64_t slot_bytes;                /* hpfg_peer_slot_bytes(world, cap) */
} HpfgPeerX;
long hpfg_peer_slot_bytes(int world, int cap);
int hpfg_peer_alloc(size_t bytes, void** ptr);                       /* zero-filled fine-grained device memory */
int hpfg_peer_free(void* ptr);
int hpfg_peer_handle(void* ptr, unsigned char* handle64);            /* HPFG_PEER_HANDLE_BYTES to send to the peers */
int hpfg_peer_open(const unsigned char* handle64, void** ptr);       /* map a peer's mailbox */
int hpfg_peer_close(void* ptr);
int hpfg_word_add(int32_t* word, int v, void* stream);               /* *word = (*word + v) & 0x7fffffff: the epoch bump, stream-ordered */
/* hpfg_bn_fwd_finalize / hpfg_bn_bwd_finalize / hpfg_seg_loss_partials with the cross-rank SUM of the per-channel (per-term) sums done by the
 * kernel itself (px->world > 1); `count` / the loss counts are the GLOBAL ones, param_grad_scale = 1 / world as with all-reduced sums */
int hpfg_bn_fwd_finalize_x(const float* partials, int nblk, const HpfgPeerX* px, double count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* bn, int C, void* stream);
int hpfg_bn_bwd_finalize_x(const float* partials, int nblk, const HpfgPeerX* px, double count, const float* gamma, float* bn, float* dgamma,
                           float* dbeta, int C, float param_grad_scale, void* stream);

/* Gradient all-reduce over the same kind of IPC-mapped memory: what DistributedDataParallel's bucketed NCCL all-reduce would be if the reference
 * ran on more than one card (main.py:44: it does not).  xGMI is point to point, so the exchange is not a ring: every rank owns one slice of the
 * buffer; (1) push: each rank stores its copy of slice p into rank p's window (all links busy at once), (2) reduce: the owner adds the
 * contributions in rank order and stores the reduced slice into every rank's window, (3) gather: each rank copies the reduced buffer back.
 * Flags carry the epoch (consecutive use counts, bumped by the call itself); polls are bounded like the mailbox polls.  Three launches on `stream`, no host code: the whole training step stays ONE hipGraph under data parallel.  Every rank receives bit-identical
 * sums (each slice is reduced once).  Window layout: 256 bytes of flags, world x slice floats of inbox, world x slice floats of result. */
typedef struct HpfgPeerBuf {
  void* win[HPFG_PEER_MAX_RANKS];    /* win[r] = rank r's window as mapped in this process */
  int32_t* epoch;                    /* device word counting the calls (the same sequence on every rank) */
  int32_t* err;                      /* device word set to 1 when a poll expires (or NULL) */
  int32_t world, rank;
  int64_t slice;                     /* floats per rank slice of THIS call: hpfg_peer_buf_slice(world, n) */
  int64_t n;                         /* floats of the buffer */
  int64_t stride;                    /* floats between the inbox regions of a window = hpfg_peer_buf_slice(world, CAPACITY the windows were sized
                                        for); the result region begins at world * stride.  The layout must not depend on the call's n: a rank
                                        that has finished call k pushes call k+1 while a peer may still copy its call-k result out */
} HpfgPeerBuf;
long hpfg_peer_buf_slice(int world, long n);                 /* ceil(n / world) rounded up to a multiple of 4 */
long hpfg_peer_buf_bytes(int world, long n);                 /* window size for buffers of up to n floats */
int hpfg_peer_allreduce_f32(const HpfgPeerBuf* pb, float* buf, void* stream);      /* buf[0..n) = SUM over ranks, in place */

/* ---- losses (main.py:164-197, medloss.py:44-56, diceloss.py:155-191, Mean-Teacher :103-106) -------------- */
typedef struct HpfgLossArgs {
  const float* logits;      /* [N,H,W,C] student logits (NHWC) */
  const float* t_logits;    /* teacher logits for the MSE consistency term, or NULL */
  const uint8_t* labels0;   /* labels for images [0,n_lab) (255 = ignore), group 0 */
  const uint8_t* labels1;   /* (pseudo-)labels for images [n_lab,N), group 1, or NULL */
  const float* coef;        /* device [8]: ce0, dice0, ce1, dice1, mse_w, 0,0,0  (per-step weights live on the device) */
  float* partials;          /* workspace [hpfg_loss_blocks()][hpfg_loss_nsum(C)] */
  float* sums;              /* out [hpfg_loss_nsum(C)] reduced sums (all-reduce these for data parallel) */
  float* out;               /* out [8]: total, ce0, dice0, ce1, dice1, mse, 0, 0 */
  float* dlogits;           /* backward output [N,H,W,C] */
  int32_t N, n_lab, H, W, C;
  int32_t world;            /* data-parallel world size (MSE / CE counts are global after the all-reduce) */
  int32_t input_is_prob;    /* 1: `logits` already holds probabilities (DiceLoss(softmax=False), diceloss.py:178); CE/MSE weights must be 0 */
  int32_t teacher_is_prob;  /* 1: `t_logits` already holds probabilities (ICT's mixed teacher prediction, 2022_02...ICT...py:126-137) */
  int32_t t_unlab_only;     /* 1: `t_logits` covers images [n_lab,N) only; 0: it is indexed like `logits` (all N images) */
  int32_t reserved0;
  const float* cons_mask;   /* [N-n_lab][H][W] 0/1 weights of the consistency term, or NULL.  With a mask the term is
                               sum(mask * d^2) / (2*sum(mask) + 1e-16)  (UAMT, 2019_07...Uncertainty_Aware...py:160-164) instead of the mean */
} HpfgLossArgs;
/* A row of `partials` / `sums`: 0 nll0, 1 cnt0, 2 nll1, 3 cnt1, 4 mse, 5 sum mask, 6..7 unused, then 8 + g * 3 * S + k * S + c for label group g,
   k = 0 / 1 / 2 = I (sum p t) / Z (sum p p) / Y (sum t t) and class c, with class stride S = 4 for C <= 4 and S = 16 above: 8 + 6 * S floats */
#define HPFG_LOSS_NSUM 32           /* C <= 4 */
#define HPFG_LOSS_NSUM_WIDE 104     /* 5 <= C <= 16 */
int hpfg_loss_blocks(int N, int H, int W);
int hpfg_loss_nsum(int C);          /* floats per row of `partials` and in `sums`: HPFG_LOSS_NSUM for C <= 4, HPFG_LOSS_NSUM_WIDE above */
int hpfg_seg_loss_partials(const HpfgLossArgs* a, void* stream);   /* softmax + CE/Dice/MSE partial sums */
int hpfg_seg_loss_partials_x(const HpfgLossArgs* a, const HpfgPeerX* px, void* stream);   /* + the cross-rank sum of `sums` (peer mailbox) */
int hpfg_seg_loss_finalize(const HpfgLossArgs* a, void* stream);   /* sums -> loss scalars (device) */
int hpfg_seg_loss_bwd(const HpfgLossArgs* a, const float* grad_scale_dev /* NULL = 1 */, void* stream);   /* dlogits */
/* pseudo-labels: argmax over classes of teacher logits, optionally CutMix-blended with labels (main.py:177-178) */
int hpfg_argmax_labels(const float* logits, int N, int H, int W, int C, const uint8_t* mix_labels, const float* mix_mask,
                       uint8_t* out, void* stream);
/* evaluation (val.py:376-387, medpy binary dc): counts[gt*C + pred] += 1 over n voxels (labels >= C are ignored); the caller
 * zeroes `counts` (C*C uint64) and derives per-class Dice = 2*n(A&B) / (n(A) + n(B)) from rows / columns */
int hpfg_confusion_counts(const uint8_t* pred, const uint8_t* gt, long n, int C, unsigned long long* counts, void* stream);
/* evaluation of Synapse volumes (val.py:243: zoom(slice, (patch/x, patch/y), order=3) of every slice on the host): the cubic B-spline resize
 * src [S][h][w] -> dst [S][H][W] (fp32, contiguous) of all slices of a volume in one call.  Spline prefilter (pole sqrt(3) - 2, mirror
 * boundaries) and interpolation are linear and separable, and the prefilter's response decays below 1e-9 within 16 samples: per axis, output
 * o is sum_t w[o][t] * in[first[o] + t] over HPFG_RESIZE_TAPS (= 4 + 2 * 16) input samples.  The caller builds that table on the host
 * (hpfg_amd/val.py::_cubic_axis_table, fp64) and passes it per axis, n_out * (HPFG_RESIZE_TAPS + 1) 4-byte words on the device:
 *   float w[n_out][HPFG_RESIZE_TAPS], then int32 first[n_out]; first[o] + min(HPFG_RESIZE_TAPS, n_in) <= n_in (taps beyond n_in carry weight 0),
 *   first[o] < 0: out[o] = 0 -- scipy writes its constant there (a last coordinate that lands a rounding error past n_in - 1).
 * taps_y: h -> H, taps_x: w -> W (16-byte aligned).  The axis-0 pass writes [S][H][w] floats into `scratch`
 * (hpfg_resize_cubic_scratch_bytes(); -1 for sizes the call refuses: an axis shorter than 2 or longer than 8192, S > 65535). */
#define HPFG_RESIZE_TAPS 36
int hpfg_resize_cubic(const float* src, int S, int h, int w, float* dst, int H, int W, const float* taps_y, const float* taps_x, void* scratch,
                      long scratch_bytes, void* stream);
long hpfg_resize_cubic_scratch_bytes(int S, int h, int w, int H, int W);
/* evaluation (val.py:376-387, medpy binary hd95 of pred == c against gt == c for every foreground class c = 1 .. C-1, no voxelspacing): the
 * surface distances of a predicted and a true label volume, uint8 [S][h][w] contiguous; labels >= C belong to no mask.  medpy's operations
 * restated: the surface of a mask is mask ^ scipy.ndimage.binary_erosion(mask, generate_binary_structure(ndim, 1)) (border_value 0): the
 * mask voxels with one of their 2 * ndim face neighbours outside the mask or outside the volume (ndim 2: S = 1 and only the in-plane
 * neighbours; ndim 3: the z neighbours count, so every voxel of an S = 1 volume is a surface voxel); the distance of a surface voxel is
 * distance_transform_edt(~other surface) there: with unit spacing the square root of an integer d^2 = dz^2 + dy^2 + dx^2 < 2^28, which the
 * device finds exactly by an exhaustive integer search.  Segment (c - 1) * 2 + side holds the surface voxels of class c, side 0 = pred, 1 = gt.
 *   hpfg_surface_counts     counts[HPFG_SURFACE_SEGS] (device; zeroed by the call) = surface voxels per segment
 *   hpfg_surface_distances  counts_host[HPFG_SURFACE_SEGS] (HOST memory): the points to keep per segment -- the counts above, or 0 for a
 *       segment to skip (a class that needs no search; both of its segments); never more points are written than it says.  Offsets are the
 *       running sum of counts_host.  workspace (device, 16-byte aligned, hpfg_surface_workspace_bytes(C, n), n = sum of counts_host):
 *         bytes [0, 256)  cursors;  from 256: int32 keys[n];  from 256 + 4 n rounded up to 256: int32 points[n] (linear voxel indices).
 *       keys[offset(seg) + i] = ((c - 1) << 28 | d^2) ^ 0x80000000 read as a signed integer, d^2 = squared distance from point i of the
 *       segment to the nearest point of the same class' other side: one signed sort of keys[0, n) orders every class' 2 segments (which are
 *       adjacent: medpy's hstack) by d^2, classes ascending, and d^2 = key & 0x0FFFFFFF.  A segment that is empty or whose partner is empty
 *       launches nothing; its keys stay 0x7F7F7F7F.  Four launches and fills whatever C is.
 * All three refuse (-1): a null pointer, ndim not 2 or 3, ndim 2 with S != 1, C outside 2 .. 16, an axis longer than 8192
 * (3 * 8191^2 < 2^28), S * h * w >= 2^31; hpfg_surface_workspace_bytes: C outside 2 .. 16, n outside 0 .. 2^31 - 1. */
#define HPFG_SURFACE_SEGS 32
int hpfg_surface_counts(const uint8_t* pred, const uint8_t* gt, int S, int h, int w, int C, int ndim, unsigned int* counts, void* stream);
int hpfg_surface_distances(const uint8_t* pred, const uint8_t* gt, int S, int h, int w, int C, int ndim, const unsigned int* counts_host,
                           void* workspace, long workspace_bytes, void* stream);
long hpfg_surface_workspace_bytes(int C, long n_points);
/* evaluation of image batches (val.py:109-151, medpy binary asd(pred, gt): the mean distance from the surface voxels of pred to the surface of
 * gt): the sum of sqrt(d^2) over the keys hpfg_surface_distances left in `workspace`, per segment, exact and independent of the order of the
 * points.  counts_host (HOST memory) and C are those of that call.  sums (device, long long [HPFG_SURFACE_SEGS][2], zeroed by the call):
 * with x = sqrt((double)d^2), hi = rint(x * 2^19) and lo = (x - hi * 2^-19) * 2^52 (an exact integer, |lo| <= 2^32), sums[s][0] = sum of hi
 * (read as unsigned), sums[s][1] = sum of lo (signed) over segment s, added with integer atomics: the segment's sum of distances is
 * sums[s][0] * 2^-19 + sums[s][1] * 2^-52 and the ASD of class c that over counts_host[s] for s = (c - 1) * 2 (pred -> gt).  A segment that is
 * empty, whose partner is empty (its keys are the 0x7F fill) or that lies beyond 2 (C - 1) is skipped: zeros.  One fill and one launch.
 * Refuses (-1): a null pointer, C outside 2 .. 16, counts beyond the segments of C classes or 2^31 points, a workspace smaller than
 * hpfg_surface_workspace_bytes(C, n) or not 16-byte aligned, sums not 8-byte aligned. */
int hpfg_surface_sums(const void* workspace, long workspace_bytes, int C, const unsigned int* counts_host, long long* sums, void* stream);
/* Training-time slice augmentation on the device (datasets/utils.py:73-117 RandomGenerator.__call__: random_rot_flip | random_rotate,
 * then scipy zoom(order=0) to the network size, image and mask alike).  The host draws the random parameters in the reference's
 * order and supplies, per sample, the source slice, the rot90/flip or rotation parameters (rotation matrix and offset exactly
 * as scipy.ndimage.rotate computes them) and scipy's 1-D zoom index tables; the kernel gathers image [B][1][H][W] and mask [B][H][W]. */
typedef struct HpfgAugSample {
  int64_t img_off, lab_off;   /* element offsets of the source slice in the pools */
  int32_t h, w;               /* source slice size */
  int32_t mode;               /* 0 none, 1 rot90 + flip, 2 rotate */
  int32_t k, axis;            /* mode 1: np.rot90(a, k) then np.flip(axis) */
  int32_t tab_off;            /* offset into tabs: H row indices then W column indices of the intermediate image */
  double m00, m01, m10, m11, off_y, off_x;   /* mode 2: input coordinate = M * output index + offset */
} HpfgAugSample;
int hpfg_augment_batch(const float* img_pool, const uint8_t* lab_pool, const HpfgAugSample* samples_dev, const int* tabs_dev, int B, int H, int W,
                       float* out_img, uint8_t* out_lab, void* stream);
/* CutMix box masks (utils/utils.py:115-173 BoxMaskGenerator.generate_params): rects int32 [n][n_boxes][y0,y1,x0,x1] (bounds already
 * normalised like Python slices), out float [n][1][H][W] = (invert ? 0 : 1) flipped once per covering box */
int hpfg_box_masks(const int* rects, int n, int n_boxes, int H, int W, int invert, float* out, void* stream);
/* per-sample linear mix out[s] = a[s]*(1-f[s]) + b[s]*f[s] (ICT input mix, 2022_02_ISBI_ICT-MedSeg_ACDC.py:111-117) */
int hpfg_mix_samples(const float* a, const float* b, const float* f, float* out, int n, long per_sample, void* stream);
/* softmax(t0)*(1-f[s]) + softmax(t1)*f[s] over NHWC logits [n,H,W,C] (ICT mixed teacher prediction, :126-129) */
int hpfg_softmax_mix(const float* t0, const float* t1, const float* f, float* out_prob, int n, int H, int W, int C, void* stream);
/* diagnostics (tools/stream_timeline.py): *slot = s_memrealtime (100 MHz) when `stream` reaches this point; capturable */
int hpfg_timestamp(unsigned long long* slot, void* stream);
/* UAMT teacher-input noise (2019_07_MICCAI_Uncertainty_Aware_ACDC.py:130,142): out[i] = x[i % n_src] + clamp(noise[i]*scale, lo, hi) */
int hpfg_noise_add(const float* x, const float* noise, float* out, long n_src, long n_out, float scale, float lo, float hi, void* stream);
/* UAMT uncertainty mask (:147-151,162-163): T stochastic teacher predictions (NHWC logits) of the same S images, prediction
 * g = t*S + s stored in block g / per_block; mask[s,h,w] = (-sum_c pm*log(pm + 1e-6) < *threshold_dev), pm = mean_t softmax */
typedef struct HpfgPredBlocks {
  const float* p[8];
  int32_t n_blocks, per_block;
} HpfgPredBlocks;
int hpfg_uncertainty_mask(const HpfgPredBlocks* pb, int T, int S, int H, int W, int C, const float* threshold_dev, float* mask /* [S,H,W] */,
                          float* uncertainty /* [S,H,W] or NULL */, void* stream);
/* CutMix image blend x1*(1-M)+xu*M (main.py:149) */
int hpfg_cutmix_blend(const float* a, const float* b, const float* mask, float* out, long n, void* stream);

/* ---- token-layout ops of the SegFormer branch (model/segformer.py).  [B,N,C] tokens == NHWC pixels. --- */
/* nn.LayerNorm(C) (eps 1e-5) over the last dimension (segformer.py:107,174,192,195,232-244); mean / rstd [rows] are kept for backward */
int hpfg_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C, void* stream);
int hpfg_ln_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta /* == dgamma + C */,
                float* partials /* [hpfg_ln_bwd_blocks(rows)][2][C] */, long rows, int C, void* stream);
int hpfg_ln_bwd_blocks(long rows);
/* LayerNorm with eps as an argument, written through the pixel shuffle of the Swin-UNet patch expanding (reference model/swinunet.py:85-111:
 * Linear, rearrange 'B H W (P1 P2 C) -> B (H P1) (W P2) C', LayerNorm(C)): x [B,H,W,P*P*C] -- the expand Linear's output, a contiguous
 * [B*H*W*P*P, C] row matrix -- row (b,h,w,p1,p2) is normalised over C and written at row (b, h*P+p1, w*P+p2) of y [B,H*P,W*P,C]; mean / rstd
 * [B*H*W*P*P] are kept per row of x.  The backward reads dy through the same map, writes dx contiguously (every element once) and sums
 * dgamma / dbeta from per-workgroup partials in a fixed order.  P 1, 2 or 4 (P = 1: plain LayerNorm with eps, the norms of the Swin-UNet at
 * 1e-6); C % 4 == 0, 4 <= C <= 1536.  With P = 1, eps = 1e-5 and C <= 1024 the bits of hpfg_ln_fwd / hpfg_ln_bwd.  Returns -1 otherwise. */
int hpfg_ln_px_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int B, int H, int W, int P, int C, float eps,
                   void* stream);
int hpfg_ln_px_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma,
                   float* dbeta /* == dgamma + C */, float* partials /* [hpfg_ln_px_bwd_blocks(rows)][2][C] */, int B, int H, int W, int P, int C, void* stream);
int hpfg_ln_px_bwd_blocks(long rows);
/* Attention.forward :122-126 without its Linear layers: out[b,i,h,:] = softmax_j(scale * q[b,i,h,:].k[b,j,h,:]) v[b,j,h,:];
 * q [B,N,heads,32], kv [B,M,2,heads,32] (the kv Linear's output as reshaped at :120), M <= 64 keys, head dim 32 */
int hpfg_attn_fwd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, float scale, void* stream);
/* backward: dq, and the matrices P, dS [B,heads,N,M] from which dV = P^T dO and dK = scale * dS^T Q follow (GEMMs) */
int hpfg_attn_bwd(const float* q, const float* kv, const float* dout, float* dq, float* P, float* dS, int B, int N, int M, int heads, float scale,
                  void* stream);
/* the same two with the head dim as an argument (32 or 64: q [B,N,heads,head_dim], kv [B,M,2,heads,head_dim]); the two above are head_dim = 32 */
int hpfg_attn_fwd_hd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, int head_dim, float scale, void* stream);
int hpfg_attn_bwd_hd(const float* q, const float* kv, const float* dout, float* dq, float* P, float* dS, int B, int N, int M, int heads, int head_dim,
                     float scale, void* stream);
/* DWConv (3x3 depthwise, pad 1, :139-146) + F.gelu (:156) on [B,H,W,C]; w9 = the [C,1,3,3] weight transposed to [9][C] */
int hpfg_dwgelu_fwd(const float* x, const float* w9, const float* bias, float* y, int B, int H, int W, int C, void* stream);
int hpfg_dwgelu_bwd(const float* x, const float* w9, const float* bias, const float* dy, float* du /* scratch [B,H,W,C] */, float* dx, float* dw9,
                    float* dbias /* == dw9 + 9*C */, float* partials /* [hpfg_dwgelu_bwd_blocks()][10][C] */, int B, int H, int W, int C, void* stream);
int hpfg_dwgelu_bwd_blocks(int B, int H, int W);
/* Depthwise k x k conv (k = 3 or 5, pad k / 2, stride 1) with no activation on [B,H,W,C], C % 4 == 0 (csrc/dwconv.hip; reference model/uniformer.py:
 * pos_embed, x + dwconv3x3(x), :91,102 and :125,135; CBlock.attn, the depthwise 5 x 5, :96,103).  wk = the [C,1,k,k] weight transposed to [k*k][C].
 *   fwd: y = (res ? res : 0) + dw_k(x) + bias; res may be x itself.  y is none of the inputs.
 *   bwd: dx = dw_k^T(dy) (+ dy when add_dy), dwk[t][c] = sum_p dy[p][c] x[p + off(t)][c], dbias[c] = sum_p dy[p][c]; the sums go through one row
 *        of partials per workgroup and a fixed-order reduction (no atomics: the same bits every run).
 * Any other k or C returns -1 and launches nothing. */
int hpfg_dwconv_fwd(const float* x, const float* wk /* [k*k][C] */, const float* bias, const float* res /* NULL or [B,H,W,C]; may be x */, float* y,
                    int B, int H, int W, int C, int k, void* stream);
int hpfg_dwconv_bwd(const float* x, const float* wk, const float* dy, float* dx, int add_dy, float* dwk /* [k*k][C] */, float* dbias /* [C] */,
                    float* partials /* [hpfg_dwconv_bwd_blocks()][k*k+1][C] */, int B, int H, int W, int C, int k, void* stream);
int hpfg_dwconv_bwd_blocks(int B, int H, int W, int k);
/* F.interpolate(mode="bilinear", align_corners=False) of SegFormerHead.forward (:314,319) on NHWC [B,h,w,C] -> [B,H,W,C]; backward is a
 * gather over the outputs that tap a source pixel (no atomics), upsampling only */
int hpfg_resize_bilinear_fwd(const float* x, float* y, int B, int h, int w, int H, int W, int C, void* stream);
/* y = base + sum_k resize(xs[k]) (same bilinear map per source; base, y: [B,H,W,C]; xs[k]: [B,hs[k],ws[k],C]; nsrc <= 3; y may alias base):
 * the head's sum over stages of F.interpolate(...) (model/segformer.py:309-314 with linear_fuse applied per stage) in one pass */
int hpfg_resize_sum_fwd(const float* base, const float* const* xs, const int* hs, const int* ws, int nsrc, float* y, int B, int H, int W, int C,
                        void* stream);
int hpfg_resize_bilinear_bwd(const float* dy, float* dx, int B, int h, int w, int H, int W, int C, void* stream);
/* ConvModule's BatchNorm2d (train) + ReLU and the head's Dropout2d (segformer.py:288-296,307,318) over tokens [R,C]:
 * column sums (sum x, sum x^2) -> the caller forms mean / rstd (and the running statistics) -> apply; mask [R/rows_per_image][C] of
 * 0/1 keeps (or NULL), scaled by inv_keep.  Backward: sums [2][C] = (sum g, sum g*xhat) = (dbeta, dgamma), then dx. */
/* residual branch with stochastic depth (Block.forward :197-198, DropPath :23-30): out[b] = x[b] + y[b] * scale[b] (scale NULL = 1); the
 * branch gradient is dout[b] * scale[b] */
int hpfg_residual_scale(const float* x, const float* y, const float* scale, float* out, int B, long per_sample, void* stream);
int hpfg_scale_rows(const float* d, const float* scale, float* out, int B, long per_sample, void* stream);
/* exact (erf) GELU on its own, 4 floats per lane (Mlp.act of the Swin blocks, reference model/swinunet.py:114-133): y = gelu(x); dx = dy gelu'(x).
 * n % 4 == 0 */
int hpfg_gelu_fwd(const float* x, float* y, long n, void* stream);
int hpfg_gelu_bwd(const float* x, const float* dy, float* dx, long n, void* stream);
/* Dropout over a flat fp32 tensor (pos_drop, proj_drop, Mlp.drop of the Swin-UNet, reference model/swinunet.py:130-132,241,440): y[i] = x[i] *
 * keep(i) / (1 - p), one hash word per four elements; keep(i) is the rule of hpfg_dropout_mask(n, p, seed, seed_dev), so that function is
 * its mask, or byte i of an explicit mask [n] (non-zero keeps).  The backward is the same call on dy.  n % 4 == 0, n < 2^32, 0 <= p < 1. */
int hpfg_token_dropout(const float* x, float* y, long n, float p, uint32_t seed, const uint32_t* seed_dev, const uint8_t* mask, void* stream);
/* PatchMerging.merging (reference model/swinunet.py:69-75) on NHWC x [B,H,W,C], H and W even, C % 4 == 0: y [B,H/2,W/2,4C] with
 * y[b][i][j][k C + c] = x[b][2 i + k % 2][2 j + k / 2][c] (the reference's concat order x0, x1, x2, x3); the backward scatters dy back, every
 * element of dx written once */
int hpfg_patch_merge_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int hpfg_patch_merge_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* im2col / col2im of PatchEmbed.proj (segformer.py:172: kernel k, stride s, padding k/2) on NHWC x [B,H,W,C]:
 * cols [B, Ho*Wo, k*k*C] with the patch ordered (u, v, c); col2im is the gather-form transpose (no atomics) */
int hpfg_im2col_nhwc(const float* x, float* cols, int B, int H, int W, int C, int k, int s, void* stream);
int hpfg_col2im_nhwc(const float* dcols, float* dx, int B, int H, int W, int C, int k, int s, void* stream);
/* weight gradient of nn.Linear over many tokens, dW[N][K] = dY[R][N]^T X[R][K] with R >> N, K (the q / kv / proj / fc1 / fc2 layers of the
 * high-resolution stages): row-split partial products + fixed-order reduction */
int hpfg_linear_wgrad(const float* dy, const float* x, float* dw, float* partials /* [hpfg_linear_wgrad_splits()][N][K] */, long R, int N, int K,
                      void* stream);
int hpfg_linear_wgrad_splits(long R, int N, int K);
/* per-channel batch statistics of tokens x [R][C]: sums[0][c] = sum_r x, sums[1][c] = sum_r (x - mean_c)^2 (centred: the biased variance
 * is sums[1] / R whatever the mean is) */
int hpfg_tok_col_stats(const float* x, long R, int C, float* partials /* [hpfg_tok_stat_blocks(R)][2][C] */, float* sums /* [2][C] */, void* stream);
int hpfg_tok_stat_blocks(long R);
int hpfg_bnrelu_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* mask, float inv_keep,
                      long rows_per_image, float* y, long R, int C, void* stream);
int hpfg_bnrelu_bwd(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* mask,
                    float inv_keep, long rows_per_image, float* dx, float* partials, float* sums, long R, int C, void* stream);
/* Train-mode BatchNorm over tokens x [R][C] with no activation (reference model/uniformer.py: CBlock.norm1 / norm2 :93,97, the stage norms
 * :292-295), every C % 4 == 0 up to 1024 (320 included, which hpfg_tok_col_stats refuses: the same kernels and, where both admit C, the same bits):
 *   stats: as hpfg_tok_col_stats, partials [hpfg_tok_stat_blocks(R)][2][C]
 *   apply: y = (x - mean) * rstd * gamma + beta (eval mode: the running statistics as mean / rstd)
 *   bwd:   sums[0] = sum_r dy (dbeta), sums[1] = sum_r dy * xhat (dgamma), dx = gamma * rstd * (dy - sums[0] / R - xhat * sums[1] / R) */
int hpfg_bn_tok_stats(const float* x, long R, int C, float* partials, float* sums /* [2][C] */, void* stream);
int hpfg_bn_tok_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* y, long R, int C, void* stream);
int hpfg_bn_tok_bwd(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma, float* dx,
                    float* partials /* [hpfg_tok_stat_blocks(R)][2][C] */, float* sums /* [2][C] */, long R, int C, void* stream);

/* ---- parameter updates --------------------------------------------------------------------------------- */
/* torch.optim.SGD(momentum, weight_decay) over a flat parameter buffer (utils/__init__.py:15-16); lr read from device */
int hpfg_sgd_step(float* p, const float* g, float* mom, long n, const float* lr_dev, float momentum, float weight_decay,
                  float grad_scale, void* stream);
/* torch.optim.AdamW (utils/__init__.py:17-19: lr, weight_decay; betas (0.9, 0.999), eps 1e-8) over flat buffers; lr and the step count
 * (float, number of steps already taken, exact up to 2^24; advanced by the call) are read from device memory, so the update replays inside
 * a hipGraph.  The betas are doubles: 1 - beta and the bias corrections 1 - beta^t are formed in double and then rounded, as torch forms
 * them (1 - float(0.999) is 1.3e-5 off 0.001). */
int hpfg_adamw_step(float* p, const float* g, float* m, float* v, long n, const float* lr_dev, float* step_dev, double beta1, double beta2, float eps,
                    float weight_decay, float grad_scale, void* stream);
/* EMA teacher: t = alpha*t + (1-alpha)*s over flat buffers (utils/utils.py:82-86); alpha read from device */
int hpfg_ema_update(float* t, const float* s, long n, const float* alpha_dev, void* stream);

/* Both in one pass over the student's flat buffers -- the last two statements of every Mean-Teacher-family iteration
 * (2017_03_NIPS_Mean-Teacher_ACDC.py:108-113: optimizer.step(); update_ema_variables(...)): t[i] = alpha*t[i] + (1-alpha)*p_new[i] for i < n_ema
 * (n_ema = n, or the leading backbone slice of main.py:68-76).  Bit-identical to hpfg_sgd_step followed by hpfg_ema_update. */
int hpfg_sgd_ema_step(float* p, const float* g, float* mom, long n, const float* lr_dev, float momentum, float weight_decay, float grad_scale,
                      float* t, long n_ema, const float* alpha_dev, void* stream);

/* hpfg_sgd_ema_step (t != NULL) or hpfg_sgd_step (t == NULL, n_ema 0, alpha_dev NULL) over [0, n) -- the same expressions, bit-identical
 * results -- that also writes, from the NEW weights, what hpfg_pack_weights produces in bf16x3 mode for the listed conv layers: the student's
 * fwd / dgrad fragments and padded bias rows and, from the new teacher weights, the teacher's fwd fragments and bias rows (bit-identical
 * too).  Only positions that hold a weight are written: the padding of a fragment buffer must have been zeroed by one hpfg_pack_weights
 * launch before.  Descriptors ascend in the flat buffer (weight, then bias of a layer); gaps = the ranges [lo, hi) between them, so that
 * descriptors and gaps tile [0, n) exactly (checked: every element is updated once). */
typedef struct HpfgUpdatePackDesc {
  long w_off, b_off;    /* flat offsets of the layer's OIHW weight and of its bias */
  void* wpk16_fwd;      /* student fragments as in HpfgPackDesc, or NULL */
  void* wpk16_dgrad;    /* or NULL */
  float* bias_pad;      /* [CoutPad] */
  void* t_wpk16_fwd;    /* teacher fwd fragments (from the new teacher weights), or NULL */
  float* t_bias_pad;    /* or NULL */
  int32_t Cout, Cin, CoutPad, CinPad, taps;
  int32_t kc, kc_t;     /* K packing of the student's / the teacher's buffers (hpfg_conv_kc) */
  int32_t reserved;
} HpfgUpdatePackDesc;
int hpfg_sgd_ema_pack_step(float* p, const float* g, float* mom, long n, const float* lr_dev, float momentum, float weight_decay, float grad_scale,
                           float* t, long n_ema, const float* alpha_dev, const HpfgUpdatePackDesc* table_dev, const HpfgUpdatePackDesc* table_host,
                           int nlayers, const long* gaps_dev, const long* gaps_host, int ngaps, void* stream);

/* ---- attention core on the matrix cores (SegFormer branch; reference model/segformer.py:92-128 after the q / kv projections) -------------- */
/* out = softmax(scale * q k^T) v per (image, head): q [B,N,heads,32], kv [B,M,2,heads,32] (the kv Linear's output), M <= 64 keys, head dim 32;
 * split-bf16 MFMA products, fp32 softmax.  Backward: dq like q, dkv like kv; scratch B * heads * hpfg_attn_mfma_blocks(N) * 2*64*32 floats
 * (per-workgroup dK / dV partials, summed in a fixed order). */
int hpfg_attn_mfma_fwd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, float scale, void* stream);
int hpfg_attn_mfma_bwd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, float* scratch, int B, int N, int M, int heads,
                       float scale, void* stream);
int hpfg_attn_mfma_blocks(int N);
/* the same kernels with the head dim as an argument: 32 (bit-identical to the entry points above, which forward here) or 64 (MiT-B1: two
 * MFMA k-steps per score tile, four d-tiles per output).  The backward's scratch holds hpfg_attn_mfma_scratch_floats(B, N, heads, head_dim)
 * floats (= B * heads * hpfg_attn_mfma_blocks(N) * 2 * 64 * head_dim; -1 for a head dim that is not built). */
int hpfg_attn_mfma_fwd_hd(const float* q, const float* kv, float* out, int B, int N, int M, int heads, int head_dim, float scale, void* stream);
int hpfg_attn_mfma_bwd_hd(const float* q, const float* kv, const float* dout, float* dq, float* dkv, float* scratch, int B, int N, int M, int heads,
                          int head_dim, float scale, void* stream);
long hpfg_attn_mfma_scratch_floats(int B, int N, int heads, int head_dim);

/* ---- attention core over 1 .. 256 keys (csrc/attn_keys.hip; reference model/segformer.py:92-128, whose Attention.forward has no key limit) -- */
/* The most keys the entry points below take: 256 = the (512 / 32)^2 keys of a MiT stage at 512 x 512 (reference model/segformer.py:92-128). */
int hpfg_attn_keys_max(void);
/* Forward (reference model/segformer.py:92-128 after the q / kv projections): out = softmax(scale * q k^T) v per (image, head) as
 * hpfg_attn_mfma_fwd_hd / hpfg_attn_fwd_hd, for 1 <= M <= hpfg_attn_keys_max() keys walked in blocks of 64; head_dim 32 or 64;
 * math = HPFG_MATH_BF16X3 (split-bf16 MFMA products; for M <= 64 bit-identical to hpfg_attn_mfma_fwd_hd) or HPFG_MATH_F32 (exact fp32).
 * lse [B,heads,N] receives the row log-sum-exp of the scaled scores (what the backward needs); it may be null (inference).  Returns -1 and
 * sets hpfg_last_error on a bad shape, head dim, math mode or a null q / kv / out. */
int hpfg_attn_keys_fwd(const float* q, const float* kv, float* out, float* lse, int B, int N, int M, int heads, int head_dim, float scale, int math,
                       void* stream);
/* Backward of the above (reference model/segformer.py:92-128 under autograd) from the saved out and lse: dq like q, dkv like kv.
 * delta = rowsum(dout . out), P = exp(S - lse), dS = P (dout V^T - delta); dK / dV partials per (query block, key block) are summed in a
 * fixed order (no atomics: bit-identical from run to run).  scratch: hpfg_attn_keys_scratch_floats(...) floats.  No pointer may be null. */
int hpfg_attn_keys_bwd(const float* q, const float* kv, const float* out, const float* lse, const float* dout, float* dq, float* dkv, float* scratch,
                       int B, int N, int M, int heads, int head_dim, float scale, int math, void* stream);
/* Floats of the backward's scratch for these arguments (reference model/segformer.py:92-128 needs none: autograd keeps the [B,heads,N,M]
 * probabilities instead); -1 with hpfg_last_error set when hpfg_attn_keys_bwd would refuse them. */
long hpfg_attn_keys_scratch_floats(int B, int N, int M, int heads, int head_dim, int math);

/* ---- shifted-window attention of the Swin blocks (csrc/attn_window.hip; reference model/swinunet.py:207-248) ----------------------------- */
/* Forward (reference model/swinunet.py:207-248, WindowAttention.forward between the qkv and the proj Linear): per (image, window, head)
 * out = softmax(scale q k^T + bias_table[idx][head] + mask) v over the window x window tokens of each window of the map rolled by -shift.
 * qkv [B,H,W,3C] is the qkv Linear's output (channel = t C + head head_dim + p, t = q, k, v; C = heads head_dim), bias_table
 * [(2 window - 1)^2, heads], out [B,H,W,C] (channel = head head_dim + p).  Roll, window partition, window reverse and the roll back are
 * addressing: position (i, j) of window (wy, wx) is the token ((wy window + i + shift) mod H, (wx window + j + shift) mod W), read and
 * written there; idx = (i1 - i2 + window - 1)(2 window - 1) + (j1 - j2 + window - 1); with shift > 0 the mask is the reference's literal
 * -100 between positions whose rolled coordinates lie in different regions (0 below H - window, 1 below H - shift, else 2, per axis).
 * window^2 <= 64, H % window == 0, W % window == 0, 0 <= shift < window, head_dim 32 or 64, heads >= 1; math = HPFG_MATH_BF16X3
 * (split-bf16 MFMA products; with shift 0 and a zero table the operation sequence of hpfg_attn_mfma_fwd_hd per window) or HPFG_MATH_F32
 * (exact fp32).  Returns -1 and sets hpfg_last_error on anything else or a null pointer. */
int hpfg_attn_window_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window, int shift,
                         float scale, int math, void* stream);
/* Backward of the above (reference model/swinunet.py:207-248 under autograd): dqkv like qkv, through the same addressing, every element
 * written exactly once; dbias like bias_table, dbias[idx][head] = sum of dS over images, windows and the pairs of that idx, from
 * per-workgroup partials added in a fixed order (no atomics: bit-identical from run to run).  scratch: hpfg_attn_window_scratch_floats(...)
 * floats.  No pointer may be null. */
int hpfg_attn_window_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B, int H, int W,
                         int heads, int head_dim, int window, int shift, float scale, int math, void* stream);
/* Floats of the backward's scratch (the bias-gradient partials; reference model/swinunet.py:207-248 needs none: autograd scatter-adds into the
 * table); -1 with hpfg_last_error set when hpfg_attn_window_bwd would refuse the shape. */
long hpfg_attn_window_scratch_floats(int B, int H, int W, int heads, int head_dim, int window, int math);
/* hpfg_attn_window_fwd / _bwd with dropout of the probabilities between the softmax and attn @ v (WindowAttention.attn_drop, reference
 * model/swinunet.py:237):  out = (P .* M / (1 - p)) V,  dP = (dO V^T) .* M / (1 - p),  dS = P .* (dP - rowsum(P .* dP)),  dV = (P .* M / (1 - p))^T dO,
 * the bias-table gradient from that dS.  Keep decision of element e = (((b nW + win) heads + h) L + l1) L + l2, L = window^2: the flat index of
 * the reference's attn tensor [B nW, heads, L, L] in its rolled, window-partitioned order -- byte e of `mask` when given (non-zero keeps), else
 * hpfg_keep(e, seed + *seed_dev, threshold(p)), the rule of the HpfgAct dropout; hpfg_attn_window_drop_mask writes that hash mask in the
 * explicit layout, hpfg_attn_window_drop_elems is its length (-1 for a bad shape; must stay below 2^32).  p = 0 without a mask runs the
 * kernels of hpfg_attn_window_fwd / _bwd.  Same scratch, same shapes, every element of dqkv written once, no atomics. */
int hpfg_attn_window_drop_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window, int shift,
                              float scale, int math, float p, uint32_t seed, const uint32_t* seed_dev, const uint8_t* mask, void* stream);
int hpfg_attn_window_drop_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B, int H, int W,
                              int heads, int head_dim, int window, int shift, float scale, int math, float p, uint32_t seed, const uint32_t* seed_dev,
                              const uint8_t* mask, void* stream);
long hpfg_attn_window_drop_elems(int B, int H, int W, int heads, int window);
int hpfg_attn_window_drop_mask(uint8_t* out, int B, int H, int W, int heads, int window, float p, uint32_t seed, const uint32_t* seed_dev, void* stream);

/* ---- the same attention for windows of at most 16 tokens, several windows per 64-row tile (csrc/attn_window_packed.hip) ------------------- */
/* The operation of hpfg_attn_window_drop_fwd (reference model/swinunet.py:219-241 with the roll / window partition / window reverse / roll
 * back of :263-276; the LIDC network of model/swinunet_LIDC.py runs it at window 3 and 4) for window 2, 3 or 4: 64 / window^2 windows of one
 * (image, head), in raster order, share a workgroup's tile; keys of another window of the tile are excluded exactly, like padding keys.
 * Same tensors, same bias and mask, same dropout elements (win = the window's index in the image), so hpfg_attn_window_drop_mask /
 * _drop_elems serve both.  p == 0 with a null mask is the no-dropout form.  HPFG_MATH_F32 runs the kernels of hpfg_attn_window_drop_fwd
 * (equal bits).  Returns -1 with hpfg_last_error naming the rule: window outside 2 .. 4, a side that is no multiple of the window, a shift
 * that is neither 0 nor window / 2, a head dim other than 32 / 64, a null pointer. */
int hpfg_attn_window_packed_fwd(const float* qkv, const float* bias_table, float* out, int B, int H, int W, int heads, int head_dim, int window, int shift,
                                float scale, int math, float p, uint32_t seed, const uint32_t* seed_dev, const uint8_t* mask, void* stream);
/* Backward of the above (the same reference lines under autograd): every element of dqkv written exactly once; dbias from per-workgroup
 * partials added in a fixed order (no atomics: two runs give the same bits).  scratch: hpfg_attn_window_packed_scratch_floats(...) floats,
 * every one of them written. */
int hpfg_attn_window_packed_bwd(const float* qkv, const float* bias_table, const float* dout, float* dqkv, float* dbias, float* scratch, int B, int H,
                                int W, int heads, int head_dim, int window, int shift, float scale, int math, float p, uint32_t seed,
                                const uint32_t* seed_dev, const uint8_t* mask, void* stream);
/* Floats of that scratch (reference model/swinunet.py:207-248 needs none: autograd scatter-adds into the table): one [heads][(2 window - 1)^2]
 * slab per (image, tile) in HPFG_MATH_BF16X3, hpfg_attn_window_scratch_floats in HPFG_MATH_F32; -1 with hpfg_last_error set for a refused shape. */
long hpfg_attn_window_packed_scratch_floats(int B, int H, int W, int heads, int head_dim, int window, int math);

/* ---- Swin-MAE pretraining (csrc/mae.hip; reference model/swin_mae.py, 2022_12_CVPR_Swin-MAE.py) ------------------------------------------ */
/* window_masking with remove=False, mask_len_sparse=False (reference model/swin_mae.py:649-710) from a given noise tensor: the S x S token map
 * is cut into d x d groups of r x r tokens (d = S / r); a group is kept iff its rank among the image's d * d noise values, ascending by
 * (noise, index) -- torch.argsort made total --, is below n_keep; mask [B, S * S] uint8 in token order y * S + x, 1 = removed.  One workgroup
 * per image ranks by counting against the noise row in LDS: d * d <= 1024.  n_keep = int(d * d * (1 - mask_ratio)) is the caller's (:673).
 * Returns -1 and sets hpfg_last_error on a null pointer, S % r != 0, more than 1024 groups or n_keep outside 0 .. d * d. */
int hpfg_mae_window_mask(const float* noise, uint8_t* mask, int B, int S, int r, int n_keep, void* stream);
/* x_masked[i, index_mask[i], :] = mask_token (reference model/swin_mae.py:706-709) over rows = B * L tokens of C channels:
 * y[row, :] = mask[row] ? token : x[row, :]; a masked row of x is not read.  C % 4 == 0, 4 <= C <= 1536. */
int hpfg_mae_mask_tokens_fwd(const float* x, const uint8_t* mask, const float* token, float* y, long rows, int C, void* stream);
/* its backward (reference model/swin_mae.py:706-709 under autograd): dx = dy on kept rows and 0 on masked ones; dtoken[c] = sum of dy[row, c]
 * over the masked rows -- per-workgroup partial sums over contiguous row ranges, then one finishing kernel that adds them in a fixed order
 * (no atomics: equal bits from run to run).  partials: hpfg_mae_mask_tokens_bwd_blocks(rows) * C floats of scratch. */
int hpfg_mae_mask_tokens_bwd(const float* dy, const uint8_t* mask, float* dx, float* dtoken, float* partials, long rows, int C, void* stream);
int hpfg_mae_mask_tokens_bwd_blocks(long rows);
/* The masked reconstruction loss and its gradient from one pass over pred (reference model/swin_mae.py:775-791 forward_loss and
 * 2022_12_CVPR_Swin-MAE.py:112): pred [B, L, patch^2 Cin] with the channel order (p, q, c) of decoder_pred, img [B, Cin, H, W] read through
 * the patchify addressing (:621-633: target[b, h Wp + w, (p patch + q) Cin + c] = img[b, c, h patch + p, w patch + q]) -- no patchified or
 * un-patchified copy is made --, mask [B, L] (non-zero = removed).  *loss = scale * sum over masked tokens of sum_j (pred - target)^2;
 * dpred = 2 scale (pred - target) on masked tokens, 0 on kept ones, whose pred rows and pixels are not read.  norm_pix != 0: the target patch is
 * normalised first, (t - mean) / sqrt(var + 1e-6) with the unbiased variance over its patch^2 Cin values (:782-785).  scale = 1 / (B Cin H W
 * mask_ratio) gives the driver's mean((pred_img - img)^2 mask_img) / mask_ratio, scale = 1 / (patch^2 Cin n_masked) forward_loss.
 * Two kernels on the stream, no host synchronisation: token sums -> one partial per workgroup (fixed tree), then one workgroup adds the
 * partials in index order and writes *loss (device).  partials: hpfg_mae_loss_blocks(B, H, W, patch) floats (-1 for a shape that is refused).
 * patch == 4, 1 <= Cin <= 4, H % 4 == 0, W % 4 == 0. */
int hpfg_mae_loss(const float* pred, const float* img, const uint8_t* mask, float scale, int norm_pix, float* loss, float* dpred, float* partials,
                  int B, int Cin, int H, int W, int patch, void* stream);
long hpfg_mae_loss_blocks(int B, int H, int W, int patch);

/* ---- projection necks + Dense_Loss (UNet_Plus; reference model/unet.py:120-152, utils/loss/dense_loss.py:17-40) ------------------------ */
/* C[m,n] = act(sum_k A(m,k) B(k,n) + bias[n]) in exact fp32 on the matrix cores; A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn], C row-major
 * (ldc); relu: max(.,0) in the epilogue; accumulate: C += (before the activation).  Replaces nn.Linear / 1x1 nn.Conv2d forward and both backward
 * products of the necks (unet.py:125-138) and torch.mm of dense_loss.py:24.  Deterministic: no atomics; this entry point does not split K, and
 * hpfg_gemm_f32_splitk below adds its partial products in split order. */
int hpfg_gemm_f32(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M, int N, int K,
                  const float* bias, int relu, int accumulate, void* stream);
/* the same with the contraction split over workgroups when the product has few output tiles and a long K (fixed-order sum of the partials);
 * scratch: hpfg_gemm_f32_splits(M, N, K) * M * N floats */
int hpfg_gemm_f32_splitk(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M, int N, int K,
                         const float* bias, int relu, int accumulate, float* scratch, void* stream);
int hpfg_gemm_f32_splits(int M, int N, int K);
/* the same contract in split-bf16 arithmetic (hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, fp32 accumulate; 128 x 128 tiles): every
 * nn.Linear / kernel==stride conv / 1x1 conv of the SegFormer branch (reference model/segformer.py:92-177, 298-320), forward and input
 * gradient, and the weight gradient of layers with few tokens.  Operands need a unit stride along one index and 4-element alignment:
 * hpfg_gemm_bf16x3_ok() tells; callers fall back to hpfg_gemm_f32 otherwise. */
int hpfg_gemm_bf16x3(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M, int N, int K,
                     const float* bias, int relu, int accumulate, void* stream);
/* The same product with the contraction split over workgroups where the output has few 128 x 128 tiles and K is long (hpfg_gemm_bf16x3_splits > 1:
 * the 1568-token layers, K up to 2048); scratch: splits * M * N floats; partial products are added in split order (deterministic) */
int hpfg_gemm_bf16x3_splits(int M, int N, int K);
int hpfg_gemm_bf16x3_splitk(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* Cm, long ldc, int M, int N, int K,
                            const float* bias, int relu, int accumulate, float* scratch, void* stream);
int hpfg_gemm_bf16x3_ok(const float* A, long sam, long sak, const float* B, long sbk, long sbn, int M, int N, int K);
/* weight gradient dW[N][K] = dY^T X over R tokens (dY [R][N], X [R][K] contiguous) in split-bf16 arithmetic: operands staged as they lie in
 * memory, fragments through the transposing LDS read, rows split over workgroups, partials summed in a fixed order.
 * with_db: the bias gradient db[N] = column sums of dY comes out of the same pass, written right behind dW (dw_db: N*K + N floats).
 * partials: hpfg_gemm_tn_splits(R, N, K) * (N*K + N) floats of scratch.  (autograd's mm / sum for the parameters of nn.Linear, segformer.py) */
int hpfg_gemm_tn_bf16x3(const float* dy, const float* x, float* dw_db, float* partials, long R, int N, int K, int with_db, void* stream);
int hpfg_gemm_tn_splits(long R, int N, int K);
int hpfg_col_sum(const float* x, long R, int M, long ldx, float* out /* [M] = sum over rows */, void* stream);   /* bias gradients */
int hpfg_col_sum2(const float* x, long R, int M, long ldx, float* out, float* scratch /* hpfg_col_sum_splits(R) * M floats */, void* stream);
int hpfg_col_sum_splits(long R);
int hpfg_relu_bwd(float* dy, const float* y, long n, void* stream);                                         /* dy *= (y > 0): nn.ReLU backward */
/* nn.AdaptiveAvgPool2d((1,1)) and ((S,S)) of an NHWC tensor in one launch (unet.py:141-142,146): gap [N,C], pool [N,S*S,C]; C <= 1024, S <= H, W */
int hpfg_neck_pool_fwd(const float* x, int pstride, int N, int H, int W, int C, int S, float* gap, float* pool, void* stream);
int hpfg_neck_pool_bwd(const float* dgap /* or NULL */, const float* dpool /* or NULL */, int N, int H, int W, int C, int S,
                       float* dx /* NHWC contiguous, overwritten */, void* stream);
/* F.normalize(x, dim=1) of x viewed as [G,D,S] with element (g,d,s) at g*D*S + d*sd + s*ss, (sd,ss) = (S,1) or (1,D) (dense_loss.py:18-19) */
int hpfg_l2norm_fwd(const float* x, int G, int D, int S, int sd, int ss, float* u, float* norms /* [G*S] */, void* stream);
int hpfg_l2norm_bwd(const float* du, const float* u, const float* norms, int G, int D, int S, int sd, int ss,
                    const float* scale /* device scalar multiplied into dx, or NULL */, float* dx, void* stream);
/* NT-Xent of dense_loss.py:24-36 from the Gram matrix [2n,2n] of the normalised rows [student ; teacher]: loss[0] = mean_i -log(pos_i / denom_i);
 * Q (or NULL) [n,2n] = dL/dGram + its transpose for the student rows, so that dL/d(student row i) = sum_j Q[i,j] * row_j */
int hpfg_ntxent_rows(const float* gram, int n, float temperature, float* loss, float* Q, void* stream);

#ifdef __cplusplus
}
#endif
#endif
