"""Shared helpers for the parity tests: run the oracle with exactly the dropout masks the HIP kernels used."""
import numpy as np
import torch

from hpfg_amd import engine as E
from oracle import rng_ref, unet_ref


def state_from_module(m):
    """Oracle state dict (CPU clones) from an hpfg_amd module."""
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def engine_masks(eng, seed_step, n, h, w):
    """Keep-masks (NCHW float) of the five encoder dropout sites for a forward that used `seed_step`."""
    masks = []
    for lvl in range(5):
        s = eng.specs[E.enc_prefix(lvl) + ".0"]
        seed = (eng.layer_seed(s) + seed_step) & 0xFFFFFFFF
        masks.append(torch.from_numpy(rng_ref.keep_mask_nchw(n, s.cout, s.h, s.w, s.drop_p, seed).astype(np.float32)))
    return masks


def nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).contiguous()


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- ad-hoc single-layer harness around the C ABI (unit tests of conv / dgrad / wgrad) ----------------------------------
import ctypes as C

from hpfg_amd import _lib as L


def pad16(c):
    return (c + 15) // 16 * 16


class AdHocConv:
    def __init__(self, cin, cout, taps, device, seed=0, hw=(16, 16)):
        k = 3 if taps == 9 else 1
        self.cin, self.cout, self.taps, self.k, self.dev = cin, cout, taps, k, device
        w, b = adhoc_weights(cin, cout, taps, seed)
        self.w, self.b = w.to(device), b.to(device)
        self.cin_pad, self.cout_pad = pad16(cin), pad16(cout)
        n = taps * self.cin_pad * self.cout_pad
        self.wpk_f = torch.empty(n, device=device)
        self.wpk_d = torch.empty(n, device=device)
        self.bias_pad = torch.empty(self.cout_pad, device=device)
        lib = L.load()
        self.kc = lib.hpfg_conv_kc(hw[0], hw[1], taps)
        self.wpk16_f = torch.empty(lib.hpfg_wpk16_elems(cin, self.cout_pad, taps, self.kc), dtype=torch.bfloat16, device=device)
        self.wpk16_d = torch.empty(lib.hpfg_wpk16_elems(cout, self.cin_pad, taps, self.kc), dtype=torch.bfloat16, device=device)
        d = (L.PackDesc * 1)()
        d[0].wpk16_fwd, d[0].wpk16_dgrad, d[0].kc = L.ptr(self.wpk16_f), L.ptr(self.wpk16_d), self.kc
        d[0].w_oihw, d[0].b, d[0].wpk_fwd, d[0].wpk_dgrad, d[0].bias_pad = (L.ptr(self.w), L.ptr(self.b), L.ptr(self.wpk_f), L.ptr(self.wpk_d),
                                                                          L.ptr(self.bias_pad))
        d[0].Cout, d[0].Cin, d[0].CoutPad, d[0].CinPad, d[0].taps = cout, cin, self.cout_pad, self.cin_pad, taps
        dev_tab = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(device)
        self._keep = (d, dev_tab)
        L.check(L.load().hpfg_pack_weights(dev_tab.data_ptr(), d, 1, stream(device)), "pack")

    def conv(self, a0, a1, N, H, W, stats=False, dgrad=False, math=0, stat_acc=None, shards=1, bwd_stats=0, bwd_of=None,
             out_pstride=None, out_coff=0, out_split=0, out2_pstride=None, out2_coff=0, stage_out=None, side_sums=None):
        """stat_acc / shards: with stats=True the BatchNorm sums ALSO go into this zeroed accumulator (HpfgConvArgs.stat_acc), next to the rows
        of partial sums.  bwd_stats / bwd_of: the dgrad epilogue's backward sums (HpfgConvArgs.bwd_stats).  self.rows = rows the launch wrote.
        out_pstride / out_coff: the output lives at channel offset out_coff of a NaN-prefilled buffer of out_pstride floats per pixel, which is
        what is returned.  out_split / out2_pstride / out2_coff: output channels >= out_split go to a second such buffer, self.out2.
        stage_out / side_sums: tensors the launch fills (HpfgConvArgs.stage_out, .side_sums)."""
        lib = L.load()
        cout = self.cin if dgrad else self.cout
        cpad = self.cin_pad if dgrad else self.cout_pad
        out = torch.full((N, H, W, out_pstride or cout), float("nan"), device=self.dev)
        ca = L.ConvArgs()
        ca.a0, ca.a1 = a0, (a1 if a1 is not None else L.Act())
        ca.math = math
        if math == L.MATH_BF16X3:
            assert lib.hpfg_conv_kc(H, W, self.taps) == self.kc, "AdHocConv was packed for a different tile class"
            ca.wpk = L.ptr(self.wpk16_d if dgrad else self.wpk16_f)
        else:
            ca.wpk = L.ptr(self.wpk_d if dgrad else self.wpk_f)
        ca.bias = None if dgrad else L.ptr(self.bias_pad)
        part = None
        if stats:
            part = torch.zeros(lib.hpfg_conv_stat_blocks(N, H, W) * 2 * cpad, device=self.dev)   # unused rows stay 0
            ca.stat_partials = L.ptr(part)
            if stat_acc is not None:
                assert stat_acc.dtype == torch.int64 and stat_acc.numel() == shards * 2 * cpad * 2
                ca.stat_acc, ca.stat_shards = L.ptr(stat_acc), shards
        if bwd_stats:
            ca.bwd_stats, ca.bwd_of = bwd_stats, bwd_of
        ca.out_pstride, ca.Cout, ca.CoutPad, ca.N, ca.H, ca.W, ca.taps = out_pstride or cout, cout, cpad, N, H, W, self.taps
        ca.out = out.data_ptr() + 4 * out_coff
        self.out2 = None
        if out_split:
            self.out2 = torch.full((N, H, W, out2_pstride or cout - out_split), float("nan"), device=self.dev)
            ca.out2, ca.out_split, ca.out2_pstride = self.out2.data_ptr() + 4 * out2_coff, out_split, self.out2.shape[-1]
        ca.stage_out, ca.side_sums = L.ptr(stage_out), L.ptr(side_sums)
        self.rows = lib.hpfg_conv_stat_rows(C.byref(ca)) if (stats or side_sums is not None) else 0
        L.check(lib.hpfg_conv_fwd(C.byref(ca), stream(self.dev)), "conv_fwd")
        return out, part

    def wgrad(self, a0, a1, g, N, H, W, math=0, slab_nan=False):
        """slab_nan: the slab workspace starts as NaN, so that a slab the launch leaves unwritten shows in the reduced gradient."""
        lib = L.load()
        wa = L.WgradArgs()
        wa.a0, wa.a1, wa.g = a0, (a1 if a1 is not None else L.Act()), g
        S = lib.hpfg_wgrad_splits(N, H, W, self.cin_pad, self.cout_pad, self.taps)
        slab = torch.empty(lib.hpfg_wgrad_slab_floats(N, H, W, self.cin_pad, self.cout_pad, self.taps), device=self.dev)
        if slab_nan:
            slab.fill_(float("nan"))
        dw = torch.full_like(self.w, float("nan"))
        wa.slab, wa.dw_oihw, wa.math = L.ptr(slab), L.ptr(dw), math
        wa.Cin, wa.CinPad, wa.Cout, wa.CoutPad, wa.N, wa.H, wa.W, wa.taps, wa.S = self.cin, self.cin_pad, self.cout, self.cout_pad, N, H, W, self.taps, S
        L.check(lib.hpfg_wgrad(C.byref(wa), stream(self.dev)), "wgrad")
        return dw


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def plain_act(t, C_, H, W):
    """PLAIN (or STRIDED when C%4 != 0) source over a contiguous NHWC tensor."""
    a = L.Act()
    a.z, a.mode, a.C, a.Hs, a.Ws, a.pstride = L.ptr(t), L.ACT_PLAIN, C_, H, W, C_
    if C_ % 4:
        a.mode = L.ACT_STRIDED
        a.sn, a.sc, a.sy, a.sx = H * W * C_, 1, W * C_, C_
    return a


# ---- BatchNorm sum accumulators (HpfgConvArgs.stat_acc / HpfgAct.bn_acc): long long [shard][which][C][limb] ---------------------------
from fractions import Fraction

ACC_SCALE = 2 ** 52      # a float t is added as hi + lo * 2^-52


def acc_encode(t_f32):
    """The two limbs hpfg_acc_add (csrc/common.h) adds for a float t, in numpy float32 like the device: r = rint(t), hi = r,
    lo = rint((t - r) * 2^52).  -> (hi, lo) int64 arrays of t's shape."""
    t = np.asarray(t_f32, dtype=np.float32)
    r = np.rint(t)
    lo = np.rint((t - r) * np.float32(ACC_SCALE))
    assert r.dtype == np.float32 and lo.dtype == np.float32
    return r.astype(np.int64), lo.astype(np.int64)


def acc_totals(acc_tensor, C_, shards):
    """Sum of an accumulator tensor over its shards as Python integers (no 64-bit wrap): object array [2 (which)][C][2 (limb)]."""
    a = acc_tensor.detach().cpu().numpy().reshape(shards, 2, C_, 2).astype(object)
    return a.sum(0)


def acc_rows_totals(rows_f32):
    """What acc_totals must give after one hpfg_acc_add per row of partial sums: rows [R][2][C] float32 -> object array [2][C][2]."""
    hi, lo = acc_encode(rows_f32)
    return np.stack([hi.astype(object).sum(0), lo.astype(object).sum(0)], -1)


def acc_decode(totals):
    """float64 [2][C]: the correctly rounded value hi + lo * 2^-52 of every (hi, lo) pair of acc_totals."""
    t = np.asarray(totals, dtype=object)
    out = np.empty(t.shape[:-1], dtype=np.float64)
    for i in np.ndindex(*out.shape):
        out[i] = float(Fraction(int(t[i][0])) + Fraction(int(t[i][1]), ACC_SCALE))
    return out


def acc_from_rows(rows_f32, shards, device=None):
    """An accumulator tensor [shards][2][C][2] (int64) holding one hpfg_acc_add per row of rows [R][2][C] float32, row r in shard r % shards."""
    rows = np.asarray(rows_f32, dtype=np.float32)
    hi, lo = acc_encode(rows)
    acc = np.zeros((shards,) + rows.shape[1:] + (2,), dtype=np.int64)
    for r in range(rows.shape[0]):
        acc[r % shards, ..., 0] += hi[r]
        acc[r % shards, ..., 1] += lo[r]
    t = torch.from_numpy(acc)
    return t if device is None else t.to(device)


# ---- the optimizer kernels of csrc/misc.hip restated in numpy float32, and float64 references of the mixing kernels ---------------------
import functools

N_SMALL = 4099                      # odd, 17 workgroups
N_BIG_OPTIM = 2048 * 256 + 257      # one element past a full pass of the optimizer launches (grid_for(n, 2048)): the grid-stride loop runs twice
N_BIG_MIX = 4096 * 256 + 257        # the same for the launches capped at 4096 workgroups
F32 = np.float32


def f32_exact(x) -> float:
    """The float32 a C `float` argument or a float32 device word holds for the Python float x, as a Python float: a float64 reference that
    is handed these sees the same hyper-parameters as the kernel."""
    return float(np.float32(x))


def sgd_ema_f32(p, g_steps, mom, lrs, momentum, wd, gscale, t=None, n_ema=0, alphas=None):
    """sgd_kernel / sgd_ema_kernel / ema_kernel (compiled with fp contract(off)) over len(lrs) steps, one float32 rounding per operation, in
    torch.optim.SGD's order:  d = g*gscale + wd*w;  buf = momentum*buf + d;  w = w - lr*buf;  t[:n_ema] = t*a + w*(1 - a), 1 - a formed in
    float32.  g_steps [steps][n].  -> (p, mom, t) float32 copies; the inputs are left alone."""
    p, mom = np.array(p, dtype=F32), np.array(mom, dtype=F32)
    t = None if t is None else np.array(t, dtype=F32)
    mu, wd, gs = F32(momentum), F32(wd), F32(gscale)
    for k, lr in enumerate(lrs):
        g = np.asarray(g_steps[k], dtype=F32)
        d = g * gs + wd * p
        mom = mu * mom + d
        p = p - F32(lr) * mom
        if t is not None and n_ema > 0:
            a = F32(alphas[k])
            t[:n_ema] = t[:n_ema] * a + p[:n_ema] * (F32(1) - a)
        assert p.dtype == F32 and mom.dtype == F32
    return p, mom, t


def sgd_ema_f64(p, g_steps, mom, lrs, momentum, wd, gscale, t, alphas):
    """The same trajectory by torch.optim.SGD itself on float64 CPU tensors (gradient pre-multiplied by gscale) and a float64 EMA
    t = t*a + w*(1 - a) over the whole buffer; hyper-parameters as the float32 words the kernel reads.  -> (p, mom, t) float64 numpy."""
    w = torch.tensor(np.asarray(p), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([w], lr=1.0, momentum=f32_exact(momentum), weight_decay=f32_exact(wd))
    if momentum != 0:
        opt.state[w]["momentum_buffer"] = torch.tensor(np.asarray(mom), dtype=torch.float64)      # (torch starts a missing buffer at d, not at 0*buf + d)
    te = torch.tensor(np.asarray(t), dtype=torch.float64)
    for k, lr in enumerate(lrs):
        opt.param_groups[0]["lr"] = f32_exact(lr)
        w.grad = torch.tensor(np.asarray(g_steps[k]), dtype=torch.float64) * f32_exact(gscale)
        opt.step()
        a = f32_exact(alphas[k])
        te = te * a + w.detach() * (1.0 - a)
    buf = opt.state[w]["momentum_buffer"].numpy() if momentum != 0 else None
    return w.detach().numpy(), buf, te.numpy()


SGD_LRS = (0.05, 0.031, 0.02, 0.011, 0.007)                     # another lr every step
SGD_ALPHAS = tuple(min(1 - 1 / (k + 1), 0.99) for k in range(5))      # utils.ema_alpha(k, 0.99): 0 (the teacher becomes the student), 1/2, 2/3, ...
SGD_HYPER = tuple((mu, wd, gs) for mu in (0.0, 0.9) for wd in (0.0, 5e-4) for gs in (1.0, 0.5, 1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def sgd_case(n, seed=7):
    """Weights, momentum buffer, teacher and five gradients of n elements for the SGD / EMA tests.  Computed once; read-only."""
    r = np.random.RandomState(seed + n % 1000)
    c = dict(p0=r.randn(n).astype(F32), mom0=(0.3 * r.randn(n)).astype(F32), t0=r.randn(n).astype(F32), g=r.randn(len(SGD_LRS), n).astype(F32))
    for a in c.values():
        a.setflags(write=False)
    return c


def sgd_f64_tolerances(p64, buf64, t64, g, wd, gscale, steps=len(SGD_LRS)):
    """Bounds on |float32 restatement - float64 torch.optim.SGD| after `steps` steps, from the operation count (u = 2^-24, one rounding):
    with B >= |g gscale| + wd |w| + |buf| and P >= |w|, M >= |t| + |w| over the trajectory (taken at its end with a factor 2 of slack),
      buf: five roundings a step (g*gscale, wd*w, their sum, momentum*buf, the sum), each of a value <= B, and the inherited error
           momentum * e_buf + wd * e_p <= e_buf + (negligible)                              -> e_buf <= steps * 6 u B
      p:   lr*buf and the difference round once each (<= u lr B, u P), plus lr * e_buf       -> e_p  <= steps * (u P + lr (u B + e_buf))
      t:   1 - a in float32 (error u, times |w|), two products and a sum (<= u M each), (1 - a) e_p  -> e_t <= steps * (4 u M + e_p)."""
    u = 2.0 ** -24
    B = 2.0 * float(np.abs(g).max() * abs(gscale) + wd * np.abs(p64).max() + (np.abs(buf64).max() if buf64 is not None else 0.0))
    P, M = 2.0 * float(np.abs(p64).max()), 2.0 * float(np.abs(t64).max() + np.abs(p64).max())
    e_buf = steps * 6 * u * B
    e_p = steps * (u * P + max(SGD_LRS) * (u * B + e_buf))
    return e_p, e_buf, steps * (4 * u * M + e_p)


ADAMW_MUTATIONS = ("t_off_by_one", "no_sqrt_on_bc2", "eps_inside_root", "coupled_decay")
ADAMW_CHECKED = (1, 2, 3, 10, 40)
ADAMW_HP = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, grad_scale=0.5)


def adamw_f32(p, g_steps, m, v, lrs, step0=0, betas=(0.9, 0.999), eps=1e-8, wd=0.05, gscale=0.5, mutation=None, checked=None):
    """adamw_kernel in numpy float32 (the kernel's operation order; the kernel may contract a product into the following sum, this does
    not).  mutation: one of ADAMW_MUTATIONS -- the mistakes the AdamW tolerance has to tell from rounding.  -> {step count: (p, m, v)} for
    the counts in `checked` (default: the last one), counted from step0 + 1."""
    assert mutation is None or mutation in ADAMW_MUTATIONS, mutation
    p, m, v = (np.array(a, dtype=F32) for a in (p, m, v))
    b1, b2, eps, wd, gs, one = F32(betas[0]), F32(betas[1]), F32(eps), F32(wd), F32(gscale), F32(1)
    omb1, omb2 = F32(1.0 - betas[0]), F32(1.0 - betas[1])      # formed in double, then rounded (as the bias corrections below)
    out = {}
    for k, lr in enumerate(lrs):
        lr = F32(lr)
        t = step0 + k + 1
        if mutation == "t_off_by_one":
            t = t + 1
        bc1 = F32(1.0 - float(betas[0]) ** t)
        bc2 = 1.0 - float(betas[1]) ** t
        bc2s = F32(bc2) if mutation == "no_sqrt_on_bc2" else F32(np.sqrt(bc2))
        step_size, decay = lr / bc1, one - lr * wd
        gi = np.asarray(g_steps[k], dtype=F32) * gs
        w = p * decay
        if mutation == "coupled_decay":
            gi, w = gi + wd * p, p
        m = b1 * m + omb1 * gi
        v = b2 * v + omb2 * gi * gi
        den = np.sqrt(v / (bc2s * bc2s) + eps) if mutation == "eps_inside_root" else np.sqrt(v) / bc2s + eps
        p = w - step_size * m / den
        assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32 and np.asarray(bc1).dtype == F32
        if checked is None or step0 + k + 1 in checked:
            out[step0 + k + 1] = (p.copy(), m.copy(), v.copy())
    if checked is None:
        out = {step0 + len(lrs): out[step0 + len(lrs)]}
    return out


def adamw_torch(p, g_steps, lrs, dtype, betas=(0.9, 0.999), eps=1e-8, wd=0.05, gscale=0.5, checked=ADAMW_CHECKED):
    """torch.optim.AdamW on CPU tensors of `dtype` from zero moments, gradient pre-multiplied by gscale.  -> {step count: (p, m, v)} numpy."""
    w = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    opt = torch.optim.AdamW([w], lr=1.0, betas=betas, eps=eps, weight_decay=wd)
    out = {}
    for k, lr in enumerate(lrs):
        opt.param_groups[0]["lr"] = float(lr)
        w.grad = torch.tensor(np.asarray(g_steps[k]), dtype=dtype) * gscale
        opt.step()
        if k + 1 in checked:
            s = opt.state[w]
            out[k + 1] = (w.detach().numpy().copy(), s["exp_avg"].numpy().copy(), s["exp_avg_sq"].numpy().copy())
    return out


def cosine_warmup_lrs(steps, base_lr=1e-2):
    """The learning rates the project's CosineWarmupLR_Scheduler hands an optimizer over `steps` iterations: a quarter of them warm-up (after the
    reference's first-step quirk: the table's LAST entry), then the cosine; every step has another value."""
    from hpfg_amd.utils import CosineWarmupLR_Scheduler
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=base_lr)
    sched = CosineWarmupLR_Scheduler(opt, warmup_epochs=1, warmup_lr=1e-4, num_epochs=4, base_lr=base_lr, final_lr=1e-5, iter_per_epoch=steps // 4)
    lrs = []
    for _ in range(steps):
        lrs.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
    return lrs


@functools.lru_cache(maxsize=None)
def adamw_case(n=N_SMALL, steps=40, seed=2024):
    """The AdamW trajectory of the host and the GPU test: weights, per-step gradients whose per-element magnitudes are spread over
    10^U(-8, 0) (elements near eps = 1e-8 pin where eps sits, large ones the bias corrections), the scheduler's learning rates, and for every
    step in ADAMW_CHECKED torch.optim.AdamW in float64 (the reference), in float32, and the tolerance
    tol[step][i] = 8 * max|float32 - float64| for i = p, m, v.  Computed once; treat as read-only."""
    r = np.random.RandomState(seed)
    p0 = r.randn(n).astype(F32)
    mag = (10.0 ** r.uniform(-8.0, 0.0, n))
    g = (mag[None, :] * r.randn(steps, n)).astype(F32)
    lrs = cosine_warmup_lrs(steps)
    ref64 = adamw_torch(p0, g, lrs, torch.float64)
    ref32 = adamw_torch(p0, g, lrs, torch.float32)
    ref_err = {s: tuple(float(np.abs(ref32[s][i].astype(np.float64) - ref64[s][i]).max()) for i in range(3)) for s in ref64}
    tol = {s: tuple(8.0 * e for e in ref_err[s]) for s in ref_err}
    for a in (p0, g):
        a.setflags(write=False)
    return dict(p0=p0, g=g, lrs=lrs, ref64=ref64, ref_err=ref_err, tol=tol)


def adamw_errors(got, ref64):
    """{step: (max|dp|, max|dm|, max|dv|)} of {step: (p, m, v)} against the float64 run."""
    return {s: tuple(float(np.abs(np.asarray(got[s][i], dtype=np.float64) - ref64[s][i]).max()) for i in range(3)) for s in got}


def adamw_within(err, tol):
    return all(err[s][i] <= tol[s][i] for s in err for i in range(3))


def blend_f64(a, b, m):
    """a(1 - m) + b m in float64 (cutmix_kernel, mix_samples_kernel) and the issue's elementwise bound 3 * 2^-24 * (|a| + |b|): 1 - m, two
    products and a sum, each rounded once (or a product fused into the sum), every intermediate at most |a| + |b|."""
    a, b, m = (np.asarray(x, dtype=np.float64) for x in (a, b, m))
    return a * (1.0 - m) + b * m, 3.0 * 2.0 ** -24 * (np.abs(a) + np.abs(b))


def softmax_mix_f64(t0, t1, f):
    """softmax(t0, dim 1)(1 - f[s]) + softmax(t1, dim 1) f[s] of [n,C,H,W] logits in float64 (torch, CPU)."""
    w = torch.as_tensor(f, dtype=torch.float64).reshape(-1, 1, 1, 1)
    return torch.softmax(t0.double(), 1) * (1.0 - w) + torch.softmax(t1.double(), 1) * w


# ---- float64 restatements of the virtual sources (csrc/stage.h, csrc/common.h act_load4) and the error bound of the split-bf16 kernels ----
# Plain torch / numpy float64 functions of the raw tensors (NHWC) and the table rows; they call no project kernel.  Each returns the value
# and `delta`, the bound on what the fp32 evaluation of the chain may differ from it (u = 2^-24, one rounding per operation, an FMA or a
# separate multiply and add alike), stated once per kind beside the code.
import torch.nn.functional as F

U24 = 2.0 ** -24
LEAKY32 = f32_exact(0.01)          # HPFG_LEAKY as the float the kernels multiply by


def bn_table(C_, seed):
    """A hand-made BatchNorm table [BN_ROWS][C] (float32): mean, rstd, scale = gamma * rstd, shift = beta - mean * scale, k1 .. k3 random."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(L.BN_ROWS, C_)
    t[L.BN_MEAN] = torch.randn(C_, generator=g) * 0.3
    t[L.BN_RSTD] = torch.rand(C_, generator=g) + 0.5
    gamma = torch.randn(C_, generator=g)
    beta = torch.randn(C_, generator=g) * 0.2
    t[L.BN_SCALE] = gamma * t[L.BN_RSTD]
    t[L.BN_SHIFT] = beta - t[L.BN_MEAN] * t[L.BN_SCALE]
    t[L.BN_K1], t[L.BN_K2], t[L.BN_K3] = torch.randn(3, C_, generator=g) * 0.5
    return t


def lrelu_slope(z64, sc, sh):
    """LeakyReLU'(z * scale + shift) as the kernels decide it in fp32; the inputs must keep every decision clear of the rounding of y."""
    y = z64 * sc + sh
    assert not bool((y.abs() <= 2.0 ** -22 * torch.maximum((z64 * sc).abs(), sh.abs().expand_as(y))).any()), "test input sits on a LeakyReLU tie"
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.01))


def keep_f64(shape, p, seed):
    """keep / (1 - p) of an NHWC tensor of `shape`: oracle.rng_ref.keep_mask_nhwc over element index pix * C + c; p as the float the kernel holds."""
    if p <= 0:
        return torch.ones(shape, dtype=torch.float64)
    n = int(np.prod(shape))
    keep = torch.from_numpy(rng_ref.keep_mask_nhwc(n, p, seed).astype(np.float64)).reshape(shape)
    return keep / (1.0 - f32_exact(p))


def _act64(z, sc, sh):
    """lrelu(z * scale + shift) and the magnitude |z scale| + |shift| its roundings are relative to"""
    z, sc, sh = z.double(), sc.double(), sh.double()
    y = z * sc + sh
    return torch.where(y > 0, y, LEAKY32 * y), (z * sc).abs() + sh.abs()


def bnact_f64(z, sc, sh, p=0.0, seed=0):
    """lrelu(z * scale + shift) * keep / (1 - p).
    delta = 6 u (|z scale| + |shift|) / (1 - p): the product and the sum of y (2), the LeakyReLU product (1), 1 - p, its reciprocal and the
    dropout product (3), each relative to a value of at most that magnitude."""
    a, mag = _act64(z, sc, sh)
    k = keep_f64(a.shape, p, seed)
    return a * k, 6.0 * U24 * mag / (1.0 - f32_exact(p))


def pool_windows(a):
    """[N, 2H, 2W, C] -> [4][N, H, W, C]: the window elements in row-major order (0,0), (0,1), (1,0), (1,1)"""
    return torch.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]])


def pool_f64(z2, sc, sh):
    """max of the four activated values of a 2 x 2 window (no dropout in front of a pool).
    delta = 3 u max over the window of (|z scale| + |shift|): y (2) and the LeakyReLU product (1); a maximum moves by at most what its
    arguments move."""
    a, mag = _act64(z2, sc, sh)
    return pool_windows(a).max(0).values, 3.0 * U24 * pool_windows(mag).max(0).values


def pool_argmax(a, delta=None):
    """index 0 .. 3 of the first maximum of every window of a [N, 2H, 2W, C] in row-major order.  With `delta` (bound on the fp32 rounding of
    a): the top two values of every window must be further apart than both may move -- the arg-max guard of the test inputs."""
    w = pool_windows(a)
    first = torch.full(w.shape[1:], 3, dtype=torch.int64)
    for k in (2, 1, 0):                                  # the lowest index among equal maxima, stated rather than left to argmax
        first = torch.where(w[k] == w.max(0).values, torch.full_like(first, k), first)
    if delta is not None:
        top2 = w.topk(2, dim=0).values
        assert bool(((top2[0] - top2[1]) > 2.0 * pool_windows(delta).max(0).values).all()), "test input sits on a max-pool tie"
    return first


def pool_scatter_f64(dP, first):
    """MaxPool2d(2) backward: dP [N, H, W, C] placed at the arg-max `first` (pool_argmax) of every window -> [N, 2H, 2W, C], zero elsewhere."""
    n, h, w, c = dP.shape
    out = torch.zeros(n, 2 * h, 2 * w, c, dtype=torch.float64)
    for k in range(4):
        out[:, (k >> 1)::2, (k & 1)::2] = torch.where(first == k, dP.double(), torch.zeros((), dtype=torch.float64))
    return out


def up2x_matrix(Lo):
    """(M, E): M = the [2 Lo][Lo] float64 matrix of the align_corners=True bilinear x2 along one axis, its weights formed in float32 by the
    kernels' law: ratio (in - 1) / (out - 1) as a float, times the output index, truncated; w1 = f - i0, w0 = 1 - w1.  E = what the fp32
    rounding of f = ratio * index may do to a row of M: the product rounds once (u f), or not at all where the compiler contracts it into
    f - i0, so a kernel's w1 lies within u f of the law's -- E[o] = u f (e_i1 - e_i0)."""
    m, e = np.zeros((2 * Lo, Lo), dtype=np.float64), np.zeros((2 * Lo, Lo), dtype=np.float64)
    r = F32(Lo - 1) / F32(2 * Lo - 1) if Lo > 1 else F32(0)
    for o in range(2 * Lo):
        f = F32(r * F32(o))
        i0 = int(f)
        i1 = i0 + (1 if i0 < Lo - 1 else 0)
        w1 = F32(f - F32(i0))
        w0 = F32(F32(1) - w1)
        m[o, i0] += float(w0)
        m[o, i1] += float(w1)
        e[o, i0] -= U24 * float(f)
        e[o, i1] += U24 * float(f)
    return torch.from_numpy(m), torch.from_numpy(e)


def up2x_f64(u):
    """bilinear x2 (align_corners=True) of u [N, h, w, C] -> [N, 2h, 2w, C], blended in float64.
    delta = 6 u * (the same blend of |u|) + |E_y u M_x| + |M_y u E_x|: four products, three sums, 1 - w twice share out to under six roundings
    of partial results that the blend of magnitudes bounds; a weight within u f of the law's (up2x_matrix) moves the value by that times the
    difference of the two rows (columns) it blends."""
    (my, ey), (mx, ex) = up2x_matrix(u.shape[1]), up2x_matrix(u.shape[2])
    u = u.double()
    blend = lambda a, t, b: torch.einsum("yi,nijc,xj->nyxc", a, t, b)
    return blend(my, u, mx), 6.0 * U24 * blend(my, u.abs(), mx) + blend(ey, u, mx).abs() + blend(my, u, ex).abs()


def upbwd_f64(g):
    """the transpose of that interpolation applied to a gradient g [N, 2h, 2w, C] -> [N, h, w, C].
    delta = 12 u * (the transpose applied to |g|) + |E_y|^T |g M_x| + |M_y^T g| |E_x|: up to 5 x 5 taps gathered as five horizontal FMAs and one
    vertical FMA per row (the weight of a doubled tap is one more sum); the weights within u f of the law's, each output row (column) on its
    own."""
    (my, ey), (mx, ex) = up2x_matrix(g.shape[1] // 2), up2x_matrix(g.shape[2] // 2)
    g = g.double()
    d = torch.einsum("yi,nyxc,xj->nijc", my, g, mx)
    dw = torch.einsum("yi,nyjc->nijc", ey.abs(), torch.einsum("nyxc,xj->nyjc", g, mx).abs()) + \
        torch.einsum("nixc,xj->nijc", torch.einsum("yi,nyxc->nixc", my, g).abs(), ex.abs())
    return d, 12.0 * U24 * torch.einsum("yi,nyxc,xj->nijc", my, g.abs(), mx) + dw


def cat_f64(z, sc, sh, u):
    """[bnact (no dropout) | up2x] along the channels; delta of each half by its own law."""
    a, da = bnact_f64(z, sc, sh)
    b, db = up2x_f64(u)
    return torch.cat([a, b], -1), torch.cat([da, db], -1)


def dz_f64(z, dA, tab, p=0.0, seed=0):
    """k1 * g + (k2 * z + k3) with g = dA * keep / (1 - p) * slope(z * scale + shift); tab = the table rows [BN_ROWS][C].
    delta = 6 u (|k1 g| + |k2 z| + |k3|): 1 - p, its reciprocal, the dropout and the slope products (4) and k1 * g and the final sum (2) on the
    first term; k2 * z, + k3 and the final sum (3) on the rest."""
    t = tab.double()
    z = z.double()
    slope = torch.where(lrelu_slope(z, t[L.BN_SCALE], t[L.BN_SHIFT]) == 1.0, 1.0, LEAKY32)      # (the float the kernels multiply by)
    g = dA.double() * keep_f64(z.shape, p, seed) * slope
    v = t[L.BN_K1] * g + (t[L.BN_K2] * z + t[L.BN_K3])
    return v, 6.0 * U24 * ((t[L.BN_K1] * g).abs() + (t[L.BN_K2] * z).abs() + t[L.BN_K3].abs())


def materialized_within_delta(got, kind, z, tab, u=None, dA=None, p=0.0, seed=0):
    """hpfg_act_materialize's result `got` (the act_load4 copy of the producer chain, csrc/common.h) against the float64 restatement of that
    kind from the raw CPU tensors, within the kind's delta.  -> largest error / delta; asserts it is at most 1."""
    sc, sh = tab[L.BN_SCALE], tab[L.BN_SHIFT]
    if kind == "plain":
        v, d = z.double(), None
    elif kind == "bnact":
        v, d = bnact_f64(z, sc, sh, p, seed)
    elif kind == "pool":
        v, d = pool_f64(z, sc, sh)
    elif kind == "cat":
        v, d = cat_f64(z, sc, sh, u)
    else:
        v, d = dz_f64(z, dA, tab, p, seed)
    err = (got.detach().cpu().double() - v).abs()
    if d is None:
        assert float(err.max()) == 0.0
        return 0.0
    ratio = float((err / d).max())
    assert ratio <= 1.0, f"hpfg_act_materialize ({kind}) is {ratio:.3g} x delta off the float64 restatement"
    return ratio


# The kernels form hi*hi + hi*lo + lo*hi with hi = bf16(x), lo = bf16(x - hi) and accumulate in fp32.  Per output element, with
# S = sum |a||w| (+ |bias|) over its T terms:
#   3 * 2^-16 * S        each operand is represented to 2^-16 relative (2), the dropped lo*lo term is at most 2^-16 (1)
#   (T + 2) * 2^-24 * S  the fp32 sum
#   sum |w| * delta_a    the fp32 rounding of the source chain, per kind as stated above
def _split_bound(S, T, chain, split=True):
    """split=False: a kernel that forms its products in exact fp32 FMAs -- the fp32 sum and the chain alone"""
    return (3.0 * 2.0 ** -16 * S if split else 0.0) + (T + 2) * U24 * S + chain


def conv_ref_bound(a, da, w, b, split=True):
    """a, da [N,H,W,Cin] float64 (value, delta), w [Cout,Cin,k,k], b [Cout] or None -> (F.conv2d in float64, bound), both [N,H,W,Cout].
    split=False: without the 3 * 2^-16 * S term of the split products (the first layer's kernels: fmaf chains in exact fp32)"""
    pad = w.shape[-1] // 2
    w64, x = w.double(), nchw(a)
    ref = F.conv2d(x, w64, None if b is None else b.double(), padding=pad)
    S = F.conv2d(x.abs(), w64.abs(), None if b is None else b.double().abs(), padding=pad)
    chain = F.conv2d(nchw(da), w64.abs(), None, padding=pad)
    T = w[0].numel() + (0 if b is None else 1)
    return ref.permute(0, 2, 3, 1).contiguous(), _split_bound(S, T, chain, split).permute(0, 2, 3, 1).contiguous()


def dgrad_ref_bound(g, dg, w):
    """g, dg [N,H,W,Cout] float64 -> (float64 autograd of F.conv2d w.r.t. its input, bound), both [N,H,W,Cin]"""
    pad = w.shape[-1] // 2
    w64 = w.double()
    n, h, wd, _ = g.shape
    x = torch.zeros(n, w.shape[1], h, wd, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w64, None, padding=pad).backward(nchw(g))
    S = F.conv_transpose2d(nchw(g).abs(), w64.abs(), padding=pad)
    chain = F.conv_transpose2d(nchw(dg), w64.abs(), padding=pad)
    T = w.shape[0] * w.shape[2] * w.shape[3]
    return x.grad.permute(0, 2, 3, 1).contiguous(), _split_bound(S, T, chain).permute(0, 2, 3, 1).contiguous()


def wgrad_ref_bound(a, da, g, dg, wshape, split=True):
    """a, da [N,H,W,Cin], g, dg [N,H,W,Cout] float64 -> (float64 autograd of F.conv2d w.r.t. its weight, bound), both [Cout,Cin,k,k]; the sum
    runs over the pixels: T = N * H * W, the chain term |a| dg + da |g| + da dg.  split=False: without the 3 * 2^-16 * S term of the split
    products (first_wgrad_kernel multiplies in fp32)"""
    from torch.nn import grad as G
    pad = wshape[-1] // 2
    x = nchw(a)
    wr = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wr, None, padding=pad).backward(nchw(g))
    cw = lambda p_, q_: G.conv2d_weight(nchw(p_), wshape, nchw(q_), padding=pad)
    S = cw(a.abs(), g.abs())
    chain = cw(a.abs(), dg) + cw(da, g.abs()) + cw(da, dg)
    return wr.grad, _split_bound(S, a.shape[0] * a.shape[1] * a.shape[2], chain, split)


def f32_conv_ratio(kind, ref, bound, *args):
    """largest error / bound that torch float32 on the CPU reaches on the same (float64-derived) operands: kind = "conv" (a, w, b),
    "dgrad" (g, w) or "wgrad" (a, g, wshape)"""
    if kind == "conv":
        a, w, b = args
        got = F.conv2d(nchw(a).float(), w.float(), None if b is None else b.float(), padding=w.shape[-1] // 2).permute(0, 2, 3, 1)
    elif kind == "dgrad":
        g, w = args
        x = torch.zeros(g.shape[0], w.shape[1], g.shape[1], g.shape[2], requires_grad=True)
        F.conv2d(x, w.float(), None, padding=w.shape[-1] // 2).backward(nchw(g).float())
        got = x.grad.permute(0, 2, 3, 1)
    else:
        a, g, wshape = args
        wr = torch.zeros(wshape, requires_grad=True)
        F.conv2d(nchw(a).float(), wr, None, padding=wshape[-1] // 2).backward(nchw(g).float())
        got = wr.grad
    return float(((got.double() - ref).abs() / bound).max())


def adhoc_weights(cin, cout, taps, seed):
    """weight [cout, cin, k, k] and bias [cout] (float32, CPU) of AdHocConv(cin, cout, taps, seed=seed)"""
    g = torch.Generator().manual_seed(seed)
    k = 3 if taps == 9 else 1
    return torch.randn(cout, cin, k, k, generator=g) * 0.2, torch.randn(cout, generator=g)


@functools.lru_cache(maxsize=None)
def conv_source(kind, seed, N, H, W, C_, p=0.0, hot=None):
    """One virtual source of a conv at N x H x W with C_ channels, on the CPU: its raw float32 tensors (unit-scale data, hand-made table),
    the float64 restatement `v` and its `delta`.  kind: plain | bnact | pool (raw tensors at 2H x 2W) | cat ([bnact C/2 | up2x C/2], the
    upsampled half at H/2 x W/2) | dz.  hot = (n, y0, x0, A): the raw tensors of the 16 x 16 tile at (y0, x0) of image n are A times as large
    (the walk cases of tests/test_gpu_tile_edges.py).  The LeakyReLU guard of lrelu_slope holds for the seeds in use.  Computed once; read-only."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * 2 + 0.5

    def heat(t, up=1.0):
        if hot is not None:
            n, y0, x0, A = hot
            t[n, int(y0 * up):int((y0 + 16) * up), int(x0 * up):int((x0 + 16) * up)] *= A
        return t

    def untie(z, tab):
        """among millions of elements a few sit on a LeakyReLU tie (the condition of lrelu_slope): those move by 1/4 (none in the small cases)"""
        zs, sh = z.double() * tab[L.BN_SCALE].double(), tab[L.BN_SHIFT].double()
        z[(zs + sh).abs() <= 2.0 ** -22 * torch.maximum(zs.abs(), sh.abs().expand_as(zs))] += 0.25
        return z

    s = dict(kind=kind, C=C_, p=p, dseed=1000 + seed)
    if kind == "plain":
        s["z"] = heat(rn(N, H, W, C_))
        s["v"], s["d"] = s["z"].double(), torch.zeros(N, H, W, C_, dtype=torch.float64)
        return s
    if kind == "dz":
        s["z"], s["dA"], s["tab"] = heat(rn(N, H, W, C_)), heat(torch.randn(N, H, W, C_, generator=g)), bn_table(C_, seed + 11)
        untie(s["z"], s["tab"])
        s["v"], s["d"] = dz_f64(s["z"], s["dA"], s["tab"], p, s["dseed"])
        return s
    ca = C_ // 2 if kind == "cat" else C_
    up = 2 if kind == "pool" else 1
    s["z"], s["tab"] = untie(heat(rn(N, up * H, up * W, ca), up), bn_table(ca, seed + 3)), bn_table(ca, seed + 3)
    sc, sh = s["tab"][L.BN_SCALE], s["tab"][L.BN_SHIFT]
    lrelu_slope(s["z"].double(), sc.double(), sh.double())          # the guard
    if kind == "bnact":
        s["v"], s["d"] = bnact_f64(s["z"], sc, sh, p, s["dseed"])
    elif kind == "pool":
        s["v"], s["d"] = pool_f64(s["z"], sc, sh)
    else:
        s["u"] = heat(rn(N, H // 2, W // 2, C_ - ca), 0.5)
        s["v"], s["d"] = cat_f64(s["z"], sc, sh, s["u"])
    return s


NARROW_OFF, NARROW_ALL = 0, 1 << 20      # HPFG_OPT_NARROW_DEEP: 0 = 64-wide slices wherever they divide, large = 32-wide slices always
# A. forward 3x3 on 4 x 16-pixel tiles: kind, p, N, H, W, cin, cout, HPFG_OPT_NARROW_DEEP (None = its default)
FWD3_CASES = [
    ("bnact", 0.0, 3, 14, 14, 32, 16, None), ("bnact", 0.3, 3, 6, 20, 64, 4, None), ("bnact", 0.3, 3, 10, 34, 40, 32, None),
    ("bnact", 0.0, 3, 14, 14, 256, 64, None), ("bnact", 0.3, 3, 10, 34, 64, 64, NARROW_OFF), ("bnact", 0.0, 3, 6, 20, 32, 64, None),
    ("pool", 0.0, 3, 14, 14, 32, 32, None), ("pool", 0.0, 3, 6, 20, 64, 64, NARROW_OFF), ("pool", 0.0, 3, 10, 34, 40, 16, None),
    ("cat", 0.0, 3, 14, 14, 64, 16, None), ("cat", 0.0, 3, 6, 20, 64, 64, NARROW_OFF), ("cat", 0.0, 3, 10, 34, 64, 32, None),
]
FWD3_PERSISTENT = ("bnact", 0.0, 12, 10, 34, 32, 256, NARROW_ALL)      # 108 tiles on 8 slices of 32 channels: 64 workgroups resident per slice
# B. dgrad 3x3: gradient source kind, p, N, H, W, layer cin (the output channels), layer cout (K), option, epilogue
DGRAD3_CASES = [
    ("dz", 0.0, 3, 14, 14, 16, 32, None, None), ("dz", 0.3, 3, 6, 20, 64, 64, NARROW_OFF, None), ("plain", 0.0, 3, 10, 34, 32, 40, None, None),
    ("dz", 0.3, 3, 10, 34, 4, 32, None, None), ("dz", 0.0, 3, 14, 14, 64, 32, None, "split"), ("dz", 0.3, 3, 10, 34, 64, 64, None, "stats1"),
    ("dz", 0.0, 3, 6, 20, 64, 32, None, "pool"), ("plain", 0.0, 3, 14, 14, 32, 64, None, "pool"),
]
# C. 1x1: forward from a bnact source (kind, p, N, H, W, cin, cout), dgrad from a plain source (N, H, W, cin, cout), UPBWD dgrad at low sizes
FWD1_CASES = [("bnact", 0.3, 3, 14, 14, 64, 32), ("bnact", 0.0, 3, 6, 20, 40, 16), ("bnact", 0.0, 3, 10, 34, 128, 64), ("bnact", 0.3, 2, 16, 32, 32, 64)]
DGRAD1_CASES = [(3, 14, 14, 32, 64), (3, 6, 20, 16, 40), (3, 10, 34, 64, 16), (2, 16, 32, 16, 32)]
UPBWD_CASES = [(3, 1, 1, 64, 32), (3, 7, 7, 128, 64), (3, 14, 9, 16, 8), (3, 5, 6, 32, 40)]      # N, H, W (low size), cin, cout (= channels of the gradient)
# D. stage_out: input kind of a 64 -> 64 layer at 3 x 10 x 34 (two 32-wide output slices in the forward conv and in the dgrad)
STAGE_CASES = [("bnact", 0.3), ("pool", 0.0), ("cat", 0.0)]
# E. weight gradient: input kind, p, gradient kind, p, N, H, W, cin, cout, taps -- pick_shape's (32, 32), (16, 64), (16, 32), (16, 16)
WGRAD_CASES = [
    ("bnact", 0.3, "dz", 0.0, 3, 14, 14, 32, 32, 9), ("pool", 0.0, "dz", 0.3, 3, 10, 34, 16, 64, 9), ("cat", 0.0, "dz", 0.0, 3, 10, 34, 32, 16, 9),
    ("cat", 0.0, "plain", 0.0, 3, 14, 14, 64, 32, 9), ("plain", 0.0, "dz", 0.3, 3, 14, 14, 16, 32, 9), ("plain", 0.0, "plain", 0.0, 2, 16, 32, 16, 16, 9),
    ("bnact", 0.0, "plain", 0.0, 3, 10, 34, 40, 64, 9), ("pool", 0.0, "plain", 0.0, 2, 16, 16, 32, 32, 9),
    ("bnact", 0.3, "plain", 0.0, 3, 14, 14, 64, 32, 1), ("plain", 0.0, "plain", 0.0, 3, 10, 34, 32, 16, 1), ("bnact", 0.0, "plain", 0.0, 2, 16, 32, 16, 16, 1),
]


def case_seed(*case):
    """a fixed seed per case tuple (the guards were checked for these)"""
    return sum((i + 1) * int(round(float(x) * 10)) for i, x in enumerate(case) if isinstance(x, (int, float))) % 9973 + sum(map(ord, str(case[0])))


def pool_epilogue_seed(case):
    """seed of pool_epilogue_source for a DGRAD3_CASES entry (offsets for which the arg-max guard passes)"""
    return case_seed(*case) + (2 if case[0] == "plain" else 1)


@functools.lru_cache(maxsize=None)
def pool_epilogue_source(seed, N, H, W, C_):
    """The layer below a max-pool whose backward rides in a dgrad epilogue (HpfgConvArgs.bwd_stats == 2): a dz-kind source at 2H x 2W (z, table,
    dA = the gradient so far) plus `first`, the arg-max of every window of its activated output -- clear of ties by pool_argmax's guard."""
    s = dict(conv_source("dz", seed, N, 2 * H, 2 * W, C_))
    a, mag = _act64(s["z"], s["tab"][L.BN_SCALE], s["tab"][L.BN_SHIFT])
    s["first"] = pool_argmax(a, 3.0 * U24 * mag)
    return s


# ---- NaN-filled layouts of the kernel-by-kernel conv tests (tests/test_gpu_conv_sources.py, tests/test_gpu_tile_edges.py) ----------------
NAN = float("nan")
PADC, COFF = 12, 4          # raw tensors: channel offset COFF inside a buffer of C + PADC floats per pixel
APAD, AOFF = 20, 8          # the dA tensor of a dz source (aux_pstride differs from pstride)
TPAD, TOFF = 16, 8          # tables: column offset TOFF (bn_coff) inside rows of C + TPAD
OPAD, OOFF = 12, 4          # outputs
O2PAD, O2OFF = 20, 8        # second output (out2)


def wide(t, pad=PADC, coff=COFF, dev="cuda:0"):
    """CPU tensor [..., C] -> (NaN-filled device buffer [..., C + pad] with t at channel offset coff, address of its first interior element)"""
    c = t.shape[-1]
    buf = torch.full(tuple(t.shape[:-1]) + (c + pad,), NAN, device=dev)
    buf[..., coff:coff + c] = t.to(dev)
    return buf, buf.data_ptr() + 4 * coff


def interior(buf, c, coff):
    """(interior [..., c], True when every element around it is still NaN)"""
    mask = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    mask[coff:coff + c] = False
    return buf[..., coff:coff + c], bool(torch.isnan(buf[..., mask]).all())


def layout_acts(kind, C_, H, W, p=0.0, dseed=0, ptr=256):
    """(a0, a1 or None) of a source of `kind` with C_ channels feeding a conv at H x W in the layout of device_source: every field but the
    addresses, which are `ptr` (enough for the host-side grid queries hpfg_conv_stat_rows / hpfg_fused_bwd_grid)"""
    ca = C_ // 2 if kind == "cat" else C_
    up = 2 if kind == "pool" else 1
    a = L.Act()
    a.z, a.C, a.Hs, a.Ws, a.pstride = ptr, ca, up * H, up * W, ca + PADC
    if kind == "plain":
        a.mode = L.ACT_PLAIN
        return a, None
    a.bn, a.bn_stride, a.bn_coff = ptr, ca + TPAD, TOFF
    a.drop_p, a.drop_seed = p, dseed
    a.mode = {"bnact": L.ACT_BNACT, "pool": L.ACT_BNACT_POOL, "cat": L.ACT_BNACT, "dz": L.ACT_DZ}[kind]
    a1 = None
    if kind == "dz":
        a.aux, a.aux_pstride = ptr, ca + APAD
    if kind == "cat":
        a1 = L.Act()
        a1.z, a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = ptr, L.ACT_UP2X, C_ - ca, H // 2, W // 2, C_ - ca + PADC
    return a, a1


def device_source(s, H, W, dev="cuda:0"):
    """conv_source dict -> (a0, a1 or None, tensors to keep alive) on the device, every tensor and table inside a wider NaN-filled one"""
    kind, C_, keep = s["kind"], s["C"], []
    a = L.Act()
    zb, a.z = wide(s["z"], dev=dev)
    keep.append(zb)
    ca = s["z"].shape[-1]
    a.C, a.Hs, a.Ws, a.pstride = ca, s["z"].shape[1], s["z"].shape[2], ca + PADC
    if kind == "plain":
        a.mode = L.ACT_PLAIN
        return a, None, keep
    tb = torch.full((L.BN_ROWS, ca + TPAD), NAN, device=dev)
    tb[:, TOFF:TOFF + ca] = s["tab"].to(dev)
    keep.append(tb)
    a.bn, a.bn_stride, a.bn_coff = L.ptr(tb), ca + TPAD, TOFF
    a.drop_p, a.drop_seed = s["p"], s["dseed"]
    a.mode = {"bnact": L.ACT_BNACT, "pool": L.ACT_BNACT_POOL, "cat": L.ACT_BNACT, "dz": L.ACT_DZ}[kind]
    a1 = None
    if kind == "dz":
        ab, a.aux = wide(s["dA"], APAD, AOFF, dev)
        a.aux_pstride = ca + APAD
        keep.append(ab)
    if kind == "cat":
        a1 = L.Act()
        ub, a1.z = wide(s["u"], dev=dev)
        keep.append(ub)
        a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = L.ACT_UP2X, C_ - ca, s["u"].shape[1], s["u"].shape[2], C_ - ca + PADC
    return a, a1, keep


def as_strided_act(a):
    """a PLAIN source over [N, Hs, Ws, pstride] read through strides instead (what the engine does when C % 4 != 0: per-lane loads)"""
    a.mode = L.ACT_STRIDED
    a.sn, a.sc, a.sy, a.sx = a.Hs * a.Ws * a.pstride, 1, a.Ws * a.pstride, a.pstride
    return a


# ---- the whole-tile kernels (tests/test_gpu_tile_edges.py): conv_thin_kernel, fused_bwd_kernel, first_wgrad_kernel -----------------------
# Tile-count edges, per instantiation: one 16 x 16 tile (seven of the eight workgroups own none), fewer tiles than workgroups with
# tiles_x != tiles_y, and the walk case -- more tiles than the launch has workgroups, so the tile loop of a workgroup runs two or three times
# (prefetch of the next tile, the drain of the last, sums and weight-gradient accumulators carried across tiles).
TILE_EDGES = {"one": (1, 16, 16), "few": (1, 32, 48)}
WALK_HW = (96, 160)                       # 6 x 10 tiles an image
SWEEP = (2, 32, 48)                       # the channel / dropout sweeps: 12 tiles on 16 workgroups, some with two tiles, some with none
HOT = (32, 48, 8.0)                       # walk cases: the tile at (y0, x0) of the middle image carries 8 x the amplitude (see walk_hot)
OLD_KERNEL = 0x4000                       # any flag bit in `math` keeps a launch on the chunked conv_bf16x3_kernel


def walk_hot(edge, N):
    """The weight-gradient bound grows with (N H W + 2) * 2^-24 * sum|a||g| -- at the 140 to 200 thousand pixels a walk needs, a missing tile
    of unit-scale data (256 pixels) is far inside it.  One interior tile of the walk cases therefore carries 8 x the amplitude in both
    operands (64 x in the products), which puts a weight gradient without that tile outside the bound (tests/test_host_logic.py)."""
    return (N // 2,) + HOT if edge == "walk" else None


def walk_conditions(nwork, rows, tiles_x, tiles_y, wgs):
    """the tile loop of a workgroup runs at least twice (three times with one workgroup per CU), unevenly, on a non-square grid of tiles"""
    return 0 < rows < nwork and -(-nwork // rows) >= (3 if wgs == 1 else 2) and nwork % rows != 0 and tiles_x != tiles_y


# conv_thin_kernel<CI, CO, kind>: source kind -> (layer cin, layer cout of the edge cases, workgroups per CU, images of the walk case)
THIN_INST = {"bnact": (16, 16, 3, 13), "pool": (16, 32, 1, 9), "cat": (32, 16, 2, 10), "dz": (64, 32, 1, 9)}
# thin case: source kind, p, N, H, W, layer cin, layer cout, edge.  kind dz = the dgrad of the 64 -> 32 layer (source of 32 channels, 64 out)
THIN_CASES = ([("bnact", p, *SWEEP, 16, co, "") for co in (4, 8, 12, 16) for p in (0.0, 0.3)] +
              [("pool", 0.0, *SWEEP, 16, co, "") for co in (20, 24, 32)] + [("cat", 0.0, *SWEEP, 32, co, "") for co in (4, 16)] +
              [("dz", p, *SWEEP, 64, 32, "") for p in (0.0, 0.3)] +
              [(k, 0.0, *TILE_EDGES[e], ci, co, e) for k, (ci, co, _, _) in THIN_INST.items() for e in TILE_EDGES] +
              [(k, 0.0, n, *WALK_HW, ci, co, "walk") for k, (ci, co, _, n) in THIN_INST.items()])
# fused_bwd_kernel<CI, CO, input kind, dZ kind>: name -> (input kind, dZ kind, cin, cout of the edge cases, workgroups per CU, images of the
# walk case); `first` = the first layer's weight-gradient-only form (NODG) on an RGB input read through its strides
FUSED_INST = {"bnact_dz": ("bnact", "dz", 16, 16, 2, 10), "bnact_plain": ("bnact", "plain", 16, 4, 2, 10), "pool_dz": ("pool", "dz", 16, 32, 1, 9),
              "bnact32_dz": ("bnact", "dz", 32, 32, 1, 9), "cat_dz": ("cat", "dz", 32, 16, 1, 9), "first": ("plain", "dz", 3, 16, 2, 10)}
# fused case: input kind, p_in, dZ kind, p_out, N, H, W, cin, cout, out_split, edge
FUSED_CASES = ([("bnact", pi, "dz", po, *SWEEP, 16, 16, 0, "") for pi, po in ((0.0, 0.0), (0.3, 0.0), (0.0, 0.3), (0.3, 0.3))] +
               [("bnact", 0.0, "dz", 0.0, *SWEEP, 16, 8, 0, "")] +
               [("bnact", 0.0, "plain", 0.0, *SWEEP, 16, co, 0, "") for co in (2, 3, 4, 5, 9, 13, 16)] +
               [("pool", 0.0, "dz", 0.3, *SWEEP, 16, co, 0, "") for co in (24, 32)] + [("bnact", 0.3, "dz", 0.0, *SWEEP, 32, co, 0, "") for co in (24, 32)] +
               [("cat", 0.0, "dz", 0.0, *SWEEP, 32, 8, 16, ""), ("cat", 0.0, "dz", 0.3, *SWEEP, 32, 16, 16, ""), ("cat", 0.0, "dz", 0.0, *SWEEP, 32, 16, 0, "")] +
               [(ak, 0.0, gk, 0.0, *TILE_EDGES[e], ci, co, 16 if ak == "cat" else 0, e) for ak, gk, ci, co, _, _ in FUSED_INST.values() for e in TILE_EDGES] +
               [(ak, 0.0, gk, 0.0, n, *WALK_HW, ci, co, 16 if ak == "cat" else 0, "walk") for ak, gk, ci, co, _, n in FUSED_INST.values()])
# first_wgrad_kernel and the tile form it replaces: N, H, W, cin, p, layout of the STRIDED input (nchw | crop | nhwc3), HPFG_OPT_FIRST_WGRAD.
# W = 64: one live load of the four a thread requests; W = 512: the parked rows exactly; N H = 784 > 768 rows: the work-item loop runs twice
FIRST_LAYOUTS = ("nchw", "crop", "nhwc3")
FIRST_CASES = ([(n, 16, w, 1, p, lay, st) for n, w in ((2, 64), (2, 80), (2, 272), (2, 512), (49, 64)) for p in (0.0, 0.05) for lay in FIRST_LAYOUTS
                for st in (1, 0)] + [(2, 16, 80, 3, 0.05, "nchw", 1)])      # (RGB: the tile form whatever the option says)
# the partial-quad contract of PLAIN sources ("channels >= C read as zero"): C, layout (tail: tight [N,H,W,C] with NaN behind the last pixel
# inside the allocation | wide: NaN between the pixels)
QUAD_C = (2, 3, 5, 9, 13)
QUAD_LAYOUTS = ("tail", "wide")
QUAD_FUSED = [("bnact", 0.0, "plain", 0.0, *SWEEP, 16, c, 0, "") for c in QUAD_C]                 # out_conv through hpfg_fused_bwd (cases of FUSED_CASES)
QUAD_DGRAD = [("plain", 0.0, 3, 10, 34, 16, c, None, None) for c in QUAD_C]                       # ... and through the chunked kernels at a size that is
QUAD_WGRAD = [("bnact", 0.0, "plain", 0.0, 3, 10, 34, 16, c, 9) for c in QUAD_C]                  # not 16-aligned (the layouts of DGRAD3_CASES / WGRAD_CASES)


@functools.lru_cache(maxsize=None)
def thin_case(case):
    """CPU data of a THIN_CASES entry: source, weights, float64 reference and bound of the output, the ratio torch float32 reaches.  Read-only."""
    kind, p, N, H, W, cin, cout, edge = case
    seed = case_seed(*case)
    w, b = adhoc_weights(cin, cout, 9, seed)
    if kind == "dz":
        s = conv_source("dz", seed, N, H, W, cout, p, walk_hot(edge, N))
        ref, bound = dgrad_ref_bound(s["v"], s["d"], w)
        f32 = f32_conv_ratio("dgrad", ref, bound, s["v"], w)
    else:
        s = conv_source(kind, seed, N, H, W, cin, p, walk_hot(edge, N))
        ref, bound = conv_ref_bound(s["v"], s["d"], w, b)
        f32 = f32_conv_ratio("conv", ref, bound, s["v"], w, b)
    return dict(s=s, w=w, b=b, ref=ref, bound=bound, f32=f32, seed=seed)


@functools.lru_cache(maxsize=None)
def fused_case(case):
    """CPU data of a FUSED_CASES entry: layer input sa, dZ source sg, weights, (reference, bound, torch-float32 ratio) of dX (None for the
    first layer, which has none) and of dW.  Read-only."""
    ak, p_in, gk, p_out, N, H, W, cin, cout, split, edge = case
    seed = case_seed(*case)
    hot = walk_hot(edge, N)
    sa, sg = conv_source(ak, seed, N, H, W, cin, p_in, hot), conv_source(gk, seed + 1, N, H, W, cout, p_out, hot)
    w, _ = adhoc_weights(cin, cout, 9, seed)
    out = dict(sa=sa, sg=sg, w=w, seed=seed, dx=None)
    if cin >= 16:
        ref, bound = dgrad_ref_bound(sg["v"], sg["d"], w)
        out["dx"] = (ref, bound, f32_conv_ratio("dgrad", ref, bound, sg["v"], w))
    ref, bound = wgrad_ref_bound(sa["v"], sa["d"], sg["v"], sg["d"], w.shape)
    out["dw"] = (ref, bound, f32_conv_ratio("wgrad", ref, bound, sa["v"], sg["v"], w.shape))
    return out


@functools.lru_cache(maxsize=None)
def first_case(N, H, W, cin, p):
    """CPU data of the FIRST_CASES entries at one shape and dropout rate: the network input x (a plain source), the dZ source of the 16
    output channels, the float64 weight gradient, its bound without the split term (the streaming kernel: exact fp32 products) and with it
    (the tile form), the torch-float32 ratio against the former.  Read-only."""
    seed = case_seed("first", N, H, W, cin, p)
    sx, sg = conv_source("plain", seed, N, H, W, cin), conv_source("dz", seed + 1, N, H, W, 16, p)
    shape = (16, cin, 3, 3)
    ref, b_stream = wgrad_ref_bound(sx["v"], sx["d"], sg["v"], sg["d"], shape, split=False)
    _, b_tile = wgrad_ref_bound(sx["v"], sx["d"], sg["v"], sg["d"], shape)
    return dict(sx=sx, sg=sg, ref=ref, b_stream=b_stream, b_tile=b_tile, f32=f32_conv_ratio("wgrad", ref, b_stream, sx["v"], sg["v"], shape), seed=seed)


def fwd_sums_ratio(part64, out):
    """rows of (sum z, sum z^2), summed in float64 -> part64 [2][C], against the float64 sums of the launch's own read-back output [.., C]: the
    fp32 summation bound of tests/test_gpu_bn_acc.py::_fwd_sums_check, (n + 2) * 2^-24 * sum|term|.  -> largest error / bound"""
    z = out.detach().cpu().double().reshape(-1, out.shape[-1])
    n = z.shape[0]
    worst = 0.0
    for which, term in enumerate((z, z * z)):
        worst = max(worst, float(((part64[which] - term.sum(0)).abs() / ((n + 2) * U24 * term.abs().sum(0))).max()))
    return worst


def bwd_sums_ratio(part64, g64, z64, tab):
    """rows of (sum g, sum g xhat), summed in float64 -> part64 [2][C], against float64 sums of g64, z64 [n][C]: the bound of
    tests/test_gpu_bn_acc.py::_bwd_sums_check -- (n + 2) * 2^-24 * sum|g| and (n + 4) * 2^-24 * rstd * (sum|g z| + |mean| sum|g|), the epilogues
    form rstd * (sum g z - mean * sum g) in fp32.  -> largest error / bound"""
    n = g64.shape[0]
    mean, rstd = tab[L.BN_MEAN].double(), tab[L.BN_RSTD].double()
    r1 = (part64[0] - g64.sum(0)).abs() / ((n + 2) * U24 * g64.abs().sum(0))
    r2 = (part64[1] - (g64 * ((z64 - mean) * rstd)).sum(0)).abs() / ((n + 4) * U24 * rstd * ((g64 * z64).abs().sum(0) + mean.abs() * g64.abs().sum(0)))
    return max(float(r1.max()), float(r2.max()))


def thin_args(case, math=L.MATH_BF16X3):
    """HpfgConvArgs of a THIN_CASES entry in the layout of tests/test_gpu_tile_edges.py, dummy addresses: for hpfg_conv_stat_rows on the host"""
    kind, p, N, H, W, cin, cout, _ = case
    dgrad = kind == "dz"
    ca = L.ConvArgs()
    a0, a1 = layout_acts(kind, cout if dgrad else cin, H, W, p)
    ca.a0, ca.a1 = a0, (a1 if a1 is not None else L.Act())
    oc = cin if dgrad else cout
    ca.wpk, ca.out, ca.math, ca.taps, ca.N, ca.H, ca.W = 256, 256, math, 9, N, H, W
    ca.Cout, ca.CoutPad, ca.out_pstride = oc, pad16(oc), oc + OPAD
    if not dgrad:
        ca.bias = ca.stat_partials = 256
    return ca


def fused_args(case):
    """HpfgFusedBwdArgs of a FUSED_CASES entry in the layout of tests/test_gpu_tile_edges.py, dummy addresses: for hpfg_fused_bwd_grid on the
    host (the grid does not depend on bwd_stats)"""
    ak, p_in, gk, p_out, N, H, W, cin, cout, split, _ = case
    fa = L.FusedBwdArgs()
    xa0, xa1 = layout_acts(ak, cin, H, W, p_in)
    if cin < 16:        # the network input: NCHW through its strides
        xa0.mode, xa0.sn, xa0.sc, xa0.sy, xa0.sx = L.ACT_STRIDED, cin * H * W, H * W, W, 1
    g, _ = layout_acts(gk, cout, H, W, p_out)
    if gk == "plain" and cout % 4:
        as_strided_act(g)
    fa.xa0, fa.xa1 = xa0, (xa1 if xa1 is not None else L.Act())
    fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = cin, pad16(cin), cout, pad16(cout)
    d = fa.d
    d.a0, d.math, d.Cout, d.CoutPad, d.N, d.H, d.W, d.taps = g, L.MATH_BF16X3, cin, pad16(cin), N, H, W, 9
    if cin >= 16:
        d.out, d.wpk = 256, 256
        d.out_pstride = (split or cin) + OPAD
        if split:
            d.out2, d.out_split, d.out2_pstride = 256, split, cin - split + O2PAD
    fa.slab = 256
    return fa


# ---- canaries around device outputs (tests/test_gpu_optim.py, tests/test_gpu_tokens_edges.py) -----------------------------------------
PAD = 67                         # elements allocated past n: no launch may touch them
NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: x != x, so only a comparison of the bits shows that it was left alone


def padded(a, n_fill=None, dev="cuda:0"):
    """Device buffer of len(a) + PAD floats: `a`, then (from n_fill on, default len(a)) the NaN pattern."""
    t = torch.full((len(a) + PAD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    k = len(a) if n_fill is None else n_fill
    t[:k] = torch.tensor(np.asarray(a[:k])).to(dev)          # (a copy: the shared inputs are read-only arrays)
    return t


def bits_kept(t, start):
    return bool((t[start:].view(torch.int32) == NAN_BITS).all())


def canary_out(n, dev="cuda:0"):
    """n + PAD floats, all of them the NaN pattern: an output buffer a launch has to fill up to n and leave alone behind n."""
    return torch.full((n + PAD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def canary_ok(t, n):
    """(every one of the first n floats was written, the tail kept its bits)"""
    return not bool((t[:n].view(torch.int32) == NAN_BITS).any()), bits_kept(t, n)


# ---- float64 laws of the token-layout kernels (csrc/tokens.hip; reference model/segformer.py, model/swinunet.py) -----------------------
# Plain restatements of the operations' definitions on torch double tensors, NHWC / [rows, C] like the kernels' buffers.
# tests/test_tokens_laws_host.py holds each against torch's own float64 op and autograd.
def chan_affine(shape, seed, gen=None):
    """N(0,1) values with a per-channel (last axis) scale in [0.25, 4] and offset in [-3, 3]: float32."""
    g = gen or torch.Generator().manual_seed(seed)
    C_ = shape[-1]
    sc = 0.25 * 16.0 ** torch.rand(C_, generator=g)
    off = 6.0 * torch.rand(C_, generator=g) - 3.0
    return (torch.randn(*shape, generator=g) * sc + off).float()


def bound_8x(ref64, t32, margin=8.0):
    """The tolerance rule of the float64 tests: `margin` x the largest error torch's own float32 CPU result `t32` makes against the float64
    law, and no less than 4 units in the last place (float32) of the largest magnitude of the law."""
    ref64 = ref64.double()
    err32 = float((t32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    top = float(ref64.abs().max()) if ref64.numel() else 0.0
    return max(margin * err32, 4.0 * float(np.spacing(np.float32(top))))


def ln_f64(x, g, b, eps=1e-5):
    """nn.LayerNorm over the last axis -> (y, mean, rstd)."""
    x, g, b = x.double(), g.double(), b.double()
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[..., None]) * rstd[..., None] * g + b, mean, rstd


def ln_bwd_f64(x, dy, g, eps=1e-5):
    """-> (dx, dgamma, dbeta) of ln_f64."""
    x, dy, g = x.double(), dy.double(), g.double()
    _, mean, rstd = ln_f64(x, g, torch.zeros_like(g), eps)
    xh = (x - mean[..., None]) * rstd[..., None]
    dg = dy * g
    dx = rstd[..., None] * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    return dx, flat(dy * xh).sum(0), flat(dy).sum(0)


def gelu_f64(u):
    u = u.double()
    return 0.5 * u * (1.0 + torch.special.erf(u / np.sqrt(2.0)))


def gelu_grad_f64(u):
    u = u.double()
    return 0.5 * (1.0 + torch.special.erf(u / np.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / np.sqrt(2.0 * np.pi)


def _shift3(t, dy_, dx_):
    """t[b, y + dy_, x + dx_, c] with zeros outside, NHWC."""
    B, H, W, C_ = t.shape
    p = torch.zeros(B, H + 2, W + 2, C_, dtype=t.dtype)
    p[:, 1:H + 1, 1:W + 1] = t
    return p[:, 1 + dy_:1 + dy_ + H, 1 + dx_:1 + dx_ + W]


def dwconv_f64(x, w9, bias):
    """Depthwise 3 x 3 cross-correlation, padding 1, NHWC x [B,H,W,C], w9 [9][C] (tap t = 3 (dy + 1) + dx + 1) -> pre-activation u."""
    x, w9, bias = x.double(), w9.double(), bias.double()
    u = bias.expand_as(x).clone()
    for t in range(9):
        u += w9[t] * _shift3(x, t // 3 - 1, t % 3 - 1)
    return u


def dwgelu_bwd_f64(x, w9, bias, dy):
    """-> (du, dx, dw9 [9][C], dbias) of gelu(dwconv_f64)."""
    x, w9, dy = x.double(), w9.double(), dy.double()
    du = dy * gelu_grad_f64(dwconv_f64(x, w9, bias))
    dx = torch.zeros_like(x)
    dw9 = torch.zeros_like(w9)
    for t in range(9):
        dx += w9[t] * _shift3(du, -(t // 3 - 1), -(t % 3 - 1))
        dw9[t] = (du * _shift3(x, t // 3 - 1, t % 3 - 1)).sum((0, 1, 2))
    return du, dx, dw9, du.sum((0, 1, 2))


def bilinear_matrix(n_in, n_out):
    """[n_out, n_in] float64 weights of F.interpolate(mode="bilinear", align_corners=False) along one axis: output o reads the source
    coordinate max(0, (o + 0.5) n_in / n_out - 0.5), its floor i0 and min(i0 + 1, n_in - 1)."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        s = max(0.0, (o + 0.5) * n_in / n_out - 0.5)
        i0 = min(int(np.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        m[o, i0] += 1.0 - (s - i0)
        m[o, i1] += s - i0
    return m


def resize_f64(x, H, W):
    """NHWC x [B,h,w,C] -> [B,H,W,C]."""
    t = torch.einsum("Yy,byxc->bYxc", bilinear_matrix(x.shape[1], H), x.double())          # (one axis at a time: two plain matrix products)
    return torch.einsum("Xx,bYxc->bYXc", bilinear_matrix(x.shape[2], W), t)


def resize_bwd_f64(dy, h, w):
    """The transpose of resize_f64: NHWC dy [B,H,W,C] -> [B,h,w,C]."""
    t = torch.einsum("Yy,bYXc->byXc", bilinear_matrix(h, dy.shape[1]), dy.double())
    return torch.einsum("Xx,byXc->byxc", bilinear_matrix(w, dy.shape[2]), t)


def col_stats_f64(x):
    """x [R, C] -> (sum_r x, sum_r (x - mean)^2)."""
    x = x.double()
    return x.sum(0), ((x - x.mean(0)) ** 2).sum(0)


def _row_mask(mask, inv_keep, rows_per_image, R, C_):
    if mask is None:
        return torch.ones(R, C_, dtype=torch.float64)
    return mask.double()[torch.arange(R) // rows_per_image] * float(np.float32(inv_keep))


def bnrelu_f64(x, mean, rstd, gamma, beta, mask=None, inv_keep=1.0, rows_per_image=1):
    """relu((x - mean) rstd gamma + beta) mask[row // rows_per_image] inv_keep on x [R, C] -> (y, pre-activation)."""
    x = x.double()
    pre = (x - mean.double()) * rstd.double() * gamma.double() + beta.double()
    return torch.relu(pre) * _row_mask(mask, inv_keep, rows_per_image, *x.shape), pre


def bnrelu_bwd_f64(x, dy, mean, rstd, gamma, beta, mask=None, inv_keep=1.0, rows_per_image=1):
    """-> (dx, sum g (= dbeta), sum g xhat (= dgamma)) with g = dy mask inv_keep [pre > 0]: train-mode BatchNorm's input gradient."""
    x = x.double()
    R = x.shape[0]
    xh = (x - mean.double()) * rstd.double()
    g = torch.where(xh * gamma.double() + beta.double() > 0, dy.double() * _row_mask(mask, inv_keep, rows_per_image, *x.shape), 0.0)
    s1, s2 = g.sum(0), (g * xh).sum(0)
    return gamma.double() * rstd.double() * (g - s1 / R - xh * s2 / R), s1, s2


def patches_f64(x, k, s):
    """im2col of a conv with kernel k, stride s, padding k // 2 over NHWC x -> [B, Ho*Wo, k*k*C], patch order (u, v, c); keeps x's dtype
    (pure data movement)."""
    B, H, W, C_ = x.shape
    cols = torch.nn.functional.unfold(x.permute(0, 3, 1, 2), k, padding=k // 2, stride=s)          # [B, C*k*k, L], channel-major
    L_ = cols.shape[-1]
    return cols.reshape(B, C_, k * k, L_).permute(0, 3, 2, 1).reshape(B, L_, k * k * C_)


def col2im_f64(dcols, H, W, C_, k, s):
    """The transpose of patches_f64: [B, Ho*Wo, k*k*C] -> NHWC [B,H,W,C] in float64."""
    B, L_, _ = dcols.shape
    t = dcols.double().reshape(B, L_, k * k, C_).permute(0, 3, 2, 1).reshape(B, C_ * k * k, L_)
    return torch.nn.functional.fold(t, (H, W), k, padding=k // 2, stride=s).permute(0, 2, 3, 1)


def patch_merge_ref(x):
    """Swin's PatchMerging gather on NHWC x: the four 2 x 2 neighbours concatenated along C (same dtype: data movement)."""
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)


# ---- float64 law of the fused loss (csrc/loss.hip) and of the entropy mask (csrc/misc.hip) ------------------------------------------------
# Written from the definitions in the header comment of csrc/loss.hip (CrossEntropyLoss(ignore_index=255), the batch-wide Dice of
# utils/loss/diceloss.py:155-191, the softmax MSE of main.py:191 and UAMT's masked form :160-164), on NHWC tensors like the kernels' buffers.
# tests/test_loss_laws_host.py holds it against oracle.losses_ref, F.cross_entropy and the reference's stored outputs.
LOSS_OFF = 8                     # first Dice slot of `sums`
LOSS_SMOOTH = 1e-5
LOSS_K = (0.5, 0.5, 0.2, 0.7, 0.3)            # ce0, dice0, ce1, dice1, mse_w
LOSS_K_DEAD = (0.5, 0.5, 0.0, 0.0, 0.3)       # group 1's supervised terms switched off: they must contribute nothing
LOSS_SHAPES = ((3, 1, 24, 24), (2, 2, 40, 28))          # (N, n_lab, H, W)
LOSS_MUTATIONS = ("ce_over_all_pixels", "z_skips_ignored", "dice_mean_over_c_minus_1", "masked_mse_without_2", "mse_count_without_c")
LOSS_SUM_GROUPS = ("nll", "cnt", "mse", "mask", "I", "Z", "Y")


def loss_stride(C_):
    """class slots per I / Z / Y block of `sums`"""
    return 4 if C_ <= 4 else 16


def loss_nsum(C_):
    return LOSS_OFF + 6 * loss_stride(C_)


def loss_sum_groups(C_):
    """{name: indices into `sums`} of the entries that share a magnitude: nll and cnt of both label groups, the MSE and the mask sum, and the
    I, Z, Y slots of both groups (all class slots, the unused ones included)."""
    S = loss_stride(C_)
    blk = lambda k: [LOSS_OFF + g * 3 * S + k * S + c for g in range(2) for c in range(S)]
    return {"nll": [0, 2], "cnt": [1, 3], "mse": [4], "mask": [5], "I": blk(0), "Z": blk(1), "Y": blk(2)}


def loss_f64(logits, labels0, labels1, n_lab, coef, t=None, teacher_is_prob=False, t_unlab_only=False, cons_mask=None, input_is_prob=False,
             world=1, grad_scale=1.0, dtype=torch.float64, mutation=None):
    """The fused loss on CPU tensors of `dtype`: logits [N,H,W,C]; labels0 [n_lab,H,W], labels1 [N-n_lab,H,W] (class ids, 255 = ignore, None =
    the group has no labels); t = the teacher's logits (or probabilities) of the whole batch or, with t_unlab_only, of the images from n_lab
    on; cons_mask one weight per pixel of those images.  coef = (ce0, dice0, ce1, dice1, mse_w) and grad_scale as the float32 words the
    kernels read.  -> (sums, out, dlogits): sums in the kernels' layout (loss_nsum(C) entries), out = [total, ce0, dice0, ce1, dice1, mse, 0, 0],
    dlogits = grad_scale * d total / d logits by autograd (with input_is_prob: with respect to the probabilities, the cross-entropy held
    constant).  dtype=torch.float32 is the float32 restatement that bound_8x measures.  mutation: one of LOSS_MUTATIONS, the mistakes the
    tolerance has to tell from rounding."""
    assert mutation is None or mutation in LOSS_MUTATIONS, mutation
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    N, Hh, W, C_ = x.shape
    S = loss_stride(C_)
    k = [torch.tensor(f32_exact(v), dtype=dtype) for v in coef]
    zero = torch.zeros((), dtype=dtype)
    sums = torch.zeros(loss_nsum(C_), dtype=dtype)
    p = x if input_is_prob else torch.softmax(x, -1)
    lse = torch.logsumexp(x, -1)
    cls = torch.arange(C_)
    terms = []
    for g, (lab, lo, hi) in enumerate(((labels0, 0, n_lab), (labels1, n_lab, N))):
        ce, dice = zero, zero
        if lab is not None and hi > lo:
            tg = lab.long().reshape(hi - lo, Hh, W)
            valid = tg < C_
            picked = x[lo:hi].gather(-1, tg.clamp(max=C_ - 1).unsqueeze(-1)).squeeze(-1)
            nll = torch.where(valid, lse[lo:hi] - picked, zero).sum()
            cnt = valid.sum().to(dtype)
            onehot = (tg.unsqueeze(-1) == cls).to(dtype)
            pg = p[lo:hi]
            I, Y = (pg * onehot).sum((0, 1, 2)), onehot.sum((0, 1, 2))
            Z = (pg * pg).sum((0, 1, 2))
            if mutation == "z_skips_ignored":
                Z = (pg * pg * (tg != 255).to(dtype).unsqueeze(-1)).sum((0, 1, 2))
            den = torch.tensor(float(valid.numel()), dtype=dtype) if mutation == "ce_over_all_pixels" else cnt
            if float(cnt) > 0:
                ce = nll / den
            per_class = 1.0 - (2.0 * I + LOSS_SMOOTH) / (Z + Y + LOSS_SMOOTH)
            dice = per_class.sum() / (C_ - 1) if mutation == "dice_mean_over_c_minus_1" else per_class.mean()
            base = LOSS_OFF + g * 3 * S
            with torch.no_grad():
                sums[2 * g], sums[2 * g + 1] = nll, cnt
                sums[base:base + C_], sums[base + S:base + S + C_], sums[base + 2 * S:base + 2 * S + C_] = I, Z, Y
        if input_is_prob:
            ce = ce.detach()
        terms += [ce, dice]
    mse = zero
    if t is not None and N > n_lab:
        q = t.detach().to(dtype)
        if not teacher_is_prob:
            q = torch.softmax(q, -1)
        if not t_unlab_only:
            q = q[n_lab:]
        w = torch.ones(N - n_lab, Hh, W, dtype=dtype) if cons_mask is None else cons_mask.detach().to(dtype).reshape(N - n_lab, Hh, W)
        s4, s5 = (w * ((p[n_lab:] - q) ** 2).sum(-1)).sum(), w.sum()
        if cons_mask is not None:
            mse = s4 / ((1.0 if mutation == "masked_mse_without_2" else 2.0) * s5 + 1e-16)
        else:
            mse = s4 / float((N - n_lab) * Hh * W * (1 if mutation == "mse_count_without_c" else C_) * world)
        with torch.no_grad():
            sums[4], sums[5] = s4, s5
    terms.append(mse)
    total = sum(kk * tt for kk, tt in zip(k, terms))
    out = torch.stack([total] + terms + [zero, zero]).detach()
    grad = torch.autograd.grad(total, x)[0] if total.requires_grad else torch.zeros_like(x)
    return sums, out, (grad * f32_exact(grad_scale)).detach()


@functools.lru_cache(maxsize=None)
def loss_case(C_, N, n_lab, Hh, W, seed=0, ignored=0.05):
    """Seeded inputs of one fused-loss case on the CPU (NHWC, computed once; read-only): logits and teacher logits = 2 * randn through
    chan_affine's per-channel law (scale in [0.25, 4], offset in [-3, 3]); labels of the whole batch with about `ignored` of the pixels at 255,
    one id in [C, 255) and class C - 1 never present; a 0 / 1 consistency mask over the images from n_lab on."""
    g = torch.Generator().manual_seed(1000 * C_ + 10 * N + n_lab + seed)
    def draw():
        sc = 0.25 * 16.0 ** torch.rand(C_, generator=g)
        off = 6.0 * torch.rand(C_, generator=g) - 3.0
        return (2.0 * torch.randn(N, Hh, W, C_, generator=g) * sc + off).float()
    logits, t_logits = draw(), draw()
    lab = torch.randint(0, C_ - 1, (N, Hh, W), generator=g)
    lab[torch.rand(N, Hh, W, generator=g) < ignored] = 255
    flat = lab.view(N, -1)
    for n in range(N):                                   # every image: the ignore value at both ends, an id in [C, 255) inside
        flat[n, 0], flat[n, -1], flat[n, flat.shape[1] // 2] = 255, 255, C_ + 1
    assert (C_ - 1) not in lab and 255 in lab and int(((lab >= C_) & (lab != 255)).sum()) >= N
    mask = (torch.rand(N - n_lab, Hh, W, generator=g) < 0.6).float()
    lab = lab.to(torch.uint8)
    return dict(C=C_, N=N, n_lab=n_lab, H=Hh, W=W, logits=logits, t_logits=t_logits, labels0=lab[:n_lab].contiguous(),
                labels1=lab[n_lab:].contiguous(), mask=mask)


LOSS_MODES = ("teacher_logits", "teacher_prob_unlab", "masked", "no_teacher", "prob_input")


def loss_mode_kwargs(case, mode, coef=LOSS_K):
    """Keyword arguments of loss_f64 (and of the GPU tests' launcher) for one of LOSS_MODES on a loss_case:
      teacher_logits       both label groups, teacher logits indexed like the batch (HPFG, CPS)
      teacher_prob_unlab   teacher probabilities of the unlabelled images only (ICT's mixed prediction)
      masked               teacher logits of the unlabelled images and the 0 / 1 mask (UAMT)
      no_teacher           the supervised terms alone
      prob_input           probabilities in, Dice only (DiceLoss(softmax=False))"""
    c, nl = case, case["n_lab"]
    kw = dict(logits=c["logits"], labels0=c["labels0"] if nl > 0 else None, labels1=c["labels1"] if nl < c["N"] else None, n_lab=nl,
              coef=tuple(coef))
    if mode == "teacher_logits":
        kw.update(t=c["t_logits"])
    elif mode == "teacher_prob_unlab":
        kw.update(t=torch.softmax(c["t_logits"][nl:], -1), teacher_is_prob=True, t_unlab_only=True)
    elif mode == "masked":
        kw.update(t=c["t_logits"][nl:].contiguous(), t_unlab_only=True, cons_mask=c["mask"])
    elif mode == "prob_input":
        kw.update(logits=torch.softmax(c["logits"], -1), input_is_prob=True, coef=(0.0, coef[1], 0.0, coef[3], 0.0))
    else:
        assert mode == "no_teacher", mode
    return kw


def loss_mutation_active(mutation, kw):
    """Whether the term a mutation changes takes part in the total of loss_f64(**kw)."""
    N, nl = kw["logits"].shape[0], kw["n_lab"]
    k = kw["coef"]
    sup = [(kw["labels0"] is not None and nl > 0, k[0], k[1]), (kw["labels1"] is not None and nl < N, k[2], k[3])]
    cons = kw.get("t") is not None and nl < N and k[4] != 0
    if mutation == "ce_over_all_pixels":
        return any(on and kce != 0 for on, kce, _ in sup) and not kw.get("input_is_prob", False)
    if mutation in ("z_skips_ignored", "dice_mean_over_c_minus_1"):
        return any(on and kd != 0 for on, _, kd in sup)
    if mutation == "masked_mse_without_2":
        return cons and kw.get("cons_mask") is not None
    return cons and kw.get("cons_mask") is None


def uncertainty_f64(preds, T, dtype=torch.float64):
    """UAMT's entropy (2019_07_MICCAI_Uncertainty_Aware_ACDC.py:147-151): preds [T*S,H,W,C] logits, prediction t of image s at t*S + s ->
    u [S,H,W] = -sum_c p log(p + 1e-6) with p the mean over t of the softmax."""
    x = preds.to(dtype)
    pm = torch.softmax(x, -1).reshape(T, x.shape[0] // T, *x.shape[1:]).mean(0)
    return -(pm * torch.log(pm + 1e-6)).sum(-1)


def uncertainty_threshold(u64):
    """-> (threshold, gap): the midpoint of the widest gap between adjacent sorted values of u64 within the middle half of the distribution,
    and that gap's width.  A threshold there lets the float64 reference alone decide every pixel of the mask."""
    s = torch.sort(u64.reshape(-1).double()).values
    n = s.numel()
    mid = s[n // 4:n - n // 4]
    d = mid[1:] - mid[:-1]
    i = int(torch.argmax(d))
    return float(0.5 * (mid[i] + mid[i + 1])), float(d[i])


@functools.lru_cache(maxsize=None)
def uncertainty_case(C_, T=8, S=3, Hh=16, W=24):
    """T stochastic predictions (2 * randn logits, NHWC [T*S,H,W,C]) of S images; computed once, read-only."""
    g = torch.Generator().manual_seed(40 + C_)
    return (2.0 * torch.randn(T * S, Hh, W, C_, generator=g)).float()


# ---- float64 laws of the attention kernels (csrc/attn.hip, attn_keys.hip, attn_window.hip, attn_window_packed.hip, tokens.hip's per-query ones) --
# One formula, softmax(scale q k^T + bias + mask) v with its closed-form backward, written three times over in plain torch: in float64
# (the law), in float32 (the yardstick of HPFG_MATH=f32) and in the arithmetic the top of csrc/attn_core.h documents (the yardstick of the
# split-bf16 kernels).  No tiles, lanes or key blocks.  tests/test_attn_laws_host.py holds the laws against float64 autograd of the
# written-out formulas and shows that each named mutation is caught; tests/test_gpu_attn_edges.py holds the kernels against the laws, and
# tests/test_gpu_attn_window_edges.py the window kernels with a dropout mask and the packed window kernels.
ATTN_MUTATIONS = ("pad_keys", "dkv_tail", "dk_no_scale")
WINDOW_MUTATIONS = ("mask_inf", "pad_keys", "bias_transposed", "bias_scaled", "mask_edge", "roll_sign", "hw_swap")
# of the dropout arithmetic (the DROP kernels of csrc/attn_window.hip and attn_window_packed.hip): f = M (no 1 / (1 - p)); dV from the
# undropped P; the row sum of dS over the unmasked dP; the mask read as M[l2][l1]
WINDOW_DROP_MUTATIONS = ("drop_no_rescale", "drop_dv_undropped", "drop_delta_undropped", "drop_transposed")
# of the packed tile (csrc/attn_window_packed.hip: 64 // w^2 consecutive raster windows of one image share a tile): the keys of the tile's
# other windows take part with the logit scale q.k (no bias); the mask indexed by the window's slot in its tile, not its index in the image
PACKED_MUTATIONS = ("tile_leak", "drop_slot_index")
# what the dQ kernels did until dP .* f became a rounded product of its own (ds_drop_t of csrc/attn_window.h): the compiler fused the product
# into `dP .* f - delta`, so dS took it unrounded while delta had summed it rounded to float32 -- invisible unless a row's dS is 0
WINDOW_DROP_ROUNDING = "drop_ds_unrounded"
ATTN_IMAGE_KEYS = 64             # keys of one LDS image: what a kernel that forgot to exclude the padding keys would normalise over
ATTN_DKV_QUERIES = 512           # queries per dK / dV workgroup (Q_PER_BLOCK of csrc/attn_core.h)
WINDOW_MASKED = -100.0           # the reference's literal (model/swinunet.py:204), not -inf


def _bf16_split(x):
    """x (float32) -> hi, lo as float64: hi = bf16 round-to-nearest of x, lo = bf16 round-to-nearest of x - hi (exact in float32)."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def _prod3(a, b):
    """a @ b of two float32 operands as the matrix cores form it: hi.hi + lo.hi + hi.lo (every bf16 product is exact), accumulated here
    without rounding and rounded once to float32."""
    ah, al = _bf16_split(a)
    bh, bl = _bf16_split(b)
    return (ah @ bh + al @ bh + ah @ bl).float()


def _attn_core(q, k, v, do, scale, bias=None, mask=None, arith=torch.float64, max_subtract=True, pad_keys=0, drop=None, mutation=None):
    """q, do [..., Lq, d], k, v [..., Lk, d], bias / mask broadcastable to [..., Lq, Lk] -> out, lse, dq, dk, dv, dS (gradient of the logits).
    arith: torch.float64 / torch.float32 (every operation in that type) or "split" (attn_core.h: scale folded into q, split-bf16 products
    rounded to float32, float32 softmax, P and dS split again for the second product).
    drop: the dropout factors f = M / (1 - p) of the probabilities, broadcastable to [..., Lq, Lk] (include/hpfg_hip.h at
    hpfg_attn_window_drop_fwd): out = (P .* f) V, dP = (dO V^T) .* f, dS = P .* (dP - rowsum(P .* dP)), dV = (P .* f)^T dO; in split
    arithmetic P .* f is what gets split.  mutation (with drop): "drop_dv_undropped" (dV from P), "drop_delta_undropped" (the row sum over
    the unmasked dP), "drop_ds_unrounded" (the row sum over dP .* f rounded to float32, dS from the unrounded one)."""
    split = arith == "split"
    dt = torch.float32 if split else arith
    q, k, v, do = (t.to(dt) for t in (q, k, v, do))
    mm = _prod3 if split else torch.matmul
    T = lambda t: t.transpose(-2, -1)
    if pad_keys:                                   # mutation: padding keys (zero rows of K and V) take part with logit 0
        z = torch.zeros(*k.shape[:-2], pad_keys, k.shape[-1], dtype=dt)
        k, v = torch.cat([k, z], -2), torch.cat([v, z], -2)
    qs = q * torch.tensor(scale, dtype=dt) if split else q
    S = mm(qs, T(k)) if split else mm(q, T(k)) * scale
    for add in (bias, mask):
        if add is not None:
            add = add.to(dt)
            if pad_keys:
                add = torch.cat([add, torch.zeros(*add.shape[:-1], pad_keys, dtype=dt)], -1)
            S = S + add
    mx = S.amax(-1, keepdim=True) if max_subtract else torch.zeros_like(S[..., :1])
    e = torch.exp(S - mx)
    den = e.sum(-1, keepdim=True)
    P = e * (1.0 / den) if split else e / den
    lse = (mx + torch.log(den)).squeeze(-1)
    Pv = P                                         # the probabilities the products with V and dO take
    if drop is None:
        out = mm(P, v)
        dP = mm(do, T(v))
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    else:
        f = drop.to(dt)
        if pad_keys:
            f = torch.cat([f, torch.ones(*f.shape[:-1], pad_keys, dtype=dt)], -1)
        Pd = P * f
        out = mm(Pd, v)
        raw = mm(do, T(v))
        dP = raw * f
        summed = raw if mutation == "drop_delta_undropped" else dP.float().to(dt) if mutation == "drop_ds_unrounded" else dP
        dS = P * (dP - (P * summed).sum(-1, keepdim=True))
        if mutation != "drop_dv_undropped":
            Pv = Pd
    if split:
        dq, dk = mm(dS, k) * torch.tensor(scale, dtype=dt), mm(T(dS), qs)          # dK carries the scale through the scaled q
    else:
        dq, dk = mm(dS, k) * scale, mm(T(dS), q) * scale
    dv = mm(T(Pv), do)
    if pad_keys:
        dk, dv, dS = dk[..., :-pad_keys, :], dv[..., :-pad_keys, :], dS[..., :-pad_keys]
    return out, lse, dq, dk, dv, dS


def attn_f64(q, kv, do, heads, d, scale, mutation=None, arith=torch.float64, max_subtract=True):
    """softmax(scale q k^T) v per (image, head) and its gradients: q, do [B,N,heads d], kv [B,M,2 heads d] laid out [.., 2, heads, d] ->
    out [B,N,heads d], lse [B,heads,N] (log of the softmax denominator), dq like q, dkv like kv; in `arith` like the inputs' shape."""
    B, N, C_ = q.shape
    M = kv.shape[1]
    qh, dh = (t.reshape(B, N, heads, d).permute(0, 2, 1, 3) for t in (q, do))
    k, v = kv.reshape(B, M, 2, heads, d).permute(2, 0, 3, 1, 4)
    pad = (-M) % ATTN_IMAGE_KEYS if mutation == "pad_keys" else 0
    out, lse, dq, dk, dv, _ = _attn_core(qh, k, v, dh, scale, arith=arith, max_subtract=max_subtract, pad_keys=pad)
    if mutation == "dkv_tail":                     # dK / dV over the full blocks of 512 queries only
        n = N // ATTN_DKV_QUERIES * ATTN_DKV_QUERIES
        _, _, _, dk, dv, _ = _attn_core(qh[:, :, :n], k, v, dh[:, :, :n], scale, arith=arith)
    if mutation == "dk_no_scale" and scale != 0:
        dk = dk / scale
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, C_)
    return back(out), lse, back(dq), torch.stack([dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, M, 2 * C_)


def attn_split_emulation(q, kv, do, heads, d, scale):
    """attn_f64 in the arithmetic of csrc/attn_core.h: the yardstick of the split-bf16 kernels."""
    return attn_f64(q, kv, do, heads, d, scale, arith="split")


def window_partition(x, w):
    """[B,H,W,...] -> [B * nW, w * w, ...] (window_partition of the reference)"""
    B, H, W = x.shape[:3]
    rest = x.shape[3:]
    k = len(rest)
    return x.reshape(B, H // w, w, W // w, w, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + k)).reshape(B * (H // w) * (W // w), w * w, *rest)


def window_reverse(xw, B, H, W, w):
    C_ = xw.shape[-1]
    return xw.reshape(B, H // w, W // w, w, w, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C_)


def window_attn_reference(qkv, table, heads, w, s, scale, drop=None):
    """WindowAttention.forward of the reference between its qkv and proj Linear, written out with the reference's own tensor operations
    (roll, partition, index table, region image, softmax, reverse, roll back); differentiable, any H x W divisible by w.
    drop = (mask, p): attn_drop, the softmax's output times mask / (1 - p) before attn @ v; mask [B nW, heads, L, L]."""
    B, H, W, C3 = qkv.shape
    C_, L_ = C3 // 3, w * w
    d = C_ // heads
    x = torch.roll(qkv, (-s, -s), (1, 2)) if s else qkv
    xw = window_partition(x, w).reshape(-1, L_, 3, heads, d).permute(2, 0, 3, 1, 4)            # [3, Bn, heads, L, d]
    q, k, v = xw[0] * scale, xw[1], xw[2]
    a = q @ k.transpose(-2, -1)
    l = torch.arange(L_)
    i, j = l // w, l % w
    idx = (i[:, None] - i[None, :] + w - 1) * (2 * w - 1) + (j[:, None] - j[None, :] + w - 1)
    a = a + table[idx.reshape(-1)].reshape(L_, L_, heads).permute(2, 0, 1)[None]
    if s:
        img = torch.zeros(1, H, W, 1, dtype=qkv.dtype)
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
        mw = window_partition(img, w).reshape(-1, L_)
        m = mw[:, None, :] - mw[:, :, None]
        m = torch.where(m != 0, torch.full_like(m, WINDOW_MASKED), torch.zeros_like(m))
        nW = m.shape[0]
        a = (a.reshape(B, nW, heads, L_, L_) + m[None, :, None]).reshape(-1, heads, L_, L_)
    a = a.softmax(-1)
    if drop is not None:
        a = a * drop[0].to(qkv.dtype) / (1.0 - drop[1])
    o = (a @ v).transpose(1, 2).reshape(-1, L_, C_)
    o = window_reverse(o, B, H, W, w)
    return torch.roll(o, (s, s), (1, 2)) if s else o


def window_tables(H, W, w, s, mutation=None):
    """The definition as index tables: tok [nW, L] = the token y W + x at position l = i w + j of window (wy, wx) of the map rolled by -s,
    region [nW, L] = 3 r(y') + r(x') of the rolled coordinate (r = 0 below n - w, 1 below n - s, else 2), idx [L, L] = the bias-table row of
    (query l1, key l2)."""
    nwy, nwx = H // w, W // w
    win, l = torch.arange(nwy * nwx), torch.arange(w * w)
    per_row = nwy if mutation == "hw_swap" else nwx
    yp = (win // per_row)[:, None] * w + (l // w)[None]
    xp = (win % per_row)[:, None] * w + (l % w)[None]
    sh = -s if mutation == "roll_sign" else s
    tok = ((yp + sh) % H) * W + (xp + sh) % W
    cut = s + 1 if mutation == "mask_edge" else s

    def region(p, n):
        return (p >= n - w).long() + (p >= n - cut).long()
    reg = 3 * region(yp, H) + region(xp, W) if s else torch.zeros_like(tok)
    i, j = l // w, l % w
    idx = (i[:, None] - i[None, :] + w - 1) * (2 * w - 1) + (j[:, None] - j[None, :] + w - 1)
    return tok, reg, idx.t() if mutation == "bias_transposed" else idx


def _drop_factors(drop, B, nW, heads, L_, dt, mutation=None):
    """drop = (mask uint8 [B nW, heads, L, L], p) -> f = M / (1 - p) as [B, nW, heads, L, L] in dt, with the mutations of the mask's use"""
    m, p = drop
    m = m.reshape(B, nW, heads, L_, L_)
    if mutation == "drop_transposed":
        m = m.transpose(-2, -1)
    if mutation == "drop_slot_index":
        m = m[:, torch.arange(nW) % (ATTN_IMAGE_KEYS // L_)]
    return m.to(dt) if mutation == "drop_no_rescale" else m.to(dt) / (1.0 - p)


def window_attn_tiles_f64(qkv, table, do, heads, w, s, scale, drop=None, mutation=None, arith=torch.float64):
    """window_attn_f64 in the view of csrc/attn_window_packed.hip: the 64 // w^2 consecutive raster windows of one image that share a tile
    are one attention over the tile's rows, whose logit between positions of different windows is -inf (the keys are excluded exactly:
    the law, equal to window_attn_f64) or, with mutation "tile_leak", scale q.k without bias or mask.  Dropout factors between windows are 1."""
    B, H, W, C3 = qkv.shape
    C_, L_ = C3 // 3, w * w
    d = C_ // heads
    dt = torch.float32 if arith == "split" else arith
    tok, reg, idx = window_tables(H, W, w, s)
    nW, per = tok.shape[0], ATTN_IMAGE_KEYS // L_
    bias = table.to(dt)[idx.reshape(-1)].reshape(L_, L_, heads).permute(2, 0, 1)
    cross = 0.0 if mutation == "tile_leak" else float("-inf")
    f_all = None if drop is None else _drop_factors(drop, B, nW, heads, L_, dt, mutation)
    out, dqkv = torch.zeros(B, H * W, C_, dtype=dt), torch.zeros(B, H * W, 3, heads, d, dtype=dt)
    dtable = torch.zeros(table.shape[0], heads, dtype=dt)
    for w0 in range(0, nW, per):
        n = min(per, nW - w0)
        tk, R = tok[w0:w0 + n].reshape(-1), n * L_
        x = qkv.reshape(B, H * W, 3, heads, d)[:, tk].permute(2, 0, 3, 1, 4)                   # [3, B, heads, R, d]
        dh = do.reshape(B, H * W, heads, d)[:, tk].permute(0, 2, 1, 3)
        add = torch.full((heads, R, R), cross, dtype=dt)
        f = None if drop is None else torch.ones(B, heads, R, R, dtype=dt)
        for i in range(n):
            own = slice(i * L_, (i + 1) * L_)
            add[:, own, own] = bias
            if s:
                r = reg[w0 + i]
                add[:, own, own] += torch.where(r[:, None] != r[None, :], WINDOW_MASKED, 0.0).to(dt)
            if drop is not None:
                f[:, :, own, own] = f_all[:, w0 + i]
        o, _, dq, dk, dv, dS = _attn_core(x[0], x[1], x[2], dh, scale, bias=add, arith=arith, drop=f)
        out[:, tk] = o.permute(0, 2, 1, 3).reshape(B, R, C_)
        dqkv[:, tk] = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4)
        for i in range(n):
            own = slice(i * L_, (i + 1) * L_)
            dtable.index_add_(0, idx.reshape(-1), dS[:, :, own, own].sum(0).permute(1, 2, 0).reshape(L_ * L_, heads))
    return out.reshape(B, H, W, C_), dqkv.reshape(B, H, W, C3), dtable


def window_attn_f64(qkv, table, do, heads, w, s, scale, mutation=None, arith=torch.float64, drop=None):
    """Shifted-window attention and its gradients from the index tables: qkv [B,H,W,3 heads d] (channel = t heads d + head d + p),
    table [(2w-1)^2, heads], do [B,H,W,heads d] -> out like do, dqkv like qkv, dtable like table.
    drop = (mask, p): dropout of the probabilities, mask uint8 [B nW, heads, L, L] in the element order include/hpfg_hip.h documents for
    hpfg_attn_window_drop_fwd (the reference's attn tensor in its rolled, window-partitioned order), f = M / (1 - p) as _attn_core states."""
    if mutation == "tile_leak":
        return window_attn_tiles_f64(qkv, table, do, heads, w, s, scale, drop, mutation, arith)
    B, H, W, C3 = qkv.shape
    C_, L_ = C3 // 3, w * w
    d = C_ // heads
    dt = torch.float32 if arith == "split" else arith
    tok, reg, idx = window_tables(H, W, w, s, mutation)
    nW = tok.shape[0]
    f = None if drop is None else _drop_factors(drop, B, nW, heads, L_, dt, mutation)
    x = qkv.reshape(B, H * W, 3, heads, d)[:, tok].permute(3, 0, 1, 4, 2, 5)                  # [3, B, nW, heads, L, d]
    dh = do.reshape(B, H * W, heads, d)[:, tok].permute(0, 1, 3, 2, 4)
    tab = table.to(dt) * (torch.tensor(scale, dtype=dt) if mutation == "bias_scaled" else 1.0)
    bias = tab[idx.reshape(-1)].reshape(L_, L_, heads).permute(2, 0, 1)                       # [heads, L, L]
    mask = None
    if s:
        differ = reg[:, :, None] != reg[:, None, :]
        mask = torch.where(differ, float("-inf") if mutation == "mask_inf" else WINDOW_MASKED, 0.0).to(dt)[:, None]      # [nW, 1, L, L]
    pad = (-L_) % ATTN_IMAGE_KEYS if mutation == "pad_keys" else 0
    o, _, dq, dk, dv, dS = _attn_core(x[0], x[1], x[2], dh, scale, bias=bias, mask=mask, arith=arith, pad_keys=pad, drop=f, mutation=mutation)
    out, dqkv = torch.zeros(B, H * W, C_, dtype=dt), torch.zeros(B, H * W, 3, heads, d, dtype=dt)
    out[:, tok] = o.permute(0, 1, 3, 2, 4).reshape(B, nW, L_, C_)
    dqkv[:, tok] = torch.stack([dq, dk, dv]).permute(1, 2, 4, 0, 3, 5)
    dtable = torch.zeros(table.shape[0], heads, dtype=dt).index_add_(0, idx.reshape(-1), dS.sum((0, 1)).permute(1, 2, 0).reshape(L_ * L_, heads))
    if mutation == "bias_scaled":
        dtable = dtable * scale
    return out.reshape(B, H, W, C_), dqkv.reshape(B, H, W, C3), dtable


def attn_tolerance(ref64, yardstick):
    """Per output tensor: 8 x the largest error the yardstick (torch float32 on the CPU for HPFG_MATH=f32, the split-bf16 emulation for the
    default mode) makes against the float64 law, and no less than 4 float32 ulp of the law's largest magnitude."""
    return tuple(bound_8x(r, y) for r, y in zip(ref64, yardstick))


ATTN_MATHS = ("f32", "bf16x3")
ATTN_YARDSTICK = {"f32": torch.float32, "bf16x3": "split"}


def _row_max_p(S):
    return torch.softmax(S.double(), -1).amax(-1)


def _attn_logits(q, kv, heads, d, scale):
    B, N, _ = q.shape
    M = kv.shape[1]
    k = kv.reshape(B, M, 2, heads, d)[:, :, 0]
    return torch.einsum("bnhd,bmhd->bhnm", q.reshape(B, N, heads, d).double(), k.double()) * scale


def attn_inputs(family, B, N, M, heads, d, scale=None):
    """q, kv, do (float32, fixed seed) of an input family, with the family's condition asserted in float64:
    unit    randn: logits about N(0, 1)
    sharp   q and k times 2 (times 2.5 above 64 keys): the median row's largest probability is at least 0.5; with N >= 128 every 16-key
            tile and the last key hold the maximum of some row
    offset  q[..., 0] = 16, k[..., 0] = 100 sqrt(d) / 16 in every head: +100 on every logit of a row, the softmax unchanged; every row's
            largest logit exceeds 89, where float32 exp overflows without the max subtraction"""
    sc = d ** -0.5 if scale is None else scale
    C_ = heads * d
    for attempt in range(16):                      # sharp: the first of 16 fixed seeds whose draw meets the condition
        g = torch.Generator().manual_seed(7919 * attempt + 1000 * d + 31 * N + M + 7 * B + heads)
        q, kv, do = torch.randn(B, N, C_, generator=g), torch.randn(B, M, 2 * C_, generator=g), torch.randn(B, N, C_, generator=g)
        if family == "unit":
            return q, kv, do
        if family == "offset":
            assert scale is None
            q.view(B, N, heads, d)[..., 0] = 16.0
            kv.view(B, M, 2, heads, d)[:, :, 0, :, 0] = 100.0 * d ** 0.5 / 16.0
            S = _attn_logits(q, kv, heads, d, sc)
            assert float(S.amax(-1).min()) > 89.0
            return q, kv, do
        assert family == "sharp"
        mul = 2.0 if M <= ATTN_IMAGE_KEYS else 2.5          # over 65 .. 256 keys times 2 leaves the median at 0.42 .. 0.54: the condition decides
        q *= mul
        kv.view(B, M, 2, heads, d)[:, :, 0] *= mul
        S = _attn_logits(q, kv, heads, d, sc)
        ok = float(_row_max_p(S).median()) >= 0.5
        if N >= 128:
            hit = torch.zeros(M, dtype=torch.bool)
            hit[S.argmax(-1).reshape(-1)] = True
            ok = ok and bool(hit[M - 1]) and all(bool(hit[t:t + 16].any()) for t in range(0, M, 16))
        if ok:
            return q, kv, do
    raise AssertionError(f"sharp: no draw met the condition for {(B, N, M, heads, d)}")


@functools.lru_cache(maxsize=None)
def attn_case(family, B, N, M, heads, d, scale=None):
    """-> dict: inputs, scale, the float64 law `ref` = (out, lse, dq, dkv), and per math mode the yardstick's results and the tolerances.
    Computed once per case and shared; read-only."""
    sc = d ** -0.5 if scale is None else scale
    q, kv, do = attn_inputs(family, B, N, M, heads, d, scale)
    ref = attn_f64(q, kv, do, heads, d, sc)
    yard = {m: attn_f64(q, kv, do, heads, d, sc, arith=a) for m, a in ATTN_YARDSTICK.items()}
    return dict(q=q, kv=kv, do=do, scale=sc, ref=ref, yard=yard, tol={m: attn_tolerance(ref, y) for m, y in yard.items()})


def _window_logits(qkv, table, heads, w, s, scale):
    """[B, nW, heads, L, L] float64 logits (bias and mask included) of the law"""
    B, H, W, C3 = qkv.shape
    d, L_ = C3 // 3 // heads, w * w
    tok, reg, idx = window_tables(H, W, w, s)
    x = qkv.double().reshape(B, H * W, 3, heads, d)[:, tok].permute(3, 0, 1, 4, 2, 5)
    S = (x[0] @ x[1].transpose(-2, -1)) * scale + table.double()[idx.reshape(-1)].reshape(L_, L_, heads).permute(2, 0, 1)
    if s:
        S = S + torch.where(reg[:, :, None] != reg[:, None, :], WINDOW_MASKED, 0.0).double()[:, None]
    return S


def window_inputs(family, B, H, W, w, s, heads, d, scale=None):
    """qkv, table, do (float32, fixed seed): unit = randn; sharp = q and k times 2 (median row-max probability at least 0.5); hot = q and k
    times 8 (logits of tens, so a masked pair at -100 still competes: its condition, that -inf for -100 moves `out` by at least four
    tolerances, is asserted by window_case, which has the tolerances)."""
    C_ = heads * d
    g = torch.Generator().manual_seed(100000 * H + 1000 * W + 100 * w + 10 * s + d + B + heads)
    qkv, do = torch.randn(B, H, W, 3 * C_, generator=g), torch.randn(B, H, W, C_, generator=g)
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g)
    mul = {"unit": 1.0, "sharp": 2.0, "hot": 8.0}[family]
    qkv[..., :2 * C_] *= mul
    if family == "sharp":
        S = _window_logits(qkv, table, heads, w, s, d ** -0.5 if scale is None else scale)
        assert float(_row_max_p(S).median()) >= 0.5
    return qkv, table, do


def window_results(res):
    """(out, dqkv, dtable) -> (out, dq, dk, dv, dtable): the window op's gradients have a tolerance each"""
    return (res[0],) + tuple(res[1].chunk(3, -1)) + (res[2],)


WINDOW_TENSORS = ("out", "dq", "dk", "dv", "dtable")


@functools.lru_cache(maxsize=None)
def window_case(family, B, H, W, w, s, heads, d, scale=None):
    """-> dict like attn_case: `ref` = (out, dq, dk, dv, dtable) of the float64 law."""
    sc = d ** -0.5 if scale is None else scale
    qkv, table, do = window_inputs(family, B, H, W, w, s, heads, d, scale)
    ref = window_results(window_attn_f64(qkv, table, do, heads, w, s, sc))
    yard = {m: window_results(window_attn_f64(qkv, table, do, heads, w, s, sc, arith=a)) for m, a in ATTN_YARDSTICK.items()}
    tol = {m: attn_tolerance(ref, y) for m, y in yard.items()}
    if family == "hot" and s:                      # the family's condition: -inf in place of the literal -100 is far outside the tolerance
        moved = window_attn_f64(qkv, table, do, heads, w, s, sc, mutation="mask_inf")[0]
        assert float((moved - ref[0]).abs().max()) >= 4.0 * max(t[0] for t in tol.values())
    return dict(qkv=qkv, table=table, do=do, scale=sc, ref=ref, yard=yard, tol=tol)


def window_drop_mask(B, nW, heads, L_, p, seed=0):
    """uint8 [B nW, heads, L, L] of keep rate 1 - p (fixed seed).  In the first window of the first image (head 0) query row 0 has every key
    dropped (out = 0 and dS = 0 there) and row L - 1 every key kept; a 1 x 1 window has one row, so its kept row is that of the second
    window.  Both are asserted."""
    g = torch.Generator().manual_seed(271828 + 7919 * seed + 101 * nW + 13 * L_ + 3 * B + heads + int(1000 * p))
    m = (torch.rand(B * nW, heads, L_, L_, generator=g) >= p).to(torch.uint8)
    kept = (0, 0, L_ - 1) if L_ > 1 else (1, 0, 0)
    m[0, 0, 0] = 0
    m[kept] = 1
    assert int(m[0, 0, 0].sum()) == 0 and int(m[kept].sum()) == L_
    return m


@functools.lru_cache(maxsize=None)
def window_drop_case(family, B, H, W, w, s, heads, d, p):
    """window_case with dropout of the probabilities: the same inputs (so the family's condition is the one window_case asserts), an
    explicit mask of keep rate 1 - p, and the law, the yardsticks and the tolerances with that mask, by the same attn_tolerance."""
    c = window_case(family, B, H, W, w, s, heads, d)
    qkv, table, do, sc = c["qkv"], c["table"], c["do"], c["scale"]
    mask = window_drop_mask(B, (H // w) * (W // w), heads, w * w, p, seed=1000 * H + 10 * W + s + d)
    ref = window_results(window_attn_f64(qkv, table, do, heads, w, s, sc, drop=(mask, p)))
    yard = {m: window_results(window_attn_f64(qkv, table, do, heads, w, s, sc, arith=a, drop=(mask, p))) for m, a in ATTN_YARDSTICK.items()}
    return dict(qkv=qkv, table=table, do=do, scale=sc, mask=mask, p=p, ref=ref, yard=yard, tol={m: attn_tolerance(ref, y) for m, y in yard.items()})


def window_hand_bounds(B, H, W, w, d, math, p=0.0):
    """The hand constants tests/test_gpu_swin.py, test_gpu_swin_dropout.py and test_gpu_attn_window_packed.py hold the window kernels to
    (out, dq, dk, dv, dtable), restated for a rectangular map: what tests/test_attn_laws_host.py compares the rule's tolerances with."""
    k = (1.0 if math == "f32" else 8.0) * (2 ** 0.5 if d == 64 else 1.0)
    kb = 1.0 if math == "f32" else 8.0
    pairs = B * (H // w) * (W // w) * w * w
    return tuple(b / (1.0 - p) for b in (2e-5 * k, 5e-5 * k, 2e-4 * k, 2e-4 * k, 2e-4 * kb * max(1.0, (pairs / 256) ** 0.5)))


def worst_ratio(got, ref, tol):
    """max over the tensors of max |got - ref| / tolerance, and the list of the ratios"""
    r = [float((g.double() - x.double()).abs().max()) / t if x.numel() else 0.0 for g, x, t in zip(got, ref, tol)]
    return max(r), r


# the cases of tests/test_gpu_attn_edges.py (tests/test_attn_laws_host.py checks the families' conditions on the same ones)
ATTN_HEAD_DIMS = (32, 64)
ATTN_M_EDGES = [(2, 65, M, 2) for M in (1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64)]           # the 16-key tile edges
ATTN_N_EDGES = [(1, N, 49, 1) for N in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 639, 640, 641)] + [(2, 513, 49, 5)]
ATTN_KEYS_EDGES = [(1, 65, 65, 1), (1, 513, 129, 1), (1, 641, 200, 1), (1, 64, 256, 1), (1, 130, 255, 1)]
ATTN_SCALE_CASES = [(2, 65, 33, 2, 0.3), (2, 65, 33, 2, 0.0)]                                  # unit family, scale != d^-0.5 and scale = 0
# (B, H, W, w, s, heads): 6, 3, 5, 8, 4, 2, 3 and 18 workgroups per head; the first and the last shift; every window size
WINDOW_EDGES = [(1, 8, 12, 4, 1, 2), (1, 4, 12, 4, 3, 1), (5, 7, 7, 7, 6, 1), (2, 6, 6, 3, 1, 2), (1, 10, 10, 5, 2, 1), (1, 12, 6, 6, 5, 1),
                (3, 2, 2, 2, 1, 1), (2, 3, 3, 1, 0, 2)]
# (B, H, W, w, s, heads) of the packed kernels: a tile holds 64 // w^2 = 16 / 7 / 4 windows (slots) of one image in raster order
PACKED_EDGES = [(1, 2, 2, 2, 0, 1),          # one of 16 slots
                (1, 8, 8, 2, 1, 1),          # exactly 16 slots
                (1, 6, 6, 2, 1, 2),          # 9 of 16 slots
                (2, 8, 10, 2, 1, 1),         # 16 + 4 slots, rectangular, two images: a partial last tile with another image behind it
                (1, 2, 34, 2, 1, 1),         # 16 + 1 slots
                (1, 3, 3, 3, 1, 1),          # one of 7 slots; tile row 63 is never live at w = 3
                (1, 3, 21, 3, 1, 1),         # exactly 7 slots
                (1, 6, 12, 3, 1, 2),         # 7 + 1 slots
                (2, 9, 6, 3, 0, 1),          # 6 slots
                (1, 4, 4, 4, 2, 1),          # window equals map
                (1, 8, 8, 4, 2, 1),          # exactly 4 slots
                (1, 4, 20, 4, 2, 1),         # 4 + 1 slots
                (3, 12, 8, 4, 2, 2)]         # 4 + 2 slots, three images
WINDOW_HOT = [(1, 14, 14, 7, 3, 1, 32), (1, 8, 12, 4, 1, 1, 32), (1, 8, 8, 4, 3, 1, 64), (1, 16, 16, 8, 7, 1, 32)]      # (.., d): where `hot` was sized


# ---- float64 laws of the dense kernels (csrc/gemm.hip, csrc/heads.hip) --------------------------------------------------------------------
# Plain restatements on double tensors: the product with its epilogue, column sums, adaptive average pooling, F.normalize and NT-Xent, each
# with the named wrong variants its tolerance has to tell from rounding.  tests/test_dense_laws_host.py holds the laws against torch's own
# float64 ops and autograd and shows every mutation caught; tests/test_gpu_gemm_edges.py and tests/test_gpu_heads_edges.py hold the kernels
# against the laws.
def ulp32(x):
    """one unit in the last place of the float32 nearest to |x|"""
    return float(np.spacing(np.float32(abs(float(x)))))


def report(name, err, bound):
    """One line per compared output: largest error / bound (pytest -s shows them; the GPU modules' docstrings quote a run)."""
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"  {name:<60s} max|err| {err:9.3e}  bound {bound:9.3e}  ratio {ratio:6.3f}")
    return ratio


def within_bound(name, buf, ref64, bound):
    """buf: canary_out(ref64.numel()) after the launch.  Every element written, the tail untouched, all finite, max |buf - ref64| <= bound.
    -> the values as float64 in ref64's shape."""
    n = ref64.numel()
    written, tail = canary_ok(buf, n)
    assert written, f"{name}: elements of the output were never written"
    assert tail, f"{name}: the launch wrote past the end of the output"
    got = buf[:n].cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite (a gap or canary element was read into the result)"
    err = float((got - ref64.double()).abs().max())
    report(name, err, bound)
    assert err <= bound, (name, err, bound)
    return got


def nan_filled(n):
    """n floats on the CPU, every one the NaN pattern of the canaries: the gaps of an operand with a leading dimension above its extent."""
    return torch.full((n,), NAN_BITS, dtype=torch.int32).view(torch.float32)


GEMM_MUTATIONS = ("lo_hi_dropped", "hi_hi_only", "last_k_dropped", "split_chunk_doubled", "bias_per_split", "relu_before_accumulate")
TN_MUTATIONS = ("db_first_tile_only", "last_split_dropped")
GEMM_TILE = {"f32": (64, 16, 32), "bf16x3": (128, 32, 16)}          # math -> (output tile edge, K chunk, largest split count)


def gemm_split_geometry(math, M, N, K):
    """(splits, kper, launched, k of the last launched split) of hpfg_gemm_{f32,bf16x3}_splitk, restated from the dispatch code: splits =
    min(256 / tiles, K / 128, cap) unless there are 128 tiles or K < 256; kper = ceil(K / splits) rounded up to the K chunk; the launch
    covers ceil(K / kper) slices, which can be fewer than `splits` (the scratch is still sized by `splits`)."""
    T, chunk, cap = GEMM_TILE[math]
    tiles = -(-M // T) * -(-N // T)
    S = 1 if tiles >= 128 or K < 256 else max(1, min(256 // tiles, K // 128, cap))
    if S <= 1:
        return 1, K, 1, K
    kper = -(-(-(-K // S)) // chunk) * chunk
    launched = -(-K // kper)
    return S, kper, launched, K - (launched - 1) * kper


def tn_geometry(R, N, K):
    """(splits, rows per split, rows of the last split) of hpfg_gemm_tn_bf16x3: 64 x 64 tiles over (N, K), splits = min(1024 / tiles,
    ceil(R / 256), 512), rows per split rounded up to the 32 rows of a step."""
    tiles = -(-N // 64) * -(-K // 64)
    S = max(1, min(1024 // tiles, -(-R // 256), 512))
    per = -(-(-(-R // S)) // 32) * 32
    return S, per, R - (S - 1) * per


def col_sum_geometry(R):
    """(splits, rows per split) of hpfg_col_sum2"""
    S = max(1, min(-(-R // 512), 256))
    return S, -(-R // S)


def _prod3_f64(a, b):
    """_prod3 before its rounding: hi.hi + lo.hi + hi.lo in float64"""
    ah, al = _bf16_split(a)
    bh, bl = _bf16_split(b)
    return ah @ bh + al @ bh + ah @ bl


def gemm_f64(A, B, bias=None, C0=None, relu=False, mutation=None, kper=None, arith=torch.float64):
    """The contract of include/hpfg_hip.h: act(A B + bias + C0), A [M,K], B [K,N], bias [N], C0 [M,N] (the accumulate switch), act = relu or
    nothing.  arith: torch.float64 (the law), torch.float32 (torch's own float32 ops: the yardstick of the fp32 kernels) or "split" (the
    three bf16 products of _prod3 summed without rounding, bias and C0 added in float64, one rounding to float32: the yardstick of the
    split-bf16 kernels).  mutation: one of GEMM_MUTATIONS, evaluated in float64; the split ones take the split's `kper`."""
    assert mutation is None or mutation in GEMM_MUTATIONS, mutation
    if arith == torch.float32:
        assert mutation is None
        v = A.float() @ B.float()
        if bias is not None:
            v = v + bias.float()
        if C0 is not None:
            v = v + C0.float()
        return torch.relu(v) if relu else v
    A32, B32 = A.float(), B.float()
    Ad, Bd = A32.double(), B32.double()
    K = A.shape[1]
    if arith == "split":
        assert mutation is None
        v = _prod3_f64(A32, B32)
    elif mutation == "lo_hi_dropped":
        (ah, al), (bh, bl) = _bf16_split(A32), _bf16_split(B32)
        v = ah @ bh + ah @ bl
    elif mutation == "hi_hi_only":
        v = _bf16_split(A32)[0] @ _bf16_split(B32)[0]
    elif mutation == "last_k_dropped":
        v = Ad[:, :K - 1] @ Bd[:K - 1]
    elif mutation == "split_chunk_doubled":
        chunk = slice(kper, min(kper + 16, K))          # the first k-chunk of the second split
        v = Ad @ Bd + Ad[:, chunk] @ Bd[chunk]
    else:
        v = Ad @ Bd
    if bias is not None:
        v = v + bias.double() * (-(-K // kper) if mutation == "bias_per_split" else 1)
    if mutation == "relu_before_accumulate":
        v = torch.relu(v) if relu else v
        return v + C0.double() if C0 is not None else v
    if C0 is not None:
        v = v + C0.double()
    v = torch.relu(v) if relu else v
    return v.float() if arith == "split" else v


def gemm_tolerance(math, law, y32, ysplit=None):
    """fp32 kernels: bound_8x against torch's float32 result.  Split-bf16 kernels: that plus bound_8x against the split emulation -- the
    second term covers the arithmetic the kernel is designed to make (hi.hi + lo.hi + hi.lo), the first its float32 accumulation over K."""
    t = bound_8x(law, y32)
    return t if math == "f32" else t + bound_8x(law, ysplit)


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, seed=0):
    """Operands of one product on the CPU (float32; computed once, read-only): A [M,K] and Bt [N,K] through chan_affine's per-k scale and
    offset (Bt times 0.2, as a weight), bias [N], C0 [M,N]; `law`, `y32`, `ysplit` and `tol` per math mode for the plain product without
    epilogue; gemm_epilogue gives the same for an epilogue."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + seed)
    A, Bt = chan_affine((M, K), 0, g), 0.2 * chan_affine((N, K), 0, g)
    bias, C0 = chan_affine((N,), 0, g), chan_affine((M, N), 0, g)
    c = dict(M=M, N=N, K=K, A=A, Bt=Bt, B=Bt.t(), bias=bias, C0=C0)
    c.update(gemm_epilogue(c, False, False, False))
    return c


def gemm_epilogue(c, bias, relu, acc):
    """law, both yardsticks and the tolerance per math mode of act(A B (+ bias) (+ C0)) on a gemm_case"""
    kw = dict(bias=c["bias"] if bias else None, C0=c["C0"] if acc else None, relu=bool(relu))
    law = gemm_f64(c["A"], c["B"], **kw)
    y32, ysplit = gemm_f64(c["A"], c["B"], arith=torch.float32, **kw), gemm_f64(c["A"], c["B"], arith="split", **kw)
    return dict(law=law, y32=y32, ysplit=ysplit, tol={m: gemm_tolerance(m, law, y32, ysplit) for m in GEMM_TILE})


def gemm_operand(vals, fast, pad):
    """vals [rows, K] (A itself, or B transposed) laid out with the NaN pattern in every gap -> (flat float32 CPU buffer, srow, sk).
    fast = "k": [rows][K + pad], (srow, sk) = (K + pad, 1).  fast = "r": [K][rows + pad], (1, rows + pad).  fast = "2": neither stride is
    1, (2 K, 2) with the pattern at every odd index."""
    rows, K = vals.shape
    if fast == "k":
        buf = nan_filled(rows * (K + pad)).view(rows, K + pad)
        buf[:, :K] = vals
        return buf.view(-1), K + pad, 1
    if fast == "r":
        buf = nan_filled(K * (rows + pad)).view(K, rows + pad)
        buf[:, :rows] = vals.t()
        return buf.view(-1), 1, rows + pad
    assert fast == "2"
    buf = nan_filled(rows * 2 * K).view(rows, K, 2)
    buf[:, :, 0] = vals
    return buf.view(-1), 2 * K, 2


GEMM_ORIENTS = (("k", "k"), ("k", "r"), ("r", "k"), ("r", "r"))          # A k-fast / m-fast  x  B k-fast / n-fast
GEMM_F32_SHAPES = ((1, 1, 1), (7, 5, 3), (64, 64, 16), (65, 63, 17), (63, 65, 15), (129, 1, 33))
GEMM_BF16_SHAPES = ((4, 4, 4), (128, 128, 32), (132, 124, 36), (124, 132, 28), (260, 4, 68))
GEMM_SCALAR_EPILOGUE = ((8, 7, 32, 7), (132, 37, 64, 37), (8, 8, 32, 11), (8, 8, 32, 16))          # (M, N, K, ldc): the last takes the vector epilogue
GEMM_EPILOGUE_SHAPES = {"f32": ((65, 63, 17), (132, 124, 36)), "bf16x3": ((132, 124, 36),)}
# (M, N, K) -> math -> (splits, kper, launched, k of the last split); None: the split-bf16 kernels do not take the shape
GEMM_SPLIT_TABLE = {
    (8, 8, 256): {"f32": (2, 128, 2, 128), "bf16x3": (2, 128, 2, 128)},
    (5, 7, 257): {"f32": (2, 144, 2, 113), "bf16x3": None},
    (8, 8, 264): {"f32": (2, 144, 2, 120), "bf16x3": (2, 160, 2, 104)},
    (65, 63, 273): {"f32": (2, 144, 2, 129), "bf16x3": None},
    (132, 68, 516): {"f32": (4, 144, 4, 84), "bf16x3": (4, 160, 4, 36)},
    (8, 8, 2080): {"f32": (16, 144, 15, 64), "bf16x3": (16, 160, 13, 160)},
}
GEMM_UNSPLIT = (64, 64, 255)
# (R, N, K, with_db) -> (splits, rows per split, rows of the last split)
TN_CASES = {
    (1, 4, 4, 1): (1, 32, 1), (31, 4, 8, 0): (1, 32, 31), (33, 36, 20, 1): (1, 64, 33), (300, 5, 7, 1): (2, 160, 140),
    (257, 68, 132, 1): (2, 160, 97), (600, 65, 64, 1): (3, 224, 152), (1000, 160, 36, 0): (4, 256, 232), (2049, 36, 20, 1): (9, 256, 1),
}
TN_EMPTY = (131073, 4, 4, 1)          # the cap of 512 splits of 288 rows: the last 56 own no rows
COL_SUM_R = {1: 1, 5: 1, 512: 1, 513: 2, 1030: 3, 2049: 5}          # R -> splits of hpfg_col_sum2
COL_SUM_M = (1, 64, 65, 129)
COL_SUM_CAP = (131073, 4, 256)                                        # R, M, splits: the cap
RELU_BWD_N = (1, 255, 257, 4099)


@functools.lru_cache(maxsize=None)
def tn_case(R, N, K):
    """dY [R,N], X [R,K] (float32, read-only), the laws dW = dY^T X and db = column sums of dY, and the tolerances: dW by the split-bf16
    rule, db by bound_8x against torch's float32 sum."""
    g = torch.Generator().manual_seed(7 * R + 131 * N + K)
    dy, x = chan_affine((R, N), 0, g), chan_affine((R, K), 0, g)
    dw, db = dy.double().t() @ x.double(), dy.double().sum(0)
    tol_dw = gemm_tolerance("bf16x3", dw, dy.t() @ x, _prod3(dy.t().contiguous(), x))
    return dict(dy=dy, x=x, dw=dw, db=db, tol_dw=tol_dw, tol_db=bound_8x(db, dy.sum(0)), old_dw=bound_8x(dw, dy.t() @ x, 64.0))


def tn_mutant(c, mutation, per):
    """-> (dW, db) of a wrong variant: db from the first 64-wide n-tile only, or the rows of the last split (from (S - 1) * per on) left out"""
    assert mutation in TN_MUTATIONS, mutation
    dy, x = c["dy"].double(), c["x"].double()
    if mutation == "db_first_tile_only":
        db = c["db"].clone()
        db[64:] = 0
        return c["dw"], db
    r = (-(-dy.shape[0] // per) - 1) * per
    return dy[:r].t() @ x[:r], dy[:r].sum(0)


def relu_bwd_case(n):
    """y with 0.0, -0.0, a denormal, a negative value, +inf and NaN among random values, dy random: -> (y, dy, dy if y > 0 else 0) float32"""
    g = torch.Generator().manual_seed(n)
    y, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -1.5, float("inf"), float("nan")])[:n]
    y[torch.randperm(n, generator=g)[:len(special)]] = special
    return y, dy, torch.where(y > 0, dy, torch.zeros_like(dy))


POOL_MUTATIONS = ("bin_end_floor", "gap_mean_of_bin_means", "bwd_divides_by_hw")
# (N, H, W, C, S, pstride)
POOL_CASES = ((2, 8, 8, 4, 4, 4), (2, 7, 5, 3, 4, 3), (1, 4, 4, 5, 4, 8), (2, 9, 6, 260, 2, 260), (1, 5, 7, 257, 3, 257), (1, 6, 6, 1024, 1, 1024),
              (1, 70, 66, 4, 2, 4), (3, 14, 14, 256, 4, 256))


def pool_bins(L_, S, mutation=None):
    """AdaptiveAvgPool's bins of an extent L_: [floor(i L / S), ceil((i + 1) L / S))"""
    if mutation == "bin_end_floor":
        return [(i * L_ // S, max((i + 1) * L_ // S, i * L_ // S + 1)) for i in range(S)]
    return [(i * L_ // S, -(-(i + 1) * L_ // S)) for i in range(S)]


def neck_pool_f64(x, S, mutation=None):
    """x [N,H,W,C] -> (gap [N,C] = the mean over the image, pool [N,S*S,C] = the mean over bin (by, bx) at index by S + bx), float64"""
    x = x.double()
    N, Hh, W, C_ = x.shape
    pool = torch.stack([x[:, y0:y1, x0:x1].mean((1, 2)) for y0, y1 in pool_bins(Hh, S, mutation) for x0, x1 in pool_bins(W, S, mutation)], 1)
    gap = pool.mean(1) if mutation == "gap_mean_of_bin_means" else x.mean((1, 2))
    return gap, pool


def neck_pool_bwd_f64(dgap, dpool, N, Hh, W, C_, S, mutation=None):
    """dx [N,H,W,C] = dgap / (H W) + sum over the bins that hold the pixel of dpool / bin size; either gradient may be None"""
    dx = torch.zeros(N, Hh, W, C_, dtype=torch.float64)
    if dgap is not None:
        dx += dgap.double()[:, None, None, :] / (Hh * W)
    if dpool is not None:
        b = 0
        for y0, y1 in pool_bins(Hh, S):
            for x0, x1 in pool_bins(W, S):
                size = Hh * W if mutation == "bwd_divides_by_hw" else (y1 - y0) * (x1 - x0)
                dx[:, y0:y1, x0:x1] += dpool.double()[:, b, None, None, :] / size
                b += 1
    return dx


@functools.lru_cache(maxsize=None)
def pool_case(N, Hh, W, C_, S):
    """x, dgap, dpool (float32, read-only), the forward and backward laws, torch's float32 adaptive_avg_pool2d and its autograd"""
    g = torch.Generator().manual_seed(10007 * Hh + 101 * W + C_ + S + N)
    x, dgap, dpool = chan_affine((N, Hh, W, C_), 0, g), chan_affine((N, C_), 0, g), chan_affine((N, S * S, C_), 0, g)
    gap, pool = neck_pool_f64(x, S)
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    g32, p32 = F.adaptive_avg_pool2d(xn, 1), F.adaptive_avg_pool2d(xn, S)
    c = dict(x=x, dgap=dgap, dpool=dpool, gap=gap, pool=pool, gap32=g32.detach().reshape(N, C_), pool32=p32.detach().reshape(N, C_, S * S).transpose(1, 2))
    for which, (a, b) in dict(gap=(dgap, None), pool=(None, dpool), both=(dgap, dpool)).items():
        out = sum(t for t in ((g32.reshape(N, C_) * a).sum() if a is not None else None,
                              (p32.reshape(N, C_, S * S).transpose(1, 2) * b).sum() if b is not None else None) if t is not None)
        c["dx_" + which] = neck_pool_bwd_f64(a, b, N, Hh, W, C_, S)
        c["dx32_" + which] = torch.autograd.grad(out, xn, retain_graph=True)[0].permute(0, 2, 3, 1)
    return c


L2NORM_MUTATIONS = ("eps_added_to_norm", "bwd_without_projection")
L2NORM_CASES = ((3, 5, 1), (2, 64, 3), (2, 65, 7), (5, 128, 16), (1, 200, 1))          # (G, D, S)
L2NORM_LAYOUTS = ("ds", "sd")          # memory [G][D][S]: (sd, ss) = (S, 1);  memory [G][S][D]: (sd, ss) = (1, D)
L2NORM_EPS = 1e-12


def l2norm_f64(x, mutation=None):
    """F.normalize(x, dim=1) of x [G,D,S] -> (u, norms [G,S]), norms = max(||x||_2 over D, 1e-12)"""
    x = x.double()
    nrm = torch.sqrt((x * x).sum(1))
    if mutation == "eps_added_to_norm":
        return x / (nrm + L2NORM_EPS)[:, None], nrm + L2NORM_EPS
    nrm = nrm.clamp(min=L2NORM_EPS)
    return x / nrm[:, None], nrm


def l2norm_bwd_f64(du, u, norms, scale=1.0, mutation=None):
    """dx = scale (du - u <u, du>) / norm per (g, s) column.  (Where the clamp holds, u = 0 and this is scale du / 1e-12: the gradient of
    x / 1e-12.)"""
    du, u = du.double(), u.double()
    dot = 0.0 if mutation == "bwd_without_projection" else (u * du).sum(1, keepdim=True)
    return scale * (du - u * dot) / norms.double()[:, None]


def l2norm_layout(t, layout):
    """logical [G,D,S] -> the flat memory image of that layout (and back with l2norm_unlayout)"""
    return (t if layout == "ds" else t.permute(0, 2, 1)).contiguous().view(-1)


def l2norm_unlayout(flat, G, D, S, layout):
    return flat.view(G, D, S) if layout == "ds" else flat.view(G, S, D).permute(0, 2, 1)


L2NORM_SPECIAL = (None, "zero", "tiny")


@functools.lru_cache(maxsize=None)
def l2norm_case(G, D, S, special=None):
    """x, du [G,D,S] float32 (read-only); laws u, norms, dx (scale 1; dx is linear in scale); torch's float32 F.normalize and its autograd.
    special: column (0, :, 0) of x is zero (the clamp's case: u = 0, norm = 1e-12, dx = du / 1e-12) or has the norm 3e-12 (just above the
    clamp, where x / (norm + eps) is a quarter short); that column's gradient is 1e12 times the others', so it is compared on its own."""
    assert special in L2NORM_SPECIAL
    g = torch.Generator().manual_seed(97 * G + 13 * D + S)
    x, du = chan_affine((G, S, D), 0, g).permute(0, 2, 1).contiguous(), torch.randn(G, D, S, generator=g)
    if special == "zero":
        x[0, :, 0] = 0.0
    elif special == "tiny":
        x[0, :, 0] *= float(3e-12 / torch.sqrt((x[0, :, 0].double() ** 2).sum()))
    u, norms = l2norm_f64(x)
    xr = x.clone().requires_grad_(True)
    u32 = F.normalize(xr, dim=1)
    dx32 = torch.autograd.grad((u32 * du).sum(), xr)[0]
    n32 = torch.linalg.vector_norm(x, dim=1).clamp(min=L2NORM_EPS)
    return dict(x=x, du=du, u=u, norms=norms, dx=l2norm_bwd_f64(du, u, norms), u32=u32.detach(), norms32=n32, dx32=dx32, special=special)


def l2norm_parts(c, t):
    """t [G,D,S] or [G,S] of an l2norm_case -> the parts compared on their own: [t] or, with a special column, [that column, the rest]"""
    if c["special"] is None:
        return [t]
    keep = torch.ones(t.shape[0], t.shape[-1], dtype=torch.bool)
    keep[0, 0] = False
    cols = t.permute(0, 2, 1) if t.dim() == 3 else t          # [G,S,D] or [G,S]
    return [p for p in (cols[0, 0], cols[keep]) if p.numel()]


NTXENT_MUTATIONS = ("diagonal_in_denominator", "positive_without_wrap", "mean_over_n_rows", "q_without_transpose")
NTXENT_N = (1, 2, 3, 32, 127, 128)
NTXENT_T = ((0.7, 16), (0.07, 1))          # (temperature, S): rows of S unit pieces, Gram diagonal S
NTXENT_FAMILIES = ("independent", "near_copy", "nonsymmetric")


def ntxent_f64(G, n, T, mutation=None, dtype=torch.float64):
    """NT-Xent from the Gram matrix G [2n,2n] of [student ; teacher] rows, read as stored: E = exp(G / T) with the diagonal masked out,
    denom_i = sum_j E_ij, p(i) = (i + n) mod 2n, loss = mean_i (log denom_i - G[i,p(i)] / T);  dL/dG_ij = (E_ij / denom_i - [j = p(i)]) / (2n T)
    and Q = (dL/dG + its transpose)[:n].  -> (loss, Q [n,2n], largest term max_i max(|log denom_i|, |G[i,p(i)]| / T)).  dtype=torch.float32:
    the yardstick (diagonal excluded by masking, as the reference's masked_select: sum - diagonal cancels to 0 at S = 16).  T is the float32
    the kernel is handed."""
    assert mutation is None or mutation in NTXENT_MUTATIONS, mutation
    m = 2 * n
    G = G.to(dtype)
    Tt = torch.tensor(f32_exact(T), dtype=dtype)
    eye = torch.eye(m, dtype=torch.bool)
    E = torch.exp(G / Tt)
    if mutation != "diagonal_in_denominator":
        E = E.masked_fill(eye, 0.0)
    denom = E.sum(1)
    i = torch.arange(m)
    p = (i + n) % m
    if mutation == "positive_without_wrap":          # the flat index i m + i + n: past the row for the teacher rows, past the matrix for the last
        pos = torch.cat([G.reshape(-1), torch.zeros(m, dtype=dtype)])[i * m + i + n]
    else:
        pos = G[i, p]
    rows = torch.log(denom) - pos / Tt
    count = n if mutation == "mean_over_n_rows" else m
    loss = rows.sum() / count
    P = torch.zeros(m, m, dtype=dtype)
    P[i, p] = 1.0
    D = (E.masked_fill(eye, 0.0) / denom[:, None] - P) / (count * Tt)
    Q = D[:n] if mutation == "q_without_transpose" else (D + D.t())[:n]
    return loss, Q, float(torch.maximum(torch.log(denom).abs(), (pos / Tt).abs()).max())


def ntxent_tolerance(law, yard):
    """(loss bound, Q bound): the loss is a difference of terms as large as S / T, so its floor is 4 float32 ulp of the largest term, not of
    the result; Q by bound_8x."""
    return max(8.0 * abs(float(yard[0]) - float(law[0])), 4.0 * ulp32(law[2])), bound_8x(law[1], yard[1])


def _unit_rows(rows, S):
    """[r, S, d] -> [r, S d] with every piece of d elements normalised (float64)"""
    rows = rows.double()
    return (rows / torch.sqrt((rows * rows).sum(-1, keepdim=True))).reshape(rows.shape[0], -1)


@functools.lru_cache(maxsize=None)
def ntxent_case(family, n, T, S, d=8):
    """The Gram matrix (built in float64 from normalised rows, rounded once to float32), the law, the float32 yardstick and the tolerances.
    independent: teacher rows drawn apart from the student's (loss of order log 2n).  near_copy: teacher = student + 1e-3 randn (loss near
    0).  nonsymmetric: independent rows, then every element of the matrix perturbed on its own at the 1e-3 level."""
    g = torch.Generator().manual_seed(1000 * n + 10 * S + NTXENT_FAMILIES.index(family))
    a = torch.randn(n, S, d, generator=g, dtype=torch.float64)
    b = a + 1e-3 * torch.randn(n, S, d, generator=g, dtype=torch.float64) if family == "near_copy" else torch.randn(n, S, d, generator=g, dtype=torch.float64)
    U = torch.cat([_unit_rows(a, S), _unit_rows(b, S)])
    G = U @ U.t()
    if family == "nonsymmetric":
        G = G * (1.0 + 1e-3 * torch.randn(2 * n, 2 * n, generator=g, dtype=torch.float64))
    G = G.float()
    law, yard = ntxent_f64(G, n, T), ntxent_f64(G, n, T, dtype=torch.float32)
    return dict(G=G, n=n, T=T, law=law, yard=yard, tol=ntxent_tolerance(law, yard))


DENSE_N = (1, 3, 32)
DENSE_D, DENSE_S = 24, 4          # feature width and positions of the dense branch ([n, D] global and [n, D, S] dense features)


@functools.lru_cache(maxsize=None)
def dense_case(n, T=0.7):
    """Student and teacher features (g [n,D], d [n,D,S], float32), float64 autograd of oracle.losses_ref.dense_loss (value, dg, dd), the same
    in float32, and the largest term of the two NT-Xent sums (for the value's floor)."""
    from oracle import losses_ref
    gen = torch.Generator().manual_seed(555 + n)
    sg, sd_ = chan_affine((n, DENSE_D), 0, gen), chan_affine((n, DENSE_S, DENSE_D), 0, gen).permute(0, 2, 1).contiguous()
    tg, td = chan_affine((n, DENSE_D), 0, gen), chan_affine((n, DENSE_S, DENSE_D), 0, gen).permute(0, 2, 1).contiguous()
    out = {}
    for dt in (torch.float64, torch.float32):
        a, b = sg.to(dt).requires_grad_(True), sd_.to(dt).requires_grad_(True)
        v = losses_ref.dense_loss((a, b), (tg.to(dt), td.to(dt)), T)
        out[dt] = (v.detach(),) + tuple(t.detach() for t in torch.autograd.grad(v, (a, b)))
    top = 0.0
    for s, t in ((sg[:, :, None], tg[:, :, None]), (sd_, td)):
        U = torch.cat([l2norm_f64(s)[0].flatten(1), l2norm_f64(t)[0].flatten(1)])
        top = max(top, ntxent_f64((U @ U.t()), n, T)[2])
    return dict(sg=sg, sd=sd_, tg=tg, td=td, ref=out[torch.float64], yard=out[torch.float32], top=top)


# ---- the first conv and the stand-alone backward kernels (tests/test_gpu_standalone_edges.py, tests/test_standalone_laws_host.py) --------
# conv_first_kernel / conv_first_mfma_kernel (csrc/conv.hip), upsample_bwd_kernel, pool_scatter_kernel, dropout_mask_kernel (csrc/misc.hip),
# channel_sum_stage1 / 2, slab_reduce_multi_kernel (csrc/wgrad.hip), bn_bwd_reduce_kernel, bn_bwd_reduce_pool_kernel (csrc/bn.hip).
# One rule: max |got - ref| / bound <= 1 against a float64 restatement, the bound (n + 2) * 2^-24 * sum|term| of a sum of n fp32 terms formed
# in exact fp32 (one more rounding where the result is rounded once more to float).  Every law takes `mutation`: a named wrong variant that
# tests/test_standalone_laws_host.py shows to lie at least 4 bounds off on some case below.
STANDALONE_MUTATIONS = {
    "first": ("halo_not_zero", "second_tile_skipped", "stats_over_partial_tiles", "taps_transposed"),
    "upbwd": ("window_one_short", "last_xcd_span_dropped", "sums_of_first_trip_only"),
    "chansum": ("idle_rows_not_zero", "last_trip_dropped"),
    "slab": ("slab_lane_16_dropped", "pad_rows_included", "scalar_path_quad_tail_dropped"),
    "poolbwd": ("last_max_wins", "slope_from_dA_sign"),
}


def _cdiv(a, b):
    return -(-a // b)


def mutation_ratio(got, ref, bound):
    """largest |got - ref| / bound; an element that is not finite, or that differs where the bound is 0 (a bit-for-bit output), counts as inf"""
    d = (got.double() - ref.double()).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(d, float(bound))
    r = torch.where(d > 0, d / b, torch.zeros_like(d))
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(r.max())


# -- 1. first conv forward.  (N, H, W, cin); statistics are requested wherever the launcher admits them (whole 16 x 16 tiles)
FIRST_FWD_SHAPES = ((2, 16, 16), (1, 32, 48), (1, 1, 1), (1, 5, 40), (2, 17, 31))      # one tile an image | 6 tiles | partial tiles, H below the tile
FIRST_FWD_WALK = ((33, 32, 256, (1, 3)), (23, 40, 250, (1, 2)))                        # 1056 whole / 1104 partial tiles on 1024 workgroups
FIRST_FWD_CASES = ([(n, h, w, c) for n, h, w in FIRST_FWD_SHAPES for c in (1, 2, 3, 4)] +
                   [(n, h, w, c) for n, h, w, cs in FIRST_FWD_WALK for c in cs])
FIRST_FWD_LAYOUT_SHAPES = ((2, 17, 31), (2, 16, 16))
FIRST_FWD_INF = (1, 32, 48)
FIRST_FWD_INF_AT = ((5, 16), (20, 15), (0, 0))      # column 0 of the tile at x0 = 16 | the halo column of that tile (LDS offset 0 of its rows, which the
#                                                     padding k-steps of the matrix-core form address) | the image's first pixel
FIRST_FWD_REFUSED_STATS = (2, 24, 32)               # statistics over partial tiles: refused by the launcher (stats_over_partial_tiles)
FIRST_GRID_CAP = 1024


def first_fwd_geometry(N, H, W):
    """conv_first_grid (csrc/conv.hip): (workgroups = rows of partial sums, tiles)"""
    nwork = N * _cdiv(H, 16) * _cdiv(W, 16)
    return min(nwork, FIRST_GRID_CAP), nwork


def first_fwd_stats(H, W):
    return H % 16 == 0 and W % 16 == 0


def first_fwd_f64(x, w, b, mutation=None):
    """x [N,H,W,cin] float64, w [16,cin,3,3], b [16] -> the float64 convolution [N,H,W,16] (conv_ref_bound's reference), or a wrong variant"""
    w64, xn = w.double(), nchw(x)
    if mutation == "taps_transposed":
        w64 = w64.transpose(-1, -2)
    if mutation == "halo_not_zero":
        out = F.conv2d(F.pad(xn, (1, 1, 1, 1), mode="replicate"), w64, b.double())
    else:
        out = F.conv2d(xn, w64, b.double(), padding=1)
    out = out.permute(0, 2, 3, 1).contiguous()
    if mutation == "second_tile_skipped":
        N, H, W, C_ = out.shape
        assert first_fwd_stats(H, W)
        grid, nwork = first_fwd_geometry(N, H, W)
        t = out.reshape(N, H // 16, 16, W // 16, 16, C_).permute(0, 1, 3, 2, 4, 5).reshape(nwork, 16, 16, C_).clone()
        t[grid:] = t[:nwork - grid]          # tile wk >= grid keeps what its workgroup computed for tile wk - grid
        out = t.reshape(N, H // 16, W // 16, 16, 16, C_).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, C_).contiguous()
    return out


def first_sums_f64(x, w, b, mutation=None):
    """(sum z, sum z^2) [2][16] in float64 and their bound (n + 2) * 2^-24 * sum|term| (fwd_sums_ratio's); stats_over_partial_tiles: summed over
    the whole 16 x 16 tiles of the zero-padded image, the pixels outside the image included"""
    N, H, W, _ = x.shape
    z = first_fwd_f64(x, w, b).reshape(-1, 16)
    n = z.shape[0]
    bound = torch.stack([(n + 2) * U24 * t.abs().sum(0) for t in (z, z * z)])
    if mutation == "stats_over_partial_tiles":
        xp = F.pad(x, (0, 0, 0, _cdiv(W, 16) * 16 - W, 0, _cdiv(H, 16) * 16 - H))
        z = first_fwd_f64(xp, w, b).reshape(-1, 16)
    return torch.stack([z.sum(0), (z * z).sum(0)]), bound


@functools.lru_cache(maxsize=None)
def first_fwd_case(N, H, W, cin):
    """CPU data of a FIRST_FWD_CASES entry: input x [N,H,W,cin] (float32), weights, float64 reference and bound (no split term), the ratio
    torch float32 reaches.  Read-only."""
    seed = case_seed("firstfwd", N, H, W, cin)
    x = conv_source("plain", seed, N, H, W, cin)["z"]
    w, b = adhoc_weights(cin, 16, 9, seed)
    ref, bound = conv_ref_bound(x.double(), torch.zeros(N, H, W, cin, dtype=torch.float64), w, b, split=False)
    return dict(x=x, w=w, b=b, ref=ref, bound=bound, f32=f32_conv_ratio("conv", ref, bound, x.double(), w, b), seed=seed)


# -- 2. hpfg_upsample2x_bwd(_sums).  (N, Hl, Wl, C)
UPB_MAXDIM = 512
UPBWD_SA_CASES = ((1, 1, 1, 4), (2, 1, 7, 8), (2, 7, 1, 8), (2, 2, 2, 4),
                  (1, 5, 6, 12), (1, 3, 3, 260),            # C/4 does not divide 256: the plain entry works, _sums refuses
                  (1, 9, 7, 256),
                  (1, 1, 511, 4), (1, 511, 1, 4),           # Hl + Wl == 512: the last admitted tap table
                  (1, 16, 30, 16),                          # 1920 quads, 8 workgroups: one per XCD, the last span short
                  (1, 13, 25, 48),                          # 3900 quads, 16 workgroups: two per XCD span (C/4 = 12: no sums)
                  (1, 20, 23, 20),                          # 2300 quads, 9 workgroups: not a multiple of 8, the linear path (C/4 = 5: no sums)
                  (3, 64, 64, 128))                         # 393 216 quads on the capped grid of 1024: one and a half trips per workgroup
UPBWD_REFUSED = (1, 2, 511, 4)                              # Hl + Wl == 513
UPBWD_SUMS_C = (4, 8, 16, 48, 64, 128, 256)                 # 48: 256 % 12 != 0, refused
UPBWD_SUMS_CASES = tuple((2, 6, 5, c) for c in UPBWD_SUMS_C) + UPBWD_SA_CASES      # every case goes through both entries


def upbwd_sums_admitted(C_):
    """the launcher's rule for channel sums (hpfg_upsample2x_bwd_sums)"""
    return C_ % 4 == 0 and 4 <= C_ <= 256 and 256 % (C_ // 4) == 0


def upbwd_geometry(N, Hl, Wl, C_):
    """hpfg_upsample2x_bwd_blocks and the XCD split of upsample_bwd_kernel: dict(total quads, blocks, nxcd, gx = workgroups per XCD span,
    span = quads per XCD in whole 256-thread rows, trips = the most trips a workgroup's loop takes)"""
    total = N * Hl * Wl * (C_ // 4)
    blocks = min(max(_cdiv(total, 256), 1), 1024)
    nxcd = 8 if blocks % 8 == 0 else 1
    span = _cdiv(_cdiv(total, nxcd), 256) * 256
    gx = blocks // nxcd
    return dict(total=total, blocks=blocks, nxcd=nxcd, gx=gx, span=span, trips=_cdiv(_cdiv(min(span, total), 256), gx))


def upbwd_trip_of(geo):
    """trip index (0, 1, ..) of the workgroup loop in which every flat output quad i = pixel * C/4 + quad is produced, and its XCD"""
    i = torch.arange(geo["total"])
    xcd = i // geo["span"]
    return ((i - xcd * geo["span"]) // 256) // geo["gx"], xcd


def upbwd_mutant(g, mutation, geo):
    """upbwd_f64's value with one thing wrong.  window_one_short: the gather window of hpfg_up_taps runs over outputs 2 lo - 2 .. 2 lo + 4, of
    which 2 lo + 2 is the last that ever carries weight (up2x_window_reach) -- the variant loses that one.  last_xcd_span_dropped: the quads
    of the eighth XCD span are never written (0)."""
    (my, _), (mx, _) = up2x_matrix(g.shape[1] // 2), up2x_matrix(g.shape[2] // 2)
    if mutation == "window_one_short":
        for m in (my, mx):
            for lo in range(m.shape[1]):
                if 2 * lo + 2 < m.shape[0]:
                    m[2 * lo + 2, lo] = 0.0
    d = torch.einsum("yi,nyxc,xj->nijc", my, g.double(), mx)
    if mutation == "last_xcd_span_dropped" and geo["nxcd"] == 8:
        _, xcd = upbwd_trip_of(geo)
        q = d.reshape(-1, 4).clone()
        q[xcd == 7] = 0.0
        d = q.reshape(d.shape)
    return d


def up2x_window_reach(Lo):
    """largest o - 2 lo over the outputs o that read source index lo with the law's fp32 weights (up2x_matrix)"""
    m, _ = up2x_matrix(Lo)
    o, lo = torch.nonzero(m, as_tuple=True)
    return int((o - 2 * lo).max()), int((o - 2 * lo).min())


def upbwd_sums_f64(dU, geo, mutation=None):
    """channel sums [C] of dU [N,Hl,Wl,C] in float64 and the bound (n + 2) * 2^-24 * sum|dU|, n = N Hl Wl.  sums_of_first_trip_only: a
    workgroup's sums forget every trip of its loop but the first"""
    dU = dU.double()
    C_ = dU.shape[-1]
    n = dU.numel() // C_
    bound = (n + 2) * U24 * dU.abs().reshape(-1, C_).sum(0)
    if mutation == "sums_of_first_trip_only":
        trip, _ = upbwd_trip_of(geo)
        dU = torch.where((trip == 0).reshape(-1, C_ // 4, 1), dU.reshape(-1, C_ // 4, 4), torch.zeros((), dtype=torch.float64))
    return dU.reshape(-1, C_).sum(0), bound


@functools.lru_cache(maxsize=None)
def upbwd_case(N, Hl, Wl, C_):
    """gradient g [N,2Hl,2Wl,C] (float32), float64 law and bound of upbwd_f64, the ratio of the same law in float32.  Read-only."""
    gen = torch.Generator().manual_seed(case_seed("upbwd", N, Hl, Wl, C_))
    g = torch.randn(N, 2 * Hl, 2 * Wl, C_, generator=gen)
    ref, bound = upbwd_f64(g)
    (my, _), (mx, _) = up2x_matrix(Hl), up2x_matrix(Wl)
    f32 = torch.einsum("yi,nyxc,xj->nijc", my.float(), g, mx.float())
    bound = torch.clamp(bound, min=1e-300)
    return dict(g=g, ref=ref, bound=bound, f32=float(((f32.double() - ref).abs() / bound).max()))


# -- 3. hpfg_channel_sum_partials / hpfg_channel_sum.  (npix, C, pstride)
CHANSUM_CASES = ((1, 4, 4), (7, 16, 16),                    # smallest vector cases
                 (1000, 12, 12),                            # 3 quads, 85 pixel lanes, one thread idle
                 (300, 256, 256),                           # 4 pixel lanes
                 (5000, 16, 24),                            # a slice of a wider buffer, vector path
                 (5000, 16, 18),                            # stride not a multiple of 4: the scalar path with C % 4 == 0
                 (5000, 1, 1), (5000, 2, 2), (5000, 3, 3), (5000, 5, 5), (5000, 9, 9), (5000, 255, 255),      # scalar path: the engine's class counts
                 (8197, 256, 256),                          # second trip of the 4x-unrolled vector loop on the capped grid of 512
                 (65539, 2, 2),                             # second trip of the scalar loop
                 (100, 64, 64))                             # 25 workgroups, 7 with pixels: 18 rows of zeros
CHANSUM_OFFSET = (999, 16, 20, 2)                           # npix, C, pstride, base offset in floats: the vector path at a 4-byte-aligned address
CHANSUM_IDLE = (100, 64, 64)


def chansum_geometry(npix, C_, pstride):
    """hpfg_channel_sum_blocks (sized by 256 / C pixel lanes) and what channel_sum_stage1 does with it: dict(blocks, vec, lanes = pixels per
    workgroup and sweep of the path taken, busy = workgroups that own a pixel, trips of the loop, sweep = pixels per trip of the launch)"""
    if C_ < 1 or C_ > 256 or npix < 1:
        return dict(blocks=0)
    blocks = min(_cdiv(npix, 256 // C_), 512)
    vec = C_ % 4 == 0 and pstride % 4 == 0
    lanes = 256 // (C_ // 4) if vec else 256 // C_
    sweep = blocks * lanes * (4 if vec else 1)
    return dict(blocks=blocks, vec=vec, lanes=lanes, busy=min(blocks, _cdiv(npix, lanes)), trips=_cdiv(npix, sweep), sweep=sweep)


def chansum_f64(g, geo, mutation=None):
    """g [npix, C] -> (float64 channel sums [C], bound (npix + 2) * 2^-24 * sum|g|).  idle_rows_not_zero: every workgroup without a pixel leaves
    a stale 1.0 per channel; last_trip_dropped: the pixels of the last trip of a loop that runs more than once are lost"""
    g = g.double()
    bound = (g.shape[0] + 2) * U24 * g.abs().sum(0)
    s = g.sum(0)
    if mutation == "idle_rows_not_zero":
        s = s + float(geo["blocks"] - geo["busy"])
    if mutation == "last_trip_dropped" and geo["trips"] > 1:
        s = g[:(geo["trips"] - 1) * geo["sweep"]].sum(0)
    return s, bound


@functools.lru_cache(maxsize=None)
def chansum_case(npix, C_, pstride, off=0):
    """buffer [off + npix * pstride] (float32; NaN pattern outside the C channels of every pixel is the caller's business: here the other
    floats are random), the interior g [npix, C], float64 sums, bound, float32 ratio.  Read-only."""
    gen = torch.Generator().manual_seed(case_seed("chansum", npix, C_, pstride, off))
    buf = torch.randn(off + npix * pstride, generator=gen)
    geo = chansum_geometry(npix, C_, pstride)
    if geo["trips"] > 1:          # the few pixels of the last trip would vanish in the summation bound of 10^4 .. 10^5 unit terms: they carry 2^12 x
        buf[off:].reshape(npix, pstride)[(geo["trips"] - 1) * geo["sweep"]:] *= 4096.0          # the amplitude (the walk_hot device)
    g = buf[off:].reshape(npix, pstride)[:, :C_]
    ref, bound = chansum_f64(g, geo)
    return dict(buf=buf, g=g, ref=ref, bound=bound, f32=float(((g.sum(0).double() - ref).abs() / bound).max()))


# -- 4. hpfg_slab_reduce_multi on synthetic slabs.  layer = (taps, Cin, CinPad, Cout, CoutPad)
SLAB_LAYERS = ((9, 3, 16, 16, 16), (1, 40, 48, 8, 16), (9, 16, 16, 5, 16)) + tuple((1, 1, 1, c, c) for c in (2, 4, 9, 16))
SLAB_S = (1, 15, 16, 17, 48, 49, 64, 65, 113)               # the edges of the `s + 48 < S` loop and of its 16-strided tail
SLAB_MIXED_S = (1, 17, 113, 113, 17, 1, 17)                 # one launch, another S per layer
SLAB_CAP_LAYERS = ((9, 128, 128, 128, 128), (1, 1, 1, 2, 2))      # per = 147 456 > 2048 * 64: the capped grid strides twice
SLAB_CAP_S = 2
SLAB_GRID_CAP = 2048


def slab_grid(layers):
    """grid x of hpfg_slab_reduce_multi and the trips its widest layer takes"""
    mx = max(t * cip * cop for t, _, cip, _, cop in layers)
    gx = min(_cdiv(mx, 64), SLAB_GRID_CAP)
    return gx, _cdiv(_cdiv(mx, 64), gx)


def slab_reduce_f64(slab, layer, mutation=None):
    """slab [S][taps][CinPad][CoutPad] -> (dw [Cout][Cin][taps] = sum_s slab[s][tap][ci][co] in float64, bound (S + 2) * 2^-24 * sum|.|).
    slab_lane_16_dropped: the last slab of each of the 16 interleaved lanes (s >= 16 * ((S - 1) // 16), S > 16) is left out; pad_rows_included:
    the entries ci >= Cin / co >= Cout are folded onto the last valid row / column; scalar_path_quad_tail_dropped: on the scalar path
    (taps * CinPad * CoutPad % 4 != 0) the elements behind the last whole quad are lost"""
    taps, cin, cip, cout, cop = layer
    s = slab.double()
    S = s.shape[0]
    bound = (S + 2) * U24 * s[:, :, :cin, :cout].abs().sum(0).permute(2, 1, 0)
    if mutation == "slab_lane_16_dropped" and S > 16:
        s = s[:16 * ((S - 1) // 16)]
    t = s.sum(0)
    per = taps * cip * cop
    if mutation == "scalar_path_quad_tail_dropped" and per % 4:
        t = t.reshape(-1).clone()
        t[per - per % 4:] = 0.0
        t = t.reshape(taps, cip, cop)
    if mutation == "pad_rows_included" and (cip > cin or cop > cout):
        t = t.clone()
        t[:, cin - 1] += t[:, cin:].sum(1)
        t[:, :, cout - 1] += t[:, :, cout:].sum(2)
    return t[:, :cin, :cout].permute(2, 1, 0).contiguous(), bound


@functools.lru_cache(maxsize=None)
def slab_case(layer, S):
    """slab [S][taps][CinPad][CoutPad] float32 with NaN in every padded entry ("nobody's result"), float64 law, bound, float32 ratio"""
    taps, cin, cip, cout, cop = layer
    gen = torch.Generator().manual_seed(case_seed("slab", *layer, S))
    slab = torch.randn(S, taps, cip, cop, generator=gen)
    slab[:, :, cin:] = NAN
    slab[:, :, :, cout:] = NAN
    ref, bound = slab_reduce_f64(slab, layer)
    f32 = slab[:, :, :cin, :cout].sum(0).permute(2, 1, 0)
    return dict(slab=slab, ref=ref, bound=bound, f32=float(((f32.double() - ref).abs() / bound).max()))


# -- 5. hpfg_bn_bwd_reduce, hpfg_bn_bwd_reduce_pool, hpfg_pool_scatter_add
BNBWD_C = (4, 8, 64, 256, 512, 1024)
BNBWD_CASES = ((1, 2, 2, 4, 0.0),                           # 4 pixels on 256 pixel lanes
               (2, 5, 7, 8, 0.3), (3, 12, 16, 64, 0.3), (2, 6, 10, 256, 0.0), (2, 3, 5, 512, 0.0),
               (2, 3, 5, 1024, 0.3))                        # one pixel lane, eight epilogue passes
POOLBWD_SHAPES = ((1, 2, 2), (2, 6, 10), (3, 12, 16))       # (N, 2 Hp, 2 Wp)
POOLBWD_CASES = tuple((n, h, w, c, False) for n, h, w in POOLBWD_SHAPES for c in BNBWD_C) + ((2, 6, 10, 8, True),)      # (.., ties on purpose)
BNBWD_REFUSED_C = (6, 12, 2048)


def bn_bwd_blocks(N, H, W, C_):
    """hpfg_bn_bwd_blocks"""
    return min(max(_cdiv(N * H * W, 256 // (C_ // 4) * 16), 1), 1024)


def bn_bwd_pool_blocks(N, Hp, Wp, C_):
    """hpfg_bn_bwd_pool_blocks"""
    return min(max(_cdiv(N * Hp * Wp, 256 // (C_ // 4) * 2), 1), 2048)


def bwd_g_f64(z, dA, tab, p=0.0, seed=0, mutation=None):
    """g = dA * keep / (1 - p) * slope(z * scale + shift): the gradient in front of the BatchNorm that the backward reductions sum (the g of
    dz_f64).  slope_from_dA_sign: the LeakyReLU slope decided by the sign of dA"""
    t, z = tab.double(), z.double()
    y = lrelu_slope(z, t[L.BN_SCALE], t[L.BN_SHIFT])
    if mutation == "slope_from_dA_sign":
        y = torch.where(dA.double() > 0, torch.ones_like(y), torch.full_like(y, 0.01))
    slope = torch.where(y == 1.0, 1.0, LEAKY32)
    return dA.double() * keep_f64(z.shape, p, seed) * slope


def bwd_sums_f64(g64, z64, tab):
    """(sum g, sum g xhat) [2][C] in float64 and the bounds of bwd_sums_ratio"""
    C_ = g64.shape[-1]
    g, z = g64.reshape(-1, C_), z64.double().reshape(-1, C_)
    n = g.shape[0]
    mean, rstd = tab[L.BN_MEAN].double(), tab[L.BN_RSTD].double()
    val = torch.stack([g.sum(0), (g * ((z - mean) * rstd)).sum(0)])
    bound = torch.stack([(n + 2) * U24 * g.abs().sum(0), (n + 4) * U24 * rstd * ((g * z).abs().sum(0) + mean.abs() * g.abs().sum(0))])
    return val, bound


@functools.lru_cache(maxsize=None)
def bnbwd_case(N, H, W, C_, p):
    """a dz source (conv_source) with its g, the sums and the ratio plain float32 sums reach.  Read-only."""
    s = conv_source("dz", case_seed("bnbwd", N, H, W, C_, p), N, H, W, C_, p)
    g64 = bwd_g_f64(s["z"], s["dA"], s["tab"], p, s["dseed"])
    val, bound = bwd_sums_f64(g64, s["z"], s["tab"])
    xh = (s["z"] - s["tab"][L.BN_MEAN]) * s["tab"][L.BN_RSTD]
    g32 = g64.float()
    f32 = torch.stack([g32.reshape(-1, C_).sum(0), (g32 * xh).reshape(-1, C_).sum(0)])
    return dict(s=s, g64=g64, val=val, bound=bound, f32=float(((f32.double() - val).abs() / bound).max()))


@functools.lru_cache(maxsize=None)
def poolbwd_case(N, H2, W2, C_, ties):
    """The layer below a max-pool at N x H2 x W2: raw output z, table, the gradient so far `base` (float32 [N,H2,W2,C]), the pooled gradient dP
    [N,H2/2,W2/2,C], `first` (pool_argmax of the activated output, every window clear of rounding ties by its guard), the completed gradient
    done = float32(base + pool_scatter_f64(dP, first)) -- a single fp32 add per element -- and its g.  ties: the BN scale row of channels 1 and
    C - 2 is 0, so all four window values are equal there and the gradient belongs to window element 0.  The seed is the first of its
    sequence for which the guards hold.  Read-only."""
    seed0 = case_seed("poolbwd", N, H2, W2, C_, int(ties))
    for seed in range(seed0, seed0 + 50):
        gen = torch.Generator().manual_seed(seed)
        z = torch.randn(N, H2, W2, C_, generator=gen) * 2 + 0.5
        tab = bn_table(C_, seed + 3)
        tied = torch.zeros(C_, dtype=torch.bool)
        if ties:
            tied[[1, C_ - 2]] = True
            tab[L.BN_SCALE][tied] = 0.0
        a, mag = _act64(z, tab[L.BN_SCALE], tab[L.BN_SHIFT])
        try:
            lrelu_slope(z.double(), tab[L.BN_SCALE].double(), tab[L.BN_SHIFT].double())
            pool_argmax(a[..., ~tied], (3.0 * U24 * mag)[..., ~tied])
        except AssertionError:
            continue
        break
    else:
        raise AssertionError("no seed clear of ties")
    first = pool_argmax(a)
    assert not ties or bool((first[..., tied] == 0).all())
    base, dP = torch.randn(N, H2, W2, C_, generator=gen), torch.randn(N, H2 // 2, W2 // 2, C_, generator=gen)
    done = (base + pool_scatter_f64(dP, first).float())
    g64 = bwd_g_f64(z, done, tab)
    val, bound = bwd_sums_f64(g64, z, tab)
    return dict(z=z, tab=tab, base=base, dP=dP, first=first, done=done, a=a, g64=g64, val=val, bound=bound, seed=seed, tied=tied)


def poolbwd_mutant(c, mutation):
    """(completed gradient float32, sums [2][C]) of a poolbwd_case with one thing wrong.  last_max_wins: among equal maxima the last window
    element takes the gradient; slope_from_dA_sign: see bwd_g_f64"""
    first = c["first"]
    if mutation == "last_max_wins":
        w = pool_windows(c["a"])
        first = torch.zeros_like(first)
        for k in (1, 2, 3):
            first = torch.where(w[k] == w.max(0).values, torch.full_like(first, k), first)
    done = c["base"] + pool_scatter_f64(c["dP"], first).float()
    g64 = bwd_g_f64(c["z"], done, c["tab"], mutation=mutation if mutation == "slope_from_dA_sign" else None)
    return done, bwd_sums_f64(g64, c["z"], c["tab"])[0]


# -- 6. hpfg_dropout_mask
DROPMASK_N = (1, 255, 257, 100003, N_BIG_MIX)
DROPMASK_P = (0.0, 0.3, 0.999)
DROPMASK_SEED = 0xDEADBEEF
DROPMASK_SEED_DEV = (0, 7, 0xFFFFFFFF)                      # seed + seed_dev wraps mod 2^32
