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
        g = torch.Generator().manual_seed(seed)
        k = 3 if taps == 9 else 1
        self.cin, self.cout, self.taps, self.k, self.dev = cin, cout, taps, k, device
        self.w = (torch.randn(cout, cin, k, k, generator=g) * 0.2).to(device)
        self.b = torch.randn(cout, generator=g).to(device)
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

    def conv(self, a0, a1, N, H, W, stats=False, dgrad=False, math=0, stat_acc=None, shards=1, bwd_stats=0, bwd_of=None):
        """stat_acc / shards: with stats=True the BatchNorm sums ALSO go into this zeroed accumulator (HpfgConvArgs.stat_acc), next to the rows
        of partial sums.  bwd_stats / bwd_of: the dgrad epilogue's backward sums (HpfgConvArgs.bwd_stats).  self.rows = rows the launch wrote."""
        lib = L.load()
        cout = self.cin if dgrad else self.cout
        cpad = self.cin_pad if dgrad else self.cout_pad
        out = torch.full((N, H, W, cout), float("nan"), device=self.dev)
        ca = L.ConvArgs()
        ca.a0, ca.a1 = a0, (a1 if a1 is not None else L.Act())
        ca.math = math
        if math == L.MATH_BF16X3:
            assert lib.hpfg_conv_kc(H, W, self.taps) == self.kc, "AdHocConv was packed for a different tile class"
            ca.wpk = L.ptr(self.wpk16_d if dgrad else self.wpk16_f)
        else:
            ca.wpk = L.ptr(self.wpk_d if dgrad else self.wpk_f)
        ca.bias = None if dgrad else L.ptr(self.bias_pad)
        ca.out = L.ptr(out)
        part = None
        if stats:
            part = torch.zeros(lib.hpfg_conv_stat_blocks(N, H, W) * 2 * cpad, device=self.dev)   # unused rows stay 0
            ca.stat_partials = L.ptr(part)
            if stat_acc is not None:
                assert stat_acc.dtype == torch.int64 and stat_acc.numel() == shards * 2 * cpad * 2
                ca.stat_acc, ca.stat_shards = L.ptr(stat_acc), shards
        if bwd_stats:
            ca.bwd_stats, ca.bwd_of = bwd_stats, bwd_of
        ca.out_pstride, ca.Cout, ca.CoutPad, ca.N, ca.H, ca.W, ca.taps = cout, cout, cpad, N, H, W, self.taps
        self.rows = lib.hpfg_conv_stat_rows(C.byref(ca)) if stats else 0
        L.check(lib.hpfg_conv_fwd(C.byref(ca), stream(self.dev)), "conv_fwd")
        return out, part

    def wgrad(self, a0, a1, g, N, H, W, math=0):
        lib = L.load()
        wa = L.WgradArgs()
        wa.a0, wa.a1, wa.g = a0, (a1 if a1 is not None else L.Act()), g
        S = lib.hpfg_wgrad_splits(N, H, W, self.cin_pad, self.cout_pad, self.taps)
        slab = torch.empty(lib.hpfg_wgrad_slab_floats(N, H, W, self.cin_pad, self.cout_pad, self.taps), device=self.dev)
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
