"""GPU: the accumulator BatchNorm route (HPFG_BN_ACC=1 with bf16x3 math -- what every training step runs), kernel by kernel against float64.

A. producers: a launch that writes rows of partial sums AND adds to a sum accumulator (HpfgConvArgs.stat_acc) does both from one register
   value, so the accumulator's integer totals equal the encoded rows limb for limb, whatever the shard count; the decoded totals agree with
   float64 sums of the launch's own read-back output within the fp32 summation bound.
B. coefficients and consumers: hpfg_bn_acc_finalize / hpfg_bn_acc_bwd_finalize against exact rational / float64 references, and every consumer
   prologue (HpfgAct.bn_acc) against the same kernel reading the table rows the finalize wrote: bit-equal outputs.
C. the overflow bound of the accumulator words.

Every exact assertion is integer equality or torch.equal; every tolerance is computed from the data by the bound stated beside it.  Each
group prints its largest error / bound ratio (pytest -s)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hpfg_amd import _lib as L
from hpfg_amd.engine import DescTable
from tests.helpers import AdHocConv, acc_decode, acc_from_rows, acc_rows_totals, acc_totals, lrelu_slope, maxerr, nchw, plain_act, stream
from tests.test_gpu_fused_bwd import _bnact, _dz
from tests.test_gpu_kernels import _bn_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U32 = 2.0 ** -24          # unit roundoff of fp32
EPS = 1e-5
B16 = L.MATH_BF16X3
SHARDS = (1, 2, 8)


def _note(group, ratio):
    print(f"[bn_acc] {group}: largest error / bound = {float(ratio):.3g}")


def _randn(g, *shape):
    """unit-scale data of the existing BatchNorm tests"""
    return torch.randn(*shape, generator=g) * 2 + 0.5


def _zero_acc(C_, shards):
    return torch.zeros(shards * 2 * C_ * 2, dtype=torch.int64, device=DEV)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


_lrelu_slope = lrelu_slope      # (the slope with its tie guard lives in tests/helpers.py, next to the float64 restatements that share it)


# ---- A. producers --------------------------------------------------------------------------------------------------------------------
def _limb_check(tag, launch, C_, cpad=None, rows_min=9):
    """launch(shards) -> (rows [R][2][cpad] float32 CPU tensor, accumulator tensor, R) of ONE launch that wrote both.  Exact limbs, shard
    invariance; -> the totals."""
    cpad = cpad or C_
    tot = {}
    for shards in SHARDS:
        rows, acc, nrows = launch(shards)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(rows).all())
        want, got = acc_rows_totals(rows.numpy()), acc_totals(acc, cpad, shards)
        assert (got[:, :C_] == want[:, :C_]).all(), f"{tag}: accumulator limbs differ from the encoded partial rows ({shards} shards)"
        tot[shards] = got[:, :C_]
        if shards == 8:
            assert nrows >= rows_min, (tag, nrows)
            used = int((acc.cpu().view(8, -1) != 0).any(1).sum())
            assert used > 1, f"{tag}: {nrows} workgroups landed in {used} of 8 shards"
    assert (tot[1] == tot[2]).all() and (tot[1] == tot[8]).all(), f"{tag}: totals depend on the shard count"
    return tot[8]


def _fwd_sums_check(tag, out, totals):
    """decoded totals against float64 sums of the read-back output: (n + 2) * 2^-24 * sum|term| (an fp32 sum of at most n terms per workgroup;
    the limbs add nothing)"""
    z = out.detach().cpu().double().reshape(-1, out.shape[-1])
    n = z.shape[0]
    dec = acc_decode(totals)
    worst = 0.0
    for which, term in enumerate((z, z * z)):
        ref, bound = term.sum(0).numpy(), (n + 2) * U32 * term.abs().sum(0).numpy()
        ratio = np.abs(dec[which] - ref) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), f"{tag}: sum {which} off by {ratio.max():.3g} x the fp32 summation bound"
    return worst


def _bwd_sums_check(tag, g64, z64, tab, totals):
    """backward sums (sum g, sum g * xhat) against float64 from read-back gradients: (n + 2) * 2^-24 * sum|g| and
    (n + 4) * 2^-24 * rstd * (sum|g z| + |mean| sum|g|) -- the epilogues form rstd * (sum g z - mean * sum g) in fp32"""
    n = g64.shape[0]
    mean, rstd = tab[L.BN_MEAN].double(), tab[L.BN_RSTD].double()
    dec = acc_decode(totals)
    ref1, b1 = g64.sum(0), (n + 2) * U32 * g64.abs().sum(0)
    ref2 = (g64 * ((z64 - mean) * rstd)).sum(0)
    b2 = (n + 4) * U32 * rstd * ((g64 * z64).abs().sum(0) + mean.abs() * g64.abs().sum(0))
    r1 = (torch.from_numpy(dec[0]) - ref1).abs() / b1
    r2 = (torch.from_numpy(dec[1]) - ref2).abs() / b2
    assert float(r1.max()) <= 1.0 and float(r2.max()) <= 1.0, f"{tag}: backward sums off by {float(r1.max()):.3g} / {float(r2.max()):.3g} x the bound"
    return max(float(r1.max()), float(r2.max()))


@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("N,H,W", [(2, 32, 48), (9, 32, 32)])
def test_first_conv_limbs_equal_partial_rows_in_both_forms(N, H, W, cin):
    lib = L.load()
    g = torch.Generator().manual_seed(N + cin)
    x = _randn(g, N, cin, H, W).to(DEV)
    w = (torch.randn(16, cin, 3, 3, generator=g) * 0.3).to(DEV)
    b = torch.randn(16, generator=g).to(DEV)
    a = L.Act()
    a.z, a.mode, a.C, a.Hs, a.Ws = L.ptr(x), L.ACT_STRIDED, cin, H, W
    a.sn, a.sc, a.sy, a.sx = x.stride()
    nblk = lib.hpfg_conv_first_rows(N, H, W)
    outs = {}

    def launch(shards):
        out = torch.full((N, H, W, 16), float("nan"), device=DEV)
        part = torch.zeros(nblk, 2, 16, device=DEV)
        acc = _zero_acc(16, shards)
        L.check(lib.hpfg_conv3x3_first_fwd_acc(C.byref(a), L.ptr(w), L.ptr(b), L.ptr(out), L.ptr(part), L.ptr(acc), shards, N, H, W, cin, 16, stream(DEV)), "first")
        outs["out"] = out
        return part.cpu(), acc, nblk

    tot = {}
    prev = lib.hpfg_set_option(L.OPT_FIRST_MFMA, 1)
    try:
        for form in (0, 1):
            lib.hpfg_set_option(L.OPT_FIRST_MFMA, form)
            tot[form] = _limb_check(f"first conv form {form}", launch, 16)
            outs[form] = outs["out"]
    finally:
        lib.hpfg_set_option(L.OPT_FIRST_MFMA, prev)
    assert (tot[0] == tot[1]).all() and torch.equal(outs[0], outs[1])      # VALU and MFMA form: the same limbs
    assert maxerr(nchw(outs[1].cpu()), F.conv2d(x.cpu(), w.cpu(), b.cpu(), padding=1)) < 1e-4
    _note("A first conv", _fwd_sums_check("first conv", outs[1], tot[1]))


def _source(kind, g, N, H, W, cin):
    """(a0, a1, keep-alive) of a forward conv's virtual input from hand-made tables"""
    if kind == "plain":
        x = _randn(g, N, H, W, cin).to(DEV)
        return plain_act(x, cin, H, W), None, (x,)
    if kind == "bnact":
        z, tab = _randn(g, N, H, W, cin).to(DEV), _bn_table(cin, 3).to(DEV)
        return _bnact(z, tab, cin, H, W), None, (z, tab)
    if kind == "pool":
        z, tab = _randn(g, N, 2 * H, 2 * W, cin).to(DEV), _bn_table(cin, 3).to(DEV)
        return _bnact(z, tab, cin, 2 * H, 2 * W, mode=L.ACT_BNACT_POOL), None, (z, tab)
    c2 = cin // 2
    z, tab = _randn(g, N, H, W, c2).to(DEV), _bn_table(c2, 3).to(DEV)
    u = _randn(g, N, H // 2, W // 2, c2).to(DEV)
    a1 = L.Act()
    a1.z, a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = L.ptr(u), L.ACT_UP2X, c2, H // 2, W // 2, c2
    return _bnact(z, tab, c2, H, W), a1, (z, tab, u)


FWD_PRODUCERS = [  # kernel, N, H, W, cin, cout, taps, source
    ("thin", 9, 32, 48, 16, 16, 9, "bnact"),
    ("chunked", 3, 12, 20, 32, 64, 9, "plain"),
    ("chunked", 3, 12, 20, 64, 64, 9, "bnact"),
    ("chunked", 3, 12, 20, 32, 64, 9, "pool"),
    ("chunked", 3, 12, 20, 64, 32, 9, "cat"),
    ("1x1", 3, 14, 14, 128, 64, 1, "bnact"),
]


@pytest.mark.parametrize("kernel,N,H,W,cin,cout,taps,kind", FWD_PRODUCERS)
def test_forward_conv_limbs_equal_partial_rows(kernel, N, H, W, cin, cout, taps, kind):
    g = torch.Generator().manual_seed(H * 3 + cin + cout)
    layer = AdHocConv(cin, cout, taps, DEV, seed=cin + 2 * cout, hw=(H, W))
    a0, a1, keep = _source(kind, g, N, H, W, cin)
    last = {}

    def launch(shards):
        acc = _zero_acc(cout, shards)
        out, part = layer.conv(a0, a1, N, H, W, stats=True, math=B16, stat_acc=acc, shards=shards)
        last["out"] = out
        return part.view(-1, 2, cout).cpu(), acc, layer.rows

    tot = _limb_check(f"{kernel} {kind}", launch, cout)
    if kernel == "thin":
        assert layer.rows % 8 == 0      # (conv_thin_kernel launches a multiple of 8 workgroups: this IS the thin kernel)
    _note(f"A forward {kernel} {kind} {cin}->{cout}", _fwd_sums_check(f"{kernel} {kind}", last["out"], tot))


@pytest.mark.parametrize("mode", [1, 2])
def test_chunked_dgrad_backward_sums_limbs_equal_partial_rows(mode):
    """bwd_stats = 1: `out` is the complete gradient of the 64-channel layer below; 2: it is the gradient w.r.t. its max-pooled output, added
    into that layer's gradient (bwd_of.aux, twice the size) in place."""
    N, H, W, Cc = (3, 12, 20, 64) if mode == 1 else (3, 6, 10, 64)
    up = mode
    g = torch.Generator().manual_seed(40 + mode)
    layer = AdHocConv(Cc, Cc, 9, DEV, seed=5, hw=(H, W))
    zo, dAo, tabo = _randn(g, N, H, W, Cc).to(DEV), torch.randn(N, H, W, Cc, generator=g).to(DEV), _bn_table(Cc, 11).to(DEV)
    gsrc = _dz(zo, tabo, dAo, Cc, H, W)
    zi, tabi = _randn(g, N, up * H, up * W, Cc).to(DEV), _bn_table(Cc, 3).to(DEV)
    dA0 = torch.randn(N, up * H, up * W, Cc, generator=g).to(DEV)
    last = {}

    def launch(shards):
        dA = dA0.clone()
        bo = _dz(zi, tabi, dA if mode == 2 else None, Cc, up * H, up * W)
        acc = _zero_acc(Cc, shards)
        out, part = layer.conv(gsrc, None, N, H, W, stats=True, dgrad=True, math=B16, stat_acc=acc, shards=shards, bwd_stats=mode, bwd_of=bo)
        torch.cuda.synchronize()
        grad = dA if mode == 2 else out
        if "grad" in last:
            assert torch.equal(grad, last["grad"])
        last["grad"] = grad
        return part.view(-1, 2, Cc).cpu(), acc, layer.rows

    # (mode 2 at 3 x 6 x 10: 6 rows of 4 x 16-pixel tiles, in two 32-channel slices -- 12 workgroups, every shard in use)
    tot = _limb_check(f"dgrad bwd_stats={mode}", launch, Cc, rows_min=9 if mode == 1 else 6)
    if mode == 2:
        assert not torch.equal(last["grad"], dA0)
    ti = tabi.cpu()
    z64 = zi.cpu().double().reshape(-1, Cc)
    g64 = last["grad"].cpu().double().reshape(-1, Cc) * _lrelu_slope(z64, ti[L.BN_SCALE].double(), ti[L.BN_SHIFT].double())
    _note(f"A backward chunked dgrad bwd_stats={mode}", _bwd_sums_check(f"dgrad bwd_stats={mode}", g64, z64, ti, tot))


def _fused_launch(layer, xa0, gsrc, N, H, W, bwd_of=None, acc=None, shards=1, want_rows=True):
    """hpfg_fused_bwd of a BNACT-input layer -> dX, slabs, rows of backward sums (or None), workgroups"""
    lib = L.load()
    fa = L.FusedBwdArgs()
    fa.xa0, fa.xa1 = xa0, L.Act()
    fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = layer.cin, layer.cin_pad, layer.cout, layer.cout_pad
    d = fa.d
    d.a0, d.a1, d.math, d.wpk = gsrc, L.Act(), B16, L.ptr(layer.wpk16_d)
    d.Cout, d.CoutPad, d.N, d.H, d.W, d.taps = layer.cin, layer.cin_pad, N, H, W, 9
    out = torch.full((N, H, W, layer.cin), float("nan"), device=DEV)
    d.out, d.out_pstride = L.ptr(out), layer.cin
    grid = lib.hpfg_fused_bwd_grid(C.byref(fa))
    assert grid > 0, lib.hpfg_last_error()
    part = None
    if bwd_of is not None:
        d.bwd_stats, d.bwd_of = 1, bwd_of
        if want_rows:
            part = torch.zeros(grid, 2, layer.cin_pad, device=DEV)
            d.stat_partials = L.ptr(part)
        if acc is not None:
            d.stat_acc, d.stat_shards = L.ptr(acc), shards
    slab = torch.full((grid, 9, layer.cin_pad, layer.cout_pad), float("nan"), device=DEV)
    fa.slab = L.ptr(slab)
    L.check(lib.hpfg_fused_bwd(C.byref(fa), stream(DEV)), "fused_bwd")
    torch.cuda.synchronize()
    return out, slab, part, grid


def test_fused_bwd_backward_sums_limbs_equal_partial_rows():
    N, H, W, Cc = 9, 32, 32, 16
    g = torch.Generator().manual_seed(77)
    layer = AdHocConv(Cc, Cc, 9, DEV, seed=8, hw=(H, W))
    zi, tabi = _randn(g, N, H, W, Cc).to(DEV), _bn_table(Cc, 3).to(DEV)
    zo, dAo, tabo = _randn(g, N, H, W, Cc).to(DEV), torch.randn(N, H, W, Cc, generator=g).to(DEV), _bn_table(Cc, 11).to(DEV)
    xa0, gsrc, bo = _bnact(zi, tabi, Cc, H, W), _dz(zo, tabo, dAo, Cc, H, W), _dz(zi, tabi, None, Cc, H, W)
    last = {}

    def launch(shards):
        acc = _zero_acc(Cc, shards)
        out, _, part, grid = _fused_launch(layer, xa0, gsrc, N, H, W, bwd_of=bo, acc=acc, shards=shards)
        last["out"] = out
        return part.cpu(), acc, grid

    tot = _limb_check("fused_bwd", launch, Cc)
    ti = tabi.cpu()
    z64 = zi.cpu().double().reshape(-1, Cc)
    g64 = last["out"].cpu().double().reshape(-1, Cc) * _lrelu_slope(z64, ti[L.BN_SCALE].double(), ti[L.BN_SHIFT].double())
    _note("A backward fused_bwd", _bwd_sums_check("fused_bwd", g64, z64, ti, tot))


@pytest.mark.parametrize("N,H,W,Cc", [(3, 12, 16, 32), (3, 4, 4, 128)])
def test_bn_bwd_reduce_acc_limbs_equal_the_rows_of_bn_bwd_reduce(N, H, W, Cc):
    lib = L.load()
    g = torch.Generator().manual_seed(Cc + H)
    z, dA, tab = _randn(g, N, H, W, Cc).to(DEV), torch.randn(N, H, W, Cc + 8, generator=g).to(DEV), _bn_table(Cc, 9).to(DEV)
    d = _dz(z, tab, dA, Cc, H, W)
    d.aux_pstride = Cc + 8
    nblk = lib.hpfg_bn_bwd_blocks(N, H, W, Cc)
    part = torch.zeros(nblk, 2, Cc, device=DEV)
    L.check(lib.hpfg_bn_bwd_reduce(C.byref(d), N, H, W, L.ptr(part), stream(DEV)), "bn_bwd_reduce")
    want = acc_rows_totals(part.cpu().numpy())
    for shards in SHARDS:
        acc = _zero_acc(Cc, shards)
        L.check(lib.hpfg_bn_bwd_reduce_acc(C.byref(d), N, H, W, L.ptr(acc), shards, stream(DEV)), "bn_bwd_reduce_acc")
        assert (acc_totals(acc, Cc, shards) == want).all(), shards      # the same kernel: the same register values
    t = tab.cpu()
    z64 = z.cpu().double().reshape(-1, Cc)
    g64 = dA.cpu().double()[..., :Cc].reshape(-1, Cc) * _lrelu_slope(z64, t[L.BN_SCALE].double(), t[L.BN_SHIFT].double())
    _note(f"A backward bn_bwd_reduce_acc C={Cc}", _bwd_sums_check("bn_bwd_reduce_acc", g64, z64, t, want))


@pytest.mark.parametrize("N,H,W,Cc", [(3, 12, 16, 32), (9, 32, 32, 16)])
def test_bn_bwd_reduce_pool_acc_limbs_and_gradient_equal_bn_bwd_reduce_pool(N, H, W, Cc):
    lib = L.load()
    g = torch.Generator().manual_seed(Cc + W)
    z, tab = _randn(g, N, H, W, Cc).to(DEV), _bn_table(Cc, 9).to(DEV)
    dP = torch.randn(N, H // 2, W // 2, Cc, generator=g).to(DEV)
    base = torch.randn(N, H, W, Cc + 16, generator=g).to(DEV)

    def act(dA):
        a = _dz(z, tab, dA, Cc, H, W)
        a.aux_pstride = Cc + 16
        return a
    nblk = lib.hpfg_bn_bwd_pool_blocks(N, H // 2, W // 2, Cc)
    part, ref = torch.zeros(nblk, 2, Cc, device=DEV), base.clone()
    L.check(lib.hpfg_bn_bwd_reduce_pool(C.byref(act(ref)), L.ptr(dP), Cc, N, H // 2, W // 2, L.ptr(part), stream(DEV)), "reduce_pool")
    want = acc_rows_totals(part.cpu().numpy())
    for shards in SHARDS:
        acc, dA = _zero_acc(Cc, shards), base.clone()
        L.check(lib.hpfg_bn_bwd_reduce_pool_acc(C.byref(act(dA)), L.ptr(dP), Cc, N, H // 2, W // 2, L.ptr(acc), shards, stream(DEV)), "reduce_pool_acc")
        assert torch.equal(dA, ref), shards                              # the in-place max-pool backward too
        assert (acc_totals(acc, Cc, shards) == want).all(), shards
        if shards == 8 and nblk > 1:
            assert int((acc.cpu().view(8, -1) != 0).any(1).sum()) > 1
    assert not torch.equal(ref, base)
    t = tab.cpu()
    z64 = z.cpu().double().reshape(-1, Cc)
    g64 = ref.cpu().double()[..., :Cc].reshape(-1, Cc) * _lrelu_slope(z64, t[L.BN_SCALE].double(), t[L.BN_SHIFT].double())
    _note(f"A backward bn_bwd_reduce_pool_acc C={Cc}", _bwd_sums_check("bn_bwd_reduce_pool_acc", g64, z64, t, want))


# ---- B1. hpfg_bn_acc_finalize ----------------------------------------------------------------------------------------------------------
def _chunk_rows(z, nrows):
    """[nrows][2][C] float32 partial sums (sum z, sum z^2) of the pixel chunks of z [npix][C] -- what producer workgroups would add"""
    ch = torch.chunk(z, nrows, 0)
    return torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in ch]).numpy()


def _coef_ref(totals, count, gamma, beta, eps32):
    """Exact rational mean / variance of the accumulator totals, then float64: mean, var (clamped), rstd, scale, shift."""
    C_ = totals.shape[1]
    mean, var = np.empty(C_), np.empty(C_)
    for c in range(C_):
        s1 = Fraction(int(totals[0, c, 0])) + Fraction(int(totals[0, c, 1]), 2 ** 52)
        s2 = Fraction(int(totals[1, c, 0])) + Fraction(int(totals[1, c, 1]), 2 ** 52)
        m = s1 / count
        mean[c], var[c] = float(m), float(max(s2 / count - m * m, Fraction(0)))
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps32)))
    scale = gamma.double().numpy() * rstd
    return mean, var, rstd, scale, beta.double().numpy() - mean * scale


def _finalize_fwd(layers, track):
    """layers: dicts with acc, gamma, beta, rm, rv, bn, C, count, shards -> rc of one hpfg_bn_acc_finalize call"""
    descs = (L.BnAccDesc * len(layers))()
    for d, l in zip(descs, layers):
        d.acc, d.gamma, d.beta, d.bn = L.ptr(l["acc"]), L.ptr(l["gamma"]), L.ptr(l["beta"]), L.ptr(l["bn"])
        d.running_mean, d.running_var = (L.ptr(l["rm"]), L.ptr(l["rv"])) if track else (None, None)
        d.C, d.count, d.shards = l["C"], float(l["count"]), l["shards"]
    tab = DescTable(descs, DEV)
    dev, host, n = tab.sub(0, len(layers))
    rc = L.load().hpfg_bn_acc_finalize(dev, host, n, 0.1, EPS, stream(DEV))
    torch.cuda.synchronize()
    return rc


def _three_layers():
    g = torch.Generator().manual_seed(21)
    layers = []
    for C_, shards, count, nrows in [(16, 1, 1, 1), (64, 4, 192, 6), (300, 8, 48, 12)]:
        z = _randn(g, count, C_)
        if C_ == 300:
            z[:, 5] = 1.5                                   # a constant channel: variance exactly 0, rstd = 1 / sqrt(eps)
            z[:, 7] = 1.0                                   # (its sum of squares is lowered below)
        acc = acc_from_rows(_chunk_rows(z, nrows), shards)
        if C_ == 300:
            acc[0, 1, 7, 1] -= 64                           # S2 / count = 1 - 2^-46 / 48 < mean^2 = 1: must clamp to 0, not go NaN
        layers.append(dict(z=z, C=C_, shards=shards, count=count, acc_host=acc, gamma=torch.randn(C_, generator=g).to(DEV),
                           beta=torch.randn(C_, generator=g).to(DEV), rm0=torch.randn(C_, generator=g) * 0.1, rv0=torch.rand(C_, generator=g) + 0.5))
    return layers


def test_bn_acc_finalize_three_layers_against_exact_coefficients():
    layers = _three_layers()
    tables = {}
    worst = 0.0
    for track in (True, False):
        for l in layers:
            l["acc"] = l["acc_host"].clone().to(DEV)
            l["bn"] = torch.full((L.BN_ROWS, l["C"]), float("nan"), device=DEV)
            l["rm"], l["rv"] = l["rm0"].clone().to(DEV), l["rv0"].clone().to(DEV)
        assert _finalize_fwd(layers, track) == 0, L.load().hpfg_last_error()
        for i, l in enumerate(layers):
            C_, count = l["C"], l["count"]
            tot = acc_totals(l["acc_host"], C_, l["shards"])
            mean, var, rstd, scale, shift = _coef_ref(tot, count, l["gamma"].cpu(), l["beta"].cpu(), EPS)
            t = l["bn"].cpu().double().numpy()
            assert np.isfinite(t[:4]).all(), i
            for row, ref in ((L.BN_MEAN, mean), (L.BN_RSTD, rstd), (L.BN_SCALE, scale)):
                r = np.abs(t[row] - ref) / _ulp32(ref)
                worst = max(worst, float(r.max()))
                assert (r <= 1.0).all(), f"layer {i} row {row}: {r.max():.3g} ulp at channel {int(r.argmax())}"
            r = np.abs(t[L.BN_SHIFT] - shift) / _ulp32(np.maximum(np.abs(l["beta"].cpu().double().numpy()), np.abs(mean * scale)))
            worst = max(worst, float(r.max()))
            assert (r <= 1.0).all(), f"layer {i} shift: {r.max():.3g} ulp"
            assert int((l["acc"] != 0).sum()) == 0, f"layer {i}: the accumulator is not zeroed"
            if C_ == 300:
                assert var[5] == 0.0 and var[7] == 0.0
                one = 1.0 / np.sqrt(float(np.float32(EPS)))
                assert abs(t[L.BN_RSTD][5] - one) <= _ulp32(one) and abs(t[L.BN_RSTD][7] - one) <= _ulp32(one)
            if track:
                unb = var * count / (count - 1) if count > 1 else var      # count == 1: unbiased == biased
                rm_ref = 0.9 * l["rm0"].double().numpy() + 0.1 * mean
                rv_ref = 0.9 * l["rv0"].double().numpy() + 0.1 * unb
                assert np.abs(l["rm"].cpu().double().numpy() - rm_ref).max() < 1e-5 and np.abs(l["rv"].cpu().double().numpy() - rv_ref).max() < 1e-4
                if count > 1:      # float64 nn.BatchNorm2d on the data itself (not on the fp32 partial sums), natural channels
                    bn = torch.nn.BatchNorm2d(C_).double()
                    with torch.no_grad():
                        bn.running_mean.copy_(l["rm0"].double())
                        bn.running_var.copy_(l["rv0"].double())
                    bn.train()
                    bn(l["z"].double().reshape(count, C_, 1, 1))
                    nat = torch.ones(C_, dtype=torch.bool)
                    if C_ == 300:
                        nat[7] = False
                    assert maxerr(l["rm"].cpu()[nat], bn.running_mean[nat]) < 1e-5 and maxerr(l["rv"].cpu()[nat], bn.running_var[nat]) < 1e-4
            else:
                assert torch.equal(l["rm"].cpu(), l["rm0"]) and torch.equal(l["rv"].cpu(), l["rv0"])
            tables.setdefault(i, []).append(l["bn"][:4].clone())
    for i in tables:
        assert torch.equal(tables[i][0], tables[i][1])      # with or without running statistics: the same rows
    _note("B1 bn_acc_finalize rows (ulp)", worst)


def test_bn_acc_finalize_rejects_bad_descriptors():
    lib = L.load()
    g = torch.Generator().manual_seed(2)

    def layer(**kw):
        z = _randn(g, 8, 16)
        acc = acc_from_rows(_chunk_rows(z, 2), 4).to(DEV)
        d = dict(C=16, shards=4, count=8, acc=acc, gamma=torch.ones(16, device=DEV), beta=torch.zeros(16, device=DEV),
                 bn=torch.zeros(L.BN_ROWS, 16, device=DEV), rm=torch.zeros(16, device=DEV), rv=torch.ones(16, device=DEV))
        d.update(kw)
        return d
    ok = layer()
    assert _finalize_fwd([ok], True) == 0
    for what, bad in (("count", layer(count=2 ** 24 + 2)), ("shards", layer(shards=3))):
        before = bad["acc"].clone()
        rc = _finalize_fwd([layer(), bad], True)
        assert rc == -1 and len(lib.hpfg_last_error()) > 0, what
        assert torch.equal(bad["acc"], before) and int((bad["bn"] != 0).sum()) == 0, what      # nothing was launched
    # only one of the two running pointers
    bad = layer()
    descs = (L.BnAccDesc * 1)()
    d = descs[0]
    d.acc, d.gamma, d.beta, d.bn, d.running_mean, d.running_var = L.ptr(bad["acc"]), L.ptr(bad["gamma"]), L.ptr(bad["beta"]), L.ptr(bad["bn"]), L.ptr(bad["rm"]), None
    d.C, d.count, d.shards = 16, 8.0, 4
    tab = DescTable(descs, DEV)
    dev, host, n = tab.sub(0, 1)
    assert lib.hpfg_bn_acc_finalize(dev, host, n, 0.1, EPS, stream(DEV)) == -1 and b"descriptor" in lib.hpfg_last_error()
    torch.cuda.synchronize()
    assert int((bad["bn"] != 0).sum()) == 0


# ---- B2. forward consumers -------------------------------------------------------------------------------------------------------------
FWD_CONSUMERS = [  # kernel, N, H, W, source channels, cout, kind, shards, bn_coff, bn_stride
    ("thin", 2, 32, 32, 16, 16, "bnact", 8, 0, 16),
    ("thin", 2, 32, 32, 16, 16, "bnact", 8, 16, 48),      # the source's channels sit at 16 .. 31 of a 48-channel table and accumulator
    ("thin", 2, 16, 16, 16, 32, "pool", 4, 0, 16),
    ("thin", 2, 32, 32, 16, 16, "cat", 2, 0, 16),
    ("chunked", 3, 12, 20, 64, 64, "bnact", 4, 0, 64),
    ("chunked", 3, 12, 20, 32, 64, "bnact", 8, 16, 48),
    ("chunked", 3, 12, 20, 32, 64, "pool", 8, 0, 32),
    ("chunked", 3, 12, 20, 32, 32, "cat", 2, 0, 32),
]


@pytest.mark.parametrize("kernel,N,H,W,cs,cout,kind,shards,coff,stride", FWD_CONSUMERS)
def test_forward_consumer_same_bits_from_accumulator_and_from_table(kernel, N, H, W, cs, cout, kind, shards, coff, stride):
    g = torch.Generator().manual_seed(H + cs + cout + coff)
    up = 2 if kind == "pool" else 1
    Hs, Ws = up * H, up * W
    cin = 2 * cs if kind == "cat" else cs
    layer = AdHocConv(cin, cout, 9, DEV, seed=cs + cout, hw=(H, W))
    z = _randn(g, N, Hs, Ws, cs)
    gamma, beta = torch.randn(stride, generator=g), torch.randn(stride, generator=g)
    # the producer's sums as N workgroups would have left them: one fp32 partial sum per image and channel, at channels coff .. coff + cs
    rows = np.asarray(_chunk_rows(_randn(g, N * 4, stride), N))
    rows[:, :, coff:coff + cs] = _chunk_rows(z.reshape(-1, cs), N)
    acc_host = acc_from_rows(rows, shards)
    count = N * Hs * Ws
    zd, gd, bd, acc = z.to(DEV), gamma.to(DEV), beta.to(DEV), acc_host.to(DEV)
    tab = torch.full((L.BN_ROWS, stride), float("nan"), device=DEV)
    a0 = L.Act()
    a0.z, a0.bn, a0.mode, a0.C, a0.Hs, a0.Ws, a0.pstride = L.ptr(zd), L.ptr(tab), (L.ACT_BNACT_POOL if kind == "pool" else L.ACT_BNACT), cs, Hs, Ws, cs
    a0.bn_stride, a0.bn_coff = stride, coff
    a0.bn_acc, a0.bn_gamma, a0.bn_beta, a0.bn_count, a0.bn_eps, a0.bn_shards = L.ptr(acc), L.ptr(gd), L.ptr(bd), float(count), EPS, shards
    a1 = None
    if kind == "cat":
        u = _randn(g, N, H // 2, W // 2, cs)
        ud = u.to(DEV)
        a1 = L.Act()
        a1.z, a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = L.ptr(ud), L.ACT_UP2X, cs, H // 2, W // 2, cs
    out_acc, _ = layer.conv(a0, a1, N, H, W, stats=True, math=B16)
    if kernel == "thin":
        assert layer.rows % 8 == 0
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), acc_host)                      # a consumer only reads the accumulator
    fin = dict(acc=acc, gamma=gd, beta=bd, bn=tab, C=stride, count=count, shards=shards)
    assert _finalize_fwd([fin], False) == 0, L.load().hpfg_last_error()
    assert int((acc != 0).sum()) == 0
    a0.bn_acc = None
    out_tab, _ = layer.conv(a0, a1, N, H, W, stats=True, math=B16)
    torch.cuda.synchronize()
    assert torch.equal(out_acc, out_tab), f"prologue and finalize disagree: {maxerr(out_acc.cpu(), out_tab.cpu())}"
    # float64: conv2d over a host BatchNorm (batch statistics of z itself) + LeakyReLU [+ max-pool | + concat with the bilinear upsample]
    z64 = nchw(z).double()
    y = F.leaky_relu(F.batch_norm(z64, None, None, gamma[coff:coff + cs].double(), beta[coff:coff + cs].double(), training=True, eps=EPS), 0.01)
    if kind == "pool":
        y = F.max_pool2d(y, 2)
    if kind == "cat":
        y = torch.cat([y, F.interpolate(nchw(u).double(), scale_factor=2, mode="bilinear", align_corners=True)], 1)
    ref = F.conv2d(y, layer.w.cpu().double(), layer.b.cpu().double(), padding=1)
    bound = 3e-4 * float(ref.abs().max())
    err = maxerr(nchw(out_acc.cpu()), ref)
    assert err < bound, (err, bound)
    _note(f"B2 forward consumer {kernel} {kind} coff={coff}", err / bound)


# ---- B3. backward consumers ------------------------------------------------------------------------------------------------------------
def _finalize_bwd(acc, gamma, bn, C_, count, shards, dgamma=None, dbeta=None):
    descs = (L.BnAccBwdDesc * 1)()
    d = descs[0]
    d.acc, d.gamma, d.bn, d.dgamma, d.dbeta, d.C, d.count, d.shards = L.ptr(acc), L.ptr(gamma), L.ptr(bn), L.ptr(dgamma), L.ptr(dbeta), C_, float(count), shards
    tab = DescTable(descs, DEV)
    dev, host, n = tab.sub(0, 1)
    L.check(L.load().hpfg_bn_acc_bwd_finalize(dev, host, n, stream(DEV)), "bn_acc_bwd_finalize")
    torch.cuda.synchronize()


BWD_CONSUMERS = [  # consumer, N, H, W, cin, cout (of the layer whose dZ is the source), shards
    ("dgrad chunked", 3, 12, 20, 64, 64, 4),
    ("dgrad thin", 2, 32, 48, 64, 32, 8),
    ("fused", 2, 32, 32, 16, 16, 8),
    ("wgrad", 3, 12, 20, 32, 64, 2),
]


@pytest.mark.parametrize("consumer,N,H,W,cin,cout,shards", BWD_CONSUMERS)
def test_backward_consumer_same_bits_from_accumulator_and_from_table(consumer, N, H, W, cin, cout, shards):
    lib = L.load()
    g = torch.Generator().manual_seed(H + cin + cout)
    layer = AdHocConv(cin, cout, 9, DEV, seed=cin + cout, hw=(H, W))
    zo, dA = _randn(g, N, H, W, cout).to(DEV), torch.randn(N, H, W, cout, generator=g).to(DEV)
    tab = _bn_table(cout, 11).to(DEV)                    # (its k rows are random: a consumer that read them instead of the sums would show)
    gamma = torch.randn(cout, generator=g).to(DEV)
    acc = _zero_acc(cout, shards)
    d = _dz(zo, tab, dA, cout, H, W)
    L.check(lib.hpfg_bn_bwd_reduce_acc(C.byref(d), N, H, W, L.ptr(acc), shards, stream(DEV)), "bn_bwd_reduce_acc")
    torch.cuda.synchronize()
    acc0 = acc.clone()
    assert int((acc0 != 0).sum()) > 0
    zi, tabi = _randn(g, N, H, W, cin).to(DEV), _bn_table(cin, 3).to(DEV)
    xi = _randn(g, N, H, W, cin).to(DEV)

    def run():
        if consumer.startswith("dgrad"):
            out, _ = layer.conv(d, None, N, H, W, dgrad=True, math=B16)
            return (out,)
        if consumer == "fused":
            out, slab, _, _ = _fused_launch(layer, _bnact(zi, tabi, cin, H, W), d, N, H, W)
            return out, slab
        return (layer.wgrad(plain_act(xi, cin, H, W), None, d, N, H, W, math=B16),)

    d.bn_acc, d.bn_gamma, d.bn_count, d.bn_shards = L.ptr(acc), L.ptr(gamma), float(N * H * W), shards
    from_acc = run()
    torch.cuda.synchronize()
    assert torch.equal(acc, acc0)
    k_before = tab[L.BN_K1:L.BN_K3 + 1].clone()
    _finalize_bwd(acc, gamma, tab, cout, N * H * W, shards)
    assert int((acc != 0).sum()) == 0 and not torch.equal(tab[L.BN_K1:L.BN_K3 + 1], k_before)
    d.bn_acc = None
    from_tab = run()
    torch.cuda.synchronize()
    for a, b in zip(from_acc, from_tab):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{consumer}: prologue and finalize disagree: {maxerr(a.cpu(), b.cpu())}"


# ---- B4. the two backward finalizes against float64 autograd ----------------------------------------------------------------------------
def test_bn_bwd_finalizes_against_float64_autograd():
    lib = L.load()
    N, H, W, Cc, shards = 3, 12, 16, 32, 2
    count = N * H * W
    g = torch.Generator().manual_seed(31)
    z, dA = _randn(g, N, H, W, Cc), torch.randn(N, H, W, Cc, generator=g)
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    zd, dAd, gd, bd = z.to(DEV), dA.to(DEV), gamma.to(DEV), beta.to(DEV)
    zz = z.reshape(-1, Cc).double()
    sums_f = torch.stack([zz.sum(0), (zz * zz).sum(0)]).to(DEV)                  # double [2][C]
    tab = torch.zeros(L.BN_ROWS, Cc, device=DEV)
    L.check(lib.hpfg_bn_fwd_finalize(None, 0, L.ptr(sums_f), float(count), L.ptr(gd), L.ptr(bd), None, None, 0.1, EPS, L.ptr(tab), Cc, stream(DEV)), "fwd_finalize")
    d = _dz(zd, tab, dAd, Cc, H, W)
    nblk = lib.hpfg_bn_bwd_blocks(N, H, W, Cc)
    part = torch.zeros(nblk, 2, Cc, device=DEV)
    L.check(lib.hpfg_bn_bwd_reduce(C.byref(d), N, H, W, L.ptr(part), stream(DEV)), "reduce")
    acc = _zero_acc(Cc, shards)
    L.check(lib.hpfg_bn_bwd_reduce_acc(C.byref(d), N, H, W, L.ptr(acc), shards, stream(DEV)), "reduce_acc")
    sums = torch.zeros(2, Cc, dtype=torch.float64, device=DEV)
    L.check(lib.hpfg_reduce_partials(L.ptr(part), nblk, Cc, L.ptr(sums), stream(DEV)), "reduce_partials")
    scale = 0.25
    res = {}
    for name in ("partials", "sums", "acc"):
        t = tab.clone()
        t[L.BN_K1:] = float("nan")
        dg, db = torch.full((Cc,), float("nan"), device=DEV), torch.full((Cc,), float("nan"), device=DEV)
        if name == "partials":
            L.check(lib.hpfg_bn_bwd_finalize(L.ptr(part), nblk, None, float(count), L.ptr(gd), L.ptr(t), L.ptr(dg), L.ptr(db), Cc, 1.0, stream(DEV)), name)
        elif name == "sums":
            L.check(lib.hpfg_bn_bwd_finalize(None, 0, L.ptr(sums), float(count), L.ptr(gd), L.ptr(t), L.ptr(dg), L.ptr(db), Cc, scale, stream(DEV)), name)
        else:
            _finalize_bwd(acc, gd, t, Cc, count, shards, dg, db)
            assert int((acc != 0).sum()) == 0
        torch.cuda.synchronize()
        res[name] = (t.cpu(), dg.cpu().double() / (scale if name == "sums" else 1.0), db.cpu().double() / (scale if name == "sums" else 1.0))
    # float64 autograd of F.batch_norm(training=True) under the LeakyReLU the DZ source applies
    z64 = nchw(z).double().requires_grad_(True)
    w64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.batch_norm(z64, None, None, w64, b64, training=True, eps=float(np.float32(EPS)))
    (F.leaky_relu(y, 0.01) * nchw(dA).double()).sum().backward()
    dz_ref = z64.grad.permute(0, 2, 3, 1).reshape(-1, Cc)
    tc = tab.cpu()
    g64 = dA.double().reshape(-1, Cc) * _lrelu_slope(zz, tc[L.BN_SCALE].double(), tc[L.BN_SHIFT].double())
    assert torch.equal(g64 != dA.double().reshape(-1, Cc), (y.detach().permute(0, 2, 3, 1).reshape(-1, Cc) <= 0))      # same LeakyReLU decisions as float64
    worst = 0.0
    for name, (t, dg, db) in res.items():
        for what, got, ref in (("dgamma", dg, w64.grad), ("dbeta", db, b64.grad)):
            r = float((got - ref).abs().max()) / (1e-5 * float(ref.abs().max()))
            worst = max(worst, r)
            assert r < 1.0, (name, what, r)
        dz = t[L.BN_K1].double() * g64 + t[L.BN_K2].double() * zz + t[L.BN_K3].double()
        r = float((dz - dz_ref).abs().max()) / (1e-5 * float(dz_ref.abs().max()))
        worst = max(worst, r)
        assert r < 1.0, (name, "dz", r)
    for name in ("sums", "acc"):      # one definition of k1 .. k3 (hpfg_bn_bwd_coef): the same rows to 1 ulp
        a, b = res["partials"][0][L.BN_K1:L.BN_K3 + 1].double().numpy(), res[name][0][L.BN_K1:L.BN_K3 + 1].double().numpy()
        assert (np.abs(a - b) <= _ulp32(a)).all(), name
    _note("B4 backward finalizes vs float64 autograd (1e-5 of max)", worst)


# ---- B5. small relatives ---------------------------------------------------------------------------------------------------------------
def test_bn_eval_table_against_float64():
    Cc = 300
    g = torch.Generator().manual_seed(4)
    gamma, beta, rm, rv = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g), torch.randn(Cc, generator=g) * 0.5, torch.rand(Cc, generator=g) * 2 + 0.01
    gd, bd, rmd, rvd = gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)
    tab = torch.full((L.BN_ROWS, Cc), float("nan"), device=DEV)
    L.check(L.load().hpfg_bn_eval_table(L.ptr(gd), L.ptr(bd), L.ptr(rmd), L.ptr(rvd), EPS, L.ptr(tab), Cc, stream(DEV)), "eval_table")
    t = tab.cpu().double().numpy()
    rstd = 1.0 / np.sqrt(rv.double().numpy() + float(np.float32(EPS)))
    scale = gamma.double().numpy() * rstd
    shift = beta.double().numpy() - rm.double().numpy() * scale
    assert np.array_equal(t[L.BN_MEAN], rm.double().numpy())
    worst = 0.0
    for row, ref, at in ((L.BN_RSTD, rstd, rstd), (L.BN_SCALE, scale, scale),
                         (L.BN_SHIFT, shift, np.maximum(np.abs(beta.double().numpy()), np.abs(rm.double().numpy() * scale)))):
        r = np.abs(t[row] - ref) / _ulp32(at)
        print(f"[bn_acc] B5 eval table row {row}: {r.max():.3g} ulp")
        worst = max(worst, float(r.max()))
    _note("B5 bn_eval_table (ulp)", worst)
    assert worst <= 1.0
    # the table it writes is the eval-mode BatchNorm: y = z * scale + shift
    z = _randn(g, 2, Cc, 3, 3)
    ref = F.batch_norm(z.double(), rm.double(), rv.double(), gamma.double(), beta.double(), training=False, eps=float(np.float32(EPS)))
    got = z.double() * torch.from_numpy(t[L.BN_SCALE]).view(1, -1, 1, 1) + torch.from_numpy(t[L.BN_SHIFT]).view(1, -1, 1, 1)
    assert maxerr(got, ref) < 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("nblk,Cc", [(1, 16), (7, 48), (1500, 33)])
def test_reduce_partials_and_finalize_from_sums(nblk, Cc):
    lib = L.load()
    g = torch.Generator().manual_seed(nblk)
    ints = torch.randint(-1000, 1000, (nblk, 2, Cc), generator=g).float()      # small integers: every order of summation is exact
    real = _randn(g, nblk, 2, Cc)
    for part, exact in ((ints, True), (real, False)):
        pd = part.to(DEV)
        sums = torch.full((2, Cc), float("nan"), dtype=torch.float64, device=DEV)
        L.check(lib.hpfg_reduce_partials(L.ptr(pd), nblk, Cc, L.ptr(sums), stream(DEV)), "reduce_partials")
        ref = part.double().sum(0)
        if exact:
            assert torch.equal(sums.cpu(), ref)
        else:
            bound = nblk * 2.0 ** -53 * part.double().abs().sum(0)
            r = float(((sums.cpu() - ref).abs() / bound).max())
            assert r <= 1.0, r
            _note(f"B5 reduce_partials nblk={nblk}", r)
    # hpfg_bn_fwd_finalize: the same table from the exact sums as from the rows (positive second sums: squares)
    part = ints.clone()
    part[:, 1] = part[:, 1].abs() + 1000.0 * 1000.0
    pd = part.to(DEV)
    sums = torch.zeros(2, Cc, dtype=torch.float64, device=DEV)
    L.check(lib.hpfg_reduce_partials(L.ptr(pd), nblk, Cc, L.ptr(sums), stream(DEV)), "reduce_partials")
    gd, bd = torch.randn(Cc, generator=g).to(DEV), torch.randn(Cc, generator=g).to(DEV)
    out = []
    for use_sums in (False, True):
        tab = torch.full((L.BN_ROWS, Cc), float("nan"), device=DEV)
        rm, rv = torch.zeros(Cc, device=DEV), torch.ones(Cc, device=DEV)
        L.check(lib.hpfg_bn_fwd_finalize(None if use_sums else L.ptr(pd), 0 if use_sums else nblk, L.ptr(sums) if use_sums else None, float(nblk * 64),
                                         L.ptr(gd), L.ptr(bd), L.ptr(rm), L.ptr(rv), 0.1, EPS, L.ptr(tab), Cc, stream(DEV)), "fwd_finalize")
        torch.cuda.synchronize()
        out.append((tab[:4].clone(), rm, rv))
    assert bool(torch.isfinite(out[0][0]).all())
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)


# ---- C. the overflow bound of the accumulator words --------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1])
def test_accumulator_reader_is_exact_at_the_documented_bound(sign):
    """HPFG_ACC_MAX_ADDS = 2048 partial sums per accumulator and pass, each with the largest low limb (+-2^51, t = k +- 0.5), on 8 shards:
    hpfg_acc_read2 adds the shards' limbs in int64, so the bound holds for the adds of ALL shards together (2048 * 2^51 = 2^62) -- with 2048
    adds PER SHARD, what the guard allowed before, the low limbs total 2^65 and wrap to 0: measured on the device, S1 = 49152 instead of
    57344 (mean 0.75 instead of 0.875 at count 65536) -- which is why HPFG_ACC_CHECK bounds the workgroups of a launch, not the workgroups per
    shard."""
    shards, adds, Cc, count = 8, 2048, 16, 4096
    per = adds // shards
    acc = torch.zeros(shards, 2, Cc, 2, dtype=torch.int64)
    acc[:, 0, :, 0] = per * 3                      # sum z: 2048 partial sums of 3 +- 0.5
    acc[:, 0, :, 1] = sign * per * 2 ** 51
    s1 = adds * 3 + sign * adds // 2
    mean = Fraction(s1, count)
    s2 = count * (mean * mean + 1)                 # variance exactly 1
    assert s2.denominator == 1
    acc[:, 1, :, 0] = (int(s2) - sign * adds // 2) // shards      # sum z^2: the same low limbs
    acc[:, 1, :, 1] = sign * per * 2 ** 51
    tot = acc_totals(acc, Cc, shards)
    assert int(tot[0, 0, 1]) == sign * 2 ** 62 and acc_decode(tot)[0, 0] == float(s1) and acc_decode(tot)[1, 0] == float(s2)
    l = dict(acc=acc.to(DEV), gamma=torch.ones(Cc, device=DEV), beta=torch.zeros(Cc, device=DEV), bn=torch.zeros(L.BN_ROWS, Cc, device=DEV),
             C=Cc, count=count, shards=shards)
    assert _finalize_fwd([l], False) == 0, L.load().hpfg_last_error()
    t = l["bn"].cpu().double().numpy()
    assert (t[L.BN_MEAN] == float(mean)).all(), t[L.BN_MEAN][:4]      # (1.75 / 1.25: exact in fp32)
    rstd = 1.0 / np.sqrt(1.0 + float(np.float32(EPS)))
    assert (np.abs(t[L.BN_RSTD] - rstd) <= _ulp32(rstd)).all()


def test_launchers_refuse_more_adds_than_the_reader_can_sum():
    """2048 workgroups on 8 shards: accepted, limbs exact; 2049: refused before anything is launched (257 per shard passed the old guard)."""
    H = W = 8
    layer = AdHocConv(16, 16, 1, DEV, seed=1, hw=(H, W))
    g = torch.Generator().manual_seed(6)
    x = _randn(g, 2049, H, W, 16).to(DEV)
    N = 2048
    acc = _zero_acc(16, 8)
    out, part = layer.conv(plain_act(x, 16, H, W), None, N, H, W, stats=True, math=B16, stat_acc=acc, shards=8)
    assert layer.rows == N
    torch.cuda.synchronize()
    tot = acc_totals(acc, 16, 8)
    assert (tot == acc_rows_totals(part.view(-1, 2, 16).cpu().numpy())).all()
    _note("C 2048-workgroup 1x1 launch", _fwd_sums_check("1x1 2048", out, tot))
    acc.zero_()
    with pytest.raises(L.HipLibraryError, match="2049 workgroups"):
        layer.conv(plain_act(x, 16, H, W), None, N + 1, H, W, stats=True, math=B16, stat_acc=acc, shards=8)
    torch.cuda.synchronize()
    assert int((acc != 0).sum()) == 0
