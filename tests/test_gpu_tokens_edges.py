"""GPU: the token-layout kernels of csrc/tokens.hip (and the epilogue switches of csrc/gemm.hip), entry point by entry point through
hpfg_amd._lib, against float64 laws (tests/helpers.py; tests/test_tokens_laws_host.py holds those against torch's float64 ops) at every
edge of the launch code: each LayerNorm variant and both sides of its boundaries, the workgroup caps of the partial-sum kernels (with the
workgroups that own no rows), a second trip of every grid-stride loop, ragged tiles and empty row splits of the row-split weight gradient,
non-integer resize ratios, 1 x 1 / 1 x N images and ragged channel slices of the depthwise conv.

Conventions.  Every output (and the part of a partial-sum scratch that the finishing reduction reads) is allocated with a tail and filled
with a quiet-NaN bit pattern: after the launch no element of the output holds the pattern and the tail kept its bits.  Pure data movement
is compared bit for bit.  Every other output must lie within 8 x the error that torch's own float32 CPU op makes against the float64 law
on the same inputs, with a floor of 4 float32 ulp of the largest magnitude of the law (helpers.bound_8x); the split-bf16 GEMMs get 8 x
that again.  Inputs carry a per-channel offset in [-3, 3] and scale in [0.25, 4].

Measured on the MI355X, largest error / bound over the cases of each family (1.0 is the limit):
  LayerNorm             y 0.22   mean 0.63   rstd 0.28   dx 0.37   dgamma, dbeta 0.35
  depthwise + GELU      y 0.18   du 0.40   dx 0.39   dw9, dbias 0.22
  bilinear resize       y 0.23   dx 0.14   resize_sum 0.13   adjoint identity 0.02
  token statistics      sum x 0.43   centred squares 0.35
  BatchNorm + ReLU      y 0.25   dx 0.17   dbeta, dgamma 0.29
  row-split dW          0.13
  col2im                0.13
  elementwise           residual_scale 0.11   scale_rows 0.10   gelu y 0.03   gelu dx 0.08
  GEMM epilogues        f32 0.62   f32 split-K 0.15   bf16x3 0.62   bf16x3 split-K 0.62 (of 8 x 8)
  batch variance of x = m + randn through bn_relu_dropout (var / y):
    m = 0: 0.13 / 0.13   m = 4: 0.10 / 0.08   m = 32: 0.12 / 0.25   m = 100: 0.10 / 0.10
    (E[x^2] - mean^2 in float32, which these sums replaced, gave var ratios 0.2, 4.5, 329 and 2051 at m = 0, 4, 32, 100.)
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hpfg_amd import _lib as L
from tests import helpers as H
from tests.helpers import bound_8x, canary_ok, canary_out, chan_affine, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STRIDE_CAP = 8192 * 256          # float4 items one pass of a grid-stride kernel covers (grid_cap(total, 8192) workgroups of 256)
GELU_GRID = [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0]


def _report(name, err, bound):
    """One line per compared output: largest error / bound (pytest -s shows them; the module docstring quotes a run)."""
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"  {name:<44s} max|err| {err:9.3e}  bound {bound:9.3e}  ratio {ratio:6.3f}")
    return ratio


def _dev(t):
    return t.contiguous().to(DEV)


def _within(name, buf, ref64, t32, margin=8.0):
    """buf: canary_out(ref64.numel()) after the launch.  Canaries, finiteness, and the 8 x rule against the float64 law."""
    n = ref64.numel()
    written, tail = canary_ok(buf, n)
    assert written, f"{name}: elements of the output were never written"
    assert tail, f"{name}: the launch wrote past the end of the output"
    got = buf[:n].cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(got).all()), name
    err = float((got - ref64.double()).abs().max())
    bound = bound_8x(ref64, t32.reshape(ref64.shape), margin)
    _report(name, err, bound)
    assert err <= bound, (name, err, bound)
    return got


def _bit_equal(name, buf, want):
    n = want.numel()
    written, tail = canary_ok(buf, n)
    assert written and tail, (name, written, tail)
    assert torch.equal(buf[:n].cpu().reshape(want.shape), want), name


def _scratch_ok(name, buf, n):
    written, tail = canary_ok(buf, n)
    assert written, f"{name}: partial sums that the finishing reduction reads were never written"
    assert tail, f"{name}: partial sums written past the scratch"


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
LN_VARIANT = {4: 8, 32: 8, 36: 16, 96: 32, 128: 32, 160: 64, 256: 64, 260: 0, 320: 0, 512: 0, 1024: 0}          # lanes per row; 0: one row per wave


def _ln_variant(C_):
    q = C_ // 4
    return 8 if q <= 8 else 16 if q <= 16 else 32 if q <= 32 else 64 if q <= 64 else 0


def _ln_run(rows, C_, x, seed, tag):
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(seed)
    g, b, dy = chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen), chan_affine((rows, C_), 0, gen)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
    y32, mean32, rstd32 = torch.native_layer_norm(xr, (C_,), gr, br, 1e-5)
    y32.backward(dy)
    y64, mean64, rstd64 = H.ln_f64(x, g, b)
    dx64, dg64, db64 = H.ln_bwd_f64(x, dy, g)
    xd, gd, bd, dyd = _dev(x), _dev(g), _dev(b), _dev(dy)
    y, mean, rstd = canary_out(rows * C_), canary_out(rows), canary_out(rows)
    L.check(lib.hpfg_ln_fwd(L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y), L.ptr(mean), L.ptr(rstd), rows, C_, st), "ln_fwd")
    nblk = lib.hpfg_ln_bwd_blocks(rows)
    dx, dgb, part = canary_out(rows * C_), canary_out(2 * C_), canary_out(nblk * 2 * C_)
    L.check(lib.hpfg_ln_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dgb), L.ptr(dgb[C_:]), L.ptr(part), rows, C_, st),
            "ln_bwd")
    torch.cuda.synchronize()
    _within(f"ln {tag} y", y, y64, y32.detach())
    _within(f"ln {tag} mean", mean, mean64, mean32.detach().reshape(-1))
    _within(f"ln {tag} rstd", rstd, rstd64, rstd32.detach().reshape(-1))
    _within(f"ln {tag} dx", dx, dx64, xr.grad)
    _scratch_ok(f"ln {tag} partials", part, nblk * 2 * C_)
    _within(f"ln {tag} dgamma,dbeta", dgb, torch.stack([dg64, db64]), torch.stack([gr.grad, br.grad]))
    return part, nblk


@pytest.mark.parametrize("C_", sorted(LN_VARIANT))
def test_layer_norm_every_variant_and_row_count(C_):
    """All five variants (8 / 16 / 32 / 64 lanes per row, one row per wave) on both sides of each boundary; 36 and 96 leave lanes of a group
    without a channel quad; rows 1, 3, 65, 193: less than one wave's rows, and a last workgroup that is not full."""
    assert _ln_variant(C_) == LN_VARIANT[C_]
    for rows in (1, 3, 65, 193):
        _ln_run(rows, C_, chan_affine((rows, C_), 1000 * C_ + rows), C_ + rows, f"C{C_} rows{rows}")


@pytest.mark.parametrize("C_", [32, 320])
def test_layer_norm_above_the_workgroup_cap(C_):
    """33 000 rows: hpfg_ln_bwd_blocks stops at 512 workgroups.  At C = 32 the rows of a workgroup are rounded up to whole sweeps (96), so
    the workgroups from 344 on own no rows and must write zero partial sums."""
    lib = L.load()
    rows = 33000
    nblk = lib.hpfg_ln_bwd_blocks(rows)
    assert nblk == 512 and (rows + 63) // 64 > 512
    per = -(-rows // nblk)
    if C_ == 32:
        step = 4 * (64 // _ln_variant(C_))
        per = -(-per // step) * step
        assert per == 96 and -(-rows // per) == 344
    part, _ = _ln_run(rows, C_, chan_affine((rows, C_), C_), C_, f"C{C_} rows{rows}")
    first_empty = -(-rows // per)
    assert first_empty < nblk
    assert not part[first_empty * 2 * C_:nblk * 2 * C_].any()          # (written -- _scratch_ok -- and zero)


def test_layer_norm_large_mean_small_spread():
    """x = 100 + 0.1 randn: the kernels take the variance around the mean (two passes over registers), so this holds; kept so."""
    rows, C_ = 65, 128
    x = (100.0 + 0.1 * torch.randn(rows, C_, generator=torch.Generator().manual_seed(5))).float()
    _ln_run(rows, C_, x, 6, "x=100+0.1n")


# ---- depthwise 3 x 3 + GELU -------------------------------------------------------------------------------------------------------------
def _dw_run(B, Hh, W, C_, seed, tag, x=None, w9=None, bias=None):
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(seed)
    x = chan_affine((B, Hh, W, C_), 0, gen) if x is None else x
    w9 = 0.15 * chan_affine((9, C_), 0, gen) if w9 is None else w9
    bias = 0.3 * chan_affine((C_,), 0, gen) if bias is None else bias
    dy = chan_affine((B, Hh, W, C_), 0, gen)
    xr, br = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    wr = w9.t().reshape(C_, 1, 3, 3).contiguous().requires_grad_(True)
    u32 = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=1, groups=C_).permute(0, 2, 3, 1)
    u32.retain_grad()
    y32 = F.gelu(u32)
    y32.backward(dy)
    y64 = H.gelu_f64(H.dwconv_f64(x, w9, bias))
    du64, dx64, dw64, db64 = H.dwgelu_bwd_f64(x, w9, bias, dy)
    n = B * Hh * W * C_
    xd, wd, bd, dyd = _dev(x), _dev(w9), _dev(bias), _dev(dy)
    y = canary_out(n)
    L.check(lib.hpfg_dwgelu_fwd(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(y), B, Hh, W, C_, st), "dwgelu_fwd")
    nblk = lib.hpfg_dwgelu_bwd_blocks(B, Hh, W)
    du, dx, dwb, part = canary_out(n), canary_out(n), canary_out(10 * C_), canary_out(nblk * 10 * C_)
    L.check(lib.hpfg_dwgelu_bwd(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(dyd), L.ptr(du), L.ptr(dx), L.ptr(dwb), L.ptr(dwb[9 * C_:]), L.ptr(part),
                                B, Hh, W, C_, st), "dwgelu_bwd")
    torch.cuda.synchronize()
    _within(f"dwgelu {tag} y", y, y64, y32.detach())
    _within(f"dwgelu {tag} du", du, du64, u32.grad)
    _within(f"dwgelu {tag} dx", dx, dx64, xr.grad)
    _scratch_ok(f"dwgelu {tag} partials", part, nblk * 10 * C_)
    _within(f"dwgelu {tag} dw9,dbias", dwb, torch.cat([dw64, db64[None]]), torch.cat([wr.grad.reshape(C_, 9).t(), br.grad[None]]))
    return nblk


@pytest.mark.parametrize("C_", [4, 96, 256, 260, 640])
def test_dwconv_gelu_thin_images_and_ragged_channel_slices(C_):
    """C = 4: one quad and 256 pixel lanes; 96: 24 quads, 10 pixel lanes and 16 idle threads; 260: a second channel slice holding one quad;
    640: three slices.  Images of 1 x 1, 1 x 7, 7 x 1 and 2 x 2 pixels (every tap of some pixel falls outside) and 5 x 9."""
    for k, (B, Hh, W) in enumerate([(1, 1, 1), (2, 1, 7), (2, 7, 1), (1, 2, 2), (3, 5, 9)]):
        _dw_run(B, Hh, W, C_, 10 * C_ + k, f"C{C_} {B}x{Hh}x{W}")


def test_dwconv_gelu_on_the_gelu_grid():
    """Pre-activations exactly on {0, +-1e-30, +-0.5, +-3, +-6, +-12, +-40} (one pixel, x = 1, the centre taps are the grid): finite, in bound."""
    C_ = 16
    w9 = 0.15 * chan_affine((9, C_), 3)
    w9[4] = torch.tensor(GELU_GRID + [1.0, -1.0])
    _dw_run(1, 1, 1, C_, 4, "grid", x=torch.ones(1, 1, 1, C_), w9=w9, bias=torch.zeros(C_))


@pytest.mark.parametrize("B,Hh,W,C_", [(1, 257, 256, 4), (2, 64, 64, 1028)], ids=["du_cap", "stride_cap"])
def test_dwconv_gelu_above_the_caps(B, Hh, W, C_):
    """(1, 257, 256, 4): 65 792 pixels, more than the 2048 workgroups x 32 pixels of the du kernel.  (2, 64, 64, 1028): 257 quads x 8192 pixels
    run the forward's and dx's grid-stride loop a second time, and the fifth channel slice of the du kernel holds a single quad."""
    lib = L.load()
    npix = B * Hh * W
    if C_ == 4:
        assert lib.hpfg_dwgelu_bwd_blocks(B, Hh, W) == 2048 and npix > 2048 * 32
    else:
        assert npix * (C_ // 4) > STRIDE_CAP and -(-(C_ // 4) // 64) == 5 and (C_ // 4) % 64 == 1
    _dw_run(B, Hh, W, C_, C_, f"C{C_} {B}x{Hh}x{W}")


# ---- bilinear resize ------------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [((3, 5), (7, 12)), ((7, 7), (10, 10)), ((5, 5), (5, 5)), ((1, 1), (8, 8)), ((1, 6), (4, 6)), ((2, 2), (56, 56)), ((9, 9), (72, 72)),
                ((7, 7), (56, 56)), ((5, 3), (15, 21))]


def _interp32(x, Hh, W):
    return F.interpolate(x.permute(0, 3, 1, 2), size=(Hh, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def _resize_run(B, h, w, Hh, W, C_, seed, tag, adjoint=True):
    # The law takes the source coordinate in float64, the kernels in float32: near an integer coordinate the two can pick different taps.
    # The interpolant (and its transpose) is continuous in the coordinate, so the results differ by rounding only: no special case.
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(seed)
    x, dy = chan_affine((B, h, w, C_), 0, gen), chan_affine((B, Hh, W, C_), 0, gen)
    xr = x.clone().requires_grad_(True)
    y32 = _interp32(xr, Hh, W)
    y32.backward(dy)
    y, dx = canary_out(B * Hh * W * C_), canary_out(B * h * w * C_)
    xd, dyd = _dev(x), _dev(dy)
    L.check(lib.hpfg_resize_bilinear_fwd(L.ptr(xd), L.ptr(y), B, h, w, Hh, W, C_, st), "resize_fwd")
    L.check(lib.hpfg_resize_bilinear_bwd(L.ptr(dyd), L.ptr(dx), B, h, w, Hh, W, C_, st), "resize_bwd")
    torch.cuda.synchronize()
    got_y = _within(f"resize {tag} y", y, H.resize_f64(x, Hh, W), y32.detach())
    got_dx = _within(f"resize {tag} dx", dx, H.resize_bwd_f64(dy, h, w), xr.grad)
    if adjoint:
        # <resize(x), dy> = <x, resize_bwd(dy)>: both kernels take their weights from the same float32 coordinate, so the identity holds up
        # to the roundings of the products and sums alone -- at most ~16 per term on either side (three lerps of three roundings, the weight
        # product, the accumulation); 64 units of 2^-24 relative to sum |x| |resize_bwd(dy)| leaves a factor 4.
        lhs, rhs = float((got_y * dy.double()).sum()), float((x.double() * got_dx).sum())
        scale = float((x.double().abs() * got_dx.abs()).sum())
        _report(f"resize {tag} adjoint", abs(lhs - rhs), 64 * 2.0 ** -24 * scale)
        assert abs(lhs - rhs) <= 64 * 2.0 ** -24 * scale, (tag, lhs, rhs, scale)


@pytest.mark.parametrize("C_", [4, 8])
@pytest.mark.parametrize("lo,hi", RESIZE_CASES, ids=[f"{a}x{b}to{c}x{d}" for (a, b), (c, d) in RESIZE_CASES])
def test_resize_bilinear_non_integer_ratios_and_adjoint(lo, hi, C_):
    """Ratios 7/3, 12/5, 10/7 (the gather's candidate window comes from 1 / scale), the identity, one source pixel, one source row, the
    integer ratios 28, 8, 8 with odd source sizes, and the odd ratios 3 and 7, where the ends of the candidate window are whole numbers."""
    _resize_run(2, lo[0], lo[1], hi[0], hi[1], C_, 100 * lo[0] + hi[1] + C_, f"{lo}->{hi} C{C_}")


def _resize_sum_run(B, Hh, W, C_, lows, seed, tag):
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(seed)
    base = chan_affine((B, Hh, W, C_), 0, gen)
    xs = [chan_affine((B, h, w, C_), 0, gen) for h, w in lows]
    y32, y64 = base.clone(), base.double()
    for x in xs:
        y32 = y32 + _interp32(x, Hh, W)
        y64 = y64 + H.resize_f64(x, Hh, W)
    bd, xd = _dev(base), [_dev(x) for x in xs]
    k = max(1, len(xs))
    ptrs = (C.c_void_p * k)(*[x.data_ptr() for x in xd])
    hs, ws = (C.c_int * k)(*[h for h, _ in lows]), (C.c_int * k)(*[w for _, w in lows])
    y = canary_out(base.numel())
    L.check(lib.hpfg_resize_sum_fwd(L.ptr(bd), ptrs, hs, ws, len(xs), L.ptr(y), B, Hh, W, C_, st), "resize_sum_fwd")
    torch.cuda.synchronize()
    _within(f"resize_sum {tag}", y, y64, y32)


@pytest.mark.parametrize("lows", [[], [(5, 3)], [(12, 10), (6, 5)], [(5, 3), (12, 10), (3, 5)]], ids=["0src", "1src", "2src", "3src"])
def test_resize_sum_source_counts(lows):
    """base [2,12,10,8] + 0..3 sources: non-integer ratios (12/5, 10/3), a source already at full size, and the integer ratio 2."""
    _resize_sum_run(2, 12, 10, 8, lows, 7 + len(lows), f"{len(lows)} sources")


def test_resize_sum_above_the_stride_cap():
    """base [3,56,56,1024] with one 28 x 28 source: 2 408 448 float4 items, a second trip of the grid-stride loop."""
    assert 3 * 56 * 56 * 256 > STRIDE_CAP
    _resize_sum_run(3, 56, 56, 1024, [(28, 28)], 11, "3x56x56x1024")


def test_resize_bwd_above_the_stride_cap():
    """dx [3,56,56,1024] from dy [3,64,64,1024] (ratio 8/7): 2 408 448 float4 items of dx, a second trip of the gather's grid-stride loop."""
    assert 3 * 56 * 56 * 256 > STRIDE_CAP
    _resize_run(3, 56, 56, 64, 64, 1024, 12, "3x56x56x1024<-64x64", adjoint=False)


# ---- token BatchNorm + ReLU + channel dropout ---------------------------------------------------------------------------------------------
TOK_C = [4, 8, 16, 32, 64, 128, 256, 512, 1024]          # every C with (C / 4) | 256: what tok_c_ok admits
BN_ROWS = {1: (1, 1), 5: (1, 5), 65: (5, 13), 4097: (17, 241)}          # R -> (images, rows per image); 13 and 241: image ends inside a workgroup


def _stats_run(R, C_, seed, tag):
    lib, st = L.load(), stream(DEV)
    x = chan_affine((R, C_), seed)
    s64, m64 = H.col_stats_f64(x)
    s32, m32 = x.sum(0), ((x - x.mean(0)) ** 2).sum(0)
    nblk = lib.hpfg_tok_stat_blocks(R)
    part, sums = canary_out(nblk * 2 * C_), canary_out(2 * C_)
    xd = _dev(x)
    L.check(lib.hpfg_tok_col_stats(L.ptr(xd), R, C_, L.ptr(part), L.ptr(sums), st), "tok_col_stats")
    torch.cuda.synchronize()
    _scratch_ok(f"col_stats {tag} partials", part, nblk * 2 * C_)
    written, tail = canary_ok(sums, 2 * C_)
    assert written and tail, tag
    got = sums[:2 * C_].cpu().double().reshape(2, C_)
    for k, (name, r64, r32) in enumerate((("sum x", s64, s32), ("sum (x-mean)^2", m64, m32))):
        err, bound = float((got[k] - r64).abs().max()), bound_8x(r64, r32)
        _report(f"col_stats {tag} {name}", err, bound)
        assert err <= bound, (tag, name, err, bound)
    return nblk


@pytest.mark.parametrize("C_", TOK_C)
def test_token_column_statistics(C_):
    """sum x and the centred sum of squares per channel, R in {1, 5, 65, 4097}; C = 1024 leaves one row lane per workgroup."""
    for R in BN_ROWS:
        _stats_run(R, C_, 31 * C_ + R, f"C{C_} R{R}")


@pytest.mark.parametrize("C_", [4, 64])
def test_token_column_statistics_above_the_workgroup_cap(C_):
    lib = L.load()
    R = 66000
    assert lib.hpfg_tok_stat_blocks(R) == 1024 and (R + 63) // 64 > 1024
    _stats_run(R, C_, C_, f"C{C_} R{R}")


def bn_case(B, N, C_, seed, mask_mode):
    """Inputs of one bnrelu_apply / bnrelu_bwd launch: x with per-channel offset and scale, its batch statistics (float64, rounded to the
    float32 the kernels take), gamma of either sign, and beta chosen per channel so that the pre-activation changes sign in the widest gap
    between two neighbouring values of the channel's middle 80 %: both signs in every channel, none within 2e-5 of the ReLU's kink, where
    float32 and float64 could disagree about the gate (four float32 roundings of terms up to 16: 4e-6).  mask_mode: None, "image" ([B, C], rows_per_image N) or "row" ([R, C], 1); the
    first image's (row's) mask is all zero."""
    R = B * N
    gen = torch.Generator().manual_seed(seed)
    x = chan_affine((R, C_), 0, gen)
    gamma = chan_affine((C_,), 0, gen).abs().clamp_min(0.25) * torch.where(torch.rand(C_, generator=gen) < 0.5, -1.0, 1.0)
    s, m2 = H.col_stats_f64(x)
    mean = (s / R).float()
    rstd = (1.0 / torch.sqrt(m2 / R + 1e-5)).float()
    xh = (x.double() - mean.double()) * rstd.double()
    if R >= 2:
        srt = xh.sort(0).values
        lo = (R - 1) // 10
        hi = max(lo + 1, (9 * (R - 1)) // 10)
        at = lo + (srt[lo + 1:hi + 1] - srt[lo:hi]).argmax(0)
        mid = 0.5 * (srt.gather(0, at[None]) + srt.gather(0, at[None] + 1))[0]
        beta = (-gamma.double() * mid).float()
    else:
        beta = torch.where(torch.arange(C_) % 2 == 0, 0.5, -0.5)
    pre = xh * gamma.double() + beta.double()
    assert float(pre.abs().min()) > 2e-5 and float(pre.abs().max()) < 64.0, (float(pre.abs().min()), float(pre.abs().max()))
    if R >= 2:
        assert bool(((pre > 0).any(0) & (pre < 0).any(0)).all())          # the ReLU gate opens and closes in every channel
    dy = chan_affine((R, C_), 0, gen)
    mask, rpi = None, N
    if mask_mode is not None:
        rpi = N if mask_mode == "image" else 1
        mask = torch.empty(R // rpi, C_).bernoulli_(0.7, generator=gen)
        mask[0] = 0.0
    return dict(x=x, gamma=gamma, beta=beta, mean=mean, rstd=rstd, dy=dy, mask=mask, rpi=rpi, keep=0.9)


def _bn_run(c, tag):
    lib, st = L.load(), stream(DEV)
    x, gamma, beta, mean, rstd, dy, mask, rpi = (c[k] for k in ("x", "gamma", "beta", "mean", "rstd", "dy", "mask", "rpi"))
    R, C_ = x.shape
    inv_keep = float(np.float32(1.0 / c["keep"]))
    rows = None if mask is None else mask[torch.arange(R) // rpi] * inv_keep
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y32 = torch.relu(torch.batch_norm(xr, gr, br, None, None, True, 0.0, 1e-5, False))          # (the ATen op: F.batch_norm refuses one row)
    y32 = y32 if rows is None else y32 * rows
    y32.backward(dy)
    y64, _ = H.bnrelu_f64(x, mean, rstd, gamma, beta, mask, inv_keep, rpi)
    dx64, s1, s2 = H.bnrelu_bwd_f64(x, dy, mean, rstd, gamma, beta, mask, inv_keep, rpi)
    xd, gd, bd, md, rd, dyd = (_dev(t) for t in (x, gamma, beta, mean, rstd, dy))
    kd = None if mask is None else _dev(mask)
    y = canary_out(R * C_)
    L.check(lib.hpfg_bnrelu_apply(L.ptr(xd), L.ptr(md), L.ptr(rd), L.ptr(gd), L.ptr(bd), L.ptr(kd), inv_keep, rpi, L.ptr(y), R, C_, st), "bnrelu_apply")
    nblk = lib.hpfg_tok_stat_blocks(R)
    dx, part, sums = canary_out(R * C_), canary_out(nblk * 2 * C_), canary_out(2 * C_)
    L.check(lib.hpfg_bnrelu_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(md), L.ptr(rd), L.ptr(gd), L.ptr(bd), L.ptr(kd), inv_keep, rpi, L.ptr(dx), L.ptr(part),
                                L.ptr(sums), R, C_, st), "bnrelu_bwd")
    torch.cuda.synchronize()
    _within(f"bnrelu {tag} y", y, y64, y32.detach())
    _within(f"bnrelu {tag} dx", dx, dx64, xr.grad)
    _scratch_ok(f"bnrelu {tag} partials", part, nblk * 2 * C_)
    _within(f"bnrelu {tag} dbeta,dgamma", sums, torch.stack([s1, s2]), torch.stack([br.grad, gr.grad]))


@pytest.mark.parametrize("C_", TOK_C)
def test_bnrelu_apply_and_backward(C_):
    """No mask, a mask per image (rows_per_image = N: 13 and 241 rows, so an image ends inside a workgroup's rows) and a mask per row
    (rows_per_image = 1: r / rows_per_image changes on every row); the first image's mask is all zero."""
    for R, (B, N) in BN_ROWS.items():
        for mode in ((None, "image", "row") if R <= 65 else ("image",)):
            _bn_run(bn_case(B, N, C_, 17 * C_ + R, mode), f"C{C_} R{R} mask={mode}")


@pytest.mark.parametrize("B,N,C_", [(3, 22000, 4), (3, 22000, 64), (3, 11000, 256)], ids=["wg_cap_C4", "wg_cap_C64", "stride_cap_C256"])
def test_bnrelu_above_the_caps(B, N, C_):
    lib = L.load()
    R = B * N
    if C_ == 256:
        assert R * (C_ // 4) > STRIDE_CAP
    else:
        assert lib.hpfg_tok_stat_blocks(R) == 1024 and (R + 63) // 64 > 1024
    _bn_run(bn_case(B, N, C_, C_, "image"), f"C{C_} R{R}")


@pytest.mark.parametrize("m", [0.0, 4.0, 32.0, 100.0])
def test_batch_variance_does_not_cancel(m):
    """bn_relu_dropout (the wrapper owns the step from the kernel's sums to the variance) on x = m + randn: var and y against float64, inside
    8 x the error of torch's float32 F.batch_norm -- at every m: the sums are centred (col_stats_kernel), not E[x^2] - mean^2."""
    from hpfg_amd.ops_tokens import bn_relu_dropout
    B, N, C_ = 2, 515, 64
    R = B * N
    gen = torch.Generator().manual_seed(int(m) + 1)
    x = (m + torch.randn(B, N, C_, generator=gen)).float()
    gamma, beta = chan_affine((C_,), 0, gen), 0.1 * chan_affine((C_,), 0, gen)
    rm, rv = torch.zeros(C_), torch.ones(C_)
    y32 = torch.relu(F.batch_norm(x.reshape(R, C_), rm, rv, gamma, beta, True, 1.0, 1e-5))
    var32 = rv.double() * (R - 1) / R          # (running_var takes the unbiased variance)
    s, m2 = H.col_stats_f64(x.reshape(R, C_))
    mean64, var64 = s / R, m2 / R
    y64 = torch.relu((x.reshape(R, C_).double() - mean64) / torch.sqrt(var64 + 1e-5) * gamma.double() + beta.double())
    y, mean, var = bn_relu_dropout(_dev(x), _dev(gamma), _dev(beta), None, 1.0, 1e-5)
    torch.cuda.synchronize()
    for name, got, r64, r32 in (("mean", mean, mean64, rm), ("var", var, var64, var32), ("y", y.reshape(R, C_), y64, y32)):
        err, bound = float((got.cpu().double() - r64).abs().max()), bound_8x(r64, r32)
        _report(f"bn variance m={m:g} {name}", err, bound)
        assert err <= bound, (m, name, err, bound)


# ---- row-split weight gradient --------------------------------------------------------------------------------------------------------------
def _wgrad_geometry(lib, R, N, K):
    S = lib.hpfg_linear_wgrad_splits(R, N, K)
    per = -(-(-(-R // S)) // 64) * 64
    return (32 if N <= 32 else 64, 32 if K <= 32 else 64), S, per


def _wgrad_run(R, N, K, seed):
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(seed)
    dy, x = chan_affine((R, N), 0, gen), chan_affine((R, K), 0, gen)
    S = lib.hpfg_linear_wgrad_splits(R, N, K)
    dw, part = canary_out(N * K), canary_out(S * N * K)
    dyd, xd = _dev(dy), _dev(x)
    L.check(lib.hpfg_linear_wgrad(L.ptr(dyd), L.ptr(xd), L.ptr(dw), L.ptr(part), R, N, K, st), "linear_wgrad")
    torch.cuda.synchronize()
    _scratch_ok(f"wgrad {(R, N, K)} partials", part, S * N * K)
    _within(f"wgrad {(R, N, K)} dW", dw, dy.double().t() @ x.double(), torch.matmul(dy.t(), x))
    return part


# (R, N, K) -> tile, splits, rows of the last split that owns any
WGRAD_EDGES = {(100, 32, 32): ((32, 32), 1, 100), (300, 4, 256): ((32, 64), 2, 108), (1000, 160, 36): ((64, 64), 4, 232), (2049, 36, 20): ((64, 32), 9, 1),
               (4100, 68, 32): ((64, 32), 17, 4), (8200, 32, 128): ((32, 64), 33, 8)}


@pytest.mark.parametrize("R,N,K", sorted(WGRAD_EDGES))
def test_linear_wgrad_tiles_and_ragged_edges(R, N, K):
    """All four tile instantiations; N = 160 / 36 / 68 / 4 and K = 36 / 20 leave a ragged last tile; R below one split, R not a multiple of
    64, and a last split of one row."""
    lib = L.load()
    tile, S, per = _wgrad_geometry(lib, R, N, K)
    assert (tile, S, R - (S - 1) * per) == WGRAD_EDGES[(R, N, K)]
    _wgrad_run(R, N, K, R + N + K)


def test_linear_wgrad_trailing_splits_own_no_rows():
    """(8200, 512, 512): 64 tiles -> 32 splits of 320 rows; the last six own no rows and must contribute zeros."""
    lib = L.load()
    R, N, K = 8200, 512, 512
    tile, S, per = _wgrad_geometry(lib, R, N, K)
    assert (tile, S, per) == ((64, 64), 32, 320) and -(-R // per) == 26
    part = _wgrad_run(R, N, K, 3)
    assert not part[26 * N * K:32 * N * K].any()


# ---- im2col / col2im ------------------------------------------------------------------------------------------------------------------------
COL_CAP = 16384 * 256


def _im2col_run(B, Hh, W, C_, k, s):
    lib, st = L.load(), stream(DEV)
    x = chan_affine((B, Hh, W, C_), Hh + C_ + k)
    want = H.patches_f64(x, k, s)
    cols = canary_out(want.numel())
    xd = _dev(x)
    L.check(lib.hpfg_im2col_nhwc(L.ptr(xd), L.ptr(cols), B, Hh, W, C_, k, s, st), "im2col")
    torch.cuda.synchronize()
    _bit_equal(f"im2col {(B, Hh, W, C_, k, s)}", cols, want)
    return want.shape


def _col2im_run(B, Hh, W, C_, k, s):
    lib, st = L.load(), stream(DEV)
    p = k // 2
    Ho, Wo = (Hh + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dcols = chan_affine((B, Ho * Wo, k * k * C_), Hh + C_ + k + 1)
    t32 = F.fold(dcols.reshape(B, Ho * Wo, k * k, C_).permute(0, 3, 2, 1).reshape(B, C_ * k * k, Ho * Wo), (Hh, W), k, padding=p, stride=s).permute(0, 2, 3, 1)
    dx = canary_out(B * Hh * W * C_)
    dd = _dev(dcols)
    L.check(lib.hpfg_col2im_nhwc(L.ptr(dd), L.ptr(dx), B, Hh, W, C_, k, s, st), "col2im")
    torch.cuda.synchronize()
    _within(f"col2im {(B, Hh, W, C_, k, s)}", dx, H.col2im_f64(dcols, Hh, W, C_, k, s), t32)


@pytest.mark.parametrize("B,Hh,W,C_,k,s", [(2, 9, 7, 3, 3, 2), (1, 2, 3, 4, 7, 4), (2, 8, 8, 4, 3, 1), (1, 5, 5, 8, 2, 2), (1, 13, 11, 1, 7, 4)])
def test_im2col_and_col2im_small_geometries(B, Hh, W, C_, k, s):
    """C = 3 and 1 take the scalar kernels; a 7 x 7 patch over a 2 x 3 image is mostly padding; k = 2 is an even kernel (padding 1)."""
    _im2col_run(B, Hh, W, C_, k, s)
    _col2im_run(B, Hh, W, C_, k, s)


def test_im2col_above_the_workgroup_cap():
    """(2, 64, 64, 256, 3, 1): 4 718 592 float4 items of cols, past the 16 384 workgroups of one pass."""
    assert 2 * 64 * 64 * 9 * 64 > COL_CAP
    _im2col_run(2, 64, 64, 256, 3, 1)


def test_col2im_above_the_workgroup_cap():
    """(2, 128, 128, 516, 2, 2): 4 227 072 float4 items of dx (the gather runs over dx), with patches of about dx's own size."""
    assert 2 * 128 * 128 * 129 > COL_CAP
    _col2im_run(2, 128, 128, 516, 2, 2)


# ---- elementwise and permutation kernels ------------------------------------------------------------------------------------------------
BIG4 = STRIDE_CAP + 257          # float4 items: one pass of 8192 workgroups and 257 more; 17 x 123 377
ELEMENTWISE_SHAPES = [(3, 4 * 37), (17, 4 * 123377)]          # (B, per_sample): per_sample / 4 odd, so a sample ends inside a wave


@pytest.mark.parametrize("B,per", ELEMENTWISE_SHAPES, ids=["small", "stride_cap"])
def test_residual_scale_and_scale_rows(B, per):
    lib, st = L.load(), stream(DEV)
    assert (per // 4) % 2 == 1 and (B * per // 4 == BIG4 or B == 3)
    gen = torch.Generator().manual_seed(per)
    x, y = chan_affine((B, per), 0, gen), chan_affine((B, per), 0, gen)
    xd, yd = _dev(x), _dev(y)
    zero_one = (torch.arange(B) % 2).float()
    for name, sc, want in (("none", None, x + y), ("0/1", zero_one, x + y * zero_one[:, None])):          # (x + y * 1 and x + y * 0 are exact)
        out = canary_out(B * per)
        L.check(lib.hpfg_residual_scale(L.ptr(xd), L.ptr(yd), L.ptr(None if sc is None else _dev(sc)), L.ptr(out), B, per, st), "residual_scale")
        torch.cuda.synchronize()
        _bit_equal(f"residual_scale scale={name}", out, want)
    out = canary_out(B * per)
    L.check(lib.hpfg_scale_rows(L.ptr(yd), L.ptr(_dev(zero_one)), L.ptr(out), B, per, st), "scale_rows")
    torch.cuda.synchronize()
    _bit_equal("scale_rows scale=0/1", out, y * zero_one[:, None])
    sc = (1.0 / (0.5 + 0.1 * torch.arange(B))).float()          # stochastic depth's 1 / keep, another per sample
    out, out2 = canary_out(B * per), canary_out(B * per)
    scd = _dev(sc)
    L.check(lib.hpfg_residual_scale(L.ptr(xd), L.ptr(yd), L.ptr(scd), L.ptr(out), B, per, st), "residual_scale")
    L.check(lib.hpfg_scale_rows(L.ptr(yd), L.ptr(scd), L.ptr(out2), B, per, st), "scale_rows")
    torch.cuda.synchronize()
    _within(f"residual_scale B{B}", out, x.double() + y.double() * sc.double()[:, None], x + y * sc[:, None])
    _within(f"scale_rows B{B}", out2, y.double() * sc.double()[:, None], y * sc[:, None])


@pytest.mark.parametrize("B,per", ELEMENTWISE_SHAPES, ids=["small", "stride_cap"])
def test_gelu_forward_and_backward(B, per):
    """Exact (erf) GELU and its derivative; the first values are the grid {0, -0, +-1e-30, +-0.5, +-3, +-6, +-12, +-40}."""
    lib, st = L.load(), stream(DEV)
    n = B * per
    gen = torch.Generator().manual_seed(n)
    x = chan_affine((n // 4, 4), 0, gen).reshape(-1)
    x[:len(GELU_GRID)] = torch.tensor(GELU_GRID)
    dy = chan_affine((n // 4, 4), 0, gen).reshape(-1)
    xr = x.clone().requires_grad_(True)
    y32 = F.gelu(xr)
    y32.backward(dy)
    y, dx = canary_out(n), canary_out(n)
    xd, dyd = _dev(x), _dev(dy)
    L.check(lib.hpfg_gelu_fwd(L.ptr(xd), L.ptr(y), n, st), "gelu_fwd")
    L.check(lib.hpfg_gelu_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(dx), n, st), "gelu_bwd")
    torch.cuda.synchronize()
    _within(f"gelu n={n} y", y, H.gelu_f64(x), y32.detach())
    _within(f"gelu n={n} dx", dx, dy.double() * H.gelu_grad_f64(x), xr.grad)


@pytest.mark.parametrize("B,Hh,W,C_", [(3, 2, 6, 12), (2, 32, 32, 4100)], ids=["small", "stride_cap"])
def test_patch_merge_is_a_permutation(B, Hh, W, C_):
    """The forward is Swin's x[:, 0::2, 0::2], [1::2, 0::2], [0::2, 1::2], [1::2, 1::2] concatenated; the backward undoes it bit for bit.
    (H and W are even and C % 4 == 0, so the float4 count is even: 2 x 32 x 32 x 1025 items are the smallest such count past the cap.)"""
    lib, st = L.load(), stream(DEV)
    assert B == 3 or B * Hh * W * (C_ // 4) > STRIDE_CAP
    x = chan_affine((B, Hh, W, C_), C_)
    n = x.numel()
    xd = _dev(x)
    y, back = canary_out(n), canary_out(n)
    L.check(lib.hpfg_patch_merge_fwd(L.ptr(xd), L.ptr(y), B, Hh, W, C_, st), "patch_merge_fwd")
    L.check(lib.hpfg_patch_merge_bwd(L.ptr(y), L.ptr(back), B, Hh, W, C_, st), "patch_merge_bwd")
    torch.cuda.synchronize()
    _bit_equal("patch_merge fwd", y, H.patch_merge_ref(x))
    _bit_equal("patch_merge bwd(fwd)", back, x)


# ---- the epilogue switches of the GEMMs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(7, 8, 12), (130, 68, 36), (1568, 32, 2048)])
def test_gemm_relu_accumulate_and_ldc(m, n, k):
    """hpfg_gemm_f32 / hpfg_gemm_bf16x3 and their split-K forms with relu = 1 (and bias), with accumulate = 1 into a non-zero C, both at
    ldc = n + 8 with the NaN pattern in the gap.  (7, 8, 12) holds A column-major with 7 rows, which the split-bf16 kernels refuse; (1568,
    32, 2048) runs split-K.  The two switches are tested one at a time, where act(A B + bias) + C0 and the header's act(A B + bias + C0)
    are the same thing."""
    lib, st = L.load(), stream(DEV)
    gen = torch.Generator().manual_seed(m + n + k)
    A, Wt, bias, C0 = chan_affine((m, k), 0, gen), 0.2 * chan_affine((n, k), 0, gen), chan_affine((n,), 0, gen), chan_affine((m, n), 0, gen)
    ldc = n + 8
    prod64 = A.double() @ Wt.double().t() + bias.double()
    prod32 = torch.addmm(bias, A, Wt.t())
    assert bool((prod64 > 0).any() and (prod64 < 0).any())
    col_major = (m, n, k) == (7, 8, 12)
    Ad = _dev(A.t()) if col_major else _dev(A)
    sam, sak = (1, m) if col_major else (k, 1)
    Wd, bd = _dev(Wt), _dev(bias)
    ok16 = bool(lib.hpfg_gemm_bf16x3_ok(L.ptr(Ad), sam, sak, L.ptr(Wd), 1, k, m, n, k))
    assert ok16 != col_major
    s32, s16 = lib.hpfg_gemm_f32_splits(m, n, k), lib.hpfg_gemm_bf16x3_splits(m, n, k)
    assert (s32 > 1 and s16 > 1) == (k == 2048)
    kernels = [("f32", lib.hpfg_gemm_f32, None, 1.0), ("f32_splitk", lib.hpfg_gemm_f32_splitk, s32, 1.0)]
    if ok16:
        kernels += [("bf16x3", lib.hpfg_gemm_bf16x3, None, 8.0), ("bf16x3_splitk", lib.hpfg_gemm_bf16x3_splitk, s16, 8.0)]
    for name, fn, splits, extra in kernels:
        for relu, acc in ((1, 0), (0, 1)):
            out = canary_out(m * ldc)
            if acc:
                out[:m * ldc].view(m, ldc)[:, :n] = _dev(C0)
            args = [L.ptr(Ad), sam, sak, L.ptr(Wd), 1, k, L.ptr(out), ldc, m, n, k, L.ptr(bd), relu, acc]
            scratch = None
            if splits is not None:
                scratch = canary_out(splits * m * n)
                args.append(L.ptr(scratch))
            L.check(fn(*args, st), name)
            torch.cuda.synchronize()
            got = out[:m * ldc].view(m, ldc)
            assert bool((got[:, n:].contiguous().view(torch.int32) == H.NAN_BITS).all()) and H.bits_kept(out, m * ldc), (name, "gap or tail written")
            assert scratch is None or H.bits_kept(scratch, splits * m * n)
            want64 = torch.relu(prod64) if relu else prod64 + C0.double()
            want32 = torch.relu(prod32) if relu else prod32 + C0
            val = got[:, :n].cpu().double()
            assert bool(torch.isfinite(val).all()), (name, "an element of C was not written")
            err, bound = float((val - want64).abs().max()), bound_8x(want64, want32, 8.0 * extra)
            _report(f"gemm {name} {(m, n, k)} relu={relu} acc={acc}", err, bound)
            assert err <= bound, (name, relu, acc, err, bound)


def test_argument_errors():
    """Shapes a kernel cannot take are refused with -1, not launched."""
    lib, st = L.load(), stream(DEV)
    t = torch.zeros(4096, device=DEV)
    p = L.ptr(t)
    assert lib.hpfg_bnrelu_apply(p, p, p, p, p, None, 1.0, 1, p, 4, 0, st) == -1          # C = 0: no channel quad (the index math divides by C / 4)
    assert lib.hpfg_bnrelu_apply(p, p, p, p, p, None, 1.0, 1, p, 4, 6, st) == -1
    assert lib.hpfg_bnrelu_apply(p, p, p, p, p, None, 1.0, 0, p, 4, 8, st) == -1
    assert lib.hpfg_bnrelu_apply(p, p, p, p, p, None, 1.0, 1, p, 4, 96, st) == 0          # grid-stride over quads: any C % 4 == 0
    assert lib.hpfg_tok_col_stats(p, 4, 96, p, p, st) == -1                               # thread <-> (quad, row lane) needs (C / 4) | 256
    assert lib.hpfg_bnrelu_bwd(p, p, p, p, p, p, None, 1.0, 1, p, p, p, 4, 96, st) == -1
    assert lib.hpfg_ln_fwd(p, p, p, p, p, p, 2, 1028, st) == -1 and lib.hpfg_ln_fwd(p, p, p, p, p, p, 2, 6, st) == -1
    assert lib.hpfg_ln_bwd(p, p, p, p, p, p, p, p, p, 2, 1028, st) == -1
    assert lib.hpfg_linear_wgrad(p, p, p, p, 8, 6, 8, st) == -1 and lib.hpfg_linear_wgrad(p, p, p, p, 8, 8, 2, st) == -1
    assert lib.hpfg_resize_bilinear_bwd(p, p, 1, 4, 4, 2, 2, 4, st) == -1                 # the gather is written for upsampling
    assert lib.hpfg_patch_merge_fwd(p, p, 1, 3, 4, 4, st) == -1 and lib.hpfg_gelu_fwd(p, p, 6, st) == -1
    assert lib.hpfg_dwgelu_fwd(p, p, p, p, 1, 2, 2, 6, st) == -1
    torch.cuda.synchronize()
