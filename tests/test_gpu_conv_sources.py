"""GPU: the chunked split-bf16 convolutions (csrc/conv_bf16_kernel.h: forward, dgrad, 1x1, their epilogues and staging side effects), the
weight gradient (csrc/wgrad_bf16_kernel.h) and the staged loaders that feed both (csrc/stage.h), kernel by kernel against float64.

Every virtual source is restated in float64 from its raw tensors and table rows (tests/helpers.py: bnact_f64, pool_f64, cat_f64, dz_f64,
upbwd_f64 -- no project kernel, no hpfg_act_materialize), the convolution is F.conv2d / its autograd in float64, and the one tolerance is the
bound stated in tests/helpers.py beside _split_bound, computed from the data of the case.  tests/test_host_logic.py checks on the CPU that the
split-product emulation itself stays inside that bound for every case below, and that the inputs are clear of LeakyReLU / arg-max ties.

Every raw tensor lives at a channel offset inside a wider NaN-filled buffer (pixel stride > C), every table inside a wider NaN-filled table
(bn_coff > 0), every output inside a wider NaN-prefilled buffer: the interior must come out finite, the neighbours untouched.

A forward 3x3 | B dgrad 3x3 | C 1x1 | D stage_out | E weight gradient.  Each test prints its largest error / bound ratio and, beside it, the
ratio torch float32 conv2d on the CPU reaches on the same operands (pytest -s); the module prints the per-group maxima at its end."""
import contextlib

import pytest
import torch

from hpfg_amd import _lib as L
from tests import helpers as T
from tests.helpers import AdHocConv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B16 = L.MATH_BF16X3
NAN = T.NAN
PADC, COFF, APAD, AOFF, TPAD, TOFF, OPAD, OOFF, O2PAD, O2OFF = T.PADC, T.COFF, T.APAD, T.AOFF, T.TPAD, T.TOFF, T.OPAD, T.OOFF, T.O2PAD, T.O2OFF
_wide, _interior, _device_source = T.wide, T.interior, T.device_source      # (shared with tests/test_gpu_tile_edges.py)
WORST = {}                  # group -> [kernel ratio, torch float32 ratio]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for grp in sorted(WORST):
        print(f"\n[conv_sources] group {grp}: largest error / bound = {WORST[grp][0]:.3g} (torch float32 on the CPU: {WORST[grp][1]:.3g})", end="")
    print()


def _id(case):
    return "-".join("x" if v is None else str(v) for v in case)


def _note(group, tag, ratio, f32_ratio=None):
    w = WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], f32_ratio or 0.0)
    ctl = "" if f32_ratio is None else f" (torch float32 on the CPU: {f32_ratio:.3g})"
    print(f"[conv_sources] {group} {tag}: largest error / bound = {ratio:.3g}{ctl}")


def _check(group, tag, got, ref, bound, f32_ratio=None):
    """got (device or CPU, any float type) against the float64 reference within the bound, elementwise"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: an element was not written (NaN) or is not finite"
    ratio = float(((got - ref).abs() / bound).max())
    _note(group, tag, ratio, f32_ratio)
    assert ratio <= 1.0, f"{tag}: {ratio:.3g} x the bound off the float64 reference"
    return ratio


@contextlib.contextmanager
def _narrow(opt):
    """HPFG_OPT_NARROW_DEEP at `opt` for the block (None: at its default, 128 workgroups), restored afterwards"""
    lib = L.load()
    if opt is None:
        assert lib.hpfg_get_option(L.OPT_NARROW_DEEP) == 128
        yield
        return
    prev = lib.hpfg_set_option(L.OPT_NARROW_DEEP, opt)
    try:
        yield
    finally:
        lib.hpfg_set_option(L.OPT_NARROW_DEEP, prev)


def _inputs_untouched(keep):
    """the NaN around every input interior is still there and the interiors are still finite (no kernel wrote into a source)"""
    return all(bool(torch.isnan(b).any()) for b in keep if b.dtype == torch.float32)


def _stats_check(group, tag, part, rows, cpad, cout, ref, bound):
    """rows of (sum z, sum z^2) summed against float64 sums of the float64 output: the fp32 summation bound of test_gpu_bn_acc._fwd_sums_check,
    (n + 2) * 2^-24 * sum|term|, plus the output bound summed (b for z; 2 |z| b + b^2 for z^2)"""
    p = part.view(-1, 2, cpad).double().cpu()
    assert bool(torch.isfinite(p).all()) and bool((p[rows:] == 0).all()), f"{tag}: a row past the {rows} the launch reports was written"
    z, b = ref.reshape(-1, cout), bound.reshape(-1, cout)
    n = z.shape[0]
    worst = 0.0
    for which, (term, tb) in enumerate(((z, b), (z * z, 2 * z.abs() * b + b * b))):
        lim = (n + 2) * T.U24 * term.abs().sum(0) + tb.sum(0)
        worst = max(worst, float(((p[:rows, which, :cout].sum(0) - term.sum(0)).abs() / lim).max()))
    _note(group, tag + " statistics rows", worst)
    assert worst <= 1.0, f"{tag}: statistics rows {worst:.3g} x the bound off the float64 sums"


def _forward(group, case, taps):
    kind, p, N, H, W, cin, cout, opt = case
    seed = T.case_seed(*case)
    s = T.conv_source(kind, seed, N, H, W, cin, p)
    w, b = T.adhoc_weights(cin, cout, taps, seed)
    ref, bound = T.conv_ref_bound(s["v"], s["d"], w, b)
    with _narrow(opt):
        layer = AdHocConv(cin, cout, taps, DEV, seed=seed, hw=(H, W))
        a0, a1, keep = _device_source(s, H, W)
        out, part = layer.conv(a0, a1, N, H, W, stats=True, math=B16, out_pstride=cout + OPAD, out_coff=OOFF)
        torch.cuda.synchronize()
    got, clean = _interior(out, cout, OOFF)
    assert clean and _inputs_untouched(keep), f"{case}: the launch wrote outside its output channels"
    tag = f"{taps == 9 and '3x3' or '1x1'} forward {_id(case)}"
    _check(group, tag, got, ref, bound, T.f32_conv_ratio("conv", ref, bound, s["v"], w, b))
    _stats_check(group, tag, part, layer.rows, layer.cout_pad, cout, ref, bound)
    return layer


# ---- A. forward 3x3 on 4 x 16-pixel tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FWD3_CASES, ids=_id)
def test_forward_3x3_against_float64(case):
    _forward("A", case, 9)


def test_forward_3x3_persistent_loop_walks_several_tiles():
    """more tiles than the workgroups persistent_grid() keeps resident (8 slices of 32 channels: 64 per slice): every workgroup walks two"""
    _, _, N, H, W, _, _, _ = T.FWD3_PERSISTENT
    layer = _forward("A", T.FWD3_PERSISTENT, 9)
    tiles = N * ((H + 3) // 4) * ((W + 15) // 16)
    assert 0 < layer.rows < tiles, (layer.rows, tiles)


# ---- B. dgrad 3x3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.DGRAD3_CASES, ids=_id)
def test_dgrad_3x3_against_float64_autograd(case):
    kind, p, N, H, W, cin, cout, opt, epi = case
    seed = T.case_seed(*case)
    s = T.conv_source(kind, seed, N, H, W, cout, p)
    w, _ = T.adhoc_weights(cin, cout, 9, seed)
    ref, bound = T.dgrad_ref_bound(s["v"], s["d"], w)
    f32 = T.f32_conv_ratio("dgrad", ref, bound, s["v"], w)
    tag = f"3x3 dgrad {_id(case)}"
    with _narrow(opt):
        layer = AdHocConv(cin, cout, 9, DEV, seed=seed, hw=(H, W))
        g0, _, keep = _device_source(s, H, W)
        if epi == "split":          # both halves land where they belong
            half = cin // 2         # (out2 is wide enough for a channel offset that forgets to subtract out_split to stay inside it)
            out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=half + OPAD, out_coff=OOFF, out_split=half,
                                out2_pstride=cin + O2PAD, out2_coff=O2OFF)
            lo, clean = _interior(out, half, OOFF)
            hi, clean2 = _interior(layer.out2, cin - half, O2OFF)
            assert clean and clean2, "out_split: a half wrote outside its channels"
            _check("B", tag + " [out]", lo, ref[..., :half], bound[..., :half], f32)
            _check("B", tag + " [out2]", hi, ref[..., half:], bound[..., half:], f32)
            return
        if epi == "pool":           # bwd_stats == 2: the max-pool backward in the epilogue, in place on bwd_of.aux
            be = T.pool_epilogue_source(T.pool_epilogue_seed(case), N, H, W, cin)
            bo, _, bkeep = _device_source(be, 2 * H, 2 * W)
            out, part = layer.conv(g0, None, N, H, W, stats=True, dgrad=True, math=B16, bwd_stats=2, bwd_of=bo, out_pstride=cin + OPAD, out_coff=OOFF)
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()), "bwd_stats == 2 does not write `out`"
            got, clean = _interior(bkeep[2], cin, AOFF)
            assert clean, "the in-place max-pool backward wrote outside the gradient's channels"
            got = got.cpu().double()
            dA = be["dA"].double()
            hit = T.pool_scatter_f64(torch.ones_like(ref), be["first"]) == 1.0
            assert torch.equal(got[~hit], dA[~hit]), "an element that is no window's arg-max changed"
            want = dA + T.pool_scatter_f64(ref, be["first"])
            lim = T.pool_scatter_f64(bound, be["first"]) + T.U24 * want.abs()          # the dgrad bound of dP, and the rounding of the fp32 add
            assert int(hit.sum()) == ref.numel()
            _check("B", tag, got[hit], want[hit], lim[hit], f32)
            assert bool(torch.isfinite(part).all())
            return
        out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + OPAD, out_coff=OOFF)
        got, clean = _interior(out, cin, OOFF)
        assert clean and _inputs_untouched(keep)
        _check("B", tag, got, ref, bound, f32)
        if epi == "stats1":         # bwd_stats == 1: the backward sums ride along, the output is unchanged
            below = T.conv_source("dz", seed + 1, N, H, W, cin, 0.3)
            bo, _, bkeep = _device_source(below, H, W)
            out1, part = layer.conv(g0, None, N, H, W, stats=True, dgrad=True, math=B16, bwd_stats=1, bwd_of=bo, out_pstride=cin + OPAD, out_coff=OOFF)
            got1, clean = _interior(out1, cin, OOFF)
            assert clean and torch.equal(got1, got), "bwd_stats == 1 changed the output"
            assert bool(torch.isfinite(part).all())


# ---- C. 1x1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FWD1_CASES, ids=_id)
def test_forward_1x1_against_float64(case):
    _forward("C", case + (None,), 1)


@pytest.mark.parametrize("case", T.DGRAD1_CASES, ids=_id)
def test_dgrad_1x1_plain_against_float64_autograd(case):
    N, H, W, cin, cout = case
    full = ("plain", 0.0) + case + (None, None)
    seed = T.case_seed(*full)
    s = T.conv_source("plain", seed, N, H, W, cout)
    w, _ = T.adhoc_weights(cin, cout, 1, seed)
    ref, bound = T.dgrad_ref_bound(s["v"], s["d"], w)
    layer = AdHocConv(cin, cout, 1, DEV, seed=seed, hw=(H, W))
    g0, _, keep = _device_source(s, H, W)
    out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + OPAD, out_coff=OOFF)
    got, clean = _interior(out, cin, OOFF)
    assert clean and _inputs_untouched(keep)
    _check("C", f"1x1 dgrad {_id(case)}", got, ref, bound, T.f32_conv_ratio("dgrad", ref, bound, s["v"], w))


@pytest.mark.parametrize("case", T.UPBWD_CASES, ids=_id)
def test_dgrad_1x1_gathers_the_upsample_backward(case):
    """HPFG_ACT_UPBWD: `out` against float64 autograd from the float64 transposed interpolation, stage_out against that gathered gradient, the
    rows of side_sums, summed, against its channel sums"""
    N, H, W, cin, cout = case
    seed = T.case_seed(*case)
    gen = torch.Generator().manual_seed(seed)
    gup = torch.randn(N, 2 * H, 2 * W, cout, generator=gen)
    v, d = T.upbwd_f64(gup)
    w, _ = T.adhoc_weights(cin, cout, 1, seed)
    ref, bound = T.dgrad_ref_bound(v, d, w)
    layer = AdHocConv(cin, cout, 1, DEV, seed=seed, hw=(H, W))
    gb, gptr = _wide(gup)
    a = L.Act()
    a.z, a.mode, a.C, a.Hs, a.Ws, a.pstride = gptr, L.ACT_UPBWD, cout, H, W, cout + PADC
    rows = N * ((H + 7) // 8) * ((W + 7) // 8)
    stage = torch.full((N, H, W, cout), NAN, device=DEV)
    side = torch.full((rows, cout), NAN, device=DEV)
    out, _ = layer.conv(a, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + OPAD, out_coff=OOFF, stage_out=stage, side_sums=side)
    torch.cuda.synchronize()
    assert layer.rows == rows
    got, clean = _interior(out, cin, OOFF)
    assert clean and _inputs_untouched([gb])
    tag = f"1x1 UPBWD dgrad {_id(case)}"
    _check("C", tag, got, ref, bound, T.f32_conv_ratio("dgrad", ref, bound, v, w))
    _check("C", tag + " [stage_out]", stage, v, d)
    npix = N * H * W
    lim = d.reshape(npix, cout).sum(0) + (npix + 2) * T.U24 * v.abs().reshape(npix, cout).sum(0)
    assert bool(torch.isfinite(side).all()), "a row of side_sums was not written"
    _check("C", tag + " [side_sums]", side.double().sum(0), v.reshape(npix, cout).sum(0), lim)


# ---- D. stage_out and the weight gradient that reads it ----------------------------------------------------------------------------------
def _pair(t):
    """(hi, lo) float64 [N,H,W,C] of a side tensor: bf16 [N][H][W][C / 8][hi 8 | lo 8] in a buffer of N*H*W*C fp32 words"""
    n, h, w, c = t.shape
    p = t.view(torch.bfloat16).reshape(n, h, w, c // 8, 2, 8).cpu()
    return p[..., 0, :].reshape(n, h, w, c).double(), p[..., 1, :].reshape(n, h, w, c).double()


def _split_act(t, C_, H, W):
    a = L.Act()
    a.z, a.mode, a.C, a.Hs, a.Ws, a.pstride = L.ptr(t), L.ACT_SPLIT16, C_, H, W, C_
    return a


@pytest.mark.parametrize("kind,p", T.STAGE_CASES)
def test_stage_out_pairs_and_the_weight_gradient_from_them(kind, p):
    N, H, W, Cc = 3, 10, 34, 64
    case = (kind, p, N, H, W, Cc, Cc)
    seed = T.case_seed(*case)
    si, sg = T.conv_source(kind, seed, N, H, W, Cc, p), T.conv_source("dz", seed + 1, N, H, W, Cc, 0.3)
    w, b = T.adhoc_weights(Cc, Cc, 9, seed)
    lib = L.load()
    assert N * 3 * 3 * (Cc // 64) <= lib.hpfg_get_option(L.OPT_NARROW_DEEP)      # 32-wide slices: two output-channel slices, slice 0 stores
    layer = AdHocConv(Cc, Cc, 9, DEV, seed=seed, hw=(H, W))
    a0, a1, keep = _device_source(si, H, W)
    g0, _, gkeep = _device_source(sg, H, W)
    stage = {}
    for name, src, dgrad, s in (("input", (a0, a1), False, si), ("dZ", (g0, None), True, sg)):
        buf = torch.full((N, H, W, Cc), NAN, device=DEV)
        out, _ = layer.conv(src[0], src[1], N, H, W, dgrad=dgrad, math=B16, stage_out=buf)
        torch.cuda.synchronize()
        first = buf.clone()
        hi, lo = _pair(buf)
        assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()), f"{name}: a pixel of the stored pair was not written"
        _check("D", f"stage_out {kind} {name} pair", hi + lo, s["v"], 2.0 ** -16 * s["v"].abs() + s["d"])
        buf.view(torch.bfloat16).fill_(NAN)          # written once per launch, whatever was there: a second launch leaves no NaN and the same bits
        out2, _ = layer.conv(src[0], src[1], N, H, W, dgrad=dgrad, math=B16, stage_out=buf)
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), first.view(torch.int32)) and torch.equal(out2, out), f"{name}: the second launch stored other bits"
        ref, bound = T.dgrad_ref_bound(s["v"], s["d"], w) if dgrad else T.conv_ref_bound(s["v"], s["d"], w, b)
        _check("D", f"stage_out {kind} {name} conv output", out, ref, bound)
        stage[name] = buf
    dw = layer.wgrad(_split_act(stage["input"], Cc, H, W), None, _split_act(stage["dZ"], Cc, H, W), N, H, W, math=B16, slab_nan=True)
    ref, bound = T.wgrad_ref_bound(si["v"], si["d"], sg["v"], sg["d"], w.shape)
    _check("D", f"stage_out {kind} weight gradient from SPLIT16 sources", dw, ref, bound, T.f32_conv_ratio("wgrad", ref, bound, si["v"], sg["v"], w.shape))
    assert _inputs_untouched(keep) and _inputs_untouched(gkeep)


# ---- E. weight gradient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.WGRAD_CASES, ids=_id)
def test_weight_gradient_against_float64_autograd(case):
    ak, pa, gk, pg, N, H, W, cin, cout, taps = case
    seed = T.case_seed(*case)
    sa, sg = T.conv_source(ak, seed, N, H, W, cin, pa), T.conv_source(gk, seed + 1, N, H, W, cout, pg)
    w, _ = T.adhoc_weights(cin, cout, taps, seed)
    ref, bound = T.wgrad_ref_bound(sa["v"], sa["d"], sg["v"], sg["d"], w.shape)
    layer = AdHocConv(cin, cout, taps, DEV, seed=seed, hw=(H, W))
    a0, a1, keep = _device_source(sa, H, W)
    g0, _, gkeep = _device_source(sg, H, W)
    dw = layer.wgrad(a0, a1, g0, N, H, W, math=B16, slab_nan=True)
    torch.cuda.synchronize()
    assert _inputs_untouched(keep) and _inputs_untouched(gkeep)
    _check("E", f"weight gradient {_id(case)}", dw, ref, bound, T.f32_conv_ratio("wgrad", ref, bound, sa["v"], sg["v"], w.shape))
