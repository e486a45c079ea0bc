"""GPU: the whole-tile kernels of the 16-pixel-aligned layers -- conv_thin_kernel (csrc/conv_thin_kernel.h), fused_bwd_kernel
(csrc/fused_bwd_kernel.h) and first_wgrad_kernel (csrc/first_wgrad.hip) with the tile form it replaces -- kernel by kernel against float64.

The method is that of tests/test_gpu_conv_sources.py: every source is a helpers.conv_source (raw float32 tensors, its float64 restatement and the
rounding of its chain; no operand is read back through hpfg_act_materialize), the references are conv_ref_bound / dgrad_ref_bound /
wgrad_ref_bound and the one tolerance is their elementwise bound.  Every raw tensor sits at a channel offset inside a wider NaN-filled
buffer (aux_pstride differs from pstride), every table inside a wider NaN-filled table (bn_coff > 0), every output -- out, out2, slabs,
rows of partial sums -- is NaN-prefilled inside a larger buffer: the interior must come out finite, everything around it still NaN.  Every
test asserts that the launch took the kernel under test.  tests/test_host_logic.py checks the cases on the CPU (guards, the emulation
inside the bound, three wrong kernels outside it).

A conv_thin_kernel, its four instantiations | B fused_bwd_kernel, five instantiations and the first layer's weight-gradient-only form |
C first_wgrad_kernel and the tile form | D the partial-quad contract of PLAIN sources ("channels >= C read as zero", csrc/common.h).
Tile-count edges of A and B: one tile, fewer tiles than workgroups, and the walk case, where every workgroup's tile loop runs two or three
times.  Each test prints its largest error / bound ratio and, beside it, the ratio torch float32 on the CPU reaches (pytest -s); the
module prints the per-group maxima at its end."""
import contextlib
import ctypes as C

import pytest
import torch

from hpfg_amd import _lib as L
from tests import helpers as T
from tests.helpers import AdHocConv, NAN, OOFF, OPAD, O2OFF, O2PAD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B16 = L.MATH_BF16X3
GUARD = 2                   # NaN rows / slabs in front of and behind the rows of partial sums and the slabs of a launch
WORST = {}                  # group -> [kernel ratio, torch float32 ratio]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for grp in sorted(WORST):
        print(f"\n[tile_edges] group {grp}: largest error / bound = {WORST[grp][0]:.3g} (torch float32 on the CPU: {WORST[grp][1]:.3g})", end="")
    print()


def _id(case):
    return "-".join("x" if v is None else (str(v) or "sweep") for v in case)


def _note(group, tag, ratio, f32_ratio=None):
    w = WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], f32_ratio or 0.0)
    ctl = "" if f32_ratio is None else f" (torch float32 on the CPU: {f32_ratio:.3g})"
    print(f"[tile_edges] {group} {tag}: largest error / bound = {ratio:.3g}{ctl}")


def _check(group, tag, got, ref, bound, f32_ratio=None):
    """got (device or CPU, any float type) against the float64 reference within the bound, elementwise"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{tag}: {bad} of {got.numel()} elements were not written (NaN) or are not finite"
    ratio = float(((got - ref).abs() / bound).max())
    _note(group, tag, ratio, f32_ratio)
    assert ratio <= 1.0, f"{tag}: {ratio:.3g} x the bound off the float64 reference"


def _untouched(keep):
    """the NaN around every input interior is still there (no kernel wrote into a source)"""
    return all(bool(torch.isnan(b).any()) for b in keep if b.dtype == torch.float32)


def _guarded(rows, *shape):
    """(NaN buffer of GUARD + rows + GUARD blocks of `shape`, address of block GUARD)"""
    buf = torch.full((rows + 2 * GUARD,) + shape, NAN, device=DEV)
    return buf, buf[GUARD].data_ptr()


def _guards_kept(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _walked(edge, nwork, rows, H, W, wgs):
    if edge == "walk":
        assert T.walk_conditions(nwork, rows, W // 16, H // 16, wgs), f"{rows} workgroups on {nwork} tiles: no workgroup's tile loop runs twice"
    elif edge:
        assert nwork < rows and (edge == "one") == (nwork == 1) and (edge == "one" or W // 16 != H // 16)


# ---- A. conv_thin_kernel -----------------------------------------------------------------------------------------------------------------
def _thin_launch(case, layer, a0, a1):
    """-> output buffer (wide), rows of partial sums [rows][2][CoutPad] or None (with their guard rows), rows"""
    kind, _, N, H, W, cin, cout, _ = case
    lib = L.load()
    dgrad = kind == "dz"
    ca = T.thin_args(case)
    ca.a0, ca.a1 = a0, (a1 if a1 is not None else L.Act())
    ca.wpk = L.ptr(layer.wpk16_d if dgrad else layer.wpk16_f)
    ca.bias = None if dgrad else L.ptr(layer.bias_pad)
    out = torch.full((N, H, W, ca.out_pstride), NAN, device=DEV)
    ca.out = out.data_ptr() + 4 * OOFF
    ca.stat_partials = 256 if not dgrad else None
    rows = lib.hpfg_conv_stat_rows(C.byref(ca))
    old = T.thin_args(case, B16 | T.OLD_KERNEL)
    assert rows > 0 and rows % 8 == 0 and rows != lib.hpfg_conv_stat_rows(C.byref(old)), f"{case}: the launch does not go to conv_thin_kernel"
    part = None
    if not dgrad:
        part, ca.stat_partials = _guarded(rows, 2, ca.CoutPad)
    L.check(lib.hpfg_conv_fwd(C.byref(ca), T.stream(DEV)), "conv_fwd")
    torch.cuda.synchronize()
    return out, part, rows


@pytest.mark.parametrize("case", T.THIN_CASES, ids=_id)
def test_thin_conv_against_float64(case):
    kind, p, N, H, W, cin, cout, edge = case
    d = T.thin_case(case)
    layer = AdHocConv(cin, cout, 9, DEV, seed=d["seed"], hw=(H, W))
    a0, a1, keep = T.device_source(d["s"], H, W)
    out, part, rows = _thin_launch(case, layer, a0, a1)
    _walked(edge, N * (H // 16) * (W // 16), rows, H, W, T.THIN_INST[kind][2])
    oc = cin if kind == "dz" else cout
    got, clean = T.interior(out, oc, OOFF)
    assert clean and _untouched(keep), f"{case}: the launch wrote outside its output channels"
    tag = f"thin {_id(case)}"
    _check("A", tag, got, d["ref"], d["bound"], d["f32"])
    if part is not None:
        assert _guards_kept(part), f"{tag}: a row outside the {rows} the launch reports was written"
        pr = part[GUARD:GUARD + rows].double().cpu()
        assert bool(torch.isfinite(pr).all()), f"{tag}: a row of partial sums was not written (a workgroup without a tile writes zeros)"
        assert bool((pr[:, :, cout:] == 0).all()), f"{tag}: a partial sum of a padded channel is not 0"
        ratio = T.fwd_sums_ratio(pr.sum(0)[:, :cout], got)
        _note("A", tag + " statistics rows", ratio)
        assert ratio <= 1.0, f"{tag}: statistics rows {ratio:.3g} x the fp32 summation bound off the float64 sums of the output"


# ---- B. fused_bwd_kernel -----------------------------------------------------------------------------------------------------------------
def _first_input(sx, layout):
    """the network input (conv_source "plain", [N,H,W,cin]) on the device as a STRIDED source -> (act, buffer).  nchw: contiguous; crop: a
    window of a wider, taller NaN-filled NCHW image (sy > W, sn > H sy); nhwc3: channel 1 of an NHWC 3-channel image, the others NaN (sx = 3)"""
    x = sx["z"].permute(0, 3, 1, 2).contiguous()
    N, cin, H, W = x.shape
    a = L.Act()
    a.mode, a.C, a.Hs, a.Ws = L.ACT_STRIDED, cin, H, W
    if layout == "nchw":
        buf = x.to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = L.ptr(buf), cin * H * W, H * W, W, 1
    elif layout == "crop":
        buf = torch.full((N, cin, H + 5, W + 7), NAN, device=DEV)
        buf[:, :, 2:2 + H, 3:3 + W] = x.to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = buf[0, 0, 2, 3:].data_ptr(), buf.stride(0), buf.stride(1), buf.stride(2), 1
    else:
        assert cin == 1
        buf = torch.full((N, H, W, 3), NAN, device=DEV)
        buf[..., 1] = x[:, 0].to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = buf[0, 0, 0, 1:].data_ptr(), H * W * 3, 1, W * 3, 3
    return a, buf


def _fused_launch(case, layer, xa0, xa1, g, bwd_of=None):
    """-> dict(out, out2: wide buffers or None; slab, part: guarded buffers (part None without bwd_of); grid)"""
    ak, _, gk, _, N, H, W, cin, cout, split, _ = case
    lib = L.load()
    fa = T.fused_args(case)
    fa.xa0, fa.xa1 = xa0, (xa1 if xa1 is not None else L.Act())
    d = fa.d
    d.a0 = g
    r = dict(out=None, out2=None, part=None)
    if cin >= 16:
        d.wpk = L.ptr(layer.wpk16_d)
        r["out"] = torch.full((N, H, W, d.out_pstride), NAN, device=DEV)
        d.out = r["out"].data_ptr() + 4 * OOFF
        if split:
            r["out2"] = torch.full((N, H, W, d.out2_pstride), NAN, device=DEV)
            d.out2 = r["out2"].data_ptr() + 4 * O2OFF
    grid = r["grid"] = lib.hpfg_fused_bwd_grid(C.byref(fa))
    assert grid > 0, f"{case}: no fused instantiation takes the layer ({lib.hpfg_last_error()})"
    if bwd_of is not None:
        r["part"], d.stat_partials = _guarded(grid, 2, fa.CinPad)
        d.bwd_stats, d.bwd_of = 1, bwd_of
    r["slab"], fa.slab = _guarded(grid, 9, fa.CinPad, fa.CoutPad)
    L.check(lib.hpfg_fused_bwd(C.byref(fa), T.stream(DEV)), "fused_bwd")
    torch.cuda.synchronize()
    return r


def _dw_of(tag, slab, grid, cin, cout):
    """the guarded slabs [.., 9, CinPad, CoutPad] of `grid` workgroups -> dW [cout, cin, 3, 3], summed in float64 (the padded rows and columns
    are nobody's result: hpfg_slab_reduce_multi reads [:Cin, :Cout])"""
    assert _guards_kept(slab), f"{tag}: a slab outside the {grid} of the launch was written"
    s = slab[GUARD:GUARD + grid, :, :cin, :cout]
    bad = int((~torch.isfinite(s)).sum())
    assert bad == 0, f"{tag}: {bad} of {s.numel()} slab elements were not written (NaN) or are not finite"
    return s.double().sum(0).permute(2, 1, 0).reshape(cout, cin, 3, 3)


def _dz_source(sg, H, W, strided_if_odd=True):
    g, _, keep = T.device_source(sg, H, W)
    if sg["kind"] == "plain" and sg["C"] % 4 and strided_if_odd:
        T.as_strided_act(g)
    return g, keep


def _fused_case(group, case, g=None, gkeep=None, tag=None):
    ak, p_in, gk, p_out, N, H, W, cin, cout, split, edge = case
    d = T.fused_case(case)
    tag = tag or f"fused {_id(case)}"
    layer = AdHocConv(cin, cout, 9, DEV, seed=d["seed"], hw=(H, W))
    if cin >= 16:
        xa0, xa1, keep = T.device_source(d["sa"], H, W)
    else:
        xa0, xb = _first_input(d["sa"], "nchw")      # (contiguous: no NaN around it)
        xa1, keep = None, []
    if g is None:
        g, gkeep = _dz_source(d["sg"], H, W)
    bwd_of = None
    if ak == "bnact" and not split:      # the backward sums of the layer below ride along wherever the kernel offers them
        bwd_of = L.Act()
        bwd_of.z, bwd_of.bn, bwd_of.mode, bwd_of.C, bwd_of.Hs, bwd_of.Ws = xa0.z, xa0.bn, L.ACT_DZ, cin, H, W
        bwd_of.pstride, bwd_of.bn_stride, bwd_of.bn_coff, bwd_of.drop_p, bwd_of.drop_seed = xa0.pstride, xa0.bn_stride, xa0.bn_coff, xa0.drop_p, xa0.drop_seed
    r = _fused_launch(case, layer, xa0, xa1, g, bwd_of)
    inst = [v for v in T.FUSED_INST.values() if v[:3] == (ak, gk, cin)][0]
    _walked(edge, N * (H // 16) * (W // 16), r["grid"], H, W, inst[4])
    assert _untouched(keep) and _untouched(gkeep), f"{tag}: the launch wrote into a source"
    dx = None
    if d["dx"] is not None:
        ref, bound, f32 = d["dx"]
        lo, clean = T.interior(r["out"], split or cin, OOFF)
        assert clean, f"{tag}: dX wrote outside its channels"
        dx = lo
        if split:
            hi, clean2 = T.interior(r["out2"], cin - split, O2OFF)
            assert clean2, f"{tag}: the second half of dX wrote outside its channels"
            dx = torch.cat([lo, hi], -1)
        _check(group, tag + " dX", dx, ref, bound, f32)
    ref, bound, f32 = d["dw"]
    _check(group, tag + " dW", _dw_of(tag, r["slab"], r["grid"], cin, cout), ref, bound, f32)
    if bwd_of is not None:
        part = r["part"]
        assert _guards_kept(part), f"{tag}: a row of backward sums outside the {r['grid']} of the launch was written"
        pr = part[GUARD:GUARD + r["grid"]].double().cpu()
        assert bool(torch.isfinite(pr).all()), f"{tag}: a row of backward sums was not written (a workgroup without a tile writes zeros)"
        # g = dX * keep / (1 - p) * LeakyReLU'(z scale + shift) of the layer below, from its raw z, its table and the launch's own dX
        sa = d["sa"]
        z64 = sa["z"].double()
        slope = torch.where(T.lrelu_slope(z64, sa["tab"][L.BN_SCALE].double(), sa["tab"][L.BN_SHIFT].double()) == 1.0, 1.0, T.LEAKY32)
        g64 = dx.cpu().double() * T.keep_f64(tuple(z64.shape), p_in, sa["dseed"]) * slope
        ratio = T.bwd_sums_ratio(pr.sum(0), g64.reshape(-1, cin), z64.reshape(-1, cin), sa["tab"])
        _note(group, tag + " backward sums", ratio)
        assert ratio <= 1.0, f"{tag}: backward sums {ratio:.3g} x the bound off the float64 sums"


@pytest.mark.parametrize("case", T.FUSED_CASES, ids=_id)
def test_fused_bwd_against_float64(case):
    _fused_case("B", case)


# ---- C. first_wgrad_kernel and the tile form ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _first_wgrad(opt):
    lib = L.load()
    prev = lib.hpfg_set_option(L.OPT_FIRST_WGRAD, opt)
    try:
        yield
    finally:
        lib.hpfg_set_option(L.OPT_FIRST_WGRAD, prev)


@pytest.mark.parametrize("case", T.FIRST_CASES, ids=_id)
def test_first_layer_weight_gradient_against_float64(case):
    N, H, W, cin, p, layout, streaming = case
    d = T.first_case(N, H, W, cin, p)
    lib = L.load()
    xa, xbuf = _first_input(d["sx"], layout)
    g, gkeep = _dz_source(d["sg"], H, W)
    fa = L.FusedBwdArgs()
    fa.xa0, fa.xa1 = xa, L.Act()
    fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = cin, 16, 16, 16
    fa.d.a0, fa.d.math, fa.d.Cout, fa.d.CoutPad, fa.d.N, fa.d.H, fa.d.W, fa.d.taps = g, B16, cin, 16, N, H, W, 9
    stream_form = bool(streaming) and cin == 1
    tag = f"first layer {_id(case)} ({'first_wgrad_kernel' if stream_form else 'tile form'})"
    with _first_wgrad(streaming):
        grid = lib.hpfg_fused_bwd_grid(C.byref(fa))
        tiles = N * (H // 16) * (W // 16)
        want = min(N * H, 768) if stream_form else min((-(-tiles // -(-tiles // 512)) + 7) // 8 * 8, 512)
        assert grid == want and (stream_form or grid != min(N * H, 768)), f"{tag}: {grid} workgroups, not the {want} of the kernel under test"
        slab, fa.slab = _guarded(grid, 9, 16, 16)
        L.check(lib.hpfg_fused_bwd(C.byref(fa), T.stream(DEV)), "fused_bwd")
        torch.cuda.synchronize()
    assert _untouched(gkeep) and (layout == "nchw" or bool(torch.isnan(xbuf).any()))
    dw = _dw_of(tag, slab, grid, cin, 16)
    _check("C", tag, dw, d["ref"], d["b_stream"] if stream_form else d["b_tile"], d["f32"])


# ---- D. the partial-quad contract of PLAIN sources ---------------------------------------------------------------------------------------
def _plain_source(sg, layout):
    """a plain conv_source with C % 4 != 0 as an HPFG_ACT_PLAIN source (whole-quad loads) -> (act, buffers).  tail: the tight tensor at the
    front of a larger allocation whose rest is NaN -- the quad of the last pixel runs into it, nothing is read outside the allocation;
    wide: a pixel stride of 4 channels more than C rounded up, NaN between the pixels"""
    z = sg["z"]
    N, H, W, c = z.shape
    a = L.Act()
    a.mode, a.C, a.Hs, a.Ws = L.ACT_PLAIN, c, H, W
    if layout == "tail":
        buf = torch.full((z.numel() + 64,), NAN, device=DEV)
        buf[:z.numel()] = z.reshape(-1).to(DEV)
        a.z, a.pstride = L.ptr(buf), c
    else:
        buf, a.z = T.wide(z, (c + 3) // 4 * 4 - c + 8, 4)
        a.pstride = buf.shape[-1]
    return a, [buf]


@pytest.mark.parametrize("layout", T.QUAD_LAYOUTS)
@pytest.mark.parametrize("case", T.QUAD_FUSED, ids=_id)
def test_plain_partial_quad_fused_bwd(case, layout):
    g, gkeep = _plain_source(T.fused_case(case)["sg"], layout)
    _fused_case("D", case, g, gkeep, tag=f"PLAIN {layout} fused {_id(case)}")


@pytest.mark.parametrize("layout", T.QUAD_LAYOUTS)
@pytest.mark.parametrize("case", T.QUAD_DGRAD, ids=_id)
def test_plain_partial_quad_chunked_dgrad(case, layout):
    kind, p, N, H, W, cin, cout, _, _ = case
    seed = T.case_seed(*case)
    s = T.conv_source(kind, seed, N, H, W, cout, p)
    w, _ = T.adhoc_weights(cin, cout, 9, seed)
    ref, bound = T.dgrad_ref_bound(s["v"], s["d"], w)
    layer = AdHocConv(cin, cout, 9, DEV, seed=seed, hw=(H, W))
    g, gkeep = _plain_source(s, layout)
    out, _ = layer.conv(g, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + OPAD, out_coff=OOFF)
    torch.cuda.synchronize()
    got, clean = T.interior(out, cin, OOFF)
    assert clean and _untouched(gkeep)
    _check("D", f"PLAIN {layout} chunked dgrad {_id(case)}", got, ref, bound, T.f32_conv_ratio("dgrad", ref, bound, s["v"], w))


@pytest.mark.parametrize("layout", T.QUAD_LAYOUTS)
@pytest.mark.parametrize("case", T.QUAD_WGRAD, ids=_id)
def test_plain_partial_quad_chunked_wgrad(case, layout):
    ak, pa, gk, pg, N, H, W, cin, cout, taps = case
    seed = T.case_seed(*case)
    sa, sg = T.conv_source(ak, seed, N, H, W, cin, pa), T.conv_source(gk, seed + 1, N, H, W, cout, pg)
    w, _ = T.adhoc_weights(cin, cout, taps, seed)
    ref, bound = T.wgrad_ref_bound(sa["v"], sa["d"], sg["v"], sg["d"], w.shape)
    layer = AdHocConv(cin, cout, taps, DEV, seed=seed, hw=(H, W))
    a0, a1, keep = T.device_source(sa, H, W)
    g, gkeep = _plain_source(sg, layout)
    dw = layer.wgrad(a0, a1, g, N, H, W, math=B16, slab_nan=True)
    torch.cuda.synchronize()
    assert _untouched(keep) and _untouched(gkeep)
    _check("D", f"PLAIN {layout} chunked wgrad {_id(case)}", dw, ref, bound, T.f32_conv_ratio("wgrad", ref, bound, sa["v"], sg["v"], w.shape))


@pytest.mark.parametrize("layout", T.QUAD_LAYOUTS)
@pytest.mark.parametrize("c", T.QUAD_C)
def test_plain_partial_quad_materialize(c, layout):
    N, H, W = 3, 10, 34
    s = T.conv_source("plain", T.case_seed("plain", N, H, W, c), N, H, W, c)
    g, gkeep = _plain_source(s, layout)
    buf = torch.full((N * H * W * c + T.PAD,), NAN, device=DEV)
    L.check(L.load().hpfg_act_materialize(C.byref(g), None, N, H, W, L.ptr(buf), T.stream(DEV)), "act_materialize")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[N * H * W * c:]).all()) and _untouched(gkeep), "hpfg_act_materialize wrote behind its output"
    assert torch.equal(buf[:N * H * W * c].cpu().reshape(N, H, W, c), s["z"]), "a PLAIN source is copied exactly"
    _note("D", f"PLAIN {layout} materialize C={c}", 0.0)
