"""GPU: the first conv forward and the stand-alone backward kernels, kernel by kernel through the C ABI against float64.

1 hpfg_conv3x3_first_fwd / _bump / _acc (conv_first_kernel, conv_first_mfma_kernel<1|3>, csrc/conv.hip) | 2 hpfg_upsample2x_bwd / _sums
(upsample_bwd_kernel, csrc/misc.hip) | 3 hpfg_channel_sum_partials / hpfg_channel_sum and 4 hpfg_slab_reduce_multi (csrc/wgrad.hip) |
5 hpfg_bn_bwd_reduce / _pool (csrc/bn.hip) and hpfg_pool_scatter_add | 6 hpfg_dropout_mask (csrc/misc.hip).

One rule: max |got - ref| / bound <= 1 against the float64 restatements of tests/helpers.py ("the first conv and the stand-alone backward
kernels"), whose bounds are derived -- (n + 2) * 2^-24 * sum|term| for a sum of n fp32 terms -- not tuned.  The cases, their reasons and the
launch geometries they aim at are stated there; tests/test_standalone_laws_host.py holds the laws against torch float64, the geometries
against the library, and shows that every named wrong kernel lies at least 4 bounds off.  Every output is a helpers.canary_out / padded
buffer: what a launch must write comes out finite, everything behind it keeps its bits.  Each test prints its worst ratio (pytest -s), the
module the per-group maxima at its end."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from oracle import rng_ref
from tests import helpers as T
from tests.helpers import NAN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for grp in sorted(WORST):
        print(f"\n[standalone_edges] group {grp}: largest error / bound = {WORST[grp]:.3g}", end="")
    print()


def _note(group, tag, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"[standalone_edges] {group} {tag}: largest error / bound = {ratio:.3g}")
    assert ratio <= 1.0, f"{group} {tag}: {ratio:.3g} x the bound off the float64 law"


def _ratio(tag, got, ref, bound):
    got = got.detach().cpu().double().reshape(ref.shape)
    bad = int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{tag}: {bad} of {got.numel()} elements are not finite"
    return float(((got - ref).abs() / bound).max())


def _filled(tag, t, n):
    written, kept = T.canary_ok(t, n)
    assert written, f"{tag}: an element of the output was not written"
    assert kept, f"{tag}: the launch wrote behind its output"


def _refused(rc, who, why):
    msg = L.load().hpfg_last_error()
    assert rc == -1 and who in msg, f"{why}: rc = {rc}, message {msg!r}"


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _id(case):
    return "-".join(str(v) for v in case)


# ---- 1. first conv forward ----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _form(value):
    lib = L.load()
    old = lib.hpfg_get_option(L.OPT_FIRST_MFMA)
    lib.hpfg_set_option(L.OPT_FIRST_MFMA, value)
    try:
        yield
    finally:
        lib.hpfg_set_option(L.OPT_FIRST_MFMA, old)


def _first_input(x, layout):
    """x [N,H,W,cin] (CPU float32) on the device as a STRIDED source -> (act, buffer).  nchw: contiguous; crop: a window of a wider, taller
    NaN-filled NCHW image (sy > W, sn > cin H sy); nhwc3: channels 1 .. cin of an NHWC image of cin + 2 channels, the others NaN (sx = cin + 2)"""
    xn = x.permute(0, 3, 1, 2).contiguous()
    N, cin, H, W = xn.shape
    a = L.Act()
    a.mode, a.C, a.Hs, a.Ws = L.ACT_STRIDED, cin, H, W
    if layout == "nchw":
        buf = xn.to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = L.ptr(buf), cin * H * W, H * W, W, 1
    elif layout == "crop":
        buf = torch.full((N, cin, H + 5, W + 7), NAN, device=DEV)
        buf[:, :, 2:2 + H, 3:3 + W] = xn.to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = buf[0, 0, 2, 3:].data_ptr(), buf.stride(0), buf.stride(1), buf.stride(2), 1
    else:
        buf = torch.full((N, H, W, cin + 2), NAN, device=DEV)
        buf[..., 1:1 + cin] = x.to(DEV)
        a.z, a.sn, a.sc, a.sy, a.sx = buf[0, 0, 0, 1:].data_ptr(), H * W * (cin + 2), 1, W * (cin + 2), cin + 2
    return a, buf


def _first_launch(a, w, b, N, H, W, cin, stats=False, acc_shards=0, bump=None, cout=16):
    """one launch of the entry the arguments ask for -> (rc, out [canary], rows of partial sums [canary] or None, accumulator or None)"""
    lib, st = L.load(), T.stream(DEV)
    out = T.canary_out(N * H * W * 16)
    rows = lib.hpfg_conv_first_rows(N, H, W)
    part = T.canary_out(rows * 32) if stats else None
    acc = torch.zeros(acc_shards, 2, 16, 2, dtype=torch.int64, device=DEV) if acc_shards else None
    if bump is not None:
        counters, n_counters, seed_word, seed_add = bump
        rc = lib.hpfg_conv3x3_first_fwd_bump(C.byref(a), L.ptr(w), L.ptr(b), L.ptr(out), L.ptr(part), L.ptr(acc), acc_shards or 1, L.ptr(counters),
                                             n_counters, L.ptr(seed_word), seed_add, N, H, W, cin, cout, st)
    elif acc_shards:
        rc = lib.hpfg_conv3x3_first_fwd_acc(C.byref(a), L.ptr(w), L.ptr(b), L.ptr(out), L.ptr(part), L.ptr(acc), acc_shards, N, H, W, cin, cout, st)
    else:
        rc = lib.hpfg_conv3x3_first_fwd(C.byref(a), L.ptr(w), L.ptr(b), L.ptr(out), L.ptr(part), N, H, W, cin, cout, st)
    torch.cuda.synchronize()
    return rc, out, part, acc


def _first_check(tag, c, N, H, W, cin, layout, stats, mask=None):
    """both forms of one case: the output within the bound and written exactly, both forms the same bits in output and rows, the rows' float64
    sum within the fp32 summation bound of the launch's own output -> (output of the VALU form, rows)"""
    a, buf = _first_input(c["x"], layout)
    before = buf.clone()
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    n = N * H * W * 16
    res = []
    for form in (0, 1):
        with _form(form):
            rc, out, part, _ = _first_launch(a, w, b, N, H, W, cin, stats)
        L.check(rc, "first conv")
        _filled(f"{tag} form {form}", out, n)
        got = out[:n].reshape(N, H, W, 16)
        if mask is None:
            _note("1 first conv", f"{tag} form {form}", _ratio(tag, got, c["ref"], c["bound"]))
        else:
            g = got.cpu().double()
            assert bool(torch.isfinite(g[mask]).all()), f"{tag} form {form}: an output outside the 3 x 3 neighbourhood of the Inf is not finite"
            assert bool(torch.isinf(g[~mask]).all()), f"{tag} form {form}: an output that reads the Inf is not infinite"
            _note("1 first conv", f"{tag} form {form}", float(((g - c["ref"]).abs() / c["bound"])[mask].max()))
        if stats:
            rows = L.load().hpfg_conv_first_rows(N, H, W)
            assert rows == T.first_fwd_geometry(N, H, W)[0]
            _filled(f"{tag} form {form} rows", part, rows * 32)
            pr = part[:rows * 32].reshape(rows, 2, 16).cpu().double()
            assert bool(torch.isfinite(pr).all()), f"{tag} form {form}: a row of partial sums is not finite"
            _note("1 first conv", f"{tag} form {form} statistics rows", T.fwd_sums_ratio(pr.sum(0), got))
        res.append((out, part))
    assert _same_bits(res[0][0], res[1][0]), f"{tag}: the two forms differ in the output"
    assert not stats or _same_bits(res[0][1], res[1][1]), f"{tag}: the two forms differ in the rows of partial sums"
    assert _same_bits(buf, before), f"{tag}: the launch wrote into its input"
    return res[0]


@pytest.mark.parametrize("case", T.FIRST_FWD_CASES, ids=_id)
def test_first_conv_against_float64(case):
    N, H, W, cin = case
    c = T.first_fwd_case(*case)
    stats = T.first_fwd_stats(H, W)
    tag = f"first {_id(case)}"
    out, _ = _first_check(tag, c, N, H, W, cin, "nchw", stats)
    if not stats:
        return
    a, _buf = _first_input(c["x"], "nchw")
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    for form in (0, 1):          # the same sums through the layer accumulator
        for shards in (1, 8):
            with _form(form):
                rc, out2, _, acc = _first_launch(a, w, b, N, H, W, cin, False, acc_shards=shards)
            L.check(rc, "first conv acc")
            assert _same_bits(out2, out), f"{tag}: hpfg_conv3x3_first_fwd_acc changes the output"
            tot = torch.from_numpy(T.acc_decode(T.acc_totals(acc, 16, shards)))
            _note("1 first conv", f"{tag} form {form} accumulator on {shards} shards",
                  T.fwd_sums_ratio(tot, out2[:N * H * W * 16].reshape(N, H, W, 16)))


@pytest.mark.parametrize("layout", T.FIRST_LAYOUTS)
@pytest.mark.parametrize("cin", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", T.FIRST_FWD_LAYOUT_SHAPES, ids=_id)
def test_first_conv_reads_its_input_through_the_strides(shape, cin, layout):
    N, H, W = shape
    c = T.first_fwd_case(N, H, W, cin)
    _first_check(f"first {_id(shape)}-{cin} {layout}", c, N, H, W, cin, layout, T.first_fwd_stats(H, W))


@pytest.mark.parametrize("at", T.FIRST_FWD_INF_AT, ids=_id)
@pytest.mark.parametrize("cin", (1, 3))
def test_first_conv_inf_stays_in_its_neighbourhood(cin, at):
    """the padding k-steps of the matrix-core form address LDS offset 0 of a tile row: a product 0 * Inf there would spread NaN over the row"""
    N, H, W = T.FIRST_FWD_INF
    y0, x0 = at
    c = dict(T.first_fwd_case(N, H, W, cin))
    c["x"] = c["x"].clone()
    c["x"][0, y0, x0, 0] = float("inf")
    mask = torch.ones(N, H, W, 16, dtype=torch.bool)
    mask[0, max(y0 - 1, 0):y0 + 2, max(x0 - 1, 0):x0 + 2] = False
    _first_check(f"first Inf at {at} cin {cin}", c, N, H, W, cin, "nchw", False, mask)


@pytest.mark.parametrize("cin", (1, 2))
def test_first_conv_bump_entry(cin):
    """workgroup 0 of more than one: every counter + 1, the seed word (seed + add) & 0x7FFFFFFF, the output of the plain entry"""
    N, H, W = 1, 32, 48
    assert T.first_fwd_geometry(N, H, W)[0] > 1
    c = T.first_fwd_case(N, H, W, cin)
    a, _buf = _first_input(c["x"], "nchw")
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    for form in (0, 1):
        with _form(form):
            rc, plain, _, _ = _first_launch(a, w, b, N, H, W, cin)
            L.check(rc, "first conv")
            for n_counters in (0, 1, 300):
                for seed0 in (5, 0x7FFFFFFE):
                    counters0 = torch.arange(n_counters + 8, dtype=torch.int64) * 3 + 1
                    counters = counters0.to(DEV)
                    word = torch.tensor([seed0, 77], dtype=torch.int32, device=DEV)
                    rc, out, _, _ = _first_launch(a, w, b, N, H, W, cin, bump=(counters if n_counters else None, n_counters, word, 3))
                    L.check(rc, "first conv bump")
                    want = counters0.clone()
                    want[:n_counters] += 1
                    assert torch.equal(counters.cpu(), want), (form, n_counters)
                    assert word.cpu().tolist() == [(seed0 + 3) & 0x7FFFFFFF, 77], (form, seed0)
                    assert _same_bits(out, plain), "hpfg_conv3x3_first_fwd_bump changes the output"


def test_first_conv_refusals():
    lib = L.load()
    N, H, W = 1, 16, 16
    c = T.first_fwd_case(2, 16, 16, 1)
    a, _buf = _first_input(c["x"][:1], "nchw")
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    plain = L.Act()
    C.memmove(C.byref(plain), C.byref(a), C.sizeof(L.Act))
    plain.mode = L.ACT_PLAIN
    xs = T.conv_source("plain", 5, *T.FIRST_FWD_REFUSED_STATS, 1)["z"]
    a24, _buf24 = _first_input(xs, "nchw")
    for form in (0, 1):
        with _form(form):
            for why, args, kw in (("Cin 0", (a, w, b, N, H, W, 0), {}), ("Cin 5", (a, w, b, N, H, W, 5), {}), ("Cout 8", (a, w, b, N, H, W, 1), dict(cout=8)),
                                  ("statistics at H = 24", (a24, w, b, *T.FIRST_FWD_REFUSED_STATS, 1), dict(stats=True)),
                                  ("accumulator at H = 24", (a24, w, b, *T.FIRST_FWD_REFUSED_STATS, 1), dict(acc_shards=1)),
                                  ("PLAIN source", (plain, w, b, N, H, W, 1), {})):
                rc, out, part, _ = _first_launch(*args, **kw)
                _refused(rc, b"conv_first", f"{why} (form {form})")
                assert T.bits_kept(out, 0) and (part is None or T.bits_kept(part, 0)), f"{why}: something was launched"
            rc, out, _, acc = _first_launch(a, w, b, N, H, W, 1, acc_shards=3)
            _refused(rc, b"conv_first_acc", "3 shards")
            assert T.bits_kept(out, 0) and not bool(acc.any())
            word = torch.zeros(2, dtype=torch.int32, device=DEV)
            rc, out, _, acc = _first_launch(a, w, b, N, H, W, 1, acc_shards=3, bump=(None, 0, word, 1))
            _refused(rc, b"conv_first_bump", "3 shards (bump)")
            assert T.bits_kept(out, 0) and not bool(acc.any()) and not bool(word.any())


# ---- 2. upsample backward -----------------------------------------------------------------------------------------------------------------
UP_OFF = 16          # the gradient lives in channels [16, 16 + C) of a wider buffer


def _upbwd_launch(g, N, Hl, Wl, C_, sums):
    """-> (rc, dU [canary], rows of channel sums [canary] or None, blocks)"""
    lib = L.load()
    gb, gptr = T.wide(g, UP_OFF, UP_OFF)
    dU = T.canary_out(N * Hl * Wl * C_)
    blocks = lib.hpfg_upsample2x_bwd_blocks(N, Hl, Wl, C_)
    if sums:
        part = T.canary_out(blocks * C_)
        rc = lib.hpfg_upsample2x_bwd_sums(gptr, UP_OFF + C_, L.ptr(dU), N, Hl, Wl, C_, L.ptr(part), T.stream(DEV))
    else:
        part = None
        rc = lib.hpfg_upsample2x_bwd(gptr, UP_OFF + C_, L.ptr(dU), N, Hl, Wl, C_, T.stream(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(gb[..., :UP_OFF]).all()), "the launch wrote into its input"
    return rc, dU, part, blocks


@pytest.mark.parametrize("case", sorted(set(T.UPBWD_SUMS_CASES)), ids=_id)
def test_upsample_bwd_against_float64(case):
    N, Hl, Wl, C_ = case
    c, geo = T.upbwd_case(*case), T.upbwd_geometry(*case)
    tag = f"upbwd {_id(case)}"
    n = N * Hl * Wl * C_
    rc, dU, _, blocks = _upbwd_launch(c["g"], N, Hl, Wl, C_, False)
    L.check(rc, "upsample2x_bwd")
    assert blocks == geo["blocks"]
    _filled(tag, dU, n)
    _note("2 upsample backward", tag, _ratio(tag, dU[:n], c["ref"], c["bound"]))
    rc, dU2, part, _ = _upbwd_launch(c["g"], N, Hl, Wl, C_, True)
    if not T.upbwd_sums_admitted(C_):
        _refused(rc, b"C=", f"{tag}: channel sums with C/4 = {C_ // 4}")
        assert T.bits_kept(dU2, 0) and T.bits_kept(part, 0), f"{tag}: the refused launch wrote"
        return
    L.check(rc, "upsample2x_bwd_sums")
    assert _same_bits(dU2, dU), f"{tag}: hpfg_upsample2x_bwd_sums changes dU"
    _filled(tag + " rows", part, blocks * C_)
    rows = part[:blocks * C_].reshape(blocks, C_).cpu().double()
    assert bool(torch.isfinite(rows).all()), f"{tag}: a row of channel sums is not finite"
    val, bound = T.upbwd_sums_f64(dU[:n].reshape(N, Hl, Wl, C_).cpu(), geo)
    _note("2 upsample backward", tag + " channel sums", float(((rows.sum(0) - val).abs() / bound).max()))


def test_upsample_bwd_refusals_follow_the_rule():
    lib, st = L.load(), T.stream(DEV)
    N, Hl, Wl, C_ = T.UPBWD_REFUSED
    g = torch.zeros(N, 2 * Hl, 2 * Wl, C_)
    for sums in (False, True):
        rc, dU, part, _ = _upbwd_launch(g, N, Hl, Wl, C_, sums)
        _refused(rc, b"upsample2x_bwd", "Hl + Wl = 513")
        assert T.bits_kept(dU, 0) and (part is None or T.bits_kept(part, 0))
    for C_ in range(4, 273, 4):          # the rule C <= 256 && 256 % (C / 4) == 0 and the refusal agree
        rc, dU, part, _ = _upbwd_launch(torch.ones(1, 2, 2, C_), 1, 1, 1, C_, True)
        if T.upbwd_sums_admitted(C_):
            assert rc == 0, C_
            _filled(f"C = {C_}", dU, C_)
        else:
            _refused(rc, b"C=", f"C = {C_}")
            assert T.bits_kept(dU, 0) and T.bits_kept(part, 0)
    assert lib.hpfg_upsample2x_bwd(None, 4, None, 1, 1, 1, 4, st) == -1 and lib.hpfg_upsample2x_bwd_blocks(1, 1, 1, 0) == 0


# ---- 3. channel sums ----------------------------------------------------------------------------------------------------------------------
def _chansum_check(case, off=0):
    npix, C_, ps = case
    lib, st = L.load(), T.stream(DEV)
    c, geo = T.chansum_case(npix, C_, ps, off), T.chansum_geometry(npix, C_, ps)
    tag = f"chansum {_id(case)}" + (f" offset {off}" if off else "")
    buf = T.padded(c["buf"].numpy())
    blocks = lib.hpfg_channel_sum_blocks(npix, C_)
    assert blocks == geo["blocks"] > 0
    part = T.canary_out(blocks * C_)
    L.check(lib.hpfg_channel_sum_partials(buf.data_ptr() + 4 * off, ps, npix, C_, L.ptr(part), st), "channel_sum_partials")
    torch.cuda.synchronize()
    _filled(tag + " rows", part, blocks * C_)
    rows = part[:blocks * C_].reshape(blocks, C_).cpu().double()
    assert bool(torch.isfinite(rows).all()), f"{tag}: a row is not finite"
    assert not bool(rows[geo["busy"]:].any()), f"{tag}: a workgroup without pixels wrote something other than zeros"
    _note("3 channel sums", tag + " rows", float(((rows.sum(0) - c["ref"]).abs() / c["bound"]).max()))
    out, scratch = T.canary_out(C_), T.canary_out(512 * C_)
    L.check(lib.hpfg_channel_sum(buf.data_ptr() + 4 * off, ps, npix, C_, L.ptr(out), L.ptr(scratch), st), "channel_sum")
    torch.cuda.synchronize()
    _filled(tag, out, C_)
    assert T.bits_kept(scratch, blocks * C_), f"{tag}: the scratch rows behind the {blocks} of the launch were written"
    assert _same_bits(scratch[:blocks * C_], part[:blocks * C_]), f"{tag}: the two entries' first stages differ"
    bound = c["bound"] + T.U24 * c["ref"].abs()          # the float64 second stage rounds once more to float
    _note("3 channel sums", tag, _ratio(tag, out[:C_], c["ref"], bound))
    assert _same_bits(buf.cpu(), T.padded(c["buf"].numpy(), dev="cpu")), f"{tag}: the launch wrote into its input"


@pytest.mark.parametrize("case", T.CHANSUM_CASES, ids=_id)
def test_channel_sum_against_float64(case):
    _chansum_check(case)


def test_channel_sum_vector_path_at_a_four_byte_aligned_address():
    npix, C_, ps, off = T.CHANSUM_OFFSET
    assert T.chansum_geometry(npix, C_, ps)["vec"] and off % 4 != 0
    _chansum_check((npix, C_, ps), off)


def test_channel_sum_refusals():
    lib, st = L.load(), T.stream(DEV)
    buf, out, scratch = T.padded(np.ones(1024, dtype=np.float32)), T.canary_out(256), T.canary_out(1024)
    for npix, C_ in ((4, 0), (1, 257), (0, 4)):
        assert lib.hpfg_channel_sum_blocks(npix, C_) == 0
        _refused(lib.hpfg_channel_sum_partials(L.ptr(buf), max(C_, 1), npix, C_, L.ptr(scratch), st), b"channel_sum_partials", (npix, C_))
        _refused(lib.hpfg_channel_sum(L.ptr(buf), max(C_, 1), npix, C_, L.ptr(out), L.ptr(scratch), st), b"channel_sum", (npix, C_))
    torch.cuda.synchronize()
    assert T.bits_kept(out, 0) and T.bits_kept(scratch, 0)


# ---- 4. slab reduce -----------------------------------------------------------------------------------------------------------------------
def _slab_launch(layers, Ss):
    """one hpfg_slab_reduce_multi over synthetic slabs -> [(dw [canary], slab_case)] per layer"""
    lib = L.load()
    d = (L.SlabDesc * len(layers))()
    keep, res = [], []
    for i, (layer, S) in enumerate(zip(layers, Ss)):
        taps, cin, cip, cout, cop = layer
        c = T.slab_case(layer, S)
        slab = T.padded(c["slab"].reshape(-1).numpy())
        dw = T.canary_out(cout * cin * taps)
        d[i].slab, d[i].dw_oihw, d[i].S, d[i].taps, d[i].Cin, d[i].CinPad, d[i].Cout, d[i].CoutPad = L.ptr(slab), L.ptr(dw), S, taps, cin, cip, cout, cop
        keep.append(slab)
        res.append((dw, c))
    tab = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8).to(DEV)
    L.check(lib.hpfg_slab_reduce_multi(tab.data_ptr(), d, len(layers), T.stream(DEV)), "slab_reduce_multi")
    torch.cuda.synchronize()
    return res


def _slab_check(tag, layers, Ss):
    first = _slab_launch(layers, Ss)
    again = _slab_launch(layers, Ss)
    for (dw, c), (dw2, _), layer, S in zip(first, again, layers, Ss):
        taps, cin, _, cout, _ = layer
        n = cout * cin * taps
        t = f"{tag} layer {_id(layer)} S {S}"
        _filled(t, dw, n)
        _note("4 slab reduce", t, _ratio(t, dw[:n], c["ref"], c["bound"]))
        assert _same_bits(dw, dw2), f"{t}: two launches differ"


@pytest.mark.parametrize("S", T.SLAB_S)
def test_slab_reduce_against_float64(S):
    _slab_check("slab", T.SLAB_LAYERS, (S,) * len(T.SLAB_LAYERS))


def test_slab_reduce_with_another_split_count_per_layer():
    _slab_check("slab mixed", T.SLAB_LAYERS, T.SLAB_MIXED_S)


def test_slab_reduce_on_the_capped_grid():
    assert T.slab_grid(T.SLAB_CAP_LAYERS) == (T.SLAB_GRID_CAP, 2)
    _slab_check("slab capped", T.SLAB_CAP_LAYERS, (T.SLAB_CAP_S,) * 2)


def test_slab_reduce_refusals():
    lib, st = L.load(), T.stream(DEV)
    d = (L.SlabDesc * 1)()
    tab = torch.zeros(C.sizeof(L.SlabDesc), dtype=torch.uint8, device=DEV)
    _refused(lib.hpfg_slab_reduce_multi(tab.data_ptr(), d, 0, st), b"slab_reduce_multi", "nlayers = 0")
    _refused(lib.hpfg_slab_reduce_multi(None, d, 1, st), b"slab_reduce_multi", "no device table")
    _refused(lib.hpfg_slab_reduce_multi(tab.data_ptr(), None, 1, st), b"slab_reduce_multi", "no host table")


# ---- 5. BatchNorm backward reductions and the max-pool scatter ---------------------------------------------------------------------------
def _rows_check(tag, part, blocks, C_, g64, z, tab):
    _filled(tag + " rows", part, blocks * 2 * C_)
    rows = part[:blocks * 2 * C_].reshape(blocks, 2, C_).cpu().double()
    assert bool(torch.isfinite(rows).all()), f"{tag}: a row of partial sums is not finite"
    _note("5 bn backward", tag, T.bwd_sums_ratio(rows.sum(0), g64.reshape(-1, C_), z.double().reshape(-1, C_), tab))


@pytest.mark.parametrize("case", T.BNBWD_CASES, ids=_id)
def test_bn_bwd_reduce_against_float64(case):
    N, H, W, C_, p = case
    lib = L.load()
    c = T.bnbwd_case(*case)
    a, _, keep = T.device_source(c["s"], H, W)
    blocks = lib.hpfg_bn_bwd_blocks(N, H, W, C_)
    assert blocks == T.bn_bwd_blocks(N, H, W, C_)
    part = T.canary_out(blocks * 2 * C_)
    L.check(lib.hpfg_bn_bwd_reduce(C.byref(a), N, H, W, L.ptr(part), T.stream(DEV)), "bn_bwd_reduce")
    torch.cuda.synchronize()
    _rows_check(f"bn_bwd_reduce {_id(case)}", part, blocks, C_, c["g64"], c["s"]["z"], c["s"]["tab"])
    assert all(bool(torch.isnan(b).any()) for b in keep), "the launch wrote into a source"


def _pool_acts(c, N, H2, W2, C_, dA):
    """(DZ source over z / table / the dA buffer, BNACT source over z / table, tensors to keep)"""
    zb, zptr = T.wide(c["z"])
    tb = torch.full((L.BN_ROWS, C_ + T.TPAD), NAN, device=DEV)
    tb[:, T.TOFF:T.TOFF + C_] = c["tab"].to(DEV)
    a = L.Act()
    a.z, a.bn, a.aux, a.mode, a.C, a.Hs, a.Ws = zptr, L.ptr(tb), L.ptr(dA), L.ACT_DZ, C_, H2, W2
    a.pstride, a.aux_pstride, a.bn_stride, a.bn_coff = C_ + T.PADC, dA.shape[-1], C_ + T.TPAD, T.TOFF
    s = L.Act()
    C.memmove(C.byref(s), C.byref(a), C.sizeof(L.Act))
    s.mode, s.aux = L.ACT_BNACT, None
    return a, s, (zb, tb)


@pytest.mark.parametrize("case", T.POOLBWD_CASES, ids=_id)
def test_pooled_bn_bwd_and_scatter_against_float64(case):
    N, H2, W2, C_, ties = case
    Hp, Wp = H2 // 2, W2 // 2
    lib, st = L.load(), T.stream(DEV)
    c = T.poolbwd_case(*case)
    tag = f"pooled {_id(case)}"
    gen = torch.Generator().manual_seed(c["seed"])
    full = torch.randn(N, H2, W2, C_ + 16, generator=gen)          # dA: the first C channels of a wider (concat) buffer
    full[..., :C_] = c["base"]
    one, two = full.to(DEV), full.to(DEV)
    dPb, dPptr = T.wide(c["dP"])
    a1, _, keep1 = _pool_acts(c, N, H2, W2, C_, one)
    a2, s2, keep2 = _pool_acts(c, N, H2, W2, C_, two)
    blocks = lib.hpfg_bn_bwd_pool_blocks(N, Hp, Wp, C_)
    assert blocks == T.bn_bwd_pool_blocks(N, Hp, Wp, C_)
    part = T.canary_out(blocks * 2 * C_)
    L.check(lib.hpfg_bn_bwd_reduce_pool(C.byref(a1), dPptr, C_ + T.PADC, N, Hp, Wp, L.ptr(part), st), "bn_bwd_reduce_pool")
    L.check(lib.hpfg_pool_scatter_add(C.byref(s2), dPptr, C_ + T.PADC, L.ptr(two), C_ + 16, N, Hp, Wp, st), "pool_scatter_add")
    torch.cuda.synchronize()
    for name, buf in (("hpfg_bn_bwd_reduce_pool", one), ("hpfg_pool_scatter_add", two)):
        got = buf.cpu()
        assert _same_bits(got[..., :C_].contiguous(), c["done"].contiguous()), f"{tag}: {name} does not leave float32(base + scatter(dP))"
        assert _same_bits(got[..., C_:].contiguous(), full[..., C_:].contiguous()), f"{tag}: {name} touched the channels behind C"
    if ties:          # (`done` holds the tie rule: in the channels whose four window values are equal the gradient sits on window element 0)
        assert int(c["tied"].sum()) == 2 and bool((c["first"][..., c["tied"]] == 0).all())
    _rows_check(tag, part, blocks, C_, c["g64"], c["z"], c["tab"])
    blocks2 = lib.hpfg_bn_bwd_blocks(N, H2, W2, C_)          # the plain reduction over the completed gradient: the same sums
    part2 = T.canary_out(blocks2 * 2 * C_)
    L.check(lib.hpfg_bn_bwd_reduce(C.byref(a2), N, H2, W2, L.ptr(part2), st), "bn_bwd_reduce")
    torch.cuda.synchronize()
    _rows_check(tag + " (scatter, then the plain reduction)", part2, blocks2, C_, c["g64"], c["z"], c["tab"])
    for b in keep1 + keep2 + (dPb,):
        assert bool(torch.isnan(b).any()), f"{tag}: a launch wrote into a source"


def test_bn_bwd_refusals():
    lib, st = L.load(), T.stream(DEV)
    c = T.poolbwd_case(2, 6, 10, 8, False)
    N, H2, W2, C_ = 2, 6, 10, 8
    dA = torch.zeros(N, H2, W2, C_ + 16, device=DEV)
    before = dA.clone()
    dPb, dPptr = T.wide(c["dP"])
    part = T.canary_out(64 * 2 * 2048)
    a, s, _keep = _pool_acts(c, N, H2, W2, C_, dA)

    def variant(src, **kw):
        v = L.Act()
        C.memmove(C.byref(v), C.byref(src), C.sizeof(L.Act))
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    for bad in T.BNBWD_REFUSED_C:
        _refused(lib.hpfg_bn_bwd_reduce(C.byref(variant(a, C=bad)), N, H2, W2, L.ptr(part), st), b"bn_bwd_reduce: unsupported C", bad)
        _refused(lib.hpfg_bn_bwd_reduce_pool(C.byref(variant(a, C=bad)), dPptr, C_ + T.PADC, N, H2 // 2, W2 // 2, L.ptr(part), st),
                 b"bn_bwd_reduce_pool: unsupported C", bad)
    pool = lambda v, ps=C_ + T.PADC: lib.hpfg_bn_bwd_reduce_pool(C.byref(v), dPptr, ps, N, H2 // 2, W2 // 2, L.ptr(part), st)
    _refused(pool(variant(a, drop_p=0.3)), b"bn_bwd_reduce_pool", "drop_p > 0")
    _refused(pool(a, C_ + T.PADC + 2), b"bn_bwd_reduce_pool", "dP stride")
    _refused(pool(variant(a, aux_pstride=C_ + 18)), b"bn_bwd_reduce_pool", "dA stride")
    _refused(pool(variant(a, pstride=C_ + T.PADC + 1)), b"bn_bwd_reduce_pool", "z stride")
    _refused(lib.hpfg_pool_scatter_add(C.byref(a), dPptr, C_ + T.PADC, L.ptr(dA), C_ + 16, N, H2 // 2, W2 // 2, st), b"pool_scatter_add", "DZ source")
    _refused(lib.hpfg_pool_scatter_add(C.byref(variant(s, mode=L.ACT_PLAIN)), dPptr, C_ + T.PADC, L.ptr(dA), C_ + 16, N, H2 // 2, W2 // 2, st),
             b"pool_scatter_add", "PLAIN source")
    torch.cuda.synchronize()
    assert T.bits_kept(part, 0) and torch.equal(dA, before)


# ---- 6. dropout mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.DROPMASK_N)
def test_dropout_mask_is_the_hash_rule(n):
    lib, st = L.load(), T.stream(DEV)
    for p in T.DROPMASK_P:
        for sd in T.DROPMASK_SEED_DEV:
            out = torch.full((n + T.PAD,), 0xAB, dtype=torch.uint8, device=DEV)
            word = torch.tensor([sd - (1 << 32) if sd >= 1 << 31 else sd], dtype=torch.int32, device=DEV)
            L.check(lib.hpfg_dropout_mask(L.ptr(out), n, p, T.DROPMASK_SEED, L.ptr(word), st), "dropout_mask")
            got = out.cpu().numpy()
            ref = rng_ref.keep_mask_nhwc(n, p, (T.DROPMASK_SEED + sd) & 0xFFFFFFFF)
            assert np.array_equal(got[:n], ref), (n, p, sd)
            assert bool((got[n:] == 0xAB).all()), "the launch wrote behind its output"
            assert p > 0 or bool(ref.all())
    out = torch.full((n + T.PAD,), 0xAB, dtype=torch.uint8, device=DEV)          # no device seed: the old call
    L.check(lib.hpfg_dropout_mask(L.ptr(out), n, 0.3, T.DROPMASK_SEED, None, st), "dropout_mask")
    assert np.array_equal(out.cpu().numpy()[:n], rng_ref.keep_mask_nhwc(n, 0.3, T.DROPMASK_SEED))


def test_dropout_mask_refusals():
    lib, st = L.load(), T.stream(DEV)
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device=DEV)
    for n, p in ((16, 1.0), (16, -0.1), (0, 0.3)):
        _refused(lib.hpfg_dropout_mask(L.ptr(out), n, p, 1, None, st), b"dropout_mask", (n, p))
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
