"""Dropout of the window-attention probabilities (the DROP kernels of csrc/attn_window.hip) and the packed small-window kernels (all of
csrc/attn_window_packed.hip) against the float64 laws of tests/helpers.py: the sibling of tests/test_gpu_attn_edges.py for the two kernel
groups that file does not reach.

Rule (helpers.attn_tolerance, unchanged): per output tensor, max |kernel - law| <= 8 x the largest error the mode's yardstick makes against
the law, and no less than 4 float32 ulp.  The law takes the dropout mask as the header states it (out = (P .* f) V, dP = (dO V^T) .* f,
dS = P .* (dP - rowsum(P .* dP)), dV = (P .* f)^T dO, f = M / (1 - p)); the masks have a fully dropped and a fully kept query row.
tests/test_attn_laws_host.py shows that the rule catches a wrong factor in any of the three places, a transposed mask, keys leaking
between the windows of a packed tile and a mask indexed by the slot in the tile, and that the rule is never looser than half the hand
constants of tests/test_gpu_swin_dropout.py and tests/test_gpu_attn_window_packed.py.
Families: unit (randn), sharp (q, k x 2), hot (q, k x 8: the mask's literal -100 competes; the packed kernel writes NEG beside it).
Shapes: helpers.WINDOW_EDGES (dropout, p = 0.1 and 0.5) and helpers.PACKED_EDGES (every count of live slots of a 16 / 7 / 4-slot tile,
rectangular maps, a partial last tile with another image behind it), both head dims, both math modes, through the C entry points on
canary buffers (every element of out, dqkv, dtable and the scratch written, nothing behind them touched).  `pytest -s` prints error /
tolerance per tensor."""
import ctypes

import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd.ops_tokens import window_attention_dropout, window_attention_packed
from tests import helpers as T
from tests.test_gpu_attn_edges import DEV, MATH, _canaries, _report, _st, _through_op

pytestmark = pytest.mark.gpu
FAMILIES = ["unit", "sharp", "hot"]
P_PACKED = 0.1
HASH_SHAPES = [(2, 8, 10, 2, 1, 1), (1, 6, 12, 3, 1, 2)]          # more than one tile an image, rectangular


def _entry(kind):
    lib = L.load()
    if kind == "packed":
        return lib.hpfg_attn_window_packed_fwd, lib.hpfg_attn_window_packed_bwd, lib.hpfg_attn_window_packed_scratch_floats
    return lib.hpfg_attn_window_drop_fwd, lib.hpfg_attn_window_drop_bwd, lib.hpfg_attn_window_scratch_floats


def _run(kind, c, shape, d, math, p=0.0, seed=0, word=None, mask=None):
    """forward and backward through the C entry points of `kind` on canary buffers -> (out, dqkv, dtable), floats of the scratch"""
    B, H, W, w, s, heads = shape
    fwd, bwd, scratch_floats = _entry(kind)
    qkv, table, do = (c[k].to(DEV) for k in ("qkv", "table", "do"))
    sc, no, nqkv, nt = c["scale"], do.numel(), qkv.numel(), table.numel()
    n_scr = scratch_floats(B, H, W, heads, d, w, MATH[math])
    assert n_scr > 0
    out, dqkv, dtab, scr = T.canary_out(no), T.canary_out(nqkv), T.canary_out(nt), T.canary_out(n_scr)
    L.check(fwd(L.ptr(qkv), L.ptr(table), L.ptr(out), B, H, W, heads, d, w, s, sc, MATH[math], p, seed, L.ptr(word), L.ptr(mask), _st()), f"{kind} fwd")
    L.check(bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, W, heads, d, w, s, sc, MATH[math], p, seed, L.ptr(word),
                L.ptr(mask), _st()), f"{kind} bwd")
    _canaries({"out": (out, no), "dqkv": (dqkv, nqkv), "dtable": (dtab, nt), "scratch": (scr, n_scr)})
    return (out[:no].view_as(do), dqkv[:nqkv].view_as(qkv), dtab[:nt].view_as(table)), n_scr


def _same_bits(got, want, what):
    for name, a, b in zip(("out", "dqkv", "dtable"), got, want):
        assert torch.equal(a, b), f"{name}: {what}"


# ---- dropout in the one-window-per-workgroup kernels: hpfg_attn_window_drop_fwd / _bwd ------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,W,w,s,heads", T.WINDOW_EDGES)
def test_window_dropout(B, H, W, w, s, heads, family, d, p, math):
    """the shapes of test_gpu_attn_edges.test_windows with an explicit mask; square maps at shift 0 or w // 2 also through
    window_attention_dropout.  (2, 3, 3, 1, 0, 2) has one key a row: dS = 0, the tolerances are the helper's floor.)"""
    shape = (B, H, W, w, s, heads)
    c = T.window_drop_case(family, *shape, d, p)
    mask = c["mask"].to(DEV)
    got, n_scr = _run("window", c, shape, d, math, p, mask=mask)
    assert n_scr == B * (H // w) * (W // w) * heads * (2 * w - 1) ** 2
    if H == W and s in (0, w // 2):
        qkv, table, do = (c[k].to(DEV) for k in ("qkv", "table", "do"))
        op = _through_op(window_attention_dropout, math, (qkv, table, heads, w, s, c["scale"], p, 0, None, mask), (0, 1), do)
        _same_bits(op, got, "window_attention_dropout against the C entry points")
    _report(f"window dropout {family} {math} p={p} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}", T.WINDOW_TENSORS, T.window_results(got), c["ref"],
            c["tol"][math])


# ---- several windows a tile: hpfg_attn_window_packed_fwd / _bwd -----------------------------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,W,w,s,heads", T.PACKED_EDGES)
def test_packed(B, H, W, w, s, heads, family, d, drop, math):
    """every count of live slots, without a mask and with one at p = 0.1.  Split-bf16 mode: held to the law by the rule.  f32 mode: the
    bits of the unpacked entry points on the same inputs (the packed entry points run those kernels), which the rule holds too.  Square
    maps also through window_attention_packed."""
    shape = (B, H, W, w, s, heads)
    p = P_PACKED if drop else 0.0
    c = T.window_drop_case(family, *shape, d, p) if drop else T.window_case(family, *shape, d)
    mask = c["mask"].to(DEV) if drop else None
    got, n_scr = _run("packed", c, shape, d, math, p, mask=mask)
    nW, T_ = (H // w) * (W // w), (2 * w - 1) ** 2
    per = T.ATTN_IMAGE_KEYS // (w * w)
    assert n_scr == (B * ((nW + per - 1) // per) * heads * T_ if math == "bf16x3" else B * nW * heads * T_)
    if math == "f32":
        _same_bits(got, _run("window", c, shape, d, math, p, mask=mask)[0], "the packed f32 entry points against the unpacked ones")
    if H == W:
        qkv, table, do = (c[k].to(DEV) for k in ("qkv", "table", "do"))
        args = (qkv, table, heads, w, s, c["scale"]) + ((p, 0, None, mask) if drop else ())
        _same_bits(_through_op(window_attention_packed, math, args, (0, 1), do), got, "window_attention_packed against the C entry points")
    _report(f"packed {family} {math} p={p} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}", T.WINDOW_TENSORS, T.window_results(got), c["ref"],
            c["tol"][math])


# ---- the hash path ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("kind", ["window", "packed"])
@pytest.mark.parametrize("B,H,W,w,s,heads", HASH_SHAPES)
def test_hash_path_is_the_explicit_mask_of_drop_mask(B, H, W, w, s, heads, kind, math):
    """the mask hpfg_attn_window_drop_mask writes for a seed plus a device seed word, fed back explicitly, gives the bits of the run that
    takes the seed: the element index is that of the window in the image in both families, on a rectangular map with more than one tile an
    image; two launches of the same call give equal bits; and the result is the law's with that mask."""
    lib = L.load()
    shape, d, p, seed = (B, H, W, w, s, heads), 32, P_PACKED, 77
    c = T.window_case("unit", *shape, d)
    word = torch.tensor([12345], dtype=torch.int32, device=DEV)
    n = lib.hpfg_attn_window_drop_elems(B, H, W, heads, w)
    assert n == B * (H // w) * (W // w) * heads * w ** 4
    m = torch.full((n + T.PAD,), 0xAB, dtype=torch.uint8, device=DEV)
    L.check(lib.hpfg_attn_window_drop_mask(L.ptr(m), B, H, W, heads, w, p, seed, L.ptr(word), _st()), "drop_mask")
    torch.cuda.synchronize()
    assert bool((m[:n] <= 1).all()) and bool((m[n:] == 0xAB).all()) and 0 < int(m[:n].sum()) < n
    mask = m[:n].clone()
    hashed, _ = _run(kind, c, shape, d, math, p, seed, word)
    _same_bits(_run(kind, c, shape, d, math, p, mask=mask)[0], hashed, "the explicit mask against the seed")
    _same_bits(_run(kind, c, shape, d, math, p, seed, word)[0], hashed, "two launches")
    drop = (mask.cpu().reshape(-1, heads, w * w, w * w), p)
    law = lambda arith: T.window_results(T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], arith=arith, drop=drop))
    ref = law(torch.float64)
    _report(f"{kind} hash mask {math} B={B} H={H} W={W} w={w} s={s} heads={heads}", T.WINDOW_TENSORS, T.window_results(hashed), ref,
            T.attn_tolerance(ref, law(T.ATTN_YARDSTICK[math])))


# ---- refusals: returned before any launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
def test_bad_dropout_arguments_are_refused(math):
    """p < 0, p = 1, p = NaN, and B nW heads L^2 = 2^32 mask elements (the hash and the kernels index them with 32 bits): -1 with the entry
    point's name in hpfg_last_error, from all four entry points"""
    lib = L.load()
    ptr = ctypes.c_void_p(256)          # never dereferenced: the argument check returns first
    small, big = (1, 8, 8, 1, 32, 2, 1), (4096, 512, 512, 1, 32, 2, 1)          # B, H, W, heads, head dim, window, shift
    assert lib.hpfg_attn_window_drop_elems(4096, 512, 512, 1, 2) == 1 << 32
    entries = [(b"attn_window_drop_fwd", lib.hpfg_attn_window_drop_fwd, 3), (b"attn_window_drop_bwd", lib.hpfg_attn_window_drop_bwd, 6),
               (b"attn_window_packed_fwd", lib.hpfg_attn_window_packed_fwd, 3), (b"attn_window_packed_bwd", lib.hpfg_attn_window_packed_bwd, 6)]
    for name, fn, n_ptr in entries:
        for geo, p in [(small, -0.1), (small, 1.0), (small, float("nan")), (big, 0.1)]:
            assert fn(*([ptr] * n_ptr), *geo, 1.0, MATH[math], p, 0, None, None, None) == -1, (name, geo, p)
            msg = lib.hpfg_last_error()
            assert name in msg and b"dropout" in msg, msg
    torch.cuda.synchronize()
