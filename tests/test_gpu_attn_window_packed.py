"""Packed small-window attention (csrc/attn_window_packed.hip, ops_tokens.window_attention_packed): windows of at most 16 tokens, 64 // w^2
of them per workgroup tile, against the reference formula in fp64 (tests/helpers.window_attn_reference; with a dropout mask the formula of
tests/test_gpu_swin_dropout.py), in both math modes; against ``window_attention`` on the same inputs (bit for bit in f32 mode); every output
element written (NaN poisoning through the C entry points, scratch included); reproducibility; the hash dropout path against the explicit
mask that hpfg_attn_window_drop_mask writes; argument errors and the scratch size.

The bounds are the ``_bounds`` law of tests/test_gpu_swin.py, restated here (the project's numbers, not new ones): out 2e-5 k, dq 5e-5 k,
dk / dv 2e-4 k with k = 1 (HPFG_MATH=f32) or 8 (split-bf16 products), times sqrt(2) at head dim 64; a bias-table entry sums dS over up to
T = B (H/w)^2 w^2 pairs: 2e-4 k max(1, sqrt(T / 256)).  With dropout every bound is divided by 1 - p (tests/test_gpu_swin_dropout.py).
Packing changes which tile rows a window's keys occupy, hence the order of the softmax sums, not the arithmetic: the same bounds hold."""
import functools

import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.ops_tokens import window_attention, window_attention_drop_mask, window_attention_dropout, window_attention_packed
from tests.helpers import maxerr
from tests.helpers import window_attn_reference as _reference
from tests.test_gpu_swin_dropout import _reference as _reference_drop

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MATH = {"f32": 0, "bf16x3": 1}
NAMES = ("out", "dq", "dk", "dv", "dtable")
P = 0.1

# (B, H = W, w, s, heads, d)
SHAPES = [(2, 6, 3, 0, 2, 32),        # one partial tile (4 of 7 slots)
          (1, 9, 3, 1, 1, 32),        # 7 + 2 windows, all nine mask regions
          (2, 12, 3, 1, 3, 32),       # 7 + 7 + 2
          (1, 8, 4, 2, 2, 32),        # one full tile
          (1, 12, 4, 2, 1, 64),       # 4 + 4 + 1
          (1, 8, 2, 1, 1, 32),        # 16 windows, one full tile
          (1, 6, 2, 0, 1, 64),        # 9 of 16 slots
          (1, 4, 4, 2, 1, 32)]        # window == map: wrap-around only


@functools.lru_cache(maxsize=None)
def _case(B, H, w, s, heads, d):
    """inputs (fp32), an explicit mask of keep rate 1 - P and the fp64 references without and with it (out, dqkv, dtable): computed once per
    shape, shared, never changed"""
    g = torch.Generator().manual_seed(7000 + 100 * H + 10 * w + s + d)
    C_ = heads * d
    qkv, do = torch.randn(B, H, H, 3 * C_, generator=g), torch.randn(B, H, H, C_, generator=g)
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g)
    mask = (torch.rand(B * (H // w) ** 2, heads, w * w, w * w, generator=g) >= P).to(torch.uint8)
    refs = []
    for m in (None, mask):
        qr, tr = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
        o = _reference(qr, tr, heads, w, s, d ** -0.5) if m is None else _reference_drop(qr, tr, m, P, heads, w, s, d ** -0.5)
        o.backward(do.double())
        refs.append((o.detach(), qr.grad, tr.grad))
    return qkv, table, do, mask, refs[0], refs[1]


def _errors(got, ref, C_):
    return (maxerr(got[0], ref[0]), maxerr(got[1][..., :C_], ref[1][..., :C_]), maxerr(got[1][..., C_:2 * C_], ref[1][..., C_:2 * C_]),
            maxerr(got[1][..., 2 * C_:], ref[1][..., 2 * C_:]), maxerr(got[2], ref[2]))


def _bounds(B, H, w, d, math):
    k = (1.0 if math == "f32" else 8.0) * (2 ** 0.5 if d == 64 else 1.0)
    kb = 1.0 if math == "f32" else 8.0
    T = B * (H // w) ** 2 * w * w
    return 2e-5 * k, 5e-5 * k, 2e-4 * k, 2e-4 * k, 2e-4 * kb * max(1.0, (T / 256) ** 0.5)


def _run(op, qkv, table, do, heads, w, s, d, math, *drop):
    qd, td = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        out = op(qd, td, heads, w, s, d ** -0.5, *drop)
        out.backward(do.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    return out.detach(), qd.grad, td.grad


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES)
def test_packed_vs_fp64_and_vs_window_attention(B, H, w, s, heads, d, math):
    qkv, table, do, _, ref, _ = _case(B, H, w, s, heads, d)
    got = [t.cpu() for t in _run(window_attention_packed, qkv, table, do, heads, w, s, d, math)]
    old = [t.cpu() for t in _run(window_attention, qkv, table, do, heads, w, s, d, math)]
    errs, diff, bnd = _errors(got, ref, heads * d), _errors(got, old, heads * d), _bounds(B, H, w, d, math)
    print(f"packed {math} B={B} H={H} w={w} s={s} heads={heads} d={d}: " +
          "  ".join(f"{n} {e:.2e} (< {b:.2e}) vs unpacked {x:.2e}" for n, e, b, x in zip(NAMES, errs, bnd, diff)))
    for n, e, x, b in zip(NAMES, errs, diff, bnd):
        assert e < b, n
        assert x < 2 * b, f"{n} against window_attention"
    if math == "f32":          # the f32 entry points run the kernels of attn_window.hip
        for a, b_ in zip(got, old):
            assert torch.equal(a, b_)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES)
def test_packed_dropout_vs_fp64_with_the_mask(B, H, w, s, heads, d, math):
    qkv, table, do, mask, _, ref = _case(B, H, w, s, heads, d)
    md = mask.to(DEV)
    got = [t.cpu() for t in _run(window_attention_packed, qkv, table, do, heads, w, s, d, math, P, 0, None, md)]
    old = [t.cpu() for t in _run(window_attention_dropout, qkv, table, do, heads, w, s, d, math, P, 0, None, md)]
    errs, diff = _errors(got, ref, heads * d), _errors(got, old, heads * d)
    bnd = [b / (1.0 - P) for b in _bounds(B, H, w, d, math)]
    print(f"packed dropout {math} B={B} H={H} w={w} s={s} heads={heads} d={d}: " +
          "  ".join(f"{n} {e:.2e} (< {b:.2e}) vs unpacked {x:.2e}" for n, e, b, x in zip(NAMES, errs, bnd, diff)))
    for n, e, x, b in zip(NAMES, errs, diff, bnd):
        assert e < b, n
        assert x < 2 * b, f"{n} against window_attention_dropout"
    if math == "f32":
        for a, b_ in zip(got, old):
            assert torch.equal(a, b_)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", [SHAPES[2], SHAPES[4], SHAPES[5]])
def test_hash_path_equals_the_explicit_mask_of_drop_mask(B, H, w, s, heads, d, math):
    """The mask hpfg_attn_window_drop_mask writes for (seed, seed word) -- the unpacked family's tool -- fed back explicitly gives the bits of
    the packed hash run: the element index uses the window's index in the image, not its slot in the tile."""
    qkv, table, do, _, _, _ = _case(B, H, w, s, heads, d)
    word = torch.tensor([4321], dtype=torch.int32, device=DEV)
    m = window_attention_drop_mask(B, H, H, heads, w, P, 55, word)
    assert 0 < int(m.sum()) < m.numel()
    a = _run(window_attention_packed, qkv, table, do, heads, w, s, d, math, P, 55, word)
    b = _run(window_attention_packed, qkv, table, do, heads, w, s, d, math, P, 0, None, m)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("B,H,w,s,heads,d", [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[6]])
def test_everything_is_written_and_two_runs_give_equal_bits(B, H, w, s, heads, d, drop, math):
    """out, dqkv, dtable and the scratch poisoned with NaN before the C entry points run: nothing may be left (partial tiles, padding rows and
    empty slots included); the values are those of the op, twice."""
    lib = L.load()
    qkv, table, do, mask, _, _ = _case(B, H, w, s, heads, d)
    qd, td, dd, md = qkv.to(DEV), table.to(DEV), do.to(DEV), (mask.to(DEV) if drop else None)
    p = P if drop else 0.0
    st = torch.cuda.current_stream(DEV).cuda_stream
    nan = float("nan")
    out, dqkv, dtab = torch.full_like(dd, nan), torch.full_like(qd, nan), torch.full_like(td, nan)
    n_scr = lib.hpfg_attn_window_packed_scratch_floats(B, H, H, heads, d, w, MATH[math])
    assert n_scr > 0
    scr = torch.full((n_scr,), nan, device=DEV)
    L.check(lib.hpfg_attn_window_packed_fwd(L.ptr(qd), L.ptr(td), L.ptr(out), B, H, H, heads, d, w, s, d ** -0.5, MATH[math], p, 0, None, L.ptr(md), st),
            "fwd")
    L.check(lib.hpfg_attn_window_packed_bwd(L.ptr(qd), L.ptr(td), L.ptr(dd), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, H, heads, d, w, s, d ** -0.5,
                                            MATH[math], p, 0, None, L.ptr(md), st), "bwd")
    for name, t in (("out", out), ("dqkv", dqkv), ("dtable", dtab), ("scratch", scr)):
        assert torch.isfinite(t).all(), name
    args = (P, 0, None, md) if drop else ()
    a = _run(window_attention_packed, qkv, table, do, heads, w, s, d, math, *args)
    b = _run(window_attention_packed, qkv, table, do, heads, w, s, d, math, *args)
    for x, y, z in zip((out, dqkv, dtab), a, b):
        assert torch.equal(x, y) and torch.equal(y, z)


def test_argument_errors_and_scratch_size():
    lib = L.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    buf = torch.zeros(1 << 16, device=DEV)
    p = L.ptr(buf)
    # (H, heads, d, w, s) and the rule the message must name
    bad = [((10, 1, 32, 5, 0), b"window must be 2, 3 or 4"), ((10, 1, 32, 3, 0), b"multiples of the window"), ((9, 1, 32, 3, 2), b"shift must be 0 or window / 2"),
           ((9, 1, 48, 3, 0), b"head dim must be 32 or 64")]
    for (H, heads, d, w, s), rule in bad:
        assert lib.hpfg_attn_window_packed_fwd(p, p, p, 1, H, H, heads, d, w, s, 1.0, 1, 0.0, 0, None, None, st) == -1
        msg = lib.hpfg_last_error()
        assert b"attn_window_packed_fwd" in msg and rule in msg, msg
        assert lib.hpfg_attn_window_packed_bwd(p, p, p, p, p, p, 1, H, H, heads, d, w, s, 1.0, 1, 0.0, 0, None, None, st) == -1
        msg = lib.hpfg_last_error()
        assert b"attn_window_packed_bwd" in msg and rule in msg, msg
    assert lib.hpfg_attn_window_packed_fwd(None, p, p, 1, 9, 9, 1, 32, 3, 0, 1.0, 1, 0.0, 0, None, None, st) == -1           # null qkv
    assert b"null pointer" in lib.hpfg_last_error()
    assert lib.hpfg_attn_window_packed_bwd(p, p, p, p, p, None, 1, 9, 9, 1, 32, 3, 0, 1.0, 1, 0.0, 0, None, None, st) == -1  # the backward needs its scratch
    assert b"null pointer" in lib.hpfg_last_error()
    assert lib.hpfg_attn_window_packed_fwd(p, p, p, 1, 9, 9, 1, 32, 3, 0, 1.0, 1, 1.0, 0, None, None, st) == -1              # p = 1
    assert lib.hpfg_attn_window_packed_scratch_floats(1, 10, 10, 1, 32, 5, 1) == -1 and b"attn_window_packed_scratch_floats" in lib.hpfg_last_error()
    assert lib.hpfg_attn_window_packed_scratch_floats(1, 10, 10, 1, 32, 3, 1) == -1
    # 16 windows of 3 x 3 per image -> 3 tiles of 7; one [heads][25] slab per (image, tile); f32: the unpacked kernels' slab per window
    assert lib.hpfg_attn_window_packed_scratch_floats(2, 12, 12, 3, 32, 3, 1) == 2 * 3 * 3 * 25
    assert lib.hpfg_attn_window_packed_scratch_floats(2, 12, 12, 3, 32, 3, 0) == lib.hpfg_attn_window_scratch_floats(2, 12, 12, 3, 32, 3, 0) == 2 * 16 * 3 * 25
    with pytest.raises(ValueError, match="outside 2 .. 4"):
        window_attention_packed(torch.zeros(1, 10, 10, 96, device=DEV), torch.zeros(81, 1, device=DEV), 1, 5, 0, 1.0)
