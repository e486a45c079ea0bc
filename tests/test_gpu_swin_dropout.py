"""GPU: dropout inside the Swin blocks.  ``window_attention_dropout`` (the DROP kernels of csrc/attn_window.hip) against the fp64 formula of
tests/test_gpu_swin.py with the mask applied after the softmax, in both math modes; the hash path against the explicit-mask path; p = 0
against ``window_attention``; reproducibility; every element of dqkv written; the keep rate; ``token_dropout`` bit for bit against its mask.

Bounds: tests/test_gpu_swin._bounds times 1 / (1 - p) -- every product the mask enters (P V, dP, dV) is scaled by at most that factor, so
the errors are."""
import functools

import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.ops_tokens import (dropout_mask, token_dropout, window_attention, window_attention_drop_mask, window_attention_dropout,
                                 window_attention_mask_elems)
from tests import helpers_swinunet as S
from tests import test_gpu_swin as SW
from tests.helpers import window_attn_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MATH = {"f32": 0, "bf16x3": 1}
# (B, H = W, w, s, heads, d): four shifted windows; window == map at head dim 64; 16 keys (the padded-key path); exactly 64 keys
SHAPES = [(2, 14, 7, 3, 2, 32), (1, 7, 7, 3, 1, 64), (1, 8, 4, 2, 3, 32), (1, 16, 8, 4, 1, 32)]
STRIDE_CAP = 8192 * 256          # float4 items of one pass of the grid-stride kernels


def _reference(qkv, table, mask, p, heads, w, s, scale):
    """SW._reference with attn_drop: the softmax's output times mask / (1 - p) before attn @ v; mask [B nW, heads, L, L].  The formula is
    the drop argument of tests/helpers.window_attn_reference."""
    return window_attn_reference(qkv, table, heads, w, s, scale, drop=(mask, p))


@functools.lru_cache(maxsize=None)
def _case(B, H, w, s, heads, d, p):
    """inputs, an explicit random mask of keep rate 1 - p, and the fp64 reference (out, dqkv, dtable): computed once, shared"""
    g = torch.Generator().manual_seed(1000 * H + 10 * w + s + d + int(100 * p))
    C_ = heads * d
    qkv, do = torch.randn(B, H, H, 3 * C_, generator=g), torch.randn(B, H, H, C_, generator=g)
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g)
    mask = (torch.rand(B * (H // w) ** 2, heads, w * w, w * w, generator=g) >= p).to(torch.uint8)
    qr, tr = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    o = _reference(qr, tr, mask, p, heads, w, s, d ** -0.5)
    o.backward(do.double())
    return qkv, table, do, mask, (o.detach(), qr.grad, tr.grad)


def _run(qkv, table, do, heads, w, s, d, math, p, seed=0, seed_dev=None, mask=None):
    qd, td = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        out = window_attention_dropout(qd, td, heads, w, s, d ** -0.5, p, seed, seed_dev, mask)
        out.backward(do.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    return out.detach(), qd.grad, td.grad


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES)
def test_window_attention_dropout_vs_fp64(B, H, w, s, heads, d, p, math):
    qkv, table, do, mask, ref = _case(B, H, w, s, heads, d, p)
    got = [t.cpu() for t in _run(qkv, table, do, heads, w, s, d, math, p, mask=mask.to(DEV))]
    errs = SW._errors(got, ref, heads * d)
    bnd = [b / (1.0 - p) for b in SW._bounds(B, H, w, d, math)]
    names = ("out", "dq", "dk", "dv", "dtable")
    print(f"window dropout {math} p={p} B={B} H={H} w={w} s={s} heads={heads} d={d}: " +
          "  ".join(f"{n} {e:.2e} (< {b:.2e})" for n, e, b in zip(names, errs, bnd)))
    for n, e, b in zip(names, errs, bnd):
        assert e < b, n


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES[:3])
def test_hash_path_equals_explicit_path(B, H, w, s, heads, d, math):
    """The mask hpfg_attn_window_drop_mask writes for (seed, seed word), fed back explicitly, gives the bits of the hash run."""
    qkv, table, do, _, _ = _case(B, H, w, s, heads, d, 0.1)
    word = torch.tensor([12345], dtype=torch.int32, device=DEV)
    m = window_attention_drop_mask(B, H, H, heads, w, 0.1, 77, word)
    assert m.numel() == window_attention_mask_elems(B, H, H, heads, w) and 0 < int(m.sum()) < m.numel()
    a = _run(qkv, table, do, heads, w, s, d, math, 0.1, 77, word)
    b = _run(qkv, table, do, heads, w, s, d, math, 0.1, mask=m)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES[:2])
def test_p_zero_gives_the_bits_of_window_attention(B, H, w, s, heads, d, math):
    """p = 0 without a mask launches the kernels of ``window_attention``, through the op and through the C entry points."""
    lib = L.load()
    qkv, table, do, _, _ = _case(B, H, w, s, heads, d, 0.1)
    want = SW._run(qkv, table, do, heads, w, s, d, math)
    for x, y in zip(_run(qkv, table, do, heads, w, s, d, math, 0.0), want):
        assert torch.equal(x, y)
    qd, td, dd = qkv.to(DEV), table.to(DEV), do.to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    out, dqkv, dtab = torch.empty_like(dd), torch.empty_like(qd), torch.empty_like(td)
    scr = torch.empty(lib.hpfg_attn_window_scratch_floats(B, H, H, heads, d, w, MATH[math]), device=DEV)
    L.check(lib.hpfg_attn_window_drop_fwd(L.ptr(qd), L.ptr(td), L.ptr(out), B, H, H, heads, d, w, s, d ** -0.5, MATH[math], 0.0, 5, None, None, st), "fwd")
    L.check(lib.hpfg_attn_window_drop_bwd(L.ptr(qd), L.ptr(td), L.ptr(dd), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, H, heads, d, w, s, d ** -0.5,
                                          MATH[math], 0.0, 5, None, None, st), "bwd")
    for x, y in zip((out, dqkv, dtab), want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_two_runs_give_equal_bits_and_every_gradient_element_is_written(math):
    """dqkv, dtable and out poisoned with NaN before the C entry points run: nothing may be left; the values are those of the op, twice."""
    lib = L.load()
    B, H, w, s, heads, d = SHAPES[2]          # 16 keys: padding keys and padding queries
    p = 0.5
    qkv, table, do, mask, _ = _case(B, H, w, s, heads, d, p)
    qd, td, dd, md = qkv.to(DEV), table.to(DEV), do.to(DEV), mask.to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    nan = float("nan")
    out, dqkv, dtab = torch.full_like(dd, nan), torch.full_like(qd, nan), torch.full_like(td, nan)
    scr = torch.full((lib.hpfg_attn_window_scratch_floats(B, H, H, heads, d, w, MATH[math]),), nan, device=DEV)
    L.check(lib.hpfg_attn_window_drop_fwd(L.ptr(qd), L.ptr(td), L.ptr(out), B, H, H, heads, d, w, s, d ** -0.5, MATH[math], p, 0, None, L.ptr(md), st), "fwd")
    L.check(lib.hpfg_attn_window_drop_bwd(L.ptr(qd), L.ptr(td), L.ptr(dd), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, H, heads, d, w, s, d ** -0.5,
                                          MATH[math], p, 0, None, L.ptr(md), st), "bwd")
    for t in (out, dqkv, dtab):
        assert torch.isfinite(t).all()
    a, b = _run(qkv, table, do, heads, w, s, d, math, p, mask=md), _run(qkv, table, do, heads, w, s, d, math, p, mask=md)
    for x, y, z in zip((out, dqkv, dtab), a, b):
        assert torch.equal(x, y) and torch.equal(y, z)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_and_seed_word(p):
    """n = 153 664 elements (B = 8 of the first shape): |rate - (1 - p)| <= 0.002 (the 8-bit threshold, csrc/common.h) + 4 sigma; another
    seed word gives another mask."""
    B, H, w, heads = 8, 14, 7, 2
    w0, w1 = (torch.tensor([v], dtype=torch.int32, device=DEV) for v in (5, 6))
    m0, m1 = (window_attention_drop_mask(B, H, H, heads, w, p, 3, wd) for wd in (w0, w1))
    n = m0.numel()
    assert n >= 150000 and tuple(m0.shape) == (B * 4, heads, 49, 49)
    rate = float(m0.float().mean())
    assert abs(rate - (1.0 - p)) <= 0.002 + 4.0 * (p * (1.0 - p) / n) ** 0.5, rate
    assert not torch.equal(m0, m1)
    assert torch.equal(m0, window_attention_drop_mask(B, H, H, heads, w, p, 3 + 5))          # the word is added to the seed
    assert torch.equal(m0.reshape(-1), dropout_mask(n, p, 3, w0))                           # the flat rule


@pytest.mark.parametrize("n", [4, 4 * (STRIDE_CAP + 3)])
def test_token_dropout_is_its_mask(n):
    """y = x * mask * (1 / (1 - p)) bit for bit with the mask of hpfg_dropout_mask, forward and backward; n = 4 (one lane) and just past one
    pass of the grid-stride loop.  The explicit path gives the same bits."""
    p, seed = 0.1, 9
    word = torch.tensor([4242], dtype=torch.int32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(n % 1000)
    x, dy = (torch.randn(n, device=DEV, generator=g) for _ in range(2))
    m = dropout_mask(n, p, seed, word)
    inv = float(S.inv_keep32(p))
    xr = x.clone().requires_grad_(True)
    y = token_dropout(xr, p, seed, word)
    y.backward(dy)
    assert torch.equal(y.detach(), x * m.float() * inv) and torch.equal(xr.grad, dy * m.float() * inv)
    assert torch.equal(token_dropout(x, p, mask=m), y.detach())
    if n > 4:
        assert abs(float(m.float().mean()) - (1.0 - p)) <= 0.002 + 4.0 * (p * (1.0 - p) / n) ** 0.5


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_block_with_dropout_vs_reference_fixture(math):
    """"dropblock" (tools/make_golden_swinunet.py): the reference block with drop = attn_drop = 0.1 and drop_path = 0.3 in train mode, its
    four recorded dropout masks and two drop-path draws replayed; the module rule 1e-3 max(1, max |reference|) per tensor."""
    import numpy as np
    import os
    from hpfg_amd.model import SwinTransformerBlock
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swinunet_dropblock.npz"))
    net = SwinTransformerBlock(32, 1, 7, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3, allow_dropout=True)
    net.load_state_dict({k[len("dropblock.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("dropblock.sd.")}, strict=True)
    net.external_draws = tuple(torch.from_numpy(r) for r in z["dropblock.draws"])
    net.external_masks = {k[len("dropblock.mask."):]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("dropblock.mask.")}
    assert sorted(net.external_masks) == ["attn.attn_drop", "attn.proj_drop", "mlp.drop1", "mlp.drop2"]
    net = net.to(DEV).train()
    y, dx, grads = SW._forward_backward(net, torch.from_numpy(z["dropblock.x"]), torch.from_numpy(z["dropblock.dy"]), math)
    pairs = [("y", y, z["dropblock.y"]), ("dx", dx, z["dropblock.dx"])] + [(f"grad.{k}", g_, z[f"dropblock.grad.{k}"]) for k, g_ in grads.items()]
    assert len(pairs) == 2 + len([k for k in z.files if k.startswith("dropblock.grad.")])
    for what, got, want in pairs:
        assert got is not None, what
        want = torch.from_numpy(want)
        err, bound = SW.maxerr(got.cpu(), want), 1e-3 * max(1.0, float(want.abs().max()))
        print(f"dropblock {math} {what}: {err:.2e} (<= {bound:.2e})")
        assert err <= bound, what
