"""Shifted-window attention (csrc/attn_window.hip, ops_tokens.window_attention) against the reference formula -- roll, window partition,
relative-position bias, shifted-window mask, softmax, window reverse, roll back -- in fp64 PyTorch on the CPU, in both math modes; its
forward against ``attention`` per window bit for bit; reproducibility; every element of dqkv written; argument errors; GELU and patch
merging; the Swin modules against the reference's fixtures (tools/make_golden_swin.py); a captured forward + backward.

Kernel bounds are those of tests/test_gpu_attn_keys.py for at most 64 keys: out 2e-5 k, dq 5e-5 k, dk / dv 2e-4 k with k = 1 (HPFG_MATH=f32)
or 8 (split-bf16 products), times sqrt(2) at head dim 64.  A bias-table entry sums dS over up to T = B (H/w)^2 w^2 (query, key) pairs, so
its bound is 2e-4 k max(1, sqrt(T / 256)) -- the random-walk rule that file uses for dK / dV sums over queries.
Module bounds: max |error| <= 1e-3 max(1, max |reference tensor|) for the output and every gradient."""
import functools
import os

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.model import BasicBlock, SwinTransformerBlock
from hpfg_amd.ops_tokens import attention, gelu, patch_merge, window_attention
from tests.helpers import maxerr
from tests.helpers import window_attn_reference as _reference
from tests.helpers import window_partition as _partition
from tests.helpers import window_reverse as _reverse

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MATH = {"f32": 0, "bf16x3": 1}

# (B, H = W, w, s, heads, d): four windows; all nine mask regions meet inside windows; window == map (wrap-around only); 16 keys (the
# padded-key path); exactly 64 keys (no padding)
SHAPES = [(2, 14, 7, 0, 2, 32), (2, 14, 7, 3, 2, 32), (1, 7, 7, 3, 1, 64), (1, 8, 4, 2, 3, 32), (1, 16, 8, 4, 1, 32)]


@functools.lru_cache(maxsize=None)
def _case(B, H, w, s, heads, d):
    """inputs (fp32) and the fp64 reference (out, dqkv, dtable), computed once per shape and shared; plus the error of the same formula in
    plain fp32 on the CPU against it"""
    g = torch.Generator().manual_seed(100 * H + 10 * w + s + d)
    C_ = heads * d
    qkv, do = torch.randn(B, H, H, 3 * C_, generator=g), torch.randn(B, H, H, C_, generator=g)
    table = torch.randn((2 * w - 1) ** 2, heads, generator=g)
    res = []
    for dt in (torch.float64, torch.float32):
        qr, tr = qkv.to(dt).clone().requires_grad_(True), table.to(dt).clone().requires_grad_(True)
        o = _reference(qr, tr, heads, w, s, d ** -0.5)
        o.backward(do.to(dt))
        res.append((o.detach(), qr.grad, tr.grad))
    f32_err = _errors(res[1], res[0], C_)
    return qkv, table, do, res[0], f32_err


def _errors(got, ref, C_):
    """(out, dq, dk, dv, dtable) max abs errors"""
    return (maxerr(got[0], ref[0]), maxerr(got[1][..., :C_], ref[1][..., :C_]), maxerr(got[1][..., C_:2 * C_], ref[1][..., C_:2 * C_]),
            maxerr(got[1][..., 2 * C_:], ref[1][..., 2 * C_:]), maxerr(got[2], ref[2]))


def _bounds(B, H, w, d, math):
    k = (1.0 if math == "f32" else 8.0) * (2 ** 0.5 if d == 64 else 1.0)
    kb = 1.0 if math == "f32" else 8.0
    T = B * (H // w) ** 2 * w * w
    return 2e-5 * k, 5e-5 * k, 2e-4 * k, 2e-4 * k, 2e-4 * kb * max(1.0, (T / 256) ** 0.5)


def _run(qkv, table, do, heads, w, s, d, math):
    qd, td = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        out = window_attention(qd, td, heads, w, s, d ** -0.5)
        out.backward(do.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    return out.detach(), qd.grad, td.grad


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", SHAPES)
def test_window_attention_vs_fp64(B, H, w, s, heads, d, math):
    qkv, table, do, ref, f32_err = _case(B, H, w, s, heads, d)
    got = [t.cpu() for t in _run(qkv, table, do, heads, w, s, d, math)]
    errs, bnd = _errors(got, ref, heads * d), _bounds(B, H, w, d, math)
    names = ("out", "dq", "dk", "dv", "dtable")
    print(f"window {math} B={B} H={H} w={w} s={s} heads={heads} d={d}: " +
          "  ".join(f"{n} {e:.2e} (< {b:.2e})" for n, e, b in zip(names, errs, bnd)) +
          "   [plain fp32 on the CPU: " + " ".join(f"{n} {e:.2e}" for n, e in zip(names, f32_err)) + "]")
    for n, e, b in zip(names, errs, bnd):
        assert e < b, n


@pytest.mark.parametrize("B,H,w,heads,d", [(2, 14, 7, 2, 32), (1, 8, 4, 3, 32), (1, 16, 8, 1, 32), (1, 7, 7, 1, 64), (1, 8, 4, 2, 64)])
def test_unshifted_zero_bias_forward_is_bitwise_attention_per_window(B, H, w, heads, d):
    """s = 0 and a zero table add exact zeros to the scores: the operation sequence, hence every bit, of attn_mfma_fwd_kernel applied to each
    window of a partitioned copy (split-bf16 mode)"""
    qkv = _case(B, H, w, 0, heads, d)[0].to(DEV)
    C_ = heads * d
    table = torch.zeros((2 * w - 1) ** 2, heads, device=DEV)
    ops_tokens.MATH["mode"] = "bf16x3"
    try:
        out = window_attention(qkv, table, heads, w, 0, d ** -0.5)
        xw = _partition(qkv, w)
        old = attention(xw[..., :C_].contiguous(), xw[..., C_:].contiguous(), heads, d ** -0.5)
    finally:
        ops_tokens.MATH["mode"] = None
    assert torch.equal(out, _reverse(old, B, H, H, w))


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", [(2, 14, 7, 3, 2, 32), (1, 7, 7, 3, 1, 64)])
def test_two_runs_give_equal_bits(B, H, w, s, heads, d, math):
    qkv, table, do, _, _ = _case(B, H, w, s, heads, d)
    a, b = _run(qkv, table, do, heads, w, s, d, math), _run(qkv, table, do, heads, w, s, d, math)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,H,w,s,heads,d", [(2, 14, 7, 3, 2, 32), (1, 8, 4, 2, 3, 32), (1, 7, 7, 3, 1, 64)])
def test_every_gradient_element_is_written(B, H, w, s, heads, d, math):
    """dqkv, dtable and out poisoned with NaN before the C entry points run: nothing may be left, and the values are those of the op"""
    lib = L.load()
    qkv, table, do, _, _ = _case(B, H, w, s, heads, d)
    qd, td, dd = qkv.to(DEV), table.to(DEV), do.to(DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    nan = float("nan")
    out, dqkv, dtab = torch.full_like(dd, nan), torch.full_like(qd, nan), torch.full_like(td, nan)
    scr = torch.full((lib.hpfg_attn_window_scratch_floats(B, H, H, heads, d, w, MATH[math]),), nan, device=DEV)
    L.check(lib.hpfg_attn_window_fwd(L.ptr(qd), L.ptr(td), L.ptr(out), B, H, H, heads, d, w, s, d ** -0.5, MATH[math], st), "fwd")
    L.check(lib.hpfg_attn_window_bwd(L.ptr(qd), L.ptr(td), L.ptr(dd), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, H, heads, d, w, s, d ** -0.5, MATH[math],
                                     st), "bwd")
    for t in (out, dqkv, dtab):
        assert torch.isfinite(t).all()
    for x, y in zip((out, dqkv, dtab), _run(qkv, table, do, heads, w, s, d, math)):
        assert torch.equal(x, y)


def test_argument_errors():
    lib = L.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    buf = torch.zeros(1 << 16, device=DEV)
    p = L.ptr(buf)
    # (H, W, heads, d, w, s): 81 keys; a side not divisible; head dim 48; no heads; shift == window
    for H, W, heads, d, w, s in ((18, 18, 1, 32, 9, 4), (15, 14, 1, 32, 7, 0), (14, 14, 1, 48, 7, 0), (14, 14, 0, 32, 7, 0), (14, 14, 1, 32, 7, 7)):
        assert lib.hpfg_attn_window_fwd(p, p, p, 1, H, W, heads, d, w, s, 1.0, 1, st) == -1
        msg = lib.hpfg_last_error()
        assert b"attn_window_fwd" in msg and b"64 keys" in msg and b"head dim" in msg
        assert lib.hpfg_attn_window_bwd(p, p, p, p, p, p, 1, H, W, heads, d, w, s, 1.0, 1, st) == -1
        assert b"attn_window_bwd" in lib.hpfg_last_error()
    assert lib.hpfg_attn_window_scratch_floats(1, 18, 18, 1, 32, 9, 1) == -1 and b"attn_window_scratch_floats" in lib.hpfg_last_error()
    assert lib.hpfg_attn_window_fwd(None, p, p, 1, 14, 14, 1, 32, 7, 0, 1.0, 1, st) == -1           # null qkv
    assert lib.hpfg_attn_window_fwd(p, p, p, 1, 14, 14, 1, 32, 7, 0, 1.0, 2, st) == -1              # no such math mode
    assert lib.hpfg_attn_window_bwd(p, p, p, p, p, None, 1, 14, 14, 1, 32, 7, 0, 1.0, 1, st) == -1  # the backward needs its scratch
    assert lib.hpfg_attn_window_scratch_floats(2, 14, 14, 3, 32, 7, 1) == 2 * 4 * 3 * 169
    assert lib.hpfg_gelu_fwd(p, p, 6, st) == -1 and lib.hpfg_patch_merge_fwd(p, p, 1, 5, 4, 8, st) == -1
    with pytest.raises(ValueError, match="square"):
        window_attention(torch.zeros(1, 14, 21, 96, device=DEV), torch.zeros(169, 1, device=DEV), 1, 7, 0, 1.0)


def test_gelu_and_patch_merge():
    """GELU against fp64 erf: fp32 erff / expf are good to a few ulp, |gelu| <= |u| <= 6 and |gelu'| <= 1.13 on these inputs, so 2e-6 forward
    (6 x 4 ulp of 6e-8) and 1e-5 backward (times |dy| <= 6); patch merging moves data only: bit-equal to the reference's slicing + concat"""
    g = torch.Generator().manual_seed(3)
    x, dy = (torch.randn(3, 5, 7, 12, generator=g) * 1.5).clamp(-6, 6), torch.randn(3, 5, 7, 12, generator=g).clamp(-6, 6)
    xd = x.to(DEV).requires_grad_(True)
    y = gelu(xd)
    y.backward(dy.to(DEV))
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.gelu(xr)
    yr.backward(dy.double())
    e_f, e_b = maxerr(y.detach().cpu(), yr.detach()), maxerr(xd.grad.cpu(), xr.grad)
    print(f"gelu: forward {e_f:.2e} (< 2e-6)  backward {e_b:.2e} (< 1e-5)")
    assert e_f < 2e-6 and e_b < 1e-5
    x = torch.randn(2, 6, 10, 8, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = patch_merge(xd)
    want = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    assert torch.equal(y.detach().cpu(), want)
    dy = torch.randn(2, 3, 5, 32, generator=g)
    y.backward(dy.to(DEV))
    xr = x.clone().requires_grad_(True)
    torch.cat([xr[:, 0::2, 0::2], xr[:, 1::2, 0::2], xr[:, 0::2, 1::2], xr[:, 1::2, 1::2]], -1).backward(dy)
    assert torch.equal(xd.grad.cpu(), xr.grad)


# ---- the modules against the reference's fixtures ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def _module_case(case):
    """(module on the device with the reference's weights, fixture, prefix of the case's arrays, prefix of its shared input arrays)"""
    if case in ("plain", "shift"):
        z, net, src = _fixture("swin_block.npz"), SwinTransformerBlock(64, 2, 7, shift=case == "shift", mlp_ratio=1.0), "plain"
    elif case == "droppath":
        z, net, src = _fixture("swin_stage.npz"), SwinTransformerBlock(32, 1, 7, shift=True, drop_path=0.3), case
    else:
        z, net, src = _fixture("swin_stage.npz"), BasicBlock(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2)), case
    pre = f"{src}.sd."
    net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)
    if case == "droppath":
        net.external_draws = tuple(torch.from_numpy(r) for r in z["droppath.draws"])
    if case == "basic":
        net.external_draws = [None, tuple(torch.from_numpy(r) for r in z["basic.draws"])]
    return net.to(DEV).train(), z, case, src


def _forward_backward(net, x, dy, math):
    xd = x.to(DEV).requires_grad_(True)
    net.zero_grad(set_to_none=True)
    ops_tokens.MATH["mode"] = math
    try:
        y = net(xd)
        y.backward(dy.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    return y.detach(), xd.grad, {k: p.grad for k, p in net.named_parameters()}


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", ["plain", "shift", "droppath", "basic"])
def test_modules_vs_reference_fixture(case, math):
    net, z, name, src = _module_case(case)
    x, dy = torch.from_numpy(z[f"{src}.x"]), torch.from_numpy(z[f"{src}.dy"])
    y, dx, grads = _forward_backward(net, x, dy, math)
    pairs = [("y", y, z[f"{name}.y"]), ("dx", dx, z[f"{name}.dx"])] + [(f"grad.{k}", g_, z[f"{name}.grad.{k}"]) for k, g_ in grads.items()]
    assert len(pairs) == 2 + len([k for k in z.files if k.startswith(f"{name}.grad.")])
    worst = ("", 0.0)
    for what, got, want in pairs:
        assert got is not None, what
        want = torch.from_numpy(want)
        err, bound = maxerr(got.cpu(), want), 1e-3 * max(1.0, float(want.abs().max()))
        if err / bound > worst[1]:
            worst = (what, err / bound)
        print(f"{case} {math} {what}: {err:.2e} (<= {bound:.2e})")
        assert err <= bound, what
    print(f"{case} {math}: worst error / bound = {worst[1]:.3f} at {worst[0]}")


def test_eval_equals_train_without_drop_path():
    net, z, _, src = _module_case("shift")
    x = torch.from_numpy(z[f"{src}.x"]).to(DEV)
    with torch.no_grad():
        y_train = net(x)
        y_eval = net.eval()(x)
    assert torch.equal(y_train, y_eval)


def test_captured_block_replays_the_eager_bits():
    """forward + backward of one shifted block captured with torch.cuda.graph, replayed twice: the eager run's bits each time.  Captured the
    way hpfg_amd.train.GraphedStep captures a step: warm-up on a side stream, thread-local capture mode (backward launches its kernels
    from the autograd engine's thread), .backward() into fresh .grad tensors that live in the graph's pool."""
    net, z, _, src = _module_case("shift")
    x, dy = torch.from_numpy(z[f"{src}.x"]).to(DEV).requires_grad_(True), torch.from_numpy(z[f"{src}.dy"]).to(DEV)
    leaves = [x] + list(net.parameters())

    def step():
        for t in leaves:
            t.grad = None
        y = net(x)
        y.backward(dy)
        return [y.detach()] + [t.grad for t in leaves]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    replays = []
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in outs])
    eager = step()
    assert len(eager) == len(outs) == 2 + len(list(net.parameters()))
    for got in replays:
        for a, b in zip(got, eager):
            assert torch.isfinite(a).all() and torch.equal(a, b)
