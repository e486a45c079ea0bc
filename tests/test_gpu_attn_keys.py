"""Attention core over 65 .. 256 keys (csrc/attn_keys.hip, ops_tokens.attention_keys) against plain PyTorch in fp64 on the CPU, in both math
modes and both head dims; its forward against the <= 64-key kernels bit for bit; reproducibility; padding keys; argument errors.

Bounds start from those of tests/test_gpu_tokens.py::test_attention_core / tests/test_gpu_attn_hd64.py for the same head dim:
out 2e-5 k, dq 5e-5 k, dkv 2e-4 k max(1, sqrt(N / 256)) with k = 1 (HPFG_MATH=f32) or 8 (split-bf16 products), times sqrt(2) at head dim 64.
A dq element is now a sum over M instead of at most 64 keys, so its bound grows by sqrt(M / 64) (a random walk over the terms); out is a
convex combination of the values and dK / dV sum over the queries, so those two bounds stay."""
import functools

import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.ops_tokens import MAX_KEYS_LONG, attention, attention_keys
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MATH = {"f32": 0, "bf16x3": 1}

# the smallest shapes where the block logic can go wrong: one key in the second block, the 288^2 stage shape with ragged queries, two full
# blocks, one key in the third, ragged third / fourth blocks, the 512^2 stage 4, a single query against four full blocks
SHAPES = [(1, 10, 65, 1), (2, 130, 81, 2), (1, 100, 128, 1), (1, 77, 129, 5), (1, 64, 200, 2), (1, 33, 255, 1), (1, 256, 256, 8), (1, 1, 256, 1)]
WIDE = (1, 16384, 256, 1)          # 512^2 stage 1 of MiT-B1


def _reference(q, kv, heads, d, scale):
    B, N, C_ = q.shape
    M = kv.shape[1]
    qh = q.reshape(B, N, heads, d).permute(0, 2, 1, 3)
    k, v = kv.reshape(B, M, 2, heads, d).permute(2, 0, 3, 1, 4)
    a = ((qh @ k.transpose(-2, -1)) * scale).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B, N, C_)


@functools.lru_cache(maxsize=None)
def _case(B, N, M, heads, d):
    """inputs (fp32) and the fp64 reference (out, dq, dkv), computed once per shape and shared by the tests; plus the error of the same
    formula in plain fp32 on the CPU against it (printed beside the device's: the scale of fp32 rounding on these inputs)"""
    g = torch.Generator().manual_seed(1000 * d + N + M)
    C_ = heads * d
    q, kv, do = torch.randn(B, N, C_, generator=g), torch.randn(B, M, 2 * C_, generator=g), torch.randn(B, N, C_, generator=g)
    res = []
    for dt in (torch.float64, torch.float32):
        qr, kr = q.to(dt).clone().requires_grad_(True), kv.to(dt).clone().requires_grad_(True)          # (clone: .to() of an fp32 tensor is the tensor)
        o = _reference(qr, kr, heads, d, d ** -0.5)
        o.backward(do.to(dt))
        res.append((o.detach(), qr.grad, kr.grad))
    f32_err = tuple(maxerr(a.double(), b) for a, b in zip(res[1], res[0]))
    return q, kv, do, res[0], f32_err


def _bounds(N, M, d, math):
    k = (1.0 if math == "f32" else 8.0) * (2 ** 0.5 if d == 64 else 1.0)
    return 2e-5 * k, 5e-5 * k * max(1.0, (M / 64) ** 0.5), 2e-4 * k * max(1.0, (N / 256) ** 0.5)


def _run(q, kv, do, heads, d, math, fn=attention_keys):
    qd, kd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        out = fn(qd, kd, heads, d ** -0.5)
        out.backward(do.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    return out.detach(), qd.grad, kd.grad


def _check(B, N, M, heads, d, math, tag):
    q, kv, do, ref, f32_err = _case(B, N, M, heads, d)
    got = _run(q, kv, do, heads, d, math)
    errs = [maxerr(a.cpu().double(), b) for a, b in zip(got, ref)]
    bnd = _bounds(N, M, d, math)
    print(f"{tag} {math} d={d} B={B} N={N} M={M} heads={heads}: out {errs[0]:.2e} (< {bnd[0]:.2e})  dq {errs[1]:.2e} (< {bnd[1]:.2e})  "
          f"dkv {errs[2]:.2e} (< {bnd[2]:.2e})   [plain fp32 on the CPU: out {f32_err[0]:.2e} dq {f32_err[1]:.2e} dkv {f32_err[2]:.2e}]")
    assert errs[0] < bnd[0]
    assert errs[1] < bnd[1]
    assert errs[2] < bnd[2]


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("B,N,M,heads", SHAPES)
def test_attention_keys_vs_fp64(B, N, M, heads, d, math):
    _check(B, N, M, heads, d, math, "keys")


def test_attention_keys_wide_stage_vs_fp64():
    """16384 queries against 256 keys at head dim 64 (stage 1 of MiT-B1 at 512 x 512): 256 forward workgroups, 32 x 4 dK / dV partials"""
    _check(*WIDE, 64, "bf16x3", "wide")


def _raw(lib, fn_fwd, fn_bwd, q, kv, do, B, N, M, heads, d, math=1, kv_out=None):
    """the C entry points directly: (out, lse, dq, dkv)"""
    st = torch.cuda.current_stream(DEV).cuda_stream
    scale = d ** -0.5
    out, dq, dkv = torch.zeros_like(q), torch.zeros_like(q), (torch.zeros_like(kv) if kv_out is None else kv_out)
    lse = torch.zeros(B, heads, N, device=DEV)
    scr = torch.zeros(lib.hpfg_attn_keys_scratch_floats(B, N, M, heads, d, math), device=DEV)
    L.check(fn_fwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), B, N, M, heads, d, scale, math, st), "fwd")
    L.check(fn_bwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, d, scale, math, st), "bwd")
    return out, lse, dq, dkv


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("B,N,M,heads", [(2, 100, 1, 1), (1, 130, 33, 2), (2, 777, 49, 5), (1, 10, 64, 1), (3, 321, 64, 2)])
def test_forward_is_bitwise_the_64_key_kernel(B, N, M, heads, d):
    """For M <= 64 the new forward runs one key block: the operation sequence of attn_mfma_fwd_kernel, hence its bits (split-bf16 mode).
    The backward rebuilds P from lse instead of the in-tile softmax, so it is compared with the fp64 reference at the usual bounds."""
    lib = L.load()
    q, kv, do, ref, _ = _case(B, N, M, heads, d)
    qd, kd, dd = q.to(DEV), kv.to(DEV), do.to(DEV)
    out, lse, dq, dkv = _raw(lib, lib.hpfg_attn_keys_fwd, lib.hpfg_attn_keys_bwd, qd, kd, dd, B, N, M, heads, d)
    old = torch.zeros_like(qd)
    L.check(lib.hpfg_attn_mfma_fwd_hd(L.ptr(qd), L.ptr(kd), L.ptr(old), B, N, M, heads, d, d ** -0.5, torch.cuda.current_stream(DEV).cuda_stream), "old fwd")
    assert torch.equal(out, old)
    # lse is the log of the softmax denominator: exp(s - lse) sums to 1 over the keys
    k = kd.view(B, M, 2, heads, d)[:, :, 0]
    s = torch.einsum("bnhd,bmhd->bhnm", qd.view(B, N, heads, d), k) * d ** -0.5
    assert maxerr(lse.cpu(), torch.logsumexp(s, -1).cpu()) < 1e-4
    bnd = _bounds(N, M, d, "bf16x3")
    e_dq, e_dkv = maxerr(dq.cpu().double(), ref[1]), maxerr(dkv.cpu().double(), ref[2])
    print(f"bitwise forward d={d} B={B} N={N} M={M} heads={heads}: dq {e_dq:.2e} (< {bnd[1]:.2e})  dkv {e_dkv:.2e} (< {bnd[2]:.2e})")
    assert e_dq < bnd[1] and e_dkv < bnd[2]


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,N,M,heads", [(2, 130, 81, 2), (1, 256, 256, 8)])
def test_two_runs_give_equal_bits(B, N, M, heads, math):
    q, kv, do, _, _ = _case(B, N, M, heads, 64)
    a, b = _run(q, kv, do, heads, 64, math), _run(q, kv, do, heads, 64, math)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("M", [65, 81, 200])
def test_padding_keys_are_never_read_as_data(M, d, math):
    """kv rows beyond M in an over-allocated buffer hold NaN: nothing may read them as data, nothing may write the dkv rows beyond M"""
    lib = L.load()
    B, N, heads, rows = 1, 70, 2, 256
    q, kv, do, _, _ = _case(B, N, M, heads, d)
    qd, dd = q.to(DEV), do.to(DEV)
    res = []
    for fill in (float("nan"), 0.0):
        buf = torch.full((B, rows, 2 * heads * d), fill, device=DEV)
        buf[:, :M] = kv.to(DEV)
        dkv = torch.full_like(buf, 7.0)
        res.append(_raw(lib, lib.hpfg_attn_keys_fwd, lib.hpfg_attn_keys_bwd, qd, buf, dd, B, N, M, heads, d, MATH[math], kv_out=dkv))
    for x, y in zip(*res):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    assert bool((res[0][3][:, M:] == 7.0).all())


def test_argument_errors():
    lib = L.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    assert lib.hpfg_attn_keys_max() == MAX_KEYS_LONG == 256
    q, kv = torch.zeros(1, 8, 64, device=DEV), torch.zeros(1, 257, 128, device=DEV)
    with pytest.raises(ValueError, match="256"):
        attention_keys(q, kv, 1, 0.125)                                   # 257 keys
    with pytest.raises(ValueError, match="head dim"):
        attention_keys(torch.zeros(1, 8, 96, device=DEV), torch.zeros(1, 70, 192, device=DEV), 2, 48 ** -0.5)
    with pytest.raises(ValueError, match="kv"):
        attention(q, torch.zeros(1, 65, 128, device=DEV), 1, 0.125)      # the <= 64-key op still refuses 65 keys
    lse, scr = torch.zeros(8, device=DEV), torch.zeros(1 << 16, device=DEV)
    p = L.ptr
    for M, d in ((257, 64), (0, 64), (70, 48)):
        assert lib.hpfg_attn_keys_fwd(p(q), p(kv), p(q), p(lse), 1, 8, M, 1, d, 0.125, 1, st) == -1
        msg = lib.hpfg_last_error()
        assert b"attn_keys_fwd" in msg and b"256 keys" in msg and b"head dim" in msg
        assert lib.hpfg_attn_keys_bwd(p(q), p(kv), p(q), p(lse), p(q), p(q), p(kv), p(scr), 1, 8, M, 1, d, 0.125, 1, st) == -1
        assert b"attn_keys_bwd" in lib.hpfg_last_error()
        assert lib.hpfg_attn_keys_scratch_floats(1, 8, M, 1, d, 1) == -1
        assert b"attn_keys_scratch_floats" in lib.hpfg_last_error()
    assert lib.hpfg_attn_keys_fwd(None, p(kv), p(q), p(lse), 1, 8, 70, 1, 64, 0.125, 1, st) == -1           # null q
    assert lib.hpfg_attn_keys_fwd(p(q), p(kv), p(q), p(lse), 1, 8, 70, 1, 64, 0.125, 2, st) == -1          # no such math mode
    assert lib.hpfg_attn_keys_bwd(p(q), p(kv), p(q), None, p(q), p(q), p(kv), p(scr), 1, 8, 70, 1, 64, 0.125, 1, st) == -1      # the backward needs lse
    assert lib.hpfg_attn_keys_scratch_floats(0, 8, 70, 1, 64, 1) == -1 and lib.hpfg_attn_keys_scratch_floats(1, 8, 70, 1, 64, 5) == -1
    assert lib.hpfg_attn_keys_scratch_floats(1, 8, 70, 1, 64, 0) == 2 * 8 * 70
    assert lib.hpfg_attn_keys_scratch_floats(2, 600, 70, 3, 64, 1) == 2 * 600 * 3 + 2 * 3 * 2 * 2 * 2 * 64 * 64
