"""Attention core at head dim 64 (MiT-B1: widths 64/128/320/512 on 1/2/5/8 heads) against plain PyTorch fp32 on the CPU, in both math modes:
the MFMA kernels of csrc/attn.hip (template over the head dim) and the exact-fp32 thread-per-query kernels of csrc/tokens.hip.

Bounds: those of tests/test_gpu_tokens.py::test_attention_core times sqrt(2) -- a score is a sum of 64 products instead of 32, so its
rounding error (a random walk over the products) grows by sqrt(2); everything downstream is linear in it."""
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.ops_tokens import attention
from tests.helpers import ATTN_YARDSTICK, attn_f64, attn_tolerance, maxerr, worst_ratio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

B1_224 = [(2, 3136, 49, 1), (1, 784, 49, 2), (1, 196, 49, 5), (1, 49, 49, 8)]          # the four stages of MiT-B1 at 224 x 224
RAGGED = [(2, 100, 1, 1), (1, 130, 4, 2), (3, 1100, 33, 5), (1, 10, 64, 1), (2, 777, 64, 2), (1, 1, 33, 8)]


def _reference(q, kv, heads, d, scale):
    B, N, C_ = q.shape
    M = kv.shape[1]
    qh = q.reshape(B, N, heads, d).permute(0, 2, 1, 3)
    k, v = kv.reshape(B, M, 2, heads, d).permute(2, 0, 3, 1, 4)
    a = ((qh @ k.transpose(-2, -1)) * scale).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B, N, C_)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,N,M,heads", B1_224 + RAGGED)
def test_attention_core_head_dim_64(B, N, M, heads, math):
    g = torch.Generator().manual_seed(N + M)
    d = 64
    C_ = heads * d
    q, kv, do = torch.randn(B, N, C_, generator=g), torch.randn(B, M, 2 * C_, generator=g), torch.randn(B, N, C_, generator=g)
    scale = d ** -0.5
    qr, kr = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    _reference(qr, kr, heads, d, scale).backward(do)
    qd, kd = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        out = attention(qd, kd, heads, scale)
        out.backward(do.to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    k = (1.0 if math == "f32" else 8.0) * 2 ** 0.5
    e_out = maxerr(out.detach().cpu(), _reference(q, kv, heads, d, scale))
    e_dq, e_dkv = maxerr(qd.grad.cpu(), qr.grad), maxerr(kd.grad.cpu(), kr.grad)
    b_out, b_dq, b_dkv = 2e-5 * k, 5e-5 * k, 2e-4 * k * max(1.0, (N / 256) ** 0.5)
    print(f"hd64 {math} B={B} N={N} M={M} heads={heads}: out {e_out:.2e} (< {b_out:.2e})  dq {e_dq:.2e} (< {b_dq:.2e})  dkv {e_dkv:.2e} (< {b_dkv:.2e})")
    assert e_out < b_out
    assert e_dq < b_dq
    assert e_dkv < b_dkv
    # and against the float64 law under the rule of tests/test_gpu_attn_edges.py: 8 x the error of the mode's yardstick against the law
    law = attn_f64(q, kv, do, heads, d, scale)
    tol = attn_tolerance(law, attn_f64(q, kv, do, heads, d, scale, arith=ATTN_YARDSTICK[math]))
    _, ratios = worst_ratio((out.detach().cpu(), qd.grad.cpu(), kd.grad.cpu()), (law[0], law[2], law[3]), (tol[0], tol[2], tol[3]))
    print(f"hd64 {math} B={B} N={N} M={M} heads={heads}: out {ratios[0]:.3f}  dq {ratios[1]:.3f}  dkv {ratios[2]:.3f}   (error / tolerance against float64)")
    assert max(ratios) < 1.0


@pytest.mark.parametrize("B,N,M,heads", [(2, 3136, 49, 1), (3, 1100, 33, 5), (1, 10, 64, 2)])
def test_head_dim_32_through_new_entry_points_is_bitwise_the_old(B, N, M, heads):
    """hpfg_attn_mfma_fwd / _bwd and hpfg_attn_fwd / _bwd (head dim 32) against the head_dim-carrying entry points with head_dim = 32.
    The old entry points forward to the new ones, so this pins the ABI (same meaning, scratch size, argument order) -- it cannot show that
    the D = 32 instantiation equals the kernels as they were before they became templates; that rests on the per-accumulator MFMA order
    being unchanged and on tests/test_gpu_tokens.py / tests/test_gpu_segformer.py passing unchanged."""
    lib = L.load()
    g = torch.Generator().manual_seed(N * 3 + M)
    C_ = heads * 32
    q, kv, do = (t.to(DEV) for t in (torch.randn(B, N, C_, generator=g), torch.randn(B, M, 2 * C_, generator=g), torch.randn(B, N, C_, generator=g)))
    scale = 32 ** -0.5
    st = torch.cuda.current_stream(DEV).cuda_stream
    n_scr = lib.hpfg_attn_mfma_scratch_floats(B, N, heads, 32)
    assert n_scr == B * heads * lib.hpfg_attn_mfma_blocks(N) * 2 * 64 * 32
    assert lib.hpfg_attn_mfma_scratch_floats(B, N, heads, 64) == 2 * n_scr and lib.hpfg_attn_mfma_scratch_floats(B, N, heads, 48) == -1

    def mfma(new):
        out, dq, dkv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(kv)
        scr = torch.zeros(n_scr, device=DEV)
        hd = (32,) if new else ()
        fwd, bwd = (lib.hpfg_attn_mfma_fwd_hd, lib.hpfg_attn_mfma_bwd_hd) if new else (lib.hpfg_attn_mfma_fwd, lib.hpfg_attn_mfma_bwd)
        L.check(fwd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, M, heads, *hd, scale, st), "fwd")
        L.check(bwd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, *hd, scale, st), "bwd")
        return out, dq, dkv

    def exact(new):
        out, dq = torch.zeros_like(q), torch.zeros_like(q)
        P, dS = torch.zeros(B, heads, N, M, device=DEV), torch.zeros(B, heads, N, M, device=DEV)
        hd = (32,) if new else ()
        fwd, bwd = (lib.hpfg_attn_fwd_hd, lib.hpfg_attn_bwd_hd) if new else (lib.hpfg_attn_fwd, lib.hpfg_attn_bwd)
        L.check(fwd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, M, heads, *hd, scale, st), "fwd")
        L.check(bwd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(P), L.ptr(dS), B, N, M, heads, *hd, scale, st), "bwd")
        return out, dq, P, dS

    for fn in (mfma, exact):
        for a, b in zip(fn(False), fn(True)):
            assert torch.equal(a, b)
    # and through the autograd op, which now calls the new entry points
    qd, kd = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    out = attention(qd, kd, heads, scale)
    out.backward(do)
    o_old, dq_old, dkv_old = mfma(False)
    if ops_tokens.gemm_math() == "bf16x3":
        assert torch.equal(out.detach(), o_old) and torch.equal(qd.grad, dq_old) and torch.equal(kd.grad, dkv_old)


def test_other_head_dims_are_rejected_with_a_clear_message():
    q, kv = torch.zeros(1, 8, 96, device=DEV), torch.zeros(1, 4, 192, device=DEV)
    with pytest.raises(ValueError, match="head dim"):
        attention(q, kv, 2, 48 ** -0.5)          # head dim 48
    with pytest.raises(ValueError, match="head dim"):
        attention(q, kv, 6, 16 ** -0.5)          # head dim 16
    lib = L.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    assert lib.hpfg_attn_mfma_fwd_hd(L.ptr(q), L.ptr(kv), L.ptr(q), 1, 8, 4, 2, 48, 1.0, st) == -1
    assert b"head dim" in lib.hpfg_last_error()
    with pytest.raises(ValueError, match="kv"):
        attention(torch.zeros(1, 8, 64, device=DEV), torch.zeros(1, 65, 128, device=DEV), 1, 0.125)          # 65 keys
