"""GPU: train-mode BatchNorm over tokens without an activation (hpfg_bn_tok_stats / _apply / _bwd of csrc/tokens.hip through hpfg_amd._lib, and
ops_tokens.batch_norm_tokens) against the float64 laws of tests/helpers_uniformer.py, by the rule of tests/test_gpu_tokens_edges.py: canaries
around every output and the partial-sum scratch, finiteness, and err <= helpers.bound_8x(law, torch's float32 CPU result).

C = 320 and 260 do not divide the workgroup into whole row lanes (80 and 65 quads: 16 and 61 idle threads), which hpfg_tok_col_stats
refuses; hpfg_bn_tok_stats admits them on the same kernels.  The kernels are the RELU = false instances of the BatchNorm + ReLU + dropout
templates, so the last test pins the bits bn_relu_dropout gave before they became templates."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens as T
from tests import helpers as H
from tests import helpers_uniformer as U
from tests.helpers import bits_kept, bound_8x, canary_ok, canary_out, chan_affine, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 1e-5


def _dev(t):
    return t.contiguous().to(DEV)


def _check(name, got, ref64, t32):
    got = got.cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(got).all()), name
    err, bound = float((got - ref64.double()).abs().max()), bound_8x(ref64, t32.reshape(ref64.shape))
    print(f"  {name:<44s} max|err| {err:9.3e}  bound {bound:9.3e}  ratio {err / bound if bound else 0.0:6.3f}")
    assert err <= bound, (name, err, bound)


def _within(name, buf, ref64, t32):
    n = ref64.numel()
    written, tail = canary_ok(buf, n)
    assert written, f"{name}: elements of the output were never written"
    assert tail, f"{name}: the launch wrote past the end of the output"
    _check(name, buf[:n], ref64, t32)


def _bn32(x, gamma, beta, dy):
    """torch's float32 CPU BatchNorm (the ATen op: F.batch_norm refuses one row) -> (y, dx, dgamma, dbeta)."""
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.batch_norm(xr, gr, br, None, None, True, 0.0, EPS, False)
    y.backward(dy)
    return y.detach(), xr.grad, gr.grad, br.grad


def _run(R, C_, seed, x=None):
    lib, st = L.load(), stream(DEV)
    tag = f"R{R} C{C_}"
    gen = torch.Generator().manual_seed(seed)
    x = chan_affine((R, C_), 0, gen) if x is None else x
    gamma = chan_affine((C_,), 0, gen).abs().clamp_min(0.25) * torch.where(torch.rand(C_, generator=gen) < 0.5, -1.0, 1.0)
    beta, dy = chan_affine((C_,), 0, gen), chan_affine((R, C_), 0, gen)
    xd, dyd, gd, bd = _dev(x), _dev(dy), _dev(gamma), _dev(beta)
    nblk = lib.hpfg_tok_stat_blocks(R)
    # the statistics
    part, sums = canary_out(nblk * 2 * C_), canary_out(2 * C_)
    L.check(lib.hpfg_bn_tok_stats(L.ptr(xd), R, C_, L.ptr(part), L.ptr(sums), st), "bn_tok_stats")
    torch.cuda.synchronize()
    assert all(canary_ok(part, nblk * 2 * C_)), f"{tag}: statistics partials"
    s64, m64 = H.col_stats_f64(x)
    _within(f"{tag} sum x, centred squares", sums, torch.stack([s64, m64]), torch.stack([x.sum(0), ((x - x.mean(0)) ** 2).sum(0)]))
    # apply and backward on the float64 statistics rounded to the float32 the kernels take
    mean64, _, rstd64 = U.batch_stats_f64(x, EPS)
    mean, rstd = mean64.float(), rstd64.float()
    y32, dx32, dg32, db32 = _bn32(x, gamma, beta, dy)
    y, dx, part2, sums2 = canary_out(R * C_), canary_out(R * C_), canary_out(nblk * 2 * C_), canary_out(2 * C_)
    md, rd = _dev(mean), _dev(rstd)
    L.check(lib.hpfg_bn_tok_apply(L.ptr(xd), L.ptr(md), L.ptr(rd), L.ptr(gd), L.ptr(bd), L.ptr(y), R, C_, st), "bn_tok_apply")
    L.check(lib.hpfg_bn_tok_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(md), L.ptr(rd), L.ptr(gd), L.ptr(dx), L.ptr(part2), L.ptr(sums2), R, C_, st), "bn_tok_bwd")
    torch.cuda.synchronize()
    assert all(canary_ok(part2, nblk * 2 * C_)), f"{tag}: backward partials"
    dx64, dbeta64, dgamma64 = U.bn_tok_bwd_f64(x, dy, mean, rstd, gamma)
    _within(f"{tag} y", y, U.bn_tok_f64(x, mean, rstd, gamma, beta), y32)
    _within(f"{tag} dx", dx, dx64, dx32)
    _within(f"{tag} dbeta, dgamma", sums2, torch.stack([dbeta64, dgamma64]), torch.stack([db32, dg32]))


@pytest.mark.parametrize("C_", [4, 64, 320, 260])
@pytest.mark.parametrize("R", [1, 2, 49, 3136 * 2])
def test_bn_tokens_entry_points(R, C_):
    _run(R, C_, 13 * R + C_)


def test_bn_tokens_constant_column_is_finite():
    """A constant column: variance 0, rstd = 1 / sqrt(eps), y = beta there; every output finite and in bound."""
    R, C_ = 49, 64
    x = chan_affine((R, C_), 3)
    x[:, 5] = 2.75
    _run(R, C_, 4, x=x)
    g, b = _dev(chan_affine((C_,), 5)), _dev(chan_affine((C_,), 6))
    y, mean, var = T.batch_norm_tokens(_dev(x), g, b, EPS)
    assert float(var[5]) == 0.0 and float(mean[5]) == 2.75 and bool((y[:, 5] == b[5]).all()) and bool(torch.isfinite(y).all())


def test_bn_tokens_mean_32_std_1():
    """x = 32 + randn, the case col_stats_kernel was written for: the variance keeps its digits (no E[x^2] - mean^2)."""
    R, C_ = 3136 * 2, 64
    gen = torch.Generator().manual_seed(8)
    x = (32.0 + torch.randn(R, C_, generator=gen)).float()
    gamma, beta, dy = chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen), chan_affine((R, C_), 0, gen)
    xd, gd, bd = (_dev(t).requires_grad_(True) for t in (x, gamma, beta))
    y, mean, var = T.batch_norm_tokens(xd.reshape(2, 56, 56, C_), gd, bd, EPS)
    y.backward(_dev(dy).reshape(2, 56, 56, C_))
    mean64, var64, rstd64 = U.batch_stats_f64(x, EPS)
    y32, dx32, dg32, db32 = _bn32(x, gamma, beta, dy)
    _check("mean-32 mean", mean, mean64, x.mean(0))
    _check("mean-32 var", var, var64, x.var(0, unbiased=False))
    dx64, dbeta64, dgamma64 = U.bn_tok_bwd_f64(x, dy, mean64, rstd64, gamma)
    _check("mean-32 y", y.detach().reshape(R, C_), U.bn_tok_f64(x, mean64, rstd64, gamma, beta), y32)
    _check("mean-32 dx", xd.grad, dx64, dx32)
    _check("mean-32 dgamma", gd.grad, dgamma64, dg32)
    _check("mean-32 dbeta", bd.grad, dbeta64, db32)


def test_bn_tokens_statistics_match_tok_col_stats_bitwise_where_both_admit():
    lib, st = L.load(), stream(DEV)
    R, C_ = 4097, 64
    xd = _dev(chan_affine((R, C_), 9))
    nblk = lib.hpfg_tok_stat_blocks(R)
    out = []
    for fn in (lib.hpfg_tok_col_stats, lib.hpfg_bn_tok_stats):
        part, sums = canary_out(nblk * 2 * C_), canary_out(2 * C_)
        L.check(fn(L.ptr(xd), R, C_, L.ptr(part), L.ptr(sums), st), "stats")
        out.append(sums)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


@pytest.mark.parametrize("R,C_", [(4, 6), (4, 1028), (0, 8), (4, 0)], ids=["C6", "C1028", "R0", "C0"])
def test_bn_tokens_refused_arguments_launch_nothing(R, C_):
    lib, st = L.load(), stream(DEV)
    src = torch.ones(8192, device=DEV)
    p = L.ptr(src)
    a, b, c = canary_out(4096), canary_out(4096), canary_out(4096)
    assert lib.hpfg_bn_tok_stats(p, R, C_, L.ptr(a), L.ptr(b), st) == -1 and b"bn_tok_stats" in lib.hpfg_last_error()
    assert lib.hpfg_bn_tok_apply(p, p, p, p, p, L.ptr(c), R, C_, st) == -1 and b"bn_tok_apply" in lib.hpfg_last_error()
    assert lib.hpfg_bn_tok_bwd(p, p, p, p, p, L.ptr(c), L.ptr(a), L.ptr(b), R, C_, st) == -1 and b"bn_tok_bwd" in lib.hpfg_last_error()
    torch.cuda.synchronize()
    assert bits_kept(a, 0) and bits_kept(b, 0) and bits_kept(c, 0)


def test_batch_norm_tokens_argument_checks_raise_value_error():
    g = torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="multiple of 4"):
        T.batch_norm_tokens(torch.zeros(4, 6, device=DEV), g[:6], g[:6], EPS)
    with pytest.raises(ValueError, match="gamma and beta"):
        T.batch_norm_tokens(torch.zeros(4, 8, device=DEV), g[:4], g, EPS)
    with pytest.raises(ValueError, match="eps"):
        T.batch_norm_tokens(torch.zeros(4, 8, device=DEV), g, g, 0.0)


def test_batch_norm_tokens_eval_is_the_affine_map_of_the_running_statistics():
    """Eval mode, with and without a gradient: y, dx = dy gamma rstd, dgamma = sum dy xhat, dbeta = sum dy against torch's eval-mode BatchNorm."""
    R, C_ = 98, 320
    gen = torch.Generator().manual_seed(12)
    x, gamma, beta, rm = chan_affine((R, C_), 0, gen), chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen)
    rv, dy = chan_affine((C_,), 0, gen).abs() + 0.1, chan_affine((R, C_), 0, gen)
    with torch.no_grad():
        y0 = T.batch_norm_tokens_eval(_dev(x), _dev(gamma), _dev(beta), _dev(rm), _dev(rv), EPS)
    xd, gd, bd = (_dev(t).requires_grad_(True) for t in (x, gamma, beta))
    y = T.batch_norm_tokens_eval(xd, gd, bd, _dev(rm), _dev(rv), EPS)
    y.backward(_dev(dy))
    assert torch.equal(y.detach(), y0)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y32 = F.batch_norm(xr, rm, rv, gr, br, False, 0.0, EPS)
    y32.backward(dy)
    rstd = 1.0 / torch.sqrt(rv.double() + EPS)
    xh = (x.double() - rm.double()) * rstd
    _check("eval y", y0, xh * gamma.double() + beta.double(), y32.detach())
    _check("eval dx", xd.grad, dy.double() * gamma.double() * rstd, xr.grad)
    _check("eval dgamma", gd.grad, (dy.double() * xh).sum(0), gr.grad)
    _check("eval dbeta", bd.grad, dy.double().sum(0), br.grad)


# ---- the BatchNorm + ReLU + dropout head keeps its bits --------------------------------------------------------------------------------------
def bnrelu_fixed_digests(bn_relu_dropout):
    """sha256 of (y, mean, var, dx, dgamma, dbeta) of bn_relu_dropout on one fixed input [2, 49, 64] with a channel mask, keep 0.9."""
    gen = torch.Generator().manual_seed(20260)
    B, N, C_ = 2, 49, 64
    x, dy = chan_affine((B, N, C_), 0, gen), chan_affine((B, N, C_), 0, gen)
    gamma, beta = chan_affine((C_,), 0, gen), 0.5 * chan_affine((C_,), 0, gen)
    mask = torch.empty(B, C_).bernoulli_(0.9, generator=gen)
    xd, gd, bd = (_dev(t).requires_grad_(True) for t in (x, gamma, beta))
    y, mean, var = bn_relu_dropout(xd, gd, bd, _dev(mask), 0.9, EPS)
    y.backward(_dev(dy))
    torch.cuda.synchronize()
    return {k: hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()[:16]
            for k, t in (("y", y), ("mean", mean), ("var", var), ("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad))}


# recorded on the MI355X from the library built at the parent commit (hpfg_bnrelu_* before the RELU template parameter)
BNRELU_PARENT_DIGESTS = {"y": "abea02bb93c0cdbe", "mean": "255fdaf88a1c3eb5", "var": "4ebf2ee966d2e801", "dx": "6ebcb0acc11aa003",
                         "dgamma": "e30e3e93201642f4", "dbeta": "840daf14ace8badd"}


def test_bn_relu_dropout_keeps_the_bits_of_the_parent_commit():
    assert bnrelu_fixed_digests(T.bn_relu_dropout) == BNRELU_PARENT_DIGESTS
