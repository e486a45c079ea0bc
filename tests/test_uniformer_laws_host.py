"""CPU: the float64 laws of tests/helpers_uniformer.py against torch's own float64 ops and autograd (the laws are what the GPU tests of
csrc/dwconv.hip and hpfg_bn_tok_* measure against, so they are pinned here first)."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers_uniformer as U
from tests.helpers import chan_affine

TOL = 1e-11


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("res", ["none", "x", "other"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 3, 3, 8), (2, 5, 9, 4), (1, 17, 6, 12)])
def test_dwconv_law_is_torch_depthwise_conv2d(k, res, shape):
    B, H, W, C_ = shape
    gen = torch.Generator().manual_seed(100 * k + H)
    x, dy = chan_affine(shape, 0, gen).double(), chan_affine(shape, 0, gen).double()
    wk, bias, other = chan_affine((k * k, C_), 0, gen).double(), chan_affine((C_,), 0, gen).double(), chan_affine(shape, 0, gen).double()
    xr, br = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    wr = wk.t().reshape(C_, 1, k, k).contiguous().requires_grad_(True)
    y = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=k // 2, groups=C_).permute(0, 2, 3, 1)
    if res == "x":
        y = y + xr
    elif res == "other":
        y = y + other
    y.backward(dy)
    law = U.dwconv_k_f64(x, wk, bias, k, {"none": None, "x": x, "other": other}[res])
    dx, dwk, db = U.dwconv_k_bwd_f64(x, wk, dy, k, add_dy=res == "x")
    assert float((law - y.detach()).abs().max()) < TOL * float(y.detach().abs().max())
    assert float((dx - xr.grad).abs().max()) < TOL * float(xr.grad.abs().max())
    assert float((dwk - wr.grad.reshape(C_, k * k).t()).abs().max()) < TOL * float(wr.grad.abs().max())
    assert float((db - br.grad).abs().max()) < TOL * float(br.grad.abs().max())


def test_dwconv_law_3x3_is_the_segformer_branch_law():
    from tests import helpers as H
    gen = torch.Generator().manual_seed(3)
    x, w9, bias = chan_affine((2, 5, 7, 8), 0, gen), chan_affine((9, 8), 0, gen), chan_affine((8,), 0, gen)
    assert torch.equal(U.dwconv_k_f64(x, w9, bias, 3), H.dwconv_f64(x, w9, bias))


@pytest.mark.parametrize("R,C_", [(2, 4), (49, 8), (301, 12)])
def test_batch_norm_law_is_torch_batch_norm(R, C_):
    gen = torch.Generator().manual_seed(R)
    x, dy = chan_affine((R, C_), 0, gen).double(), chan_affine((R, C_), 0, gen).double()
    gamma, beta = chan_affine((C_,), 0, gen).double(), chan_affine((C_,), 0, gen).double()
    eps = 1e-5
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.batch_norm(xr, None, None, gr, br, True, 0.0, eps)
    y.backward(dy)
    mean, var, rstd = U.batch_stats_f64(x, eps)
    assert float((var - x.var(0, unbiased=False)).abs().max()) < TOL * float(var.max())
    law = U.bn_tok_f64(x, mean, rstd, gamma, beta)
    dx, dbeta, dgamma = U.bn_tok_bwd_f64(x, dy, mean, rstd, gamma)
    assert float((law - y.detach()).abs().max()) < TOL * float(y.detach().abs().max())
    assert float((dx - xr.grad).abs().max()) < 1e-9 * float(xr.grad.abs().max())
    assert float((dgamma - gr.grad).abs().max()) < TOL * float(gr.grad.abs().max())
    assert float((dbeta - br.grad).abs().max()) < TOL * float(br.grad.abs().max())
