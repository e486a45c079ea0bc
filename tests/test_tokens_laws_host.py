"""CPU: the float64 laws of tests/helpers.py that tests/test_gpu_tokens_edges.py holds the token-layout kernels against, each against
torch's own float64 op and autograd at two small shapes -- so that the laws can be checked on a machine without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import helpers as H

TOL = 1e-11          # float64 laws against float64 torch: a few hundred roundings of O(10) values at the most


def _close(a, b, what):
    err = float((a.double() - b.double()).abs().max())
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("rows,C_", [((3,), 36), ((2, 5), 8)])
def test_layer_norm_law(rows, C_):
    x = H.chan_affine((*rows, C_), 1).double().requires_grad_(True)
    g, b = (H.chan_affine((C_,), s).double().requires_grad_(True) for s in (2, 3))
    dy = H.chan_affine((*rows, C_), 4).double()
    y = F.layer_norm(x, (C_,), g, b)
    y.backward(dy)
    y64, mean, rstd = H.ln_f64(x.detach(), g.detach(), b.detach())
    _close(y64, y.detach(), "y")
    _close(mean, x.detach().mean(-1), "mean")
    _close(rstd, 1.0 / torch.sqrt(x.detach().var(-1, unbiased=False) + 1e-5), "rstd")
    dx, dg, db = H.ln_bwd_f64(x.detach(), dy, g.detach())
    _close(dx, x.grad, "dx"), _close(dg, g.grad, "dgamma"), _close(db, b.grad, "dbeta")


@pytest.mark.parametrize("B,Hh,W,C_", [(2, 1, 4, 4), (1, 5, 3, 8)])
def test_depthwise_gelu_law(B, Hh, W, C_):
    x = H.chan_affine((B, Hh, W, C_), 5).double().requires_grad_(True)
    w = (0.3 * H.chan_affine((3, 3, C_), 6).double()).permute(2, 0, 1).reshape(C_, 1, 3, 3).contiguous().requires_grad_(True)
    b = H.chan_affine((C_,), 7).double().requires_grad_(True)
    dy = H.chan_affine((B, Hh, W, C_), 8).double()
    u = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1, groups=C_).permute(0, 2, 3, 1)
    y = F.gelu(u)
    y.backward(dy)
    w9 = w.detach().reshape(C_, 9).t()
    _close(H.dwconv_f64(x.detach(), w9, b.detach()), u.detach(), "u")
    _close(H.gelu_f64(u.detach()), y.detach(), "y")
    du, dx, dw9, db = H.dwgelu_bwd_f64(x.detach(), w9, b.detach(), dy)
    _close(dx, x.grad, "dx"), _close(dw9, w.grad.reshape(C_, 9).t(), "dw9"), _close(db, b.grad, "dbias")
    ur = u.detach().clone().requires_grad_(True)
    F.gelu(ur).backward(dy)
    _close(du, ur.grad, "du")


@pytest.mark.parametrize("h,w,Hh,W", [(3, 5, 7, 12), (1, 6, 4, 6)])
def test_bilinear_resize_law(h, w, Hh, W):
    x = H.chan_affine((2, h, w, 4), 9).double().requires_grad_(True)
    dy = H.chan_affine((2, Hh, W, 4), 10).double()
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(Hh, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    y.backward(dy)
    _close(H.resize_f64(x.detach(), Hh, W), y.detach(), "y")
    _close(H.resize_bwd_f64(dy, h, w), x.grad, "dx")


@pytest.mark.parametrize("B,N,C_,masked", [(2, 3, 4, False), (3, 7, 8, True)])
def test_token_batchnorm_relu_dropout_law(B, N, C_, masked):
    R = B * N
    x = H.chan_affine((R, C_), 11).double().requires_grad_(True)
    g, b = (H.chan_affine((C_,), s).double().requires_grad_(True) for s in (12, 13))
    dy = H.chan_affine((R, C_), 14).double()
    mask = torch.empty(B, C_).bernoulli_(0.6, generator=torch.Generator().manual_seed(15)).double() if masked else None
    inv_keep = 1.0 / 0.5          # (exact in float32)
    rm, rv = torch.zeros(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64)
    y = torch.relu(F.batch_norm(x, rm, rv, g, b, training=True, momentum=1.0, eps=1e-5))
    if masked:
        y = y * mask[torch.arange(R) // N] * inv_keep
    y.backward(dy)
    s, m2 = H.col_stats_f64(x.detach())
    mean, var = s / R, m2 / R
    _close(mean, rm, "mean"), _close(var * R / (R - 1), rv, "var")
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    y64, pre = H.bnrelu_f64(x.detach(), mean, rstd, g.detach(), b.detach(), mask, inv_keep if masked else 1.0, N)
    assert float(pre.abs().min()) > 1e-6          # (no pre-activation on the ReLU's kink: autograd and the law agree on the gate)
    _close(y64, y.detach(), "y")
    dx, s1, s2 = H.bnrelu_bwd_f64(x.detach(), dy, mean, rstd, g.detach(), b.detach(), mask, inv_keep if masked else 1.0, N)
    _close(dx, x.grad, "dx"), _close(s1, b.grad, "dbeta"), _close(s2, g.grad, "dgamma")


@pytest.mark.parametrize("B,Hh,W,C_,k,s", [(2, 9, 7, 3, 3, 2), (1, 5, 5, 4, 2, 2)])
def test_patches_law_is_the_conv(B, Hh, W, C_, k, s):
    """patches_f64 (F.unfold reordered to (u, v, c)) times the weights in that order is F.conv2d; col2im_f64 (F.fold) is its transpose."""
    x = H.chan_affine((B, Hh, W, C_), 16).double().requires_grad_(True)
    w = H.chan_affine((5, C_, k, k), 17).double()
    y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=s, padding=k // 2)
    dy = H.chan_affine(tuple(y.shape), 18).double()
    y.backward(dy)
    cols = H.patches_f64(x.detach(), k, s)
    wm = w.permute(0, 2, 3, 1).reshape(5, -1)
    _close(cols @ wm.t(), y.detach().flatten(2).transpose(1, 2), "conv")
    dcols = dy.flatten(2).transpose(1, 2) @ wm
    _close(H.col2im_f64(dcols, Hh, W, C_, k, s), x.grad, "dx")


def test_patch_merge_and_gelu_laws():
    x = H.chan_affine((3, 4, 6, 4), 19)
    y = H.patch_merge_ref(x)
    assert tuple(y.shape) == (3, 2, 3, 16)
    for k_, (di, dj) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
        assert torch.equal(y[:, 1, 2, 4 * k_:4 * k_ + 4], x[:, 2 + di, 4 + dj])
    u = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0, 40.0, -40.0], dtype=torch.float64, requires_grad=True)
    F.gelu(u).sum().backward()
    _close(H.gelu_f64(u.detach()), F.gelu(u.detach()), "gelu")
    _close(H.gelu_grad_f64(u.detach()), u.grad, "gelu'")


def test_bound_rule_has_a_floor():
    ref = torch.tensor([1.0, -3.0], dtype=torch.float64)
    assert H.bound_8x(ref, ref.float()) == 4 * 2.0 ** -22          # exactly representable: 4 ulp of 3.0
    assert H.bound_8x(ref, ref.float() + 1e-3) == pytest.approx(8e-3, rel=1e-3)
