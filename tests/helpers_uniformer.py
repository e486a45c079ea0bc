"""float64 laws of the kernels the UniFormer branch adds (csrc/dwconv.hip, hpfg_bn_tok_* of csrc/tokens.hip; reference model/uniformer.py): plain
restatements of the operations' definitions on torch double tensors, NHWC / [rows, C] like the kernels' buffers.
tests/test_uniformer_laws_host.py holds each against torch's own float64 op and autograd."""
import torch


def shift_k(t, dy_, dx_):
    """t[b, y + dy_, x + dx_, c] with zeros outside the map, NHWC, any shift."""
    B, H, W, C_ = t.shape
    p = max(abs(dy_), abs(dx_))
    big = torch.zeros(B, H + 2 * p, W + 2 * p, C_, dtype=t.dtype)
    big[:, p:p + H, p:p + W] = t
    return big[:, p + dy_:p + dy_ + H, p + dx_:p + dx_ + W]


def taps(k):
    """(t, dy, dx) of the k x k taps in the order of the [k*k][C] weight: t = k (dy + k // 2) + dx + k // 2."""
    return [(i * k + j, i - k // 2, j - k // 2) for i in range(k) for j in range(k)]


def dwconv_k_f64(x, wk, bias, k, res=None):
    """(res or 0) + depthwise k x k cross-correlation (padding k // 2) + bias; x [B,H,W,C], wk [k*k][C]."""
    x, wk = x.double(), wk.double()
    y = bias.double().expand_as(x).clone()
    for t, dy_, dx_ in taps(k):
        y += wk[t] * shift_k(x, dy_, dx_)
    return y if res is None else y + res.double()


def dwconv_k_bwd_f64(x, wk, dy, k, add_dy=False):
    """-> (dx, dwk [k*k][C], dbias) of dwconv_k_f64; add_dy: dx of x + dwconv(x)."""
    x, wk, dy = x.double(), wk.double(), dy.double()
    dx = dy.clone() if add_dy else torch.zeros_like(x)
    dwk = torch.zeros_like(wk)
    for t, dy_, dx_ in taps(k):
        dx += wk[t] * shift_k(dy, -dy_, -dx_)
        dwk[t] = (dy * shift_k(x, dy_, dx_)).sum((0, 1, 2))
    return dx, dwk, dy.sum((0, 1, 2))


def bn_tok_f64(x, mean, rstd, gamma, beta):
    """(x - mean) rstd gamma + beta on x [R, C]."""
    return (x.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()


def bn_tok_bwd_f64(x, dy, mean, rstd, gamma):
    """-> (dx, sum dy (= dbeta), sum dy xhat (= dgamma)): train-mode BatchNorm's input gradient when mean / rstd are the batch's own."""
    x, dy = x.double(), dy.double()
    R = x.shape[0]
    xh = (x - mean.double()) * rstd.double()
    s1, s2 = dy.sum(0), (dy * xh).sum(0)
    return gamma.double() * rstd.double() * (dy - s1 / R - xh * s2 / R), s1, s2


def batch_stats_f64(x, eps):
    """x [R, C] -> (mean, biased variance, rstd) in float64."""
    x = x.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps)
