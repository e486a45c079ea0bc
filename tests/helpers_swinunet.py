"""Shared pieces of the Swin-UNet tests: float64 laws of the kernels this network added (LayerNorm with eps through the pixel shuffle of
the patch expanding, window attention with dropout of the probabilities) and small host helpers.  Plain restatements of the definitions on
torch double tensors, like the laws in tests/helpers.py."""
import numpy as np
import torch

from tests import helpers as H


def px_shuffle(t, P):
    """rearrange(t, 'B H W (P1 P2 C) -> B (H P1) (W P2) C') (reference model/swinunet.py:96,109): pure data movement, any dtype."""
    B, Hh, W, PPC = t.shape
    C_ = PPC // (P * P)
    return t.reshape(B, Hh, W, P, P, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, Hh * P, W * P, C_)


def px_unshuffle(t, P):
    """The inverse of px_shuffle: [B, H P, W P, C] -> [B, H, W, P P C]."""
    B, HP, WP, C_ = t.shape
    Hh, W = HP // P, WP // P
    return t.reshape(B, Hh, P, W, P, C_).permute(0, 1, 3, 2, 4, 5).reshape(B, Hh, W, P * P * C_)


def ln_px_f64(x, g, b, P, eps):
    """x [B,H,W,P*P*C] -> (y [B,HP,WP,C], mean, rstd [B*H*W*P*P]): LayerNorm(C, eps) of every row of the [B H W P^2, C] matrix, shuffled."""
    B, Hh, W, PPC = x.shape
    C_ = PPC // (P * P)
    y, mean, rstd = H.ln_f64(x.reshape(B, Hh, W, P * P, C_), g, b, eps)
    return px_shuffle(y.reshape(B, Hh, W, PPC), P), mean.reshape(-1), rstd.reshape(-1)


def ln_px_bwd_f64(x, dy, g, P, eps):
    """dy [B,HP,WP,C] -> (dx like x, dgamma, dbeta)."""
    B, Hh, W, PPC = x.shape
    C_ = PPC // (P * P)
    dx, dg, db = H.ln_bwd_f64(x.reshape(-1, C_), px_unshuffle(dy, P).reshape(-1, C_), g, eps)
    return dx.reshape(x.shape), dg, db


def inv_keep32(p):
    """1 / (1 - p) as the kernels form it: in float32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def window_partition_index(Hh, W, w, s):
    """tok [nW, L]: the token (y W + x) at position l of window n of the map rolled by -s (reference model/swinunet.py:27-49 with the roll of
    :262): position (i, j) of window (wy, wx) is the rolled coordinate (wy w + i, wx w + j), i.e. the token ((y' + s) % H, (x' + s) % W)."""
    ys = (torch.arange(Hh) + s) % Hh
    xs = (torch.arange(W) + s) % W
    tok = ys[:, None] * W + xs[None, :]
    return tok.reshape(Hh // w, w, W // w, w).permute(0, 2, 1, 3).reshape(-1, w * w)
