"""The Swin blocks of the reference's Swin-UNet (model/swinunet.py:52-82 PatchMerging, :114-133 Mlp, :136-248 WindowAttention, :251-278
SwinTransformerBlock, :281-330 BasicBlock) on the HIP token kernels.

Same constructor signatures, construction order, parameter and buffer names (``attn.relative_position_index`` included) as the reference, so
``state_dict()`` interchanges and a seed gives the same initial weights.  Tokens stay an NHWC map [B, H, W, C] throughout, as in the
reference.  Where the work runs, forward and backward, all through ``hpfg_amd.ops_tokens``:

* ``window_attention`` (``csrc/attn_window.hip``): the attention inside w x w windows with the relative-position bias, the cyclic shift and
  the shifted-window mask.  The reference's roll / window partition / window reverse / roll back are the kernel's addressing -- no copy of
  qkv or of the output is made -- and because the proj Linear acts per token it commutes with window reverse and the roll back, so it is
  applied to the un-partitioned map;
* ``layer_norm``, ``linear`` (qkv, proj, fc1, fc2, reduction), ``gelu``, ``residual_scale`` (the residual add with its drop-path factor),
  ``patch_merge`` (the 2 x 2 gather of PatchMerging and its scatter backward).

Stochastic depth draws from the torch device generator; ``external_draws`` replays given draws (parity tests): a pair of [B] tensors
(attention branch, MLP branch) on a block, a list of such pairs on a BasicBlock.  Dropout inside the blocks is refused: the reference
never sets ``drop`` / ``attn_drop`` above zero.  The encoder / decoder assembly is not built here and ``build_model`` still refuses "swinunet".
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops_tokens import gelu, layer_norm, linear, patch_merge, residual_scale, window_attention


def _no_dropout(who: str, **rates) -> None:
    for name, rate in rates.items():
        if rate != 0.0:
            raise ValueError(f"{who}: {name} = {rate} is not built (the HIP Swin blocks have no dropout inside; the reference leaves it at 0)")


def _only(who: str, what: str, got, want) -> None:
    if got is not want:
        raise ValueError(f"{who}: {what} must be {want.__name__} (the HIP kernels implement nothing else), got {got!r}")


class PatchMerging(nn.Module):
    def __init__(self, dim: int, norm_layer=nn.LayerNorm):
        super().__init__()
        _only("PatchMerging", "norm_layer", norm_layer, nn.LayerNorm)
        self.dim = dim
        self.norm = norm_layer(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        x = patch_merge(x)
        x = layer_norm(x, self.norm.weight, self.norm.bias)
        return linear(x, self.reduction.weight)


class Mlp(nn.Module):
    def __init__(self, in_features: int, hidden_features: int = None, out_features: int = None, act_layer=nn.GELU, drop: float = 0.):
        super().__init__()
        _only("Mlp", "act_layer", act_layer, nn.GELU)
        _no_dropout("Mlp", drop=drop)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return linear(gelu(linear(x, self.fc1.weight, self.fc1.bias)), self.fc2.weight, self.fc2.bias)


class WindowAttention(nn.Module):
    def __init__(self, dim: int, window_size: int, num_heads: int, qkv_bias: bool = True, attn_drop: float = 0., proj_drop: float = 0.,
                 shift: bool = False):
        super().__init__()
        _no_dropout("WindowAttention", attn_drop=attn_drop, proj_drop=proj_drop)
        self.window_size = window_size
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.shift_size = window_size // 2 if shift else 0
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        # the index the kernel computes from the positions, kept as the buffer the reference's state_dict carries
        ij = torch.arange(window_size)
        coords = torch.stack(torch.meshgrid(ij, ij, indexing="ij")).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
        rel += window_size - 1
        rel[:, :, 0] *= 2 * window_size - 1
        self.register_buffer("relative_position_index", rel.sum(-1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        qkv = linear(x, self.qkv.weight, self.qkv.bias)
        a = window_attention(qkv, self.relative_position_bias_table, self.num_heads, self.window_size, self.shift_size, self.scale)
        return linear(a, self.proj.weight, self.proj.bias)


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift=False, mlp_ratio=4., qkv_bias=True, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        _only("SwinTransformerBlock", "norm_layer", norm_layer, nn.LayerNorm)
        _no_dropout("SwinTransformerBlock", drop=drop, attn_drop=attn_drop)
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=window_size, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, shift=shift)
        self.dpr = float(drop_path)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.external_draws = None        # (attention-branch draw, MLP-branch draw), each [B]: replay given uniform draws (tests)

    def _keep_scale(self, batch, draw, device):
        """Per-sample factor of a residual branch (DropPath, swinunet.py:9-24): floor(keep + U) / keep, or None when nothing is dropped."""
        if self.dpr == 0.0 or not self.training:
            return None
        kp = 1.0 - self.dpr
        r = torch.rand((batch,), dtype=torch.float32, device=device) if draw is None else draw.to(device).reshape(batch).float()
        return (kp + r).floor() / kp

    def forward(self, x, draws=None):
        if not x.is_cuda:
            raise RuntimeError("hpfg_amd.SwinTransformerBlock runs on the GPU only: its LayerNorm / window-attention / GELU kernels have no CPU fallback")
        d = draws if draws is not None else (self.external_draws if self.external_draws is not None else (None, None))
        B = x.shape[0]
        a = self.attn(layer_norm(x, self.norm1.weight, self.norm1.bias))
        x = residual_scale(x, a, self._keep_scale(B, d[0], x.device))
        m = self.mlp(layer_norm(x, self.norm2.weight, self.norm2.bias))
        return residual_scale(x, m, self._keep_scale(B, d[1], x.device))


class BasicBlock(nn.Module):
    def __init__(self, index: int, embed_dim: int = 96, window_size: int = 7, depths: tuple = (2, 2, 6, 2), num_heads: tuple = (3, 6, 12, 24),
                 mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0., attn_drop_rate: float = 0., drop_path: float = 0.1,
                 norm_layer=nn.LayerNorm, patch_merging: bool = True):
        super().__init__()
        depth = depths[index]
        dim = embed_dim * 2 ** index
        dpr = [rate.item() for rate in torch.linspace(0, drop_path, sum(depths))]
        rates = dpr[sum(depths[:index]):sum(depths[:index + 1])]
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads[index], window_size=window_size, shift=i % 2 == 1, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                 drop=drop_rate, attn_drop=attn_drop_rate, drop_path=rates[i], norm_layer=norm_layer)
            for i in range(depth)])
        self.downsample = PatchMerging(dim=dim, norm_layer=norm_layer) if patch_merging else None
        self.external_draws = None        # one (attention, MLP) pair of [B] draws per block

    def forward(self, x):
        for i, layer in enumerate(self.blocks):
            x = layer(x, None if self.external_draws is None else self.external_draws[i])
        if self.downsample is not None:
            x = self.downsample(x)
        return x
