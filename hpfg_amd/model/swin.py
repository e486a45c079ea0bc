"""The Swin blocks of the reference's Swin-UNet (model/swinunet.py:52-82 PatchMerging, :114-133 Mlp, :136-248 WindowAttention, :251-278
SwinTransformerBlock, :281-330 BasicBlock) on the HIP token kernels.

Same constructor signatures, construction order, parameter and buffer names (``attn.relative_position_index`` included) as the reference, so
``state_dict()`` interchanges and a seed gives the same initial weights.  Tokens stay an NHWC map [B, H, W, C] throughout, as in the
reference.  Where the work runs, forward and backward, all through ``hpfg_amd.ops_tokens``:

* ``window_attention`` (``csrc/attn_window.hip``): the attention inside w x w windows with the relative-position bias, the cyclic shift and
  the shifted-window mask.  The reference's roll / window partition / window reverse / roll back are the kernel's addressing -- no copy of
  qkv or of the output is made -- and because the proj Linear acts per token it commutes with window reverse and the roll back, so it is
  applied to the un-partitioned map;
* ``window_attention_packed`` (``csrc/attn_window_packed.hip``) instead, where a module is built with the keyword-only ``packed=True``
  (windows 2 .. 4 only): 64 // w^2 windows share one 64-row tile.  Same bias, mask and dropout elements; the LIDC factory of
  ``model/swinunet.py`` sets it per stage from measurements, everything else leaves the default ``False`` and runs the kernels it ran before;
* ``layer_norm``, ``linear`` (qkv, proj, fc1, fc2, reduction), ``gelu``, ``residual_scale`` (the residual add with its drop-path factor),
  ``patch_merge`` (the 2 x 2 gather of PatchMerging and its scatter backward).

Stochastic depth draws from the torch device generator; ``external_draws`` replays given draws (parity tests): a pair of [B] tensors
(attention branch, MLP branch) on a block, a list of such pairs on a BasicBlock.

Dropout.  The reference's networks (``get_swinunet``, ``get_swinunet_plus``, ``get_swinunet_LIDC``) run the blocks with ``drop_rate = 0.1`` and
``attn_drop_rate = 0.1``.  The constructors here still refuse non-zero rates unless the keyword-only ``allow_dropout=True`` is passed, which the
encoder / decoder of ``model/swinunet.py`` do: ``attn_drop`` then runs inside the window-attention kernels (``window_attention_dropout``),
``proj_drop`` / ``Mlp.drop1`` / ``Mlp.drop2`` as ``token_dropout``.  Every site has a constant layer seed (``drop_seeds``, numbered by a
block, a stage and a network in turn, so that no two sites under one module share one) and draws keep(e) = hash(e, layer seed + seed word);
the forward's own copy of the network's seed word and, for tests, explicit masks come in as a ``DropState``.  A block or stage used on its
own has no seed word: its sites differ from each other, but every forward repeats the same masks -- the word, its advance and the
per-instance base seed belong to the networks of ``model/swinunet.py``.  Eval mode launches no dropout.  ``build_model`` opens
"swinunet_plus" and "swinunet_lidc" and still refuses "swinunet".
"""
from __future__ import annotations

import functools

import torch
import torch.nn as nn

from ..ops_tokens import (MAX_PACKED_WINDOW, gelu, layer_norm, linear, patch_merge, residual_scale, token_dropout, window_attention,
                          window_attention_dropout, window_attention_packed)


def _no_dropout(who: str, allow: bool = False, **rates) -> None:
    for name, rate in rates.items():
        if rate != 0.0 and not allow:
            raise ValueError(f"{who}: {name} = {rate} is not built without allow_dropout=True (the Swin-UNet assembly passes it; see model/swin.py)")
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"{who}: {name} = {rate} must be in [0, 1)")


def _only(who: str, what: str, got, want) -> None:
    """``want`` itself, or -- for nn.LayerNorm -- functools.partial(nn.LayerNorm, eps=...) as the reference's networks build their norms."""
    if want is nn.LayerNorm and isinstance(got, functools.partial) and got.func is nn.LayerNorm and not got.args and set(got.keywords) <= {"eps"}:
        return
    if got is not want:
        raise ValueError(f"{who}: {what} must be {want.__name__} (the HIP kernels implement nothing else), got {got!r}")


def norm(x, ln: nn.LayerNorm):
    """``ln(x)`` on the HIP LayerNorm with the module's own eps."""
    return layer_norm(x, ln.weight, ln.bias, ln.eps)


def site_seed(k: int, base: int = 0) -> int:
    """Layer seed of dropout site k of the network instance with base seed ``base``: a 32-bit mix of both, so that the hash streams of the
    sites, and of the same site in two networks, are unrelated."""
    h = (k * 0x9E3779B1 + 0x5BD1E995 + (base & 0xFFFFFFFF) * 0x85EBCA6B) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x85EBCA6B) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def assign_site_seeds(module: nn.Module, first: int = 0, base: int = 0) -> int:
    """Number the dropout sites under ``module`` in module order from ``first`` on and give each its layer seed (two per WindowAttention:
    attn_drop, proj_drop; two per Mlp: drop1, drop2); returns the next free number."""
    k = first
    for m in module.modules():
        if hasattr(m, "drop_seeds"):
            m.drop_seeds = (site_seed(k, base), site_seed(k + 1, base))
            k += 2
    return k


class DropState:
    """What a forward hands its dropout sites: ``word``, its own one-element int32 device copy of the network's seed word (None: the layer
    seeds alone), and ``masks``, explicit uint8 keep masks by site name relative to the module that receives the state (tests)."""

    def __init__(self, word=None, masks=None):
        self.word, self.masks = word, masks or {}

    def sub(self, prefix: str) -> "DropState":
        pre = prefix + "."
        return DropState(self.word, {k[len(pre):]: v for k, v in self.masks.items() if k.startswith(pre)})

    def mask(self, name: str, like: torch.Tensor):
        """The explicit mask of site ``name`` on ``like``'s device, or None."""
        m = self.masks.get(name)
        return None if m is None else m.to(device=like.device, dtype=torch.uint8).contiguous()


NO_DROP = DropState()


def dropout(x, p: float, seed: int, training: bool, drop: DropState, name: str):
    """nn.Dropout(p) of a module in train mode on the HIP token dropout; nothing is launched in eval mode or at p = 0."""
    if p == 0.0 or not training:
        return x
    return token_dropout(x, p, seed, drop.word, drop.mask(name, x))


class PatchMerging(nn.Module):
    def __init__(self, dim: int, norm_layer=nn.LayerNorm):
        super().__init__()
        _only("PatchMerging", "norm_layer", norm_layer, nn.LayerNorm)
        self.dim = dim
        self.norm = norm_layer(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        x = patch_merge(x)
        return linear(norm(x, self.norm), self.reduction.weight)


class Mlp(nn.Module):
    def __init__(self, in_features: int, hidden_features: int = None, out_features: int = None, act_layer=nn.GELU, drop: float = 0., *,
                 allow_dropout: bool = False):
        super().__init__()
        _only("Mlp", "act_layer", act_layer, nn.GELU)
        _no_dropout("Mlp", allow_dropout, drop=drop)
        self.drop = float(drop)
        self.drop_seeds = (site_seed(2), site_seed(3))          # drop1, drop2; an enclosing block / stage / network numbers its sites anew
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x, drop: DropState = NO_DROP):
        x = dropout(gelu(linear(x, self.fc1.weight, self.fc1.bias)), self.drop, self.drop_seeds[0], self.training, drop, "drop1")
        return dropout(linear(x, self.fc2.weight, self.fc2.bias), self.drop, self.drop_seeds[1], self.training, drop, "drop2")


class WindowAttention(nn.Module):
    def __init__(self, dim: int, window_size: int, num_heads: int, qkv_bias: bool = True, attn_drop: float = 0., proj_drop: float = 0.,
                 shift: bool = False, *, allow_dropout: bool = False, packed: bool = False):
        super().__init__()
        _no_dropout("WindowAttention", allow_dropout, attn_drop=attn_drop, proj_drop=proj_drop)
        if packed and not 2 <= window_size <= MAX_PACKED_WINDOW:
            raise ValueError(f"WindowAttention: packed=True is for windows 2 .. {MAX_PACKED_WINDOW} (csrc/attn_window_packed.hip), got {window_size}")
        self.packed = bool(packed)          # which kernel family runs: chosen once, here, never in a launch path
        self.attn_drop, self.proj_drop = float(attn_drop), float(proj_drop)
        self.drop_seeds = (site_seed(0), site_seed(1))          # attn_drop, proj_drop; an enclosing block / stage / network numbers its sites anew
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

    def forward(self, x, drop: DropState = NO_DROP):
        qkv = linear(x, self.qkv.weight, self.qkv.bias)
        if self.packed:
            on = self.attn_drop != 0.0 and self.training
            a = window_attention_packed(qkv, self.relative_position_bias_table, self.num_heads, self.window_size, self.shift_size, self.scale,
                                        self.attn_drop if on else 0.0, self.drop_seeds[0], drop.word if on else None,
                                        drop.mask("attn_drop", qkv) if on else None)
        elif self.attn_drop == 0.0 or not self.training:
            a = window_attention(qkv, self.relative_position_bias_table, self.num_heads, self.window_size, self.shift_size, self.scale)
        else:          # the mask is in the reference's attn layout [B nW, heads, L, L] (rolled, window-partitioned order)
            a = window_attention_dropout(qkv, self.relative_position_bias_table, self.num_heads, self.window_size, self.shift_size, self.scale,
                                         self.attn_drop, self.drop_seeds[0], drop.word, drop.mask("attn_drop", qkv))
        # proj_drop acts on the un-partitioned map here (proj commutes with window reverse and the roll back), so its explicit mask is in map
        # order: the reference's mask after window reverse + roll back
        return dropout(linear(a, self.proj.weight, self.proj.bias), self.proj_drop, self.drop_seeds[1], self.training, drop, "proj_drop")


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift=False, mlp_ratio=4., qkv_bias=True, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, *, allow_dropout: bool = False, packed: bool = False):
        super().__init__()
        _only("SwinTransformerBlock", "norm_layer", norm_layer, nn.LayerNorm)
        _no_dropout("SwinTransformerBlock", allow_dropout, drop=drop, attn_drop=attn_drop)
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=window_size, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, shift=shift,
                                    allow_dropout=allow_dropout, packed=packed)
        self.dpr = float(drop_path)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop, allow_dropout=allow_dropout)
        self.external_draws = None        # (attention-branch draw, MLP-branch draw), each [B]: replay given uniform draws (tests)
        self.external_masks = None        # {"attn.attn_drop", "attn.proj_drop", "mlp.drop1", "mlp.drop2": uint8 keep mask}: replay given masks (tests)
        assign_site_seeds(self)

    def _keep_scale(self, batch, draw, device):
        """Per-sample factor of a residual branch (DropPath, swinunet.py:9-24): floor(keep + U) / keep, or None when nothing is dropped."""
        if self.dpr == 0.0 or not self.training:
            return None
        kp = 1.0 - self.dpr
        r = torch.rand((batch,), dtype=torch.float32, device=device) if draw is None else draw.to(device).reshape(batch).float()
        return (kp + r).floor() / kp

    def forward(self, x, draws=None, drop: DropState = None):
        if not x.is_cuda:
            raise RuntimeError("hpfg_amd.SwinTransformerBlock runs on the GPU only: its LayerNorm / window-attention / GELU kernels have no CPU fallback")
        d = draws if draws is not None else (self.external_draws if self.external_draws is not None else (None, None))
        if drop is None:
            drop = NO_DROP if self.external_masks is None else DropState(None, self.external_masks)
        B = x.shape[0]
        a = self.attn(norm(x, self.norm1), drop.sub("attn"))
        x = residual_scale(x, a, self._keep_scale(B, d[0], x.device))
        m = self.mlp(norm(x, self.norm2), drop.sub("mlp"))
        return residual_scale(x, m, self._keep_scale(B, d[1], x.device))


class BasicBlock(nn.Module):
    def __init__(self, index: int, embed_dim: int = 96, window_size: int = 7, depths: tuple = (2, 2, 6, 2), num_heads: tuple = (3, 6, 12, 24),
                 mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0., attn_drop_rate: float = 0., drop_path: float = 0.1,
                 norm_layer=nn.LayerNorm, patch_merging: bool = True, *, allow_dropout: bool = False, packed: bool = False):
        super().__init__()
        depth = depths[index]
        dim = embed_dim * 2 ** index
        dpr = [rate.item() for rate in torch.linspace(0, drop_path, sum(depths))]
        rates = dpr[sum(depths[:index]):sum(depths[:index + 1])]
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads[index], window_size=window_size, shift=i % 2 == 1, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                 drop=drop_rate, attn_drop=attn_drop_rate, drop_path=rates[i], norm_layer=norm_layer, allow_dropout=allow_dropout,
                                 packed=packed)
            for i in range(depth)])
        self.downsample = PatchMerging(dim=dim, norm_layer=norm_layer) if patch_merging else None
        self.external_draws = None        # one (attention, MLP) pair of [B] draws per block
        assign_site_seeds(self)          # the blocks of a stage draw different masks

    def forward(self, x, drop: DropState = NO_DROP, draws=None):
        draws = draws if draws is not None else self.external_draws
        for i, layer in enumerate(self.blocks):
            x = layer(x, None if draws is None else draws[i], drop.sub(f"blocks.{i}"))
        if self.downsample is not None:
            x = self.downsample(x)
        return x
