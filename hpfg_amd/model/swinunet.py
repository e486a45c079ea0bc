"""The Swin-UNet of the reference (model/swinunet.py:27-49 PatchEmbedding, :85-111 PatchExpanding / FinalPatchExpanding, :333-379 BasicBlockUp,
:382-536 encoder / decoder, :575-717 SwinUnet / SwinUnet_Plus, :720-778 the factories; model/swinunet_LIDC.py: the same network with
``patch_size`` handed down to the final patch expanding, and ``get_swinunet_LIDC``) assembled from the Swin blocks of ``model/swin.py`` on
the HIP token kernels.  Same constructor signatures, construction order, ``state_dict`` keys and ``init_weights`` pass as the reference, so a
seed gives the reference's weights.

Where the work runs (all through ``hpfg_amd.ops_tokens``; tokens stay an NHWC map):
* patch embedding: kernel == stride, so the NCHW image is reshaped to [B, H/p, W/p, Cin * p^2] (p = patch_size: 4, or 2 in the LIDC network;
  torch plumbing on the smallest tensor) and goes through ``linear``;
* patch expanding: ``linear`` then ``expand_layer_norm`` -- the pixel shuffle is the LayerNorm kernel's row map, so the expanded tensor (the
  network's largest: [B,224,224,96] after the final one) is written once instead of copied and then normalised;
* the skip connection: ``torch.cat`` + ``linear``; the head: ``linear`` with the prediction rows padded to a multiple of four, returned as
  an NCHW view of the NHWC logits;
* every norm through ``layer_norm`` with the module's eps (1e-6 in the factories; the third PatchMerging norm has 1536 channels).

Dropout (drop_rate = attn_drop_rate = 0.1 in the factories): a network owns one device seed word (``drop_word``, a non-persistent buffer) and
gives each dropout site a constant layer seed mixed from the site's number and the instance's base seed (``dropout_seed``, from the
process-wide instance counter of ``model/unet.py``, not from torch's generator: construction consumes the RNG like the reference's).  Two
networks, and a ``deepcopy`` of one (the EMA teacher), therefore draw independent masks for the same input, as the reference's separate
nn.Dropout calls do; ``reset_dropout_streams()`` restarts the numbering for run-to-run reproducibility.  A training forward advances the word with a kernel and hands its ops its own copy, so a
replayed hipGraph draws new masks and a backward uses the seed of its own forward even if the network ran again in between.  Eval mode
launches no dropout.  ``external_draws`` = (drop-path pairs per block in forward order or None, {site name: uint8 keep mask} or None) replays
given draws (tests); site names are module paths such as "encoder.pos_drop" or "decoder.layers_up.0.blocks.1.attn.attn_drop".
"""
from __future__ import annotations

import copy
from functools import partial

import torch
import torch.nn as nn

from .. import heads
from ..ops_tokens import LN_PX_FACTORS, expand_layer_norm, linear, seed_word_add
from .swin import NO_DROP, BasicBlock, DropState, SwinTransformerBlock, _only, assign_site_seeds, dropout, norm, site_seed
from .unet import _fresh_dropout_seed, _neck

NECK_POOL = 4          # projection_conv's AdaptiveAvgPool2d((4, 4)) (model/swinunet.py:544,555)


class PatchEmbedding(nn.Module):
    def __init__(self, patch_size: int = 4, in_c: int = 3, embed_dim: int = 96, norm_layer=None):
        super().__init__()
        if norm_layer is not None:
            _only("PatchEmbedding", "norm_layer", norm_layer, nn.LayerNorm)
        self.patch_size = patch_size
        self.proj = nn.Conv2d(in_c, embed_dim, kernel_size=(patch_size,) * 2, stride=(patch_size,) * 2)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def forward(self, x):
        B, C_, H, W = x.shape
        p = self.patch_size
        if H % p or W % p:
            raise ValueError(f"PatchEmbedding: image sides {H} x {W} must be multiples of the patch size {p} (the padding branch is not built)")
        x = x.float().reshape(B, C_, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B, H // p, W // p, C_ * p * p)
        x = linear(x, self.proj.weight.reshape(self.proj.weight.shape[0], -1), self.proj.bias)
        return norm(x, self.norm) if isinstance(self.norm, nn.LayerNorm) else x


class _Expanding(nn.Module):
    factor = 2

    def forward(self, x):
        return expand_layer_norm(linear(x, self.expand.weight), self.norm.weight, self.norm.bias, self.factor, self.norm.eps)


class PatchExpanding(_Expanding):
    def __init__(self, dim: int, norm_layer=nn.LayerNorm):
        super().__init__()
        _only("PatchExpanding", "norm_layer", norm_layer, nn.LayerNorm)
        self.dim = dim
        self.expand = nn.Linear(dim, 2 * dim, bias=False)
        self.norm = norm_layer(dim // 2)


class FinalPatchExpanding(_Expanding):
    def __init__(self, dim: int, norm_layer=nn.LayerNorm, patch_size: int = 4):
        super().__init__()
        _only("FinalPatchExpanding", "norm_layer", norm_layer, nn.LayerNorm)
        if patch_size not in LN_PX_FACTORS:
            raise ValueError(f"FinalPatchExpanding: patch_size {patch_size} is not built; expand_layer_norm has the factors {LN_PX_FACTORS}")
        self.dim = dim
        self.patch_size = self.factor = patch_size          # reference model/swinunet_LIDC.py:101-111 (4 in model/swinunet.py)
        self.expand = nn.Linear(dim, patch_size ** 2 * dim, bias=False)
        self.norm = norm_layer(dim)


class BasicBlockUp(nn.Module):
    def __init__(self, index: int, embed_dim: int = 96, window_size: int = 7, depths: tuple = (2, 2, 6, 2), num_heads: tuple = (3, 6, 12, 24),
                 mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0., attn_drop_rate: float = 0., drop_path: float = 0.1,
                 patch_expanding: bool = True, norm_layer=nn.LayerNorm, *, allow_dropout: bool = False, packed: bool = False):
        super().__init__()
        index = len(depths) - index - 2          # the mirrored encoder stage: its depth, width, heads and drop-path slice (swinunet.py:348-354)
        depth = depths[index]
        dim = embed_dim * 2 ** index
        dpr = [rate.item() for rate in torch.linspace(0, drop_path, sum(depths))]
        rates = dpr[sum(depths[:index]):sum(depths[:index + 1])]
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads[index], window_size=window_size, shift=i % 2 == 1, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                 drop=drop_rate, attn_drop=attn_drop_rate, drop_path=rates[i], norm_layer=norm_layer, allow_dropout=allow_dropout,
                                 packed=packed)
            for i in range(depth)])
        self.upsample = PatchExpanding(dim=dim, norm_layer=norm_layer) if patch_expanding else nn.Identity()
        self.external_draws = None        # one (attention, MLP) pair of [B] draws per block
        assign_site_seeds(self)          # the blocks of a stage draw different masks

    def forward(self, x, drop: DropState = NO_DROP, draws=None):
        draws = draws if draws is not None else self.external_draws
        for i, layer in enumerate(self.blocks):
            x = layer(x, None if draws is None else draws[i], drop.sub(f"blocks.{i}"))
        return self.upsample(x)


def _per_stage(packed, stages: int) -> tuple:
    """``packed`` of the encoder / decoder / network constructors as one flag per encoder stage: a bool for all, or a sequence of ``stages``
    bools (stage i of the encoder and the decoder stage that mirrors it run the same map size, so they share the flag)."""
    if isinstance(packed, bool):
        return (packed,) * stages
    packed = tuple(bool(f) for f in packed)
    if len(packed) != stages:
        raise ValueError(f"packed {packed} must be a bool or one flag per stage ({stages})")
    return packed


def _stage_draws(draws, layers):
    """The network's list of drop-path pairs (forward order) cut into one list per stage."""
    if draws is None:
        return [None] * len(layers), 0
    out, k = [], 0
    for layer in layers:
        out.append(draws[k:k + len(layer.blocks)])
        k += len(layer.blocks)
    return out, k


class SwinUnetEncoder(nn.Module):
    def __init__(self, patch_size: int = 4, in_chans: int = 3, embed_dim: int = 96, window_size: int = 7, depths: tuple = (2, 2, 6, 2),
                 num_heads: tuple = (3, 6, 12, 24), mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0., attn_drop_rate: float = 0.,
                 drop_path_rate: float = 0.1, norm_layer=nn.LayerNorm, patch_norm: bool = True, *, packed=False):
        super().__init__()
        self.num_layers = len(depths)
        packed = _per_stage(packed, len(depths))
        self.patch_embed = PatchEmbedding(patch_size=patch_size, in_c=in_chans, embed_dim=embed_dim, norm_layer=norm_layer if patch_norm else None)
        self.drop_rate = float(drop_rate)
        self.pos_drop_seed = site_seed(4)
        self.layers = nn.ModuleList([
            BasicBlock(index=i, depths=depths, embed_dim=embed_dim, num_heads=num_heads, drop_path=drop_path_rate, window_size=window_size,
                       mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, norm_layer=norm_layer,
                       patch_merging=i != len(depths) - 1, allow_dropout=True, packed=packed[i])
            for i in range(len(depths))])

    def forward(self, x, drop: DropState = NO_DROP, draws=None):
        x = self.patch_embed(x)
        x = dropout(x, self.drop_rate, self.pos_drop_seed, self.training, drop, "pos_drop")
        per, _ = _stage_draws(draws, self.layers)
        feats = []
        for i, layer in enumerate(self.layers):
            if i != self.num_layers - 1:
                feats.append(x)
            x = layer(x, drop.sub(f"layers.{i}"), per[i])
        feats.append(x)
        return feats


class SwinUnetDecoder(nn.Module):
    def __init__(self, num_classes: int = 1000, embed_dim: int = 96, window_size: int = 7, depths: tuple = (2, 2, 6, 2),
                 num_heads: tuple = (3, 6, 12, 24), mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0., attn_drop_rate: float = 0.,
                 drop_path_rate: float = 0.1, norm_layer=nn.LayerNorm, patch_size: int = 4, *, packed=False):
        super().__init__()
        _only("SwinUnetDecoder", "norm_layer", norm_layer, nn.LayerNorm)
        n = len(depths)
        packed = _per_stage(packed, n)
        self.patch_size = patch_size
        self.num_layers = n
        self.first_patch_expanding = PatchExpanding(dim=embed_dim * 2 ** (n - 1), norm_layer=norm_layer)
        self.layers_up = nn.ModuleList([
            BasicBlockUp(index=i, depths=depths, embed_dim=embed_dim, num_heads=num_heads, drop_path=drop_path_rate, window_size=window_size,
                         mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, patch_expanding=i < n - 2,
                         norm_layer=norm_layer, allow_dropout=True, packed=packed[n - 2 - i])
            for i in range(n - 1)])
        self.skip_connection_layers = nn.ModuleList([nn.Linear(embed_dim * 2 ** (n - 2 - i) * 2, embed_dim * 2 ** (n - 2 - i)) for i in range(n - 1)])
        self.norm_up = norm_layer(embed_dim)
        self.final_patch_expanding = FinalPatchExpanding(dim=embed_dim, norm_layer=norm_layer, patch_size=patch_size)
        self.head = nn.Conv2d(in_channels=embed_dim, out_channels=num_classes, kernel_size=(1, 1), bias=False)

    def forward(self, feats, drop: DropState = NO_DROP, draws=None):
        per, _ = _stage_draws(draws, self.layers_up)
        x = self.first_patch_expanding(feats[-1])
        for i, layer in enumerate(self.layers_up):
            skip = self.skip_connection_layers[i]
            x = linear(torch.cat([x, feats[len(feats) - i - 2]], -1), skip.weight, skip.bias)
            x = layer(x, drop.sub(f"layers_up.{i}"), per[i])
        x = self.final_patch_expanding(norm(x, self.norm_up))
        wp, ncls = self.head.weight.reshape(self.head.weight.shape[0], -1), self.head.weight.shape[0]
        if ncls % 4:          # the GEMM's fast path moves 4 output columns at a time: pad the head with zero rows, slice them off after
            wp = torch.cat([wp, wp.new_zeros(4 - ncls % 4, wp.shape[1])], 0)
        return linear(x, wp)[..., :ncls].permute(0, 3, 1, 2)          # NCHW view of the NHWC logits


def _init_weights(m):
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


class SwinUnet(nn.Module):
    def __init__(self, patch_size: int = 4, in_chans: int = 3, num_classes: int = 1000, embed_dim: int = 96, window_size: int = 7,
                 depths: tuple = (2, 2, 6, 2), num_heads: tuple = (3, 6, 12, 24), mlp_ratio: float = 4., qkv_bias: bool = True, drop_rate: float = 0.,
                 attn_drop_rate: float = 0., drop_path_rate: float = 0.1, norm_layer=nn.LayerNorm, patch_norm: bool = True, *, packed=False):
        super().__init__()
        self.encoder = SwinUnetEncoder(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, window_size=window_size, depths=depths,
                                       num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                                       drop_path_rate=drop_path_rate, norm_layer=norm_layer, patch_norm=patch_norm, packed=packed)
        self.decoder = SwinUnetDecoder(num_classes=num_classes, embed_dim=embed_dim, window_size=window_size, depths=depths, num_heads=num_heads,
                                       mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                                       drop_path_rate=drop_path_rate, norm_layer=norm_layer, patch_size=patch_size, packed=packed)
        self._build_necks(embed_dim * 2 ** (len(depths) - 1), num_classes)
        self.apply(self.init_weights)          # the necks' nn.Linear layers included, as the reference's apply does
        self.has_dropout = drop_rate > 0.0 or attn_drop_rate > 0.0
        self.register_buffer("drop_word", torch.zeros(1, dtype=torch.int32), persistent=False)          # not in state_dict: the reference has none
        self.external_draws = None        # (drop-path pairs per block in forward order, {site name: uint8 keep mask}): replay given draws (tests)
        self._new_dropout_stream()

    init_weights = staticmethod(_init_weights)

    def _build_necks(self, top_channels, num_classes):
        """What a subclass constructs between the decoder and the init_weights pass (SwinUnet_Plus: the projection necks)."""

    def _new_dropout_stream(self):
        """A base seed of this instance's own and, from it, one layer seed per dropout site in module order."""
        self.dropout_seed = _fresh_dropout_seed()
        self.encoder.pos_drop_seed = site_seed(0, self.dropout_seed)
        assign_site_seeds(self, 1, self.dropout_seed)

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__ = copy.deepcopy(self.__dict__, memo)
        new._new_dropout_stream()          # a copy (EMA teacher) draws its own masks
        return new

    def _features(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"hpfg_amd.{type(self).__name__} runs on the GPU only: its LayerNorm / window-attention / GELU kernels have no CPU fallback")
        draws, masks = self.external_draws if self.external_draws is not None else (None, None)
        drop = NO_DROP
        if self.training and self.has_dropout:
            seed_word_add(self.drop_word, 1)
            drop = DropState(self.drop_word.clone(), masks)          # this forward's own copy: its backward reads it, whatever runs in between
        n_enc = sum(len(layer.blocks) for layer in self.encoder.layers)
        feats = self.encoder(x, drop.sub("encoder"), None if draws is None else draws[:n_enc])
        return self.decoder(feats, drop.sub("decoder"), None if draws is None else draws[n_enc:]), feats[-1]

    def forward(self, x):
        return self._features(x)[0]

    def val(self, x):
        return self.forward(x)

    def bump_graph_seed(self):
        """GraphedStep hook: nothing to do -- every training forward advances ``drop_word`` with a kernel of its own, which a captured graph
        replays, and drop-path draws from the torch device generator, whose state a captured graph advances by itself."""


class SwinUnet_Plus(SwinUnet):
    """SwinUnet + the two ``projection_conv`` necks (reference model/swinunet.py:643-717; same construction order and ``state_dict`` keys).
    ``forward`` returns ``(logits, high, head)``, each neck output a ``(global [N,128], dense [N,128,16])`` pair: ``high`` on the last encoder
    map (NHWC already, what ``heads.projection_neck`` prefers), ``head`` on the logits.  ``skip_necks`` (set by a step that discards them,
    HPFG's first student) leaves them uncomputed.  The high neck takes embed_dim * 2^(stages - 1) channels: the reference's literal
    embed_dim * 8 at its four stages."""

    skip_necks = False

    def _build_necks(self, top_channels, num_classes):
        self.dense_projection_high = _neck(top_channels, 2048)
        self.dense_projection_head = _neck(num_classes, 1024)

    def backbone_numel(self) -> int:
        """encoder + decoder parameters: the leading part of ``parameters()`` (and of the flat buffers an optimizer lays them into)."""
        return sum(p.numel() for m in (self.encoder, self.decoder) for p in m.parameters())

    def val(self, x):
        return self._features(x)[0]

    def forward(self, x):
        logits, top = self._features(x)
        if self.skip_necks:
            return logits, None, None
        if top.shape[1] < NECK_POOL or top.shape[2] < NECK_POOL:
            raise ValueError(f"SwinUnet_Plus: the last encoder map is {top.shape[1]} x {top.shape[2]}, smaller than the necks' {NECK_POOL} x {NECK_POOL} "
                             f"adaptive pooling")
        high = heads.projection_neck(self.dense_projection_high, top.permute(0, 3, 1, 2), NECK_POOL)
        head = heads.projection_neck(self.dense_projection_head, logits, NECK_POOL)
        return logits, high, head


def _factory(cls, img_size, patch_size, in_channels, num_classes):
    if img_size == 224:
        window_size = 7
    elif img_size == 256:
        window_size = 8
    else:
        raise NotImplementedError(f"{cls.__name__}: image side {img_size} is not built (224: window 7, 256: window 8)")
    return cls(patch_size=patch_size, in_chans=in_channels, num_classes=num_classes, embed_dim=96, window_size=window_size, depths=(2, 2, 6, 2),
               num_heads=(3, 6, 12, 24), mlp_ratio=4., qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2,
               norm_layer=partial(nn.LayerNorm, eps=1e-6))


def get_swinunet(img_size: int = 224, patch_size: int = 4, in_channels: int = 3, num_classes: int = 4):
    return _factory(SwinUnet, img_size, patch_size, in_channels, num_classes)


def get_swinunet_plus(img_size: int = 224, patch_size: int = 4, in_channels: int = 3, num_classes: int = 4):
    return _factory(SwinUnet_Plus, img_size, patch_size, in_channels, num_classes)


# Which encoder stages (and the decoder stages that mirror them) of the LIDC network run the packed small-window kernels, by window.  The rule
# (profiles/swinunet_lidc_timing.txt): a stage keeps ``packed`` only where the measured (min .. max) range of the packed forward + backward
# pair lies wholly below the unpacked pair's at the configuration's batch; the choice is made here, at construction, never in a launch path.
# Measured at batch 64: window 3 (96 x 96) packed 0.22 / 0.27 / 0.35 / 0.54 of the unpacked pair on the 48 / 24 / 12 / 6 maps; window 4 (64 x 64)
# 0.38 / 0.44 / 0.86 on the 32 / 16 / 8 maps, and on the 4 x 4 map -- one window per image, as many workgroups either way -- the ranges overlap.
LIDC_PACKED = {3: (True, True, True, True), 4: (True, True, True, False)}


def get_swinunet_LIDC(img_size: int = 96, patch_size: int = 2, in_channels: int = 3, num_classes: int = 4):
    """The reference's LIDC Swin-UNet (model/swinunet_LIDC.py:619-646): patch 2, window 3 at 96 x 96 (token maps 48 / 24 / 12 / 6) or window 4
    at 64 x 64 (32 / 16 / 8 / 4), otherwise the rates and depths of ``get_swinunet``."""
    if img_size == 96:
        window_size = 3
    elif img_size == 64:
        window_size = 4
    else:
        raise NotImplementedError(f"get_swinunet_LIDC: image side {img_size} is not built (96: window 3, 64: window 4)")
    return SwinUnet(patch_size=patch_size, in_chans=in_channels, num_classes=num_classes, embed_dim=96, window_size=window_size, depths=(2, 2, 6, 2),
                    num_heads=(3, 6, 12, 24), mlp_ratio=4., qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.2,
                    norm_layer=partial(nn.LayerNorm, eps=1e-6), packed=LIDC_PACKED[window_size])
