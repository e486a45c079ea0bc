"""UniFormer-S and Uniformer_Plus (UniFormer-S + SegFormerHead + the two projection necks): the fourth backbone the reference ships its HPFG
method for (model/uniformer.py; config/ccnet_uniformer_30k_224x224_ACDC.yaml).

Same module tree, parameter names and constructor order as the reference's ``model/uniformer.py`` (Mlp :18-34, CMlp :37-53, Attention :56-81,
CBlock :84-103, SABlock :106-140, PatchEmbed :174-199, UniFormer :202-328, uniformer_small :331-338, Uniformer_Plus :508-527), so
``state_dict()`` interchanges and a seed gives the same initial weights -- up to ``trunc_normal_``, which is torch's here and ``timm``'s
there.  The modules without parameters (DropPath, Dropout(0), GELU) are not registered: they own no ``state_dict`` key and draw nothing
at construction.  Only the configuration ``uniformer_small`` builds is supported: patch stem, no layer scale, no dropout.

Where the work runs, forward and backward, all through ``hpfg_amd.ops_tokens``:
* the network works on NHWC tokens [B, H, W, C] throughout; the reference's NCHW <-> token transposes between SABlocks are views here;
* ``pos_embed`` (x + depthwise 3x3) and ``CBlock.attn`` (depthwise 5x5): ``dwconv`` (csrc/dwconv.hip), the residual inside the kernel;
* ``CBlock.norm1 / norm2`` and the four stage norms (nn.BatchNorm2d): ``batch_norm_tokens`` (hpfg_bn_tok_*), running statistics updated
  here; eval mode is the affine map of the running statistics on the same apply kernel (``batch_norm_tokens_eval``, differentiable, so
  an eval-mode forward may carry gradients as in the reference);
* every 1x1 conv and Linear, and the patch embeddings (kernel == stride: a GEMM over non-overlapping patches): ``linear``;
* SABlock attention: global self-attention, head dim 64, (side / 16)^2 or (side / 32)^2 keys: ``attention_for`` (csrc/attn.hip up to 64
  keys, csrc/attn_keys.hip up to 256).  The qkv weight is sliced by rows into a C-row and a 2C-row ``linear``, which gives q [B,N,heads,64]
  and kv [B,N,2,heads,64] in the layouts the attention kernels read, with no copy of the activations;
* LayerNorm (eps 1e-6 in the blocks, 1e-5 in PatchEmbed), GELU, residual adds with their drop-path factor: ``layer_norm``, ``gelu``,
  ``residual_scale``.

Stochastic depth draws from the torch device generator, two draws per block in block order (none for a block whose rate is 0: the first);
``external_draws = (drop_path_draws, dropout_mask)`` replays given draws, ``drop_path_draws`` holding two entries per block (None where
nothing is drawn), as in ``SegFormer_Plus``.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from .. import heads
from ..ops_tokens import (MAX_KEYS_LONG, attention_for, batch_norm_tokens, batch_norm_tokens_eval, dwconv, gelu, layer_norm, linear,
                          residual_scale)
from .segformer import NECK_POOL, SegFormerHead

MIN_SIDE, MAX_SIDE = 32 * NECK_POOL, 256          # the necks pool a 4 x 4 map of the stage-4 (side / 32)^2 tokens; stage 3 has (side / 16)^2 keys


def check_side(who: str, height: int, width: int) -> int:
    """The image sizes Uniformer_Plus is built for: square (the reference passes img_size=image_size[0]), a multiple of 32, 128 to 256."""
    height, width = int(height), int(width)
    if height != width:
        raise ValueError(f"{who}: square inputs only (got {height} x {width}); the reference builds its patch embeddings from image_size[0]")
    if height % 32:
        raise ValueError(f"{who}: the image side must be a multiple of 32, the total stride of the four patch embeddings (got {height})")
    if height < MIN_SIDE:
        raise ValueError(f"{who}: a side of {height} gives a {height // 32} x {height // 32} stage-4 map, smaller than the necks' {NECK_POOL} x "
                         f"{NECK_POOL} adaptive pooling; the side must be at least {MIN_SIDE}")
    if (height // 16) ** 2 > MAX_KEYS_LONG or height > MAX_SIDE:
        raise ValueError(f"{who}: a side of {height} gives {(height // 16) ** 2} keys per attention row in stage 3; the attention kernels take "
                         f"at most {MAX_KEYS_LONG}: the side must be at most {MAX_SIDE}")
    return height


def _bn_tokens(bn: nn.BatchNorm2d, x, training: bool):
    """nn.BatchNorm2d on NHWC tokens: batch statistics + running update in train mode, the running statistics' affine map in eval mode."""
    if not training:
        return batch_norm_tokens_eval(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    y, mu, var = batch_norm_tokens(x, bn.weight, bn.bias, bn.eps)
    with torch.no_grad():
        n = x.numel() // x.shape[-1]
        bn.running_mean.mul_(1 - bn.momentum).add_(mu, alpha=bn.momentum)
        bn.running_var.mul_(1 - bn.momentum).add_(var * (n / max(n - 1, 1)), alpha=bn.momentum)
        bn.num_batches_tracked += 1
    return y


def _conv1x1(conv: nn.Conv2d, x):
    return linear(x, conv.weight.reshape(conv.weight.shape[0], -1), conv.bias)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _only_zero("Mlp", "drop", drop)
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return linear(gelu(linear(x, self.fc1.weight, self.fc1.bias)), self.fc2.weight, self.fc2.bias)


class CMlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _only_zero("CMlp", "drop", drop)
        self.fc1 = nn.Conv2d(in_features, hidden_features or in_features, 1)
        self.fc2 = nn.Conv2d(hidden_features or in_features, out_features or in_features, 1)

    def forward(self, x):
        return _conv1x1(self.fc2, gelu(_conv1x1(self.fc1, x)))


def _only_zero(who, name, value):
    if value:
        raise NotImplementedError(f"{who}: {name}={value} is not built (uniformer_small uses 0)")


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        _only_zero("Attention", "attn_drop", attn_drop)
        _only_zero("Attention", "proj_drop", proj_drop)
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        """x [B, N, C].  The rows of the qkv weight are (q | k | v) x (head, channel): rows [0, C) give q, rows [C, 3C) give kv [B,N,2,heads,d]."""
        C = x.shape[-1]
        w, b = self.qkv.weight, self.qkv.bias
        q = linear(x, w[:C], None if b is None else b[:C])
        kv = linear(x, w[C:], None if b is None else b[C:])
        return linear(attention_for(kv.shape[1])(q, kv, self.num_heads, self.scale), self.proj.weight, self.proj.bias)


class _Block(nn.Module):
    def _keep_scale(self, batch, draw, device):
        """Per-sample factor of a residual branch (DropPath; the law of the reference's model/segformer.py:23-30): floor(keep + U) / keep."""
        if self.dpr == 0.0 or not self.training:
            return None
        kp = 1.0 - self.dpr
        r = torch.rand((batch, 1, 1), dtype=torch.float32, device=device) if draw is None else draw.to(device)
        return (kp + r).floor() / kp


class CBlock(_Block):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.pos_embed = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.norm1 = nn.BatchNorm2d(dim)
        self.conv1 = nn.Conv2d(dim, dim, 1)
        self.conv2 = nn.Conv2d(dim, dim, 1)
        self.attn = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.dpr = float(drop_path)
        self.norm2 = nn.BatchNorm2d(dim)
        self.mlp = CMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, draws=(None, None)):
        """x NHWC [B, H, W, C]"""
        B = x.shape[0]
        x = dwconv(x, self.pos_embed.weight, self.pos_embed.bias, 3, residual=x)
        h = _conv1x1(self.conv1, _bn_tokens(self.norm1, x, self.training))
        h = _conv1x1(self.conv2, dwconv(h, self.attn.weight, self.attn.bias, 5))
        x = residual_scale(x, h, self._keep_scale(B, draws[0], x.device))
        h = self.mlp(_bn_tokens(self.norm2, x, self.training))
        return residual_scale(x, h, self._keep_scale(B, draws[1], x.device))


class SABlock(_Block):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0., act_layer=nn.GELU,
                 norm_layer=nn.LayerNorm):
        super().__init__()
        self.pos_embed = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)
        self.dpr = float(drop_path)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, draws=(None, None)):
        """x NHWC [B, H, W, C]: the tokens [B, H W, C] are a view of it"""
        B, H, W, C = x.shape
        t = dwconv(x, self.pos_embed.weight, self.pos_embed.bias, 3, residual=x).view(B, H * W, C)
        a = self.attn(layer_norm(t, self.norm1.weight, self.norm1.bias, self.norm1.eps))
        t = residual_scale(t, a, self._keep_scale(B, draws[0], x.device))
        m = self.mlp(layer_norm(t, self.norm2.weight, self.norm2.bias, self.norm2.eps))
        return residual_scale(t, m, self._keep_scale(B, draws[1], x.device)).view(B, H, W, C)


class PatchEmbed(nn.Module):
    """Image to patch embedding: kernel = stride = patch, no padding, then LayerNorm (eps 1e-5)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size, self.patch_size = (int(img_size),) * 2, (int(patch_size),) * 2
        self.num_patches = (self.img_size[1] // self.patch_size[1]) * (self.img_size[0] // self.patch_size[0])
        self.norm = nn.LayerNorm(embed_dim)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)

    def forward(self, x):
        """x NHWC [B, H, W, Cin] -> NHWC [B, H / p, W / p, E]: the non-overlapping patches gathered with rows ordered (u, v, channel), one GEMM."""
        B, H, W, Cin = x.shape
        p = self.patch_size[0]
        if (H, W) != self.img_size:
            raise ValueError(f"PatchEmbed: input size {H} x {W} does not match the model's {self.img_size[0]} x {self.img_size[1]}")
        t = x.reshape(B, H // p, p, W // p, p, Cin).permute(0, 1, 3, 2, 4, 5).reshape(B, H // p, W // p, p * p * Cin)
        wt = self.proj.weight.permute(0, 2, 3, 1).reshape(self.proj.weight.shape[0], -1)
        return layer_norm(linear(t, wt, self.proj.bias), self.norm.weight, self.norm.bias, self.norm.eps)


class UniFormer(nn.Module):
    def __init__(self, depth=[3, 4, 8, 3], img_size=224, in_chans=3, num_classes=1000, embed_dim=[64, 128, 320, 512], head_dim=64, mlp_ratio=4.,
                 qkv_bias=True, qk_scale=None, representation_size=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=None,
                 conv_stem=False):
        super().__init__()
        if conv_stem:
            raise NotImplementedError("UniFormer: the conv-stem variants are not built (uniformer_small uses the patch stem)")
        _only_zero("UniFormer", "drop_rate", drop_rate)
        if head_dim != 64 or any(d % head_dim for d in embed_dim):
            raise NotImplementedError(f"UniFormer: head_dim {head_dim} with dims {embed_dim}: the global attention is built for head dim 64")
        self.num_classes = num_classes
        self.num_features = self.embed_dim = self.embed_dims = embed_dim
        self.depth = list(depth)
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.patch_embed1 = PatchEmbed(img_size=img_size, patch_size=4, in_chans=in_chans, embed_dim=embed_dim[0])
        self.patch_embed2 = PatchEmbed(img_size=img_size // 4, patch_size=2, in_chans=embed_dim[0], embed_dim=embed_dim[1])
        self.patch_embed3 = PatchEmbed(img_size=img_size // 8, patch_size=2, in_chans=embed_dim[1], embed_dim=embed_dim[2])
        self.patch_embed4 = PatchEmbed(img_size=img_size // 16, patch_size=2, in_chans=embed_dim[2], embed_dim=embed_dim[3])
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depth))]      # stochastic depth decay rule, indexed across all blocks
        num_heads = [dim // head_dim for dim in embed_dim]
        cur = 0
        for s in range(4):
            block = CBlock if s < 2 else SABlock
            setattr(self, f"blocks{s + 1}", nn.ModuleList([
                block(dim=embed_dim[s], num_heads=num_heads[s], mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                      attn_drop=attn_drop_rate, drop_path=dpr[cur + i], norm_layer=norm_layer) for i in range(depth[s])]))
            setattr(self, f"norm{s + 1}", nn.BatchNorm2d(embed_dim[s]))
            cur += depth[s]
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, x, draws=None):
        """NCHW input -> the four stage outputs as tokens [(tokens [B,N,C], H, W)] (the reference returns them as NCHW images)."""
        x = x.permute(0, 2, 3, 1)                                # NCHW -> NHWC (a view; contiguous already when C == 1)
        feats, bi = [], 0
        for s in range(4):
            x = getattr(self, f"patch_embed{s + 1}")(x)
            for blk in getattr(self, f"blocks{s + 1}"):
                x = blk(x, (None, None) if draws is None else (draws[2 * bi], draws[2 * bi + 1]))
                bi += 1
            x = _bn_tokens(getattr(self, f"norm{s + 1}"), x, self.training)
            B, H, W, C = x.shape
            feats.append((x.view(B, H * W, C), H, W))
        return feats


def uniformer_small(**kwargs):
    return UniFormer(depth=[3, 4, 8, 3], embed_dim=[64, 128, 320, 512], head_dim=64, mlp_ratio=4, qkv_bias=True,
                     norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


class Uniformer_Plus(nn.Module):
    """UniFormer-S + SegFormerHead + the two ``projection_conv`` necks (reference model/uniformer.py:508-527; same construction order and
    ``state_dict`` keys).  ``forward`` returns ``(logits, high, head)``, each neck output a ``(global [N,128], dense [N,128,16])`` pair;
    ``skip_necks`` (set by a step that discards them, HPFG's first student) leaves them uncomputed.  Square inputs, side a multiple of 32
    from 128 (the necks pool a 4 x 4 map) to 256 (stage 3 has (side / 16)^2 <= 256 keys)."""

    def __init__(self, image_size=[224, 224], in_channels=3, num_classes=4):
        super().__init__()
        from .unet import _neck
        self.side = check_side("Uniformer_Plus", *image_size)
        self.encoder = uniformer_small(img_size=self.side, in_chans=in_channels)
        self.decoder = SegFormerHead(self.encoder.embed_dims, image_size=image_size, embed_dim=256, num_classes=num_classes)
        self.dense_projection_high = _neck(self.encoder.embed_dims[-1], 2048)
        self.dense_projection_head = _neck(num_classes, 1024)
        self.external_draws = None        # (drop_path_draws, dropout_mask): replay given random draws (tests)
        self.skip_necks = False

    def backbone_numel(self) -> int:
        """encoder + decoder parameters: the leading part of ``parameters()`` (and of the flat buffers an optimizer lays them into)."""
        return sum(p.numel() for m in (self.encoder, self.decoder) for p in m.parameters())

    def _backbone(self, x):
        if check_side("Uniformer_Plus", x.shape[-2], x.shape[-1]) != self.side:
            raise ValueError(f"Uniformer_Plus: a {x.shape[-2]} x {x.shape[-1]} input, but the model was built for {self.side} x {self.side}")
        if not x.is_cuda:
            raise RuntimeError("hpfg_amd.Uniformer_Plus runs on the GPU only: its depthwise conv / BatchNorm / attention kernels have no CPU fallback")
        dp, mask = self.external_draws if self.external_draws is not None else (None, None)
        feats = self.encoder(x.float(), dp)
        return self.decoder(feats, mask), feats[-1]

    def val(self, x):
        return self._backbone(x)[0]

    def forward(self, x):
        logits, (t4, H4, W4) = self._backbone(x)
        if self.skip_necks:
            return logits, None, None
        B = t4.shape[0]
        high = heads.projection_neck(self.dense_projection_high, t4.view(B, H4, W4, -1).permute(0, 3, 1, 2), NECK_POOL)
        head = heads.projection_neck(self.dense_projection_head, logits, NECK_POOL)
        return logits, high, head

    def bump_graph_seed(self):
        """GraphedStep hook: nothing to do -- drop-path and Dropout2d draw from the torch device generator, whose state a captured graph
        advances by itself at every replay (see SegFormer.bump_graph_seed)."""
