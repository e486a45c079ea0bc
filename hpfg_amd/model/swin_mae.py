"""The Swin-MAE of the reference (model/swin_mae.py:27-74 the sin-cos table, :559-619 SwinMAE's constructor and initialize_weights, :621-647
patchify / unpatchify, :649-710 window_masking, :750-800 the forward passes, :803-811 the factory) assembled from the Swin blocks of
``model/swin.py`` and the patch embedding / expanding of ``model/swinunet.py`` on the HIP token kernels.  Same constructor signatures,
construction order, ``state_dict`` keys and ``initialize_weights`` pass (xavier-uniform on every Linear, ``mask_token`` normal with std 0.02),
so a seed gives the reference's weights.  An encoder of four stages, a decoder of three without skip connections, ``decoder_pred`` a Linear
with bias onto the 16 Cin values of a patch.

What the reference does on the host runs here as kernels of ``csrc/mae.hip`` (through ``hpfg_amd.ops_tokens``), so a training step is
capturable into a hipGraph:
* window masking -- ``mae_window_mask`` ranks the per-image noise on the device (the reference: argsort, then a per-image np.setdiff1d on
  ``.cpu().numpy()`` copies) and writes the uint8 token mask;
* the mask-token substitution -- ``mae_mask_tokens`` (the reference: a per-image Python loop);
* the loss -- ``mae_loss`` reads the image through the patchify addressing and writes the loss and its gradient in one pass over the
  prediction; neither the un-patchified prediction nor the mask image exists on that path (``reconstruction_loss``).  ``forward`` still
  returns the reference's ``(pred_img, mask_img)`` pair, built with torch reshapes: it is not what the step calls.

The masking noise is ``torch.rand(B, d * d, device=...)`` from the torch device generator, whose state a captured graph advances by itself
(as drop-path's draws do); ``external_noise`` replays a given [B, d * d] tensor and ``external_draws`` a list of drop-path pairs per block in
forward order (tests).  ``pos_embed`` is kept as the frozen parameter the reference's ``state_dict`` carries, computed in float64 like the
reference's (its ``np.float``); the reference's ``forward_encoder`` never adds it, and neither does this one.

Not built: dropout inside the blocks (the factory's rates are 0), ``remove=True`` sparse masking, patch sizes other than 4.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch
import torch.nn as nn

from ..ops_tokens import (HEAD_DIMS, MAE_MAX_CIN, MAE_MAX_GROUPS, MAE_PATCH, MAX_WINDOW_KEYS, linear, mae_keep_count, mae_loss, mae_mask_tokens,
                          mae_window_mask)
from .swin import BasicBlock, _only, norm
from .swinunet import BasicBlockUp, PatchEmbedding, PatchExpanding, _stage_draws

MASK_GROUP = 4          # r of window_masking: r x r neighbouring tokens are masked together (model/swin_mae.py:649)


def sincos_1d(embed_dim: int, pos: np.ndarray) -> np.ndarray:
    """get_1d_sincos_pos_embed_from_grid (model/swin_mae.py:56-74) with omega in float64, what the reference's ``np.float`` was."""
    omega = np.arange(embed_dim // 2, dtype=np.float64)
    omega /= embed_dim / 2.
    omega = 1. / 10000 ** omega
    out = np.einsum('m,d->md', pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_2d(embed_dim: int, grid_size: int) -> np.ndarray:
    """get_2d_sincos_pos_embed without a class token (model/swin_mae.py:27-53): [grid_size^2, embed_dim] float64, the first half of the
    channels from the column coordinate ("w goes first"), the second from the row."""
    if embed_dim % 4:
        raise ValueError(f"sincos_2d: embed_dim {embed_dim} must be a multiple of 4 (sin and cos halves per axis)")
    g = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(g, g), axis=0).reshape([2, 1, grid_size, grid_size])
    return np.concatenate([sincos_1d(embed_dim // 2, grid[0]), sincos_1d(embed_dim // 2, grid[1])], axis=1)


class SwinMAE(nn.Module):
    def __init__(self, img_size: int = 224, patch_size: int = 4, mask_ratio: float = 0.75, in_chans: int = 3, decoder_embed_dim=512,
                 norm_pix_loss=False, depths: tuple = (2, 2, 6, 2), embed_dim: int = 96, num_heads: tuple = (3, 6, 12, 24), window_size: int = 7,
                 qkv_bias: bool = True, mlp_ratio: float = 4., drop_path_rate: float = 0.1, drop_rate: float = 0., attn_drop_rate: float = 0.,
                 norm_layer=None, patch_norm: bool = True):
        super().__init__()
        self._refuse(img_size, patch_size, mask_ratio, in_chans, decoder_embed_dim, depths, embed_dim, num_heads, window_size, drop_rate,
                     attn_drop_rate, norm_layer)
        self.mask_ratio = mask_ratio
        self.img_size = img_size
        self.in_chans = in_chans
        self.num_patches = (img_size // patch_size) ** 2
        self.patch_size = patch_size
        self.norm_pix_loss = norm_pix_loss
        self.num_layers = len(depths)
        self.depths = depths
        self.embed_dim = embed_dim

        self.patch_embed = PatchEmbedding(patch_size=patch_size, in_c=in_chans, embed_dim=embed_dim, norm_layer=norm_layer if patch_norm else None)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_patches, embed_dim), requires_grad=False)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        stage = dict(depths=depths, embed_dim=embed_dim, num_heads=num_heads, drop_path=drop_path_rate, window_size=window_size, mlp_ratio=mlp_ratio,
                     qkv_bias=qkv_bias, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, norm_layer=norm_layer)
        n = self.num_layers
        self.layers = nn.ModuleList([BasicBlock(index=i, patch_merging=i != n - 1, **stage) for i in range(n)])
        self.first_patch_expanding = PatchExpanding(dim=decoder_embed_dim, norm_layer=norm_layer)
        self.layers_up = nn.ModuleList([BasicBlockUp(index=i, patch_expanding=i < n - 2, **stage) for i in range(n - 1)])
        self.norm_up = norm_layer(embed_dim)
        self.decoder_pred = nn.Linear(decoder_embed_dim // 8, patch_size ** 2 * in_chans, bias=True)
        self.initialize_weights()
        self.external_noise = None        # [B, d * d]: replay a given masking noise (tests)
        self.external_draws = None        # drop-path pairs per block in forward order: replay given draws (tests)

    @staticmethod
    def _refuse(img_size, patch_size, mask_ratio, in_chans, decoder_embed_dim, depths, embed_dim, num_heads, window_size, drop_rate, attn_drop_rate,
                norm_layer):
        """Every shape the assembly or a kernel under it cannot run is refused here, by the rule it breaks."""
        _only("SwinMAE", "norm_layer", norm_layer, nn.LayerNorm)
        if len(depths) != 4 or len(num_heads) != 4:
            raise ValueError(f"SwinMAE: depths {tuple(depths)} / num_heads {tuple(num_heads)} must have four stages: decoder_pred takes "
                             f"decoder_embed_dim // 8 channels, which is the decoder's last width only after three patch expandings")
        if decoder_embed_dim != 8 * embed_dim:
            raise ValueError(f"SwinMAE: decoder_embed_dim = {decoder_embed_dim} must be 8 * embed_dim = {8 * embed_dim}: the first patch expanding "
                             f"takes the last encoder stage's channels")
        if patch_size != MAE_PATCH:
            raise ValueError(f"SwinMAE: patch_size = {patch_size} is not built; the loss kernel reads {MAE_PATCH} x {MAE_PATCH} patches")
        if not 1 <= in_chans <= MAE_MAX_CIN:
            raise ValueError(f"SwinMAE: in_chans = {in_chans} is not built; the loss kernel takes 1 to {MAE_MAX_CIN} image channels")
        if not 0.0 < mask_ratio < 1.0:
            raise ValueError(f"SwinMAE: mask_ratio = {mask_ratio} must be in (0, 1)")
        if drop_rate != 0.0 or attn_drop_rate != 0.0:
            raise ValueError(f"SwinMAE: drop_rate = {drop_rate} / attn_drop_rate = {attn_drop_rate}: dropout inside the blocks is not built for this "
                             f"network (the reference's factory sets both to 0)")
        if img_size < patch_size or img_size % patch_size:
            raise ValueError(f"SwinMAE: img_size = {img_size} must be a positive multiple of the patch size {patch_size}")
        side = img_size // patch_size
        if side % MASK_GROUP:
            raise ValueError(f"SwinMAE: the token side {side} (img_size {img_size} / patch {patch_size}) must be divisible by the masking group "
                             f"r = {MASK_GROUP}")
        if (side // MASK_GROUP) ** 2 > MAE_MAX_GROUPS:
            raise ValueError(f"SwinMAE: {side // MASK_GROUP} x {side // MASK_GROUP} masking groups; the mask kernel ranks at most {MAE_MAX_GROUPS}")
        if window_size < 1 or window_size * window_size > MAX_WINDOW_KEYS:
            raise ValueError(f"SwinMAE: a {window_size} x {window_size} window has {window_size ** 2} keys; the window kernels take at most "
                             f"{MAX_WINDOW_KEYS} keys (window <= 8)")
        for i in range(4):
            if side % 2 ** i or (side // 2 ** i) % window_size:
                raise ValueError(f"SwinMAE: stage {i} has a token side of {side} / {2 ** i}, which must be a whole number divisible by the window "
                                 f"{window_size}")
            dim = embed_dim * 2 ** i
            if num_heads[i] < 1 or dim % num_heads[i] or dim // num_heads[i] not in HEAD_DIMS:
                raise ValueError(f"SwinMAE: stage {i} has head dim {dim}/{num_heads[i]}; the HIP attention kernels exist for head dims {HEAD_DIMS}")

    def initialize_weights(self):
        pos_embed = sincos_2d(self.pos_embed.shape[-1], int(self.num_patches ** .5))
        self.pos_embed.data.copy_(torch.from_numpy(pos_embed).float().unsqueeze(0))
        torch.nn.init.normal_(self.mask_token, std=.02)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            torch.nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---- the reference's reshapes (off the training path) ----
    def patchify(self, imgs):
        """imgs [N, C, H, W] -> [N, L, p^2 C], channel order (p, q, c)."""
        p = self.patch_size
        if imgs.shape[2] != imgs.shape[3] or imgs.shape[2] % p:
            raise ValueError(f"patchify: images {tuple(imgs.shape)} must be square with a side divisible by the patch {p}")
        h = w = imgs.shape[2] // p
        x = imgs.reshape(imgs.shape[0], self.in_chans, h, p, w, p)
        return x.permute(0, 2, 4, 3, 5, 1).reshape(imgs.shape[0], h * w, p ** 2 * self.in_chans)

    def unpatchify(self, x):
        """x [N, L, p^2 C] -> [N, C, H, W]."""
        p = self.patch_size
        h = w = int(x.shape[1] ** .5)
        if h * w != x.shape[1]:
            raise ValueError(f"unpatchify: {x.shape[1]} tokens are not a square map")
        x = x.reshape(x.shape[0], h, w, p, p, self.in_chans)
        return x.permute(0, 5, 1, 3, 2, 4).reshape(x.shape[0], self.in_chans, h * p, h * p)

    # ---- masking ----
    def keep_count(self, side: int) -> int:
        return mae_keep_count(side // MASK_GROUP, self.mask_ratio)

    def masked_per_image(self, side: int) -> int:
        """Ones in every row of the mask: L - n_keep r^2, known on the host."""
        return side * side - self.keep_count(side) * MASK_GROUP ** 2

    def window_masking(self, x: torch.Tensor, r: int = MASK_GROUP):
        """x [B, S, S, C] -> (x with the masked tokens replaced by ``mask_token``, uint8 mask [B, S * S], 1 = removed)."""
        B, S = x.shape[0], x.shape[1]
        d = S // r
        if self.external_noise is not None:
            noise = self.external_noise.to(x.device).float()
            if tuple(noise.shape) != (B, d * d):
                raise ValueError(f"SwinMAE: external_noise {tuple(noise.shape)} must be [B, d * d] = [{B}, {d * d}]")
        else:
            noise = torch.rand(B, d * d, device=x.device)
        mask = mae_window_mask(noise, S, r, mae_keep_count(d, self.mask_ratio))
        return mae_mask_tokens(x, mask, self.mask_token), mask

    # ---- the forward passes ----
    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("hpfg_amd.SwinMAE runs on the GPU only: its masking / LayerNorm / window-attention kernels have no CPU fallback")
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.in_chans, self.img_size, self.img_size):
            raise ValueError(f"SwinMAE: input {tuple(x.shape)} must be [B, {self.in_chans}, {self.img_size}, {self.img_size}] (the network was built "
                             f"and checked for that size)")

    def forward_encoder(self, x):
        self._check_input(x)
        x = self.patch_embed(x)
        x, mask = self.window_masking(x)
        per, _ = _stage_draws(self.external_draws, self.layers)
        for i, layer in enumerate(self.layers):
            x = layer(x, draws=per[i])
        return x, mask

    def forward_decoder(self, x):
        n_enc = sum(len(layer.blocks) for layer in self.layers)
        per, _ = _stage_draws(None if self.external_draws is None else self.external_draws[n_enc:], self.layers_up)
        x = self.first_patch_expanding(x)
        for i, layer in enumerate(self.layers_up):
            x = layer(x, draws=per[i])
        x = norm(x, self.norm_up)
        x = linear(x, self.decoder_pred.weight, self.decoder_pred.bias)
        return x.reshape(x.shape[0], -1, x.shape[-1])

    def forward_loss(self, imgs, pred, mask, n_masked: int = None):
        """mean over masked tokens of the per-patch mean squared error (model/swin_mae.py:775-791), honouring ``norm_pix_loss``.  n_masked: the
        mask's number of ones when the caller knows it (``masked_per_image`` times the batch for a mask this network drew); None counts them on
        the device and reads the count back, the one synchronisation on this path."""
        if n_masked is None:
            n_masked = int(mask.sum())
        if n_masked <= 0:
            raise ValueError("SwinMAE.forward_loss: the mask removes no token (the reference divides by zero here)")
        return mae_loss(pred, imgs, mask, 1.0 / (self.patch_size ** 2 * self.in_chans * n_masked), self.norm_pix_loss)

    def reconstruction_loss(self, x, with_parts: bool = False):
        """The driver's loss ``mean((pred_img - img)^2 * mask_img) / mask_ratio`` (2022_12_CVPR_Swin-MAE.py:112) without either image: a 0-dim
        device tensor; with_parts also returns (pred [B, L, 16 Cin], mask uint8 [B, L])."""
        latent, mask = self.forward_encoder(x)
        pred = self.forward_decoder(latent)
        loss = mae_loss(pred, x, mask, 1.0 / (x.numel() * self.mask_ratio))
        return (loss, pred, mask) if with_parts else loss

    def forward(self, x):
        """(pred_img [B, C, H, W], mask_img [B, C, H, W] float, 1 = removed), as the reference returns them."""
        latent, mask = self.forward_encoder(x)
        pred = self.forward_decoder(latent)
        mask_img = self.unpatchify(mask.to(pred.dtype).unsqueeze(-1).repeat(1, 1, self.patch_size ** 2 * self.in_chans))
        return self.unpatchify(pred), mask_img

    def bump_graph_seed(self):
        """GraphedStep hook: nothing to do -- the masking noise and the drop-path draws come from the torch device generator, whose state a
        captured graph advances by itself."""


def swin_mae(in_channels=3, **kwargs):
    return SwinMAE(img_size=224, patch_size=4, in_chans=in_channels, decoder_embed_dim=768, depths=(2, 2, 2, 2), embed_dim=96,
                   num_heads=(3, 6, 12, 24), window_size=7, qkv_bias=True, mlp_ratio=4, drop_path_rate=0.1, drop_rate=0, attn_drop_rate=0,
                   norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
