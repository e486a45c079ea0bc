"""Writes the Swin-MAE fixtures from the reference's own model/swin_mae.py, loaded by path from its checkout -- arrays, seeds, shapes and
SHA-256 hashes only:

  tests/golden/swinmae.json        seeds and, per case, keys, shapes and SHA-256 of every state_dict tensor right after the seeded
                                   construction: "mae224" = swin_mae(in_channels=1, mask_ratio=0.5) after torch.manual_seed(1), "net" = the
                                   small network below.  No weights are stored anywhere: the tests rebuild them from the seed and the hashes
                                   prove the seeded init equal to the reference's.
  tests/golden/swinmae_net.npz     "net": SwinMAE(img_size=128, in_chans=1, mask_ratio=0.5, decoder_embed_dim=256, depths=(2, 2, 2, 2),
                                   embed_dim=32, num_heads=(1, 2, 4, 8), window_size=4, mlp_ratio=1, drop_path_rate=0.2, norm eps 1e-6) in
                                   train mode on 2 x 1 x 128 x 128 (token sides 32 / 16 / 8 / 4, d = 8, 32 of 64 groups kept): x, noise
                                   [B, 64], draws [blocks, 2, B] (zeros where a block has drop-path 0 and draws nothing), mask [B, 1024]
                                   uint8, pred [B, 1024, 16], loss_driver (2022_12_CVPR_Swin-MAE.py:112), loss_model / loss_model_norm_pix
                                   (forward_loss with norm_pix_loss off / on), and the driver loss's gradients grad.<name> of mask_token,
                                   patch_embed.proj.weight, decoder_pred.weight / .bias and the first block's attn.qkv.weight of every
                                   encoder stage.  The widest of those (768 x 256, stage 3) would not fit the size limit of a committed
                                   file beside x and pred, so it is stored as grad_rows4.<name>: every fourth row (rows of q, k and v of
                                   every head are among them).
  tests/golden/trace_swinmae.npz   three iterations of that network with torch.optim.AdamW(lr 1e-4, weight_decay 0.05) on the same x:
                                   noise [3, B, 64] and draws [3, blocks, 2, B] per iteration, loss [3], the final mask_token.

The reference file uses np.float / np.int, which numpy 2 removed: this process sets ``np.float = float; np.int = int`` before loading it
(np.float was an alias of the float64 Python float).  Every ``torch.rand`` result is recorded in call order -- per forward the masking noise
first, then two drop-path draws per block whose rate is not 0.

Run where the reference checkout is, from the repository root:  python -m tools.make_golden_swinmae   (HPFG_REFERENCE overrides its place)
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.make_golden_swin import OUT, save          # noqa: E402
from tools.make_golden_swinunet import sd_meta          # noqa: E402

SEEDS = {"mae224": 1, "net": 31, "data": 2026, "forward": 9, "trace": 10}
NET = dict(img_size=128, in_chans=1, mask_ratio=0.5, decoder_embed_dim=256, depths=(2, 2, 2, 2), embed_dim=32, num_heads=(1, 2, 4, 8), window_size=4,
           mlp_ratio=1, drop_path_rate=0.2)
GRADS = ("mask_token", "patch_embed.proj.weight", "decoder_pred.weight", "decoder_pred.bias", "layers.0.blocks.0.attn.qkv.weight",
         "layers.1.blocks.0.attn.qkv.weight", "layers.2.blocks.0.attn.qkv.weight")
GRADS_ROWS4 = ("layers.3.blocks.0.attn.qkv.weight",)


def load_mae():
    from oracle.make_golden import REF
    path = os.path.join(os.environ.get("HPFG_REFERENCE", REF), "model", "swin_mae.py")
    if not os.path.exists(path):
        sys.exit(f"make_golden_swinmae: {path} not found -- this tool needs the reference checkout (set HPFG_REFERENCE); nothing written")
    np.float, np.int = float, int          # removed in numpy 2; the reference's table and index code still name them
    spec = importlib.util.spec_from_file_location("ref_swin_mae", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class RandLog:
    """torch.rand with every result kept, in call order."""

    def __init__(self):
        self.calls, self._rand = [], torch.rand

    def __enter__(self):
        def rand(*a, **k):
            r = self._rand(*a, **k)
            self.calls.append(r.detach().clone())
            return r
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self._rand


def split_draws(R, net, calls, B):
    """(noise [B, d * d], draws [blocks, 2, B]) from one forward's torch.rand calls."""
    blocks = [m for _, m in net.named_modules() if isinstance(m, R.SwinTransformerBlock)]
    noise, rest = calls[0], calls[1:]
    draws = np.zeros((len(blocks), 2, B), dtype=np.float32)
    k = 0
    for i, b in enumerate(blocks):
        if isinstance(b.drop_path, R.DropPath) and b.drop_path.drop_prob > 0.:
            draws[i, 0], draws[i, 1] = rest[k].reshape(B).numpy(), rest[k + 1].reshape(B).numpy()
            k += 2
    assert k == len(rest), f"{len(rest)} draws recorded, {k} expected"
    return noise.numpy(), draws


def driver_loss(net, x):
    """2022_12_CVPR_Swin-MAE.py:109-112 with one model call; also the pieces the fixtures keep."""
    latent, mask = net.forward_encoder(x)
    pred = net.forward_decoder(latent)
    mask_img = net.unpatchify(mask.unsqueeze(-1).repeat(1, 1, net.patch_embed.patch_size ** 2 * net.in_chans))
    loss = torch.mean((net.unpatchify(pred) - x) ** 2 * mask_img) / net.mask_ratio
    return loss, pred, mask


def main():
    torch.set_num_threads(4)
    R = load_mae()
    norm = partial(nn.LayerNorm, eps=1e-6)
    meta = {"seeds": SEEDS, "net_kwargs": {k: (list(v) if isinstance(v, tuple) else v) for k, v in NET.items()}, "norm_eps": 1e-6}

    torch.manual_seed(SEEDS["mae224"])
    meta["mae224"] = sd_meta(R.swin_mae(in_channels=1, mask_ratio=0.5).state_dict())

    torch.manual_seed(SEEDS["net"])
    net = R.SwinMAE(norm_layer=norm, **NET).train()
    meta["net"] = sd_meta(net.state_dict())
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(2, 1, 128, 128, generator=torch.Generator().manual_seed(SEEDS["data"]))
    B = x.shape[0]

    # ---- net: one forward + backward of the driver's loss ----
    torch.manual_seed(SEEDS["forward"])
    with RandLog() as log:
        loss, pred, mask = driver_loss(net, x)
    noise, draws = split_draws(R, net, log.calls, B)
    loss.backward()
    assert noise.shape == (B, 64) and mask.shape == (B, 1024) and int(mask.sum()) == B * 512
    assert all(len(np.unique(row)) == row.size for row in noise), "no two equal noise values inside an image"
    assert (draws != 0).any(axis=(1, 2)).tolist() == [False] + [True] * 11 + [False, True], "blocks 0 and 12 have drop-path 0"
    out = {"x": x.numpy(), "noise": noise, "draws": draws, "mask": mask.numpy().astype(np.uint8), "pred": pred.detach().numpy(),
           "loss_driver": np.float32(loss.item())}
    with torch.no_grad():
        for name, flag in (("loss_model", False), ("loss_model_norm_pix", True)):
            net.norm_pix_loss = flag
            out[name] = np.float32(net.forward_loss(x, pred, mask).item())
        net.norm_pix_loss = False
    grads = dict(net.named_parameters())
    for k in GRADS:
        out[f"grad.{k}"] = grads[k].grad.numpy().copy()
    for k in GRADS_ROWS4:
        out[f"grad_rows4.{k}"] = grads[k].grad.numpy()[::4].copy()
    save("swinmae_net.npz", out)

    # ---- trace: three AdamW iterations from the same initial weights ----
    net.load_state_dict(init)
    net.zero_grad(set_to_none=True)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.05)
    torch.manual_seed(SEEDS["trace"])
    tr = {"noise": [], "draws": [], "loss": []}
    for _ in range(3):
        with RandLog() as log:
            loss, _, _ = driver_loss(net, x)
        n_, d_ = split_draws(R, net, log.calls, B)
        opt.zero_grad()
        loss.backward()
        opt.step()
        tr["noise"].append(n_)
        tr["draws"].append(d_)
        tr["loss"].append(np.float32(loss.item()))
    save("trace_swinmae.npz", {"noise": np.stack(tr["noise"]), "draws": np.stack(tr["draws"]), "loss": np.array(tr["loss"], dtype=np.float32),
                               "mask_token": net.mask_token.detach().numpy().copy()})

    path = os.path.join(OUT, "swinmae.json")
    with open(path, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=False)
    assert os.path.getsize(path) <= 1 << 20
    print(f"swinmae.json written: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
