"""Writes the Swin-UNet fixtures from the reference's own model/swinunet.py, loaded by path from its checkout -- arrays and a JSON of names,
shapes and hashes only:

  tests/golden/swinunet_dropblock.npz   "dropblock": SwinTransformerBlock(32, 1, 7, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3) in train
                                        mode on 4 x 7 x 7 x 32.  Its four nn.Dropout modules are swapped for a recording one (same law:
                                        x * mask / (1 - p)), so the masks are stored: mask.attn.attn_drop in the layout of the reference's attn
                                        tensor [B nW, heads, L, L], mask.attn.proj_drop transformed to map order (window reverse + roll
                                        back), mask.mlp.drop1 / mask.mlp.drop2 as they are; draws [2, B] the drop-path draws.
  tests/golden/swinunet_net2.npz        "net2": SwinUnet(in_chans=1, num_classes=4, embed_dim=32, depths=(2, 2), num_heads=(1, 2), mlp_ratio=1,
                                        no dropout, drop_path_rate=0.2, norm eps 1e-6) in train mode on 2 x 1 x 56 x 56: x, y, dy, dx, every
                                        parameter gradient, draws [blocks, 2, B] (zeros where a block has drop-path 0 and draws nothing).
  tests/golden/swinunet_net3.npz        "net3": the same with depths (2, 2, 2), heads (1, 2, 4) on 2 x 1 x 112 x 112 in eval mode (reaches a
                                        BasicBlockUp with an upsample): x, y.
  tests/golden/swinunet.json            seeds of the cases and, per case, keys, shapes and SHA-256 of every state_dict tensor right after the
                                        seeded construction ("plus224": get_swinunet_plus(224, in_channels=1, num_classes=4) after
                                        torch.manual_seed(1)).  net2 / net3 store no weights: the test rebuilds them from the seed and the
                                        hashes prove the seeded init equal to the reference's.

Run where the reference checkout is, from the repository root:  python -m tools.make_golden_swinunet   (HPFG_REFERENCE overrides its place)
"""
from __future__ import annotations

import hashlib
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

from tools.make_golden_swin import OUT, load_swin, save          # noqa: E402

SEEDS = {"dropblock": 21, "net2": 22, "net3": 23, "plus224": 1}
NET = dict(in_chans=1, num_classes=4, embed_dim=32, window_size=7, mlp_ratio=1., drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2)


class RecordingDropout(nn.Module):
    """nn.Dropout(p) in train mode with its keep mask kept: y = x * mask / (1 - p), mask = rand >= p."""

    def __init__(self, p):
        super().__init__()
        self.p, self.mask = p, None

    def forward(self, x):
        self.mask = torch.rand_like(x) >= self.p
        return x * self.mask / (1.0 - self.p)


class RecordingDropPath(nn.Module):
    """DropPath of the reference (x / keep * floor(keep + U), U one uniform per sample) with its draws kept, in call order."""

    def __init__(self, p):
        super().__init__()
        self.p, self.draws = p, []

    def forward(self, x):
        if self.p == 0. or not self.training:
            return x
        u = torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype)
        self.draws.append(u.reshape(-1).clone())
        return x.div(1 - self.p) * (1 - self.p + u).floor()


def swap(net, S):
    """nn.Dropout -> RecordingDropout, the reference's DropPath -> RecordingDropPath, in place; returns {module path: recorder}."""
    rec = {}
    for name, m in list(net.named_modules()):
        for child_name, child in list(m.named_children()):
            path = f"{name}.{child_name}" if name else child_name
            if isinstance(child, nn.Dropout):
                rec[path] = RecordingDropout(child.p)
                setattr(m, child_name, rec[path])
            elif isinstance(child, S.DropPath):
                rec[path] = RecordingDropPath(child.drop_prob)
                setattr(m, child_name, rec[path])
    return rec


def sd_meta(sd):
    return {k: {"shape": list(v.shape), "dtype": str(v.dtype).split(".")[1], "sha256": hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()}
            for k, v in sd.items()}


def main():
    torch.set_num_threads(4)
    S = load_swin()
    meta = {"seeds": SEEDS, "net": {k: v for k, v in NET.items()}, "norm_eps": 1e-6}
    g = torch.Generator().manual_seed(2025)

    # ---- dropblock ----
    torch.manual_seed(SEEDS["dropblock"])
    blk = S.SwinTransformerBlock(32, 1, 7, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3).train()
    with torch.no_grad():          # the initial table (std 0.02) would leave the bias path almost untested
        blk.attn.relative_position_bias_table.mul_(25.0)
    rec = swap(blk, S)
    x, dy = torch.randn(4, 7, 7, 32, generator=g), torch.randn(4, 7, 7, 32, generator=g)
    out = {f"dropblock.sd.{k}": v.detach().numpy().copy() for k, v in blk.state_dict().items()}
    torch.manual_seed(8)
    xr = x.clone().requires_grad_(True)
    y = blk(xr)
    y.backward(dy)
    out.update({"dropblock.x": x.numpy(), "dropblock.y": y.detach().numpy(), "dropblock.dy": dy.numpy(), "dropblock.dx": xr.grad.numpy()})
    for k, p in blk.named_parameters():
        out[f"dropblock.grad.{k}"] = p.grad.numpy().copy()
    out["dropblock.draws"] = torch.stack(rec["drop_path"].draws).numpy()
    assert out["dropblock.draws"].shape == (2, 4)
    kept = np.floor(0.7 + out["dropblock.draws"])
    assert 0 < kept.sum() < 8, "choose a draw seed that drops some samples and keeps others"
    s = blk.attn.shift_size
    pm = rec["attn.proj_drop"].mask          # [Bn, Mh, Mw, C] in the rolled, partitioned order; one 7 x 7 window per image here
    assert pm.shape == (4, 7, 7, 32)
    out["dropblock.mask.attn.proj_drop"] = torch.roll(pm, (s, s), (1, 2)).numpy().astype(np.uint8)
    assert rec["attn.attn_drop"].mask.shape == (4, 1, 49, 49)
    out["dropblock.mask.attn.attn_drop"] = rec["attn.attn_drop"].mask.numpy().astype(np.uint8)
    out["dropblock.mask.mlp.drop1"] = rec["mlp.drop1"].mask.numpy().astype(np.uint8)
    out["dropblock.mask.mlp.drop2"] = rec["mlp.drop2"].mask.numpy().astype(np.uint8)
    save("swinunet_dropblock.npz", out)

    # ---- net2: train mode, drop-path only ----
    norm = partial(nn.LayerNorm, eps=1e-6)
    torch.manual_seed(SEEDS["net2"])
    net = S.SwinUnet(depths=(2, 2), num_heads=(1, 2), norm_layer=norm, **NET).train()
    meta["net2"] = sd_meta(net.state_dict())
    rec = swap(net, S)
    blocks = [f"encoder.layers.{i}.blocks.{j}" for i in range(2) for j in range(2)] + [f"decoder.layers_up.0.blocks.{j}" for j in range(2)]
    x, dy = torch.randn(2, 1, 56, 56, generator=g), torch.randn(2, 4, 56, 56, generator=g)
    torch.manual_seed(6)
    xr = x.clone().requires_grad_(True)
    y = net(xr)
    y.backward(dy)
    draws = np.zeros((len(blocks), 2, 2), dtype=np.float32)
    for i, b in enumerate(blocks):
        r = rec.get(b + ".drop_path")
        if r is not None and r.draws:
            draws[i] = torch.stack(r.draws).numpy()
    assert (draws != 0).any(axis=(1, 2)).tolist() == [False, True, True, True, False, True]
    out = {"net2.x": x.numpy(), "net2.y": y.detach().numpy(), "net2.dy": dy.numpy(), "net2.dx": xr.grad.numpy(), "net2.draws": draws}
    for k, p in net.named_parameters():
        out[f"net2.grad.{k}"] = p.grad.numpy().copy()
    save("swinunet_net2.npz", out)

    # ---- net3: eval mode, three stages ----
    torch.manual_seed(SEEDS["net3"])
    net = S.SwinUnet(depths=(2, 2, 2), num_heads=(1, 2, 4), norm_layer=norm, **NET).eval()
    meta["net3"] = sd_meta(net.state_dict())
    x = torch.randn(2, 1, 112, 112, generator=g)
    with torch.no_grad():
        y = net(x)
    save("swinunet_net3.npz", {"net3.x": x.numpy(), "net3.y": y.numpy()})

    # ---- plus224: the layout and seeded init of the full network ----
    torch.manual_seed(SEEDS["plus224"])
    meta["plus224"] = sd_meta(S.get_swinunet_plus(224, in_channels=1, num_classes=4).state_dict())
    path = os.path.join(OUT, "swinunet.json")
    with open(path, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=False)
    assert os.path.getsize(path) <= 1 << 20
    print(f"swinunet.json written: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
