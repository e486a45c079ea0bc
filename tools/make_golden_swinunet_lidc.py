"""Writes the fixtures of the LIDC Swin-UNet (patch 2, window 3 / 4) from the reference's own model/swinunet_LIDC.py, loaded by path from its
checkout -- arrays and a JSON of names, shapes and hashes only:

  tests/golden/swinunet_lidc.json           seeds and, per case, keys, shapes and SHA-256 of every state_dict tensor right after the seeded
                                            construction: "lidc96" = get_swinunet_LIDC(96, in_channels=3, num_classes=2), "lidc64" the same at
                                            64, "net2" / "net3" the small networks below; "opt": the optimizer recipe of the trace.
  tests/golden/swinunet_lidc_dropblock.npz  "dropblock": SwinTransformerBlock(32, 1, 3, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3) in
                                            train mode on 4 x 6 x 6 x 32 (four 3 x 3 windows per image), in the layout of the "dropblock" case
                                            of tools/make_golden_swinunet.py: mask.attn.attn_drop as the reference's attn tensor
                                            [B nW, heads, L, L], mask.attn.proj_drop in map order (window reverse + roll back), draws [2, B].
  tests/golden/swinunet_lidc_net2.npz       "net2": SwinUnet(patch_size=2, in_chans=3, num_classes=2, embed_dim=32, window_size=3,
                                            depths=(2, 2), num_heads=(1, 2), mlp_ratio=1, no dropout, drop_path_rate=0.2, norm eps 1e-6) in
                                            train mode on 2 x 3 x 24 x 24 (token maps 12 x 12: 16 windows per image, and 6 x 6: 4 windows):
                                            x, y, dy, dx, every parameter gradient, draws [blocks, 2, B].
  tests/golden/swinunet_lidc_net3.npz       "net3": the same with window 4, depths (2, 2, 2), heads (1, 2, 4) on 2 x 3 x 32 x 32 in eval mode
                                            (maps 16 / 8 / 4: 16, 4 and 1 windows; the last is window == map): x, y.
  tests/golden/trace_swinunet_lidc.npz      three iterations of the supervised law (sup_ACDC.py:83-93: forward, Med_Sup_Loss, zero_grad,
                                            backward, optimizer.step, lr_scheduler.step) on the net2 network and input with
                                            torch.optim.AdamW and the reference's CosineWarmupLR_Scheduler ("opt" of the JSON): label, the
                                            drop-path draws per iteration [3, blocks, 2, B], the loss per iteration and the eval-mode logits
                                            after the third update.  net2 has no nn.Dropout, so there are no masks to record.

Run where the reference checkout is, from the repository root:  python -m tools.make_golden_swinunet_lidc   (HPFG_REFERENCE overrides its place)
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
from tools.make_golden_swinunet import sd_meta, swap          # noqa: E402

SEEDS = {"dropblock": 41, "net2": 42, "net3": 43, "lidc96": 1, "lidc64": 2, "data": 2027, "trace": 12}
NET = dict(patch_size=2, in_chans=3, num_classes=2, embed_dim=32, mlp_ratio=1., drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2)
OPT = dict(opt="adamW", lr=5e-4, weight_decay=0.05, momentum=0.9, sched="cosine", warmup_epochs=1, warmup_lr=1e-5, min_lr=1e-6, total_itrs=40,
           step_size=4)          # a four-iteration warm-up: the rate changes in every iteration of the trace
NET2_BLOCKS = [f"encoder.layers.{i}.blocks.{j}" for i in range(2) for j in range(2)] + [f"decoder.layers_up.0.blocks.{j}" for j in range(2)]


def load_lidc():
    from oracle.make_golden import REF
    path = os.path.join(os.environ.get("HPFG_REFERENCE", REF), "model", "swinunet_LIDC.py")
    if not os.path.exists(path):
        sys.exit(f"make_golden_swinunet_lidc: {path} not found -- this tool needs the reference checkout (set HPFG_REFERENCE); nothing written")
    spec = importlib.util.spec_from_file_location("ref_swinunet_lidc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def block_draws(rec, blocks, B):
    """[blocks, 2, B] drop-path draws of one forward (zeros where a block has drop-path 0 and draws nothing); empties the recorders."""
    draws = np.zeros((len(blocks), 2, B), dtype=np.float32)
    for i, b in enumerate(blocks):
        r = rec.get(b + ".drop_path")
        if r is not None and r.draws:
            draws[i] = torch.stack(r.draws).numpy()
            r.draws.clear()
    return draws


def main():
    torch.set_num_threads(4)
    S = load_lidc()
    from oracle.make_golden import load_reference
    R = load_reference()
    meta = {"seeds": SEEDS, "net": dict(NET), "norm_eps": 1e-6, "opt": OPT}
    g = torch.Generator().manual_seed(SEEDS["data"])
    norm = partial(nn.LayerNorm, eps=1e-6)

    # ---- dropblock at window 3: four windows per image ----
    torch.manual_seed(SEEDS["dropblock"])
    blk = S.SwinTransformerBlock(32, 1, 3, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3).train()
    with torch.no_grad():          # the initial table (std 0.02) would leave the bias path almost untested
        blk.attn.relative_position_bias_table.mul_(25.0)
    rec = swap(blk, S)
    x, dy = torch.randn(4, 6, 6, 32, generator=g), torch.randn(4, 6, 6, 32, generator=g)
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
    pm = rec["attn.proj_drop"].mask          # [B nW, Mh, Mw, C] in the rolled, partitioned order
    assert s == 1 and pm.shape == (16, 3, 3, 32)
    pm = pm.view(4, 2, 2, 3, 3, 32).permute(0, 1, 3, 2, 4, 5).reshape(4, 6, 6, 32)          # window reverse
    out["dropblock.mask.attn.proj_drop"] = torch.roll(pm, (s, s), (1, 2)).numpy().astype(np.uint8)
    assert rec["attn.attn_drop"].mask.shape == (16, 1, 9, 9)
    out["dropblock.mask.attn.attn_drop"] = rec["attn.attn_drop"].mask.numpy().astype(np.uint8)
    out["dropblock.mask.mlp.drop1"] = rec["mlp.drop1"].mask.numpy().astype(np.uint8)
    out["dropblock.mask.mlp.drop2"] = rec["mlp.drop2"].mask.numpy().astype(np.uint8)
    save("swinunet_lidc_dropblock.npz", out)

    # ---- net2: train mode, drop-path only ----
    torch.manual_seed(SEEDS["net2"])
    net = S.SwinUnet(window_size=3, depths=(2, 2), num_heads=(1, 2), norm_layer=norm, **NET).train()
    meta["net2"] = sd_meta(net.state_dict())
    init = {k: v.clone() for k, v in net.state_dict().items()}
    rec = swap(net, S)
    x, dy = torch.randn(2, 3, 24, 24, generator=g), torch.randn(2, 2, 24, 24, generator=g)
    torch.manual_seed(6)
    xr = x.clone().requires_grad_(True)
    y = net(xr)
    y.backward(dy)
    draws = block_draws(rec, NET2_BLOCKS, 2)
    assert (draws != 0).any(axis=(1, 2)).tolist() == [False, True, True, True, False, True]
    out = {"net2.x": x.numpy(), "net2.y": y.detach().numpy(), "net2.dy": dy.numpy(), "net2.dx": xr.grad.numpy(), "net2.draws": draws}
    for k, p in net.named_parameters():
        out[f"net2.grad.{k}"] = p.grad.numpy().copy()
    save("swinunet_lidc_net2.npz", out)

    # ---- trace: three iterations of the supervised law on net2 ----
    net.load_state_dict(init)
    net.zero_grad(set_to_none=True)
    label = torch.randint(0, 2, (2, 6, 6), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    crit = R.med.Med_Sup_Loss(2)
    opt = torch.optim.AdamW(net.parameters(), lr=OPT["lr"], weight_decay=OPT["weight_decay"])
    sched = R.coslr.CosineWarmupLR_Scheduler(optimizer=opt, base_lr=OPT["lr"], warmup_epochs=OPT["warmup_epochs"], warmup_lr=OPT["warmup_lr"],
                                             final_lr=OPT["min_lr"], iter_per_epoch=OPT["step_size"], num_epochs=OPT["total_itrs"] // OPT["step_size"])
    torch.manual_seed(SEEDS["trace"])
    tr = {"draws": [], "loss": [], "lr": []}
    for _ in range(3):
        tr["lr"].append(np.float32(opt.param_groups[0]["lr"]))
        loss = crit(net(x), label.long())
        tr["draws"].append(block_draws(rec, NET2_BLOCKS, 2))
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        tr["loss"].append(np.float32(loss.item()))
    net.eval()
    with torch.no_grad():
        logits = net(x)
    save("trace_swinunet_lidc.npz", {"label": label.numpy().astype(np.uint8), "draws": np.stack(tr["draws"]), "loss": np.array(tr["loss"], dtype=np.float32),
                                     "lr": np.array(tr["lr"], dtype=np.float32), "logits": logits.numpy()})

    # ---- net3: eval mode, three stages at window 4 ----
    torch.manual_seed(SEEDS["net3"])
    net = S.SwinUnet(window_size=4, depths=(2, 2, 2), num_heads=(1, 2, 4), norm_layer=norm, **NET).eval()
    meta["net3"] = sd_meta(net.state_dict())
    x = torch.randn(2, 3, 32, 32, generator=g)
    with torch.no_grad():
        y = net(x)
    save("swinunet_lidc_net3.npz", {"net3.x": x.numpy(), "net3.y": y.numpy()})

    # ---- the layout and seeded init of the full networks ----
    for case, side in (("lidc96", 96), ("lidc64", 64)):
        torch.manual_seed(SEEDS[case])
        meta[case] = sd_meta(S.get_swinunet_LIDC(side, in_channels=3, num_classes=2).state_dict())
    path = os.path.join(OUT, "swinunet_lidc.json")
    with open(path, "w") as f:
        json.dump(meta, f, indent=0, sort_keys=False)
    assert os.path.getsize(path) <= 1 << 20
    print(f"swinunet_lidc.json written: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
