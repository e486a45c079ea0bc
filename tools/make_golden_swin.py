"""Writes the Swin-block fixtures from the reference's own model/swinunet.py, loaded by path from its checkout -- arrays only, all fp32
(the buffer ``attn.relative_position_index`` stays int64):

  tests/golden/swin_block.npz   SwinTransformerBlock(64, 2, 7, mlp_ratio=1) on a 2 x 14 x 14 x 64 map, unshifted ("plain") and shifted
                                ("shift"), drop-path 0; the two share weights, input and upstream gradient, stored once as plain.sd.* /
                                plain.x / plain.dy
  tests/golden/swin_stage.npz   "droppath": SwinTransformerBlock(32, 1, 7, shift=True, drop_path=0.3) on 4 x 7 x 7 x 32 in train mode with its two
                                uniform draws recorded; "basic": BasicBlock(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2)) on
                                2 x 14 x 14 x 32 in train mode (second block: drop-path 1/30, draws recorded); "init": the state_dict of
                                SwinTransformerBlock(64, 2, 7, shift=True) built right after torch.manual_seed(7)

Per case NAME: NAME.sd.<key> the reference's state_dict, NAME.x input, NAME.y output, NAME.dy upstream gradient, NAME.dx input gradient,
NAME.grad.<parameter> every parameter gradient, NAME.draws [n, B] the drop-path draws in the order the forward takes them.
Two files because no committed file may exceed 1 MiB: four 100 KB activation tensors per full-size block case leave no room for the rest.
(mlp_ratio=1 in the two full-size cases for the same reason; the MLP's width changes no code path.)

Run where the reference checkout is, from the repository root:  python -m tools.make_golden_swin   (HPFG_REFERENCE overrides its place)
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden")
LIMIT = 1 << 20


def load_swin():
    from oracle.make_golden import REF
    path = os.path.join(os.environ.get("HPFG_REFERENCE", REF), "model", "swinunet.py")
    if not os.path.exists(path):
        sys.exit(f"make_golden_swin: {path} not found -- this tool needs the reference checkout (set HPFG_REFERENCE); nothing written")
    spec = importlib.util.spec_from_file_location("ref_swinunet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(name, net, x, dy, draw_seed=None, n_draws=0):
    """forward + backward of the reference module; with draw_seed the forward's DropPath draws (torch.rand((B,1,1,1)) each, nothing else
    draws) are the first n_draws draws after torch.manual_seed(draw_seed), recorded here by drawing them first from the same seed"""
    out = {}
    B = x.shape[0]
    if draw_seed is not None:
        torch.manual_seed(draw_seed)
        out[f"{name}.draws"] = np.stack([torch.rand((B, 1, 1, 1)).reshape(B).numpy() for _ in range(n_draws)])
        torch.manual_seed(draw_seed)
    for k, v in net.state_dict().items():
        out[f"{name}.sd.{k}"] = v.detach().numpy().copy()
    xr = x.clone().requires_grad_(True)
    y = net(xr)
    if draw_seed is not None:          # the forward consumed exactly the recorded draws
        probe = torch.rand(1)
        torch.manual_seed(draw_seed)
        for _ in range(n_draws):
            torch.rand((B, 1, 1, 1))
        assert torch.equal(probe, torch.rand(1)), f"{name}: the forward did not take {n_draws} draws"
    y.backward(dy)
    out.update({f"{name}.x": x.numpy(), f"{name}.y": y.detach().numpy(), f"{name}.dy": dy.numpy(), f"{name}.dx": xr.grad.numpy()})
    for k, p in net.named_parameters():
        out[f"{name}.grad.{k}"] = p.grad.numpy().copy()
    assert all(v.dtype in (np.float32, np.int64) for v in out.values())
    return out


def save(fname, arrays):
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= LIMIT, f"{fname}: {size} bytes exceed the 1 MiB limit of a committed file"
    print(f"{fname} written: {len(arrays)} arrays, {size} bytes")


def main():
    torch.set_num_threads(4)
    S = load_swin()
    g = torch.Generator().manual_seed(2024)
    x = torch.randn(2, 14, 14, 64, generator=g)
    dy = torch.randn(2, 14, 14, 64, generator=g)
    blocks = {}
    for name, shift in (("plain", False), ("shift", True)):
        torch.manual_seed(11)
        net = S.SwinTransformerBlock(64, 2, 7, shift=shift, mlp_ratio=1.0).train()
        with torch.no_grad():          # the initial table (std 0.02) would leave the bias path almost untested
            net.attn.relative_position_bias_table.mul_(25.0)
        blocks.update(run_case(name, net, x, dy))
    for k in [k for k in blocks if k.startswith("shift.sd.") or k in ("shift.x", "shift.dy")]:          # stored once, under "plain"
        assert np.array_equal(blocks[k], blocks["plain" + k[5:]])
        del blocks[k]
    save("swin_block.npz", blocks)

    stage = {}
    torch.manual_seed(12)
    net = S.SwinTransformerBlock(32, 1, 7, shift=True, drop_path=0.3).train()
    with torch.no_grad():
        net.attn.relative_position_bias_table.mul_(25.0)
    xs, dys = torch.randn(4, 7, 7, 32, generator=g), torch.randn(4, 7, 7, 32, generator=g)
    case = run_case("droppath", net, xs, dys, draw_seed=5, n_draws=2)
    kept = np.floor(0.7 + case["droppath.draws"])
    assert 0 < kept[0].sum() < 4 or 0 < kept[1].sum() < 4, "choose a draw seed that drops some samples and keeps others"
    stage.update(case)
    torch.manual_seed(13)
    net = S.BasicBlock(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2)).train()
    with torch.no_grad():
        for blk in net.blocks:
            blk.attn.relative_position_bias_table.mul_(25.0)
    xb, dyb = torch.randn(2, 14, 14, 32, generator=g), torch.randn(2, 7, 7, 64, generator=g)
    stage.update(run_case("basic", net, xb, dyb, draw_seed=6, n_draws=2))          # block 0 has drop-path 0 (no draw), block 1 draws twice
    torch.manual_seed(7)
    for k, v in S.SwinTransformerBlock(64, 2, 7, shift=True).state_dict().items():
        stage[f"init.sd.{k}"] = v.detach().numpy().copy()
    save("swin_stage.npz", stage)


if __name__ == "__main__":
    main()
