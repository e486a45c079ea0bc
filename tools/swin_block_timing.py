"""Forward + backward time of one Swin-T stage-1 block (16 x 56 x 56 x 96 tokens, 3 heads, window 7) on one GPU, unshifted and shifted:
hpfg_amd.model.SwinTransformerBlock on the HIP kernels beside the same block written with plain torch ops (roll / rearrange / matmul /
softmax, the formulation of the reference's forward in this tool's own words, fp32, whatever libraries torch dispatches to), same weights,
same input, same GPU.  Both run eagerly: forward, then backward to the input and every parameter.

Method: warm-up, then alternating blocks of steps (HIP block, torch block, HIP block, ...) in one process, device-event time per block,
median (min .. max) over the rounds.  Before timing, the two forms' outputs and input gradients are compared once at the timed size.
Appends to --out (default profiles/swin_block_timing.txt).  Needs a GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SIDE, DIM, HEADS, WINDOW = 16, 56, 96, 3, 7
ROUNDS, BLOCK, WARMUP = 9, 10, 5


def torch_block(net, x):
    """SwinTransformerBlock.forward with torch ops only, reading the module's parameters"""
    import torch
    import torch.nn.functional as F
    a, w, s, h = net.attn, net.attn.window_size, net.attn.shift_size, net.attn.num_heads
    Bx, H, W, C = x.shape
    y = F.layer_norm(x, (C,), net.norm1.weight, net.norm1.bias)
    if s:
        y = torch.roll(y, (-s, -s), (1, 2))
    y = y.view(Bx, H // w, w, W // w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w, C)
    qkv = F.linear(y, a.qkv.weight, a.qkv.bias).view(-1, w * w, 3, h, C // h).permute(2, 0, 3, 1, 4)
    att = (qkv[0] * a.scale) @ qkv[1].transpose(-2, -1)
    att = att + a.relative_position_bias_table[a.relative_position_index.view(-1)].view(w * w, w * w, h).permute(2, 0, 1)[None]
    if s:
        img = torch.zeros(1, H, W, 1, device=x.device)
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
                img[:, hs, ws, :] = cnt
                cnt += 1
        mw = img.view(1, H // w, w, W // w, w, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, w * w)
        m = mw[:, None, :] - mw[:, :, None]
        m = m.masked_fill(m != 0, -100.0)
        att = (att.view(Bx, -1, h, w * w, w * w) + m[None, :, None]).view(-1, h, w * w, w * w)
    y = (att.softmax(-1) @ qkv[2]).transpose(1, 2).reshape(-1, w * w, C)
    y = F.linear(y, a.proj.weight, a.proj.bias)
    y = y.view(Bx, H // w, W // w, w, w, C).permute(0, 1, 3, 2, 4, 5).reshape(Bx, H, W, C)
    if s:
        y = torch.roll(y, (s, s), (1, 2))
    x = x + y
    y = F.layer_norm(x, (C,), net.norm2.weight, net.norm2.bias)
    return x + F.linear(F.gelu(F.linear(y, net.mlp.fc1.weight, net.mlp.fc1.bias)), net.mlp.fc2.weight, net.mlp.fc2.bias)


def main(out):
    import torch
    from hpfg_amd.model import SwinTransformerBlock
    from hpfg_amd.ops_tokens import gemm_math
    if not torch.cuda.is_available():
        raise SystemExit("swin_block_timing: no GPU; nothing measured")
    dev = torch.device("cuda:0")
    lines = ["", f"== one Swin-T stage-1 block, forward + backward, {B} x {SIDE} x {SIDE} x {DIM} tokens, {HEADS} heads, window {WINDOW}; "
                 f"{torch.cuda.get_device_name(0)}",
             f"   eager steps, device-event time per step in ms, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK} steps after {WARMUP} warm-up steps",
             f"   hip = hpfg_amd.model.SwinTransformerBlock (HPFG_MATH={gemm_math()}); torch = the same block in plain torch ops, fp32",
             f"   {'shift':>5} | {'hip, ms':>26} | {'torch, ms':>26} | max |y diff|  max |dx diff|"]
    for shift in (False, True):
        torch.manual_seed(1)
        net = SwinTransformerBlock(DIM, HEADS, WINDOW, shift=shift).to(dev).train()
        g = torch.Generator().manual_seed(2)
        x = torch.randn(B, SIDE, SIDE, DIM, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(B, SIDE, SIDE, DIM, generator=g).to(dev)
        params = [x] + list(net.parameters())

        def step(fn):
            y = fn(x)
            return y, torch.autograd.grad(y, params, dy)

        forms = [lambda t: net(t), lambda t: torch_block(net, t)]
        (ya, ga), (yb, gb) = step(forms[0]), step(forms[1])
        dy_, dx_ = float((ya - yb).detach().abs().max()), float((ga[0] - gb[0]).abs().max())
        del ya, yb, ga, gb
        for f in forms:
            for _ in range(WARMUP):
                step(f)
        torch.cuda.synchronize()
        rows = ([], [])
        for _ in range(ROUNDS):
            for f, r in zip(forms, rows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BLOCK):
                    step(f)
                e1.record()
                e1.synchronize()
                r.append(e0.elapsed_time(e1) / BLOCK)
        fmt = lambda v: f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"          # noqa: E731
        lines.append(f"   {str(shift):>5} | {fmt(rows[0]):>26} | {fmt(rows[1]):>26} | {dy_:.2e}      {dx_:.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_block_timing.txt"))
    main(ap.parse_args().out)
