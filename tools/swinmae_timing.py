"""Times the Swin-MAE pretraining step at the shipped config's size (16 x 1 x 224 x 224, config/swinmae_30k_224x224_ACDC.yaml) on one GPU and
writes profiles/swinmae_timing.txt:

* the step captured by ``GraphedStep``: ms per replay (device events around batches of replays);
* the three kernels of csrc/mae.hip alone, at the step's shapes -- window mask, mask tokens (forward + backward), loss (forward launch + the
  gradient hand-over of its backward): us per call, both replayed from a hipGraph of their own (device time) and launched eagerly (host
  time included), their sum as a share of the step, and the bytes/s they achieve against the bytes they must move (computed from the
  shapes below, not measured);
* a composition of the same three laws from torch device ops (argsort ranks, torch.where under autograd, patchify + masked squared error
  under autograd -- no host round trip either, so the comparison is with the best torch can do, not with the reference's numpy loops), on
  the same device in the same process, the two alternating round by round.

Recorded, not asserted.  Run on a GPU from the repository root:  python -m tools.swinmae_timing [--rounds 5] [--iters 50]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hpfg_amd.model import build_model          # noqa: E402
from hpfg_amd.ops_tokens import mae_keep_count, mae_loss, mae_mask_tokens, mae_window_mask          # noqa: E402
from hpfg_amd.train import GraphedStep, SwinMAEStep          # noqa: E402
from hpfg_amd.utils import loadyaml          # noqa: E402


NOT_CAPTURED = []


def timed(fn, iters):
    """us per call of fn over `iters` calls between two device events (the calls are queued back to back; the events bound the device time)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinmae_timing.txt"))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("swinmae_timing: no GPU -- nothing measured, nothing written")
    dev = torch.device("cuda:0")
    args = loadyaml(os.path.join(ROOT, "config", "swinmae_30k_224x224_ACDC.yaml"))
    args.device = "cuda:0"
    B, Cin, H = int(args.batch_size), int(args.in_channels), int(args.train_crop_size[0])
    S, r, C_, D = H // 4, 4, 96, 16 * Cin
    d, Ltok = S // r, S * S
    n_keep = mae_keep_count(d, args.mask_ratio)
    masked = (Ltok - n_keep * r * r) / Ltok          # fraction of tokens removed

    # ---- the graphed step ----
    torch.manual_seed(args.seed)
    net = build_model(args).to(dev).train()
    st = SwinMAEStep(net, args)
    img = torch.randn(B, Cin, H, H, device=dev)
    st.step(img, 1)
    runner = GraphedStep(st, [img], warmup=0, alias_inputs=True)
    k = [1]

    def replay():
        k[0] += 1
        runner.step([img], k[0])

    for _ in range(5):
        replay()
    torch.cuda.synchronize()

    # ---- the three laws alone, fused and composed from torch ops, on the step's shapes ----
    g = torch.Generator(device=dev).manual_seed(3)
    noise = torch.rand(B, d * d, device=dev, generator=g)
    x = torch.randn(B, S, S, C_, device=dev, generator=g)
    token = torch.randn(1, 1, C_, device=dev, generator=g)
    dy = torch.randn(B, S, S, C_, device=dev, generator=g)
    pred = torch.randn(B, Ltok, D, device=dev, generator=g)
    scale = 1.0 / (img.numel() * args.mask_ratio)
    one = torch.ones((), device=dev)

    def fused_mask():
        return mae_window_mask(noise, S, r, n_keep)

    def torch_mask():
        rank = torch.argsort(torch.argsort(noise, dim=1), dim=1)          # (no ties in uniform noise: the law of the kernel)
        rm = (rank >= n_keep).reshape(B, d, d)
        return rm.repeat_interleave(r, 1).repeat_interleave(r, 2).reshape(B, Ltok).to(torch.uint8)

    mask = fused_mask()
    assert torch.equal(mask, torch_mask())

    def fused_tokens():
        xr, tr = x.detach().requires_grad_(True), token.detach().requires_grad_(True)
        mae_mask_tokens(xr, mask, tr).backward(dy)
        return xr.grad, tr.grad

    def torch_tokens():
        xr, tr = x.detach().requires_grad_(True), token.detach().requires_grad_(True)
        torch.where(mask.reshape(B, S, S, 1).bool(), tr.reshape(1, 1, 1, C_), xr).backward(dy)
        return xr.grad, tr.grad

    def fused_loss():
        pr = pred.detach().requires_grad_(True)
        loss = mae_loss(pr, img, mask, scale)
        loss.backward(one)
        return loss.detach(), pr.grad

    def torch_loss():
        pr = pred.detach().requires_grad_(True)
        target = img.reshape(B, Cin, S, 4, S, 4).permute(0, 2, 4, 3, 5, 1).reshape(B, Ltok, D)
        loss = (((pr - target) ** 2).sum(-1) * mask).sum() * scale
        loss.backward(one)
        return loss.detach(), pr.grad

    fx, ft = fused_tokens(), torch_tokens()
    fl, tl = fused_loss(), torch_loss()
    agree = [torch.equal(fx[0], ft[0]), float((fx[1] - ft[1]).abs().max()), float((fl[0] - tl[0]).abs()), float((fl[1] - tl[1]).abs().max())]

    pairs = [("window mask", fused_mask, torch_mask), ("mask tokens fwd+bwd", fused_tokens, torch_tokens), ("loss fwd+bwd", fused_loss, torch_loss)]
    for _, a, b in pairs:
        for f in (a, b):
            for _ in range(5):
                f()
    torch.cuda.synchronize()
    replays = {name: (captured(a), captured(b)) for name, a, b in pairs}          # each law as a hipGraph of its own: device time without the host
    eager = {name: ([], []) for name, _, _ in pairs}
    graph = {name: ([], []) for name, _, _ in pairs}
    step_ms = []
    for _ in range(o.rounds):          # fused, torch, fused, torch ... and the step, round by round
        for name, a, b in pairs:
            eager[name][0].append(timed(a, o.iters))
            eager[name][1].append(timed(b, o.iters))
            ra, rb = replays[name]
            graph[name][0].append(timed(ra, o.iters))
            graph[name][1].append(timed(rb, o.iters))
        step_ms.append(timed(replay, o.iters) / 1e3)

    # bytes each fused law must move (fp32 = 4 bytes; a masked row of x / a kept row of pred and its pixels are not read)
    need = {
        "window mask": B * d * d * 4 + B * Ltok,
        "mask tokens fwd+bwd": int(B * Ltok * (C_ * 4 * ((1 - masked) + 1) + 1) + B * Ltok * (C_ * 4 * 2 + 1) + C_ * 4 * 2),
        "loss fwd+bwd": int(B * Ltok * (D * 4 * masked * 2 + D * 4 + 1) + B * Ltok * D * 4 * 2),
    }
    head = (f"Swin-MAE pretraining step, {B} x {Cin} x {H} x {H}, mask ratio {args.mask_ratio} ({n_keep} of {d * d} groups kept), math mode default; "
            f"{torch.cuda.get_device_name(0)}; {o.rounds} rounds of {o.iters} calls, fused and torch alternating; medians (min .. max)")
    lines = report(head, [name for name, _, _ in pairs], eager, graph, step_ms, need, agree)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def captured(fn):
    """fn captured into a hipGraph of its own (after a warm-up on a side stream); returns the replay callable."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            keep = fn()
    except RuntimeError as e:          # an op that cannot be captured: its line of table (a) is then the eager call, and says so
        NOT_CAPTURED.append(f"{fn.__name__}: {str(e).splitlines()[0]}")
        torch.cuda.synchronize()
        return fn
    g.keep = keep          # the outputs stay alive with the graph
    return g.replay


def table(title, names, times, need=None):
    med = statistics.median
    out = [title, f"{'':22s} {'fused (csrc/mae.hip)':>32s} {'torch device ops':>32s} {'torch / fused':>14s}" + (f" {'bytes needed':>13s} {'achieved':>12s}" if need else "")]
    tf = tt = 0.0
    for name in names:
        f, t = times[name]
        tf, tt = tf + med(f), tt + med(t)
        row = f"{name:22s} {med(f):10.2f} ({min(f):8.2f} .. {max(f):8.2f}) {med(t):10.2f} ({min(t):8.2f} .. {max(t):8.2f}) {med(t) / med(f):14.2f}"
        if need:
            row += f" {need[name]:13d} {need[name] / (med(f) * 1e-6) / 1e9:7.1f} GB/s"
        out.append(row)
    out.append(f"{'sum':22s} {tf:10.2f} {'':21s} {tt:10.2f} {'':21s} {tt / tf:14.2f}")
    return out, tf, tt


def report(head, names, eager, graph, step_ms, need, agree):
    med = statistics.median
    lines = [head, "", f"graphed step (one hipGraph replay, forward + loss + backward + AdamW): {med(step_ms):.3f} ms ({min(step_ms):.3f} .. {max(step_ms):.3f})", ""]
    g_lines, gf, gt = table("(a) the three laws alone at the step's shapes, each captured into a hipGraph of its own and replayed -- device time, us per replay:",
                            names, graph, need)
    e_lines, ef, et = table("(b) the same calls launched eagerly, us per call -- host time of the autograd bookkeeping and the launches included:", names, eager)
    lines += g_lines + [""] + e_lines + [""]
    slower = [n for n in names if med(graph[n][0]) > med(graph[n][1])]
    lines += [f"share of the graphed step taken by the three fused laws (a): {100.0 * gf / (med(step_ms) * 1e3):.2f} %",
              f"fused path {'NOT slower' if gf <= gt else 'SLOWER'} than the torch composition measured beside it: {gf:.1f} us against {gt:.1f} us replayed (a), "
              f"{ef:.1f} us against {et:.1f} us eager (b)" + (f"; slower law(s) in (a): {', '.join(slower)}" if slower else "; no single law slower in (a)"),
              f"agreement of the two on these inputs: mask equal; dx equal: {agree[0]}; max |dtoken difference| {agree[1]:.3e}; |loss difference| {agree[2]:.3e}; "
              f"max |dpred difference| {agree[3]:.3e}"]
    lines += [f"not capturable, timed eagerly in (a): {n}" for n in NOT_CAPTURED]
    return lines


if __name__ == "__main__":
    main()
