"""Timings of the LIDC Swin-UNet feature on one GPU (diagnostics; the benchmark driver has no line for it).

  kernels   the packed small-window attention (``window_attention_packed``, csrc/attn_window_packed.hip) next to the unpacked kernels
            (``window_attention_dropout``, csrc/attn_window.hip), forward + backward with dropout 0.1, at the four stage shapes of
            ``get_swinunet_LIDC(96)`` at the config's batch 64 (48^2 x 3 heads, 24^2 x 6, 12^2 x 12, 6^2 x 24; window 3, head dim 32) and of
            ``get_swinunet_LIDC(64)`` (32^2, 16^2, 8^2, 4^2; window 4) -- alternating blocks of launches in one process, device-event time per
            forward + backward pair, median (min .. max) over the rounds.  The last column is the rule of ``LIDC_PACKED`` in
            hpfg_amd/model/swinunet.py: a stage keeps ``packed`` only where the packed range lies wholly below the unpacked range.
  step      ms per replayed (hipGraph) supervised step of config/swinunet_30k_96x96_LIDC.yaml (batch 64 at 96 x 96, adamW) with ``packed`` on
            every stage and on none, alternating blocks of replays, and the share of each kernel family in the device time of the packed one
            (torch.profiler kernel records, grouped by kernel name)

Every mode appends its table to --out (default profiles/swinunet_lidc_timing.txt).
"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 64
# (image side, window, [(token map side, heads)] per stage): embed 96, heads (3, 6, 12, 24), head dim 32
NETS = [(96, 3, [(48, 3), (24, 6), (12, 12), (6, 24)]), (64, 4, [(32, 3), (16, 6), (8, 12), (4, 24)])]
D, P_DROP = 32, 0.1
ROUNDS, BLOCK = 9, 10
FAMILIES = [("window attention (packed)", r"attn_window_packed"), ("window attention (unpacked, bias sum)", r"attn_window"),
            ("GEMM (Linear fwd / dX / dW)", r"gemm|linear_wgrad|col_sum|rows_sum"), ("LayerNorm (+ pixel shuffle)", r"ln_fwd|ln_bwd|ln_px|col_reduce"),
            ("token dropout", r"token_dropout"), ("GELU", r"gelu"), ("residual + drop-path", r"residual_scale|scale_rows"),
            ("patch merging", r"patch_merge"), ("losses", r"loss|argmax"), ("optimizer", r"sgd|adamw"), ("seed word", r"word_add")]


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def _fmt(v):
    return f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"


def kernels(out):
    import torch
    from hpfg_amd.ops_tokens import window_attention_dropout, window_attention_packed
    dev = torch.device("cuda:0")
    lines = ["", f"== (a) window attention forward + backward with dropout {P_DROP}, B = {B}, head dim {D}, shifted (s = w // 2), split-bf16 math; "
                 f"{torch.cuda.get_device_name(0)}",
             f"   device-event us per forward + backward pair, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK}",
             f"   {'image':>5} {'w':>2} {'map':>7} {'heads':>5} {'workgroups':>19} | {'packed':>30} | {'unpacked':>30} | packed / unpacked | keeps packed"]
    for side, w, stages in NETS:
        for Hh, heads in stages:
            g = torch.Generator().manual_seed(Hh + w)
            C_ = heads * D
            qkv = torch.randn(B, Hh, Hh, 3 * C_, generator=g).to(dev).requires_grad_(True)
            table = torch.randn((2 * w - 1) ** 2, heads, generator=g).to(dev).requires_grad_(True)
            dy = torch.randn(B, Hh, Hh, C_, generator=g).to(dev)
            word = torch.zeros(1, dtype=torch.int32, device=dev)
            s, scale = w // 2, D ** -0.5
            nw = (Hh // w) ** 2
            per = 64 // (w * w)

            def packed():
                window_attention_packed(qkv, table, heads, w, s, scale, P_DROP, 7, word).backward(dy)

            def unpacked():
                window_attention_dropout(qkv, table, heads, w, s, scale, P_DROP, 7, word).backward(dy)

            res = {"packed": [], "unpacked": []}
            for f in (packed, unpacked):
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            for _ in range(ROUNDS):
                for name, f in (("packed", packed), ("unpacked", unpacked)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(BLOCK):
                        f()
                    e1.record()
                    e1.synchronize()
                    res[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
            keeps = max(res["packed"]) < min(res["unpacked"])
            wgs = f"{-(-nw // per) * heads * B} vs {nw * heads * B}"
            lines.append(f"   {side:5d} {w:2d} {Hh:3d}x{Hh:<3d} {heads:5d} {wgs:>19} | {_fmt(res['packed']):>30} | {_fmt(res['unpacked']):>30} | "
                         f"{statistics.median(res['packed']) / statistics.median(res['unpacked']):17.2f} | {'yes' if keeps else 'NO'}")
    _emit(out, lines)


def step(out):
    import torch
    from hpfg_amd.datasets.synthetic import synth_batch
    from hpfg_amd.model import WindowAttention, build_model
    from hpfg_amd.train import GraphedStep, SupervisedStep
    from hpfg_amd.utils import loadyaml
    dev = torch.device("cuda:0")
    a = loadyaml(os.path.join(ROOT, "config", "swinunet_30k_96x96_LIDC.yaml"))
    N, HW = a.batch_size, a.train_crop_size[0]
    x, y = synth_batch(10, N, HW, HW, a.in_channels, a.num_classes, 16)
    inputs = [x.to(dev), y.to(dev)]
    runs = {}
    for name in ("packed", "unpacked"):
        torch.manual_seed(a.seed)
        m = build_model(a)
        if name == "unpacked":          # the same network on the kernels of csrc/attn_window.hip (flipped before the first forward)
            for mod in m.modules():
                if isinstance(mod, WindowAttention):
                    mod.packed = False
        m = m.to(dev).train()
        gs = GraphedStep(SupervisedStep(m, a), inputs, warmup=3, alias_inputs=True)
        runs[name] = [gs, 10, []]
        for _ in range(3):
            runs[name][1] += 1
            gs.step(inputs, runs[name][1])
    torch.cuda.synchronize()
    for _ in range(7):
        for name in ("packed", "unpacked"):
            gs = runs[name][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                runs[name][1] += 1
                r = gs.step(inputs, runs[name][1])
            e1.record()
            e1.synchronize()
            runs[name][2].append(e0.elapsed_time(e1) / 5)
            assert bool(torch.isfinite(r["loss"]))
    lines = ["", f"== (b) replayed supervised step (one hipGraph), {N} images of {HW} x {HW}, swinunet_lidc (adamW, dropout 0.1 / 0.1, drop-path 0.2); "
                 f"{torch.cuda.get_device_name(0)}",
             "   ms per step over blocks of 5 replays (device events), median (min .. max) of 7 alternating blocks"]
    for name in ("packed", "unpacked"):
        v = runs[name][2]
        lines.append(f"   {name + ' on every stage':<26s} {statistics.median(v):8.2f} ms/step ({min(v):.2f} .. {max(v):.2f}) = {N / statistics.median(v) * 1e3:.0f} img/s")
    try:
        from torch.profiler import ProfilerActivity, profile
        gs = runs["packed"][0]
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                runs["packed"][1] += 1
                gs.step(inputs, runs["packed"][1])
            torch.cuda.synchronize()
        share, total = {}, 0.0
        for ev in prof.key_averages():
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            if t <= 0.0:
                continue
            fam = next((nm for nm, pat in FAMILIES if re.search(pat, ev.key)), "other (torch elementwise, copies, cat)")
            share[fam] = share.get(fam, 0.0) + t
            total += t
        lines.append(f"   kernel families of the packed step over 3 replays (torch.profiler kernel records, {total / 3e3:.2f} ms of kernel time per step):")
        for fam, t in sorted(share.items(), key=lambda kv: -kv[1]):
            lines.append(f"     {fam:<40s} {t / 3e3:8.2f} ms/step  {100.0 * t / total:5.1f} %")
    except Exception as e:          # the share is a diagnostic: the step times above stand without it
        lines.append(f"   kernel-family share not recorded: the profiler failed with {type(e).__name__}: {e}")
    _emit(out, lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinunet_lidc_timing.txt"))
    a = ap.parse_args()
    kernels(a.out) if a.mode == "kernels" else step(a.out)
