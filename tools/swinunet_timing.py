"""Timings of the Swin-UNet feature on one GPU (diagnostics; the benchmark driver has no line for it).

  expand    the fused patch expanding (``expand_layer_norm``: LayerNorm written through the pixel shuffle, one launch forward, one backward)
            next to the two-launch composition (hpfg_ln_px with P = 1, then ``permute().contiguous()``; backward: the copy back, then the
            LayerNorm backward) at the four expand shapes of the network at 32 images of 224 x 224 -- alternating blocks of launches in one
            process, device-event time per forward + backward, median over the rounds
  step      ms per replayed (hipGraph) HPFG step at the config's batch (8 + 24 images of 224 x 224) with three ``swinunet_plus`` networks
            (config/hpfg_swinunet_plus_30k_224x224_ACDC.yaml), and the share of each kernel family in the device time of the replayed steps
            (torch.profiler kernel records, grouped by kernel name)

Every mode appends its table to --out (default profiles/swinunet_timing.txt).
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 32
# (H = W of the input map, P, C of the LayerNorm): first_patch_expanding, layers_up[0].upsample, layers_up[1].upsample, final_patch_expanding
EXPANDS = [(7, 2, 384), (14, 2, 192), (28, 2, 96), (56, 4, 96)]
ROUNDS, BLOCK = 9, 10
FAMILIES = [("window attention", r"attn_window"), ("GEMM (Linear fwd / dX / dW)", r"gemm|linear_wgrad|col_sum|rows_sum"),
            ("LayerNorm (+ pixel shuffle)", r"ln_fwd|ln_bwd|col_reduce"), ("token dropout", r"token_dropout"), ("GELU", r"gelu"),
            ("residual + drop-path", r"residual_scale|scale_rows"), ("patch merging", r"patch_merge"), ("losses", r"loss|argmax|ntxent|l2norm|cutmix"),
            ("necks", r"neck_pool|relu_bwd"), ("optimizer + EMA", r"sgd|adamw|ema"), ("seed word", r"word_add")]


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def expand(out):
    import torch
    from hpfg_amd.ops_tokens import expand_layer_norm, layer_norm
    dev = torch.device("cuda:0")
    lines = ["", f"== (a) patch expanding after its Linear, B = {B}: LayerNorm(eps 1e-6) through the pixel shuffle; {torch.cuda.get_device_name(0)}",
             f"   forward + backward, device-event us per pair, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK}",
             f"   {'map':>9} {'P':>2} {'C':>4} {'out MB':>7} | {'fused (2 launches)':>30} | {'LayerNorm, then copy (4 launches)':>34} | fused / two-step"]
    for Hh, P, C_ in EXPANDS:
        g = torch.Generator().manual_seed(Hh)
        x = torch.randn(B, Hh, Hh, P * P * C_, generator=g).to(dev).requires_grad_(True)
        gam, bet = (torch.randn(C_, generator=g).to(dev).requires_grad_(True) for _ in range(2))
        dy = torch.randn(B, Hh * P, Hh * P, C_, generator=g).to(dev)

        def fused():
            expand_layer_norm(x, gam, bet, P, 1e-6).backward(dy)

        def two_step():
            y = layer_norm(x.view(B, Hh, Hh, P * P, C_), gam, bet, 1e-6)
            y.view(B, Hh, Hh, P, P, C_).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hh * P, Hh * P, C_).backward(dy)

        res = {"fused": [], "two": []}
        for f in (fused, two_step):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for name, f in (("fused", fused), ("two", two_step)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BLOCK):
                    f()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
        fa, fb = (f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})" for v in (res["fused"], res["two"]))
        lines.append(f"   {Hh:4d}x{Hh:<4d} {P:2d} {C_:4d} {dy.numel() * 4 / 1e6:7.1f} | {fa:>30} | {fb:>34} | "
                     f"{statistics.median(res['fused']) / statistics.median(res['two']):.2f}")
    _emit(out, lines)


def step(out):
    import torch
    from copy import deepcopy
    from hpfg_amd.datasets.synthetic import synth_batch
    from hpfg_amd.model import build_model
    from hpfg_amd.train import GraphedStep, HPFGStep
    from hpfg_amd.utils import loadyaml
    dev = torch.device("cuda:0")
    a = loadyaml(os.path.join(ROOT, "config", "hpfg_swinunet_plus_30k_224x224_ACDC.yaml"))
    NL, NU, HW = a.batch_size, a.unlabel_batch_size, a.train_crop_size[0]
    xl, yl = synth_batch(10, NL, HW, HW, 1, 4, 32)
    xl1, yl1 = synth_batch(12, NL, HW, HW, 1, 4, 32)
    xu, _ = synth_batch(11, NU, HW, HW, 1, 4, 32)
    rep = NU // NL
    torch.manual_seed(a.seed)
    m1, m2 = build_model(a).to(dev), build_model(a).to(dev)
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    st = HPFGStep(m1, m2, em, a)
    cm = st.make_cutmix_mask(NU, (HW, HW), device=dev)
    inputs = [xl.to(dev), yl.to(dev), xl1.repeat(rep, 1, 1, 1).to(dev), yl1.repeat(rep, 1, 1).to(dev), xu.to(dev), cm]
    gs = GraphedStep(st, inputs, warmup=3, alias_inputs=True)
    it = 10
    for _ in range(3):
        it += 1
        gs.step(inputs, it)
    torch.cuda.synchronize()
    both = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(5):
            it += 1
            r = gs.step(inputs, it)
        e1.record()
        torch.cuda.synchronize()
        both.append(((time.perf_counter() - t0) * 2e2, e0.elapsed_time(e1) / 5))
        assert bool(torch.isfinite(r["loss"]))
    ms, dev_ms = [b[0] for b in both], [b[1] for b in both]
    lines = ["", f"== (b) replayed HPFG step (one hipGraph), {NL} + {NU} images of {HW} x {HW}, three swinunet_plus networks (SGD, dropout 0.1 / 0.1, "
                 f"drop-path 0.2); {torch.cuda.get_device_name(0)}",
             "   per step over blocks of 5 replays, median (min .. max) of 7 blocks: device events | host clock ending in a synchronise",
             f"   {statistics.median(dev_ms):8.2f} ms/step ({min(dev_ms):.2f} .. {max(dev_ms):.2f}) | {statistics.median(ms):8.2f} ms/step "
             f"({min(ms):.2f} .. {max(ms):.2f}) = {(NL + NU) / statistics.median(ms) * 1e3:.0f} img/s"]
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                it += 1
                gs.step(inputs, it)
            torch.cuda.synchronize()
        share, total = {}, 0.0
        for ev in prof.key_averages():
            t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            if t <= 0.0:
                continue
            fam = next((name for name, pat in FAMILIES if re.search(pat, ev.key)), "other (torch elementwise, copies, cat)")
            share[fam] = share.get(fam, 0.0) + t
            total += t
        lines.append(f"   kernel families over 3 replayed steps (torch.profiler kernel records, {total / 3e3:.2f} ms of kernel time per step):")
        for fam, t in sorted(share.items(), key=lambda kv: -kv[1]):
            lines.append(f"     {fam:<40s} {t / 3e3:8.2f} ms/step  {100.0 * t / total:5.1f} %")
    except Exception as e:          # the share is a diagnostic: the step time above stands without it
        lines.append(f"   kernel-family share not recorded: the profiler failed with {type(e).__name__}: {e}")
    _emit(out, lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["expand", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swinunet_timing.txt"))
    a = ap.parse_args()
    expand(a.out) if a.mode == "expand" else step(a.out)
