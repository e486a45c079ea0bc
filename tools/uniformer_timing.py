"""Timings of the Uniformer_Plus feature on one GPU (diagnostics; the benchmark driver has no line for it).

  ops    the depthwise k x k conv (csrc/dwconv.hip; k = 3, 5) and the token BatchNorm (hpfg_bn_tok_*), forward and backward, at the four stage
         shapes of a 32 x 224 x 224 batch (56^2 x 64, 28^2 x 128, 14^2 x 320, 7^2 x 512), next to torch's own op on the same device and the same
         NHWC data (F.conv2d(groups=C) / F.batch_norm on the channels-last view) -- alternating blocks of calls in one process, device-event
         time per call, median over the rounds.  Both sides are timed through autograd (ops_tokens.dwconv / batch_norm_tokens against torch's
         functions), so allocation of the outputs is inside both.  For the two large shapes the least bytes the op must move over the time,
         as a fraction of the HBM peak.
  step   ms per replayed (hipGraph) HPFG step at 8 + 24 images of 224 x 224: three Uniformer_Plus networks (AdamW, the committed config)

Every mode appends its table to --out (default profiles/uniformer_timing.txt).
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
SHAPES = [(56, 64), (28, 128), (14, 320), (7, 512)]
ROUNDS, BLOCK = 7, 20
HBM_PEAK = 8.0e12          # bytes / s
FAMILIES = [("depthwise conv (dwconv.hip)", r"dwconv"), ("token BatchNorm", r"bnrelu|col_stats"), ("attention", r"attn_"),
            ("GEMM (Linear / 1x1 conv fwd, dX, dW)", r"gemm|linear_wgrad|col_sum|rows_sum"), ("LayerNorm", r"ln_fwd|ln_bwd|col_reduce"),
            ("GELU", r"gelu"), ("residual + drop-path", r"residual_scale|scale_rows"), ("head resize", r"resize"),
            ("losses", r"loss|argmax|ntxent|l2norm|cutmix"), ("necks", r"neck_pool|relu_bwd"), ("optimizer + EMA", r"sgd|adamw|ema")]


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def _alternate(fns):
    """fns: name -> callable; -> name -> list of us per call over ROUNDS alternating blocks"""
    import torch
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
    return res


def _fmt(v):
    return f"{statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})"


def ops(out):
    import torch
    import torch.nn.functional as F
    from hpfg_amd import ops_tokens as T
    dev = torch.device("cuda:0")
    lines = ["", f"== (a) depthwise k x k conv and token BatchNorm, B = {B}, NHWC float32; {torch.cuda.get_device_name(0)}",
             f"   device-event us per call, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK} calls; bwd = the autograd backward of the call",
             f"   HBM fraction (56^2 x 64 and 28^2 x 128 only): least bytes the op moves / time / {HBM_PEAK / 1e12:.0f} TB/s",
             f"   {'op':>10} {'map':>9} {'call':>4} | {'this library, us':>28} | {'torch, us':>28} | ours/torch | HBM fraction"]
    for side, C_ in SHAPES:
        g = torch.Generator().manual_seed(side)
        x = torch.randn(B, side, side, C_, generator=g).to(dev).requires_grad_(True)
        dy = torch.randn(B, side, side, C_, generator=g).to(dev)
        xt = x.detach().permute(0, 3, 1, 2).requires_grad_(True)          # the same NHWC data as a channels-last NCHW tensor
        dyt = dy.permute(0, 3, 1, 2)
        nbytes = x.numel() * 4
        for k in (3, 5):
            w = (0.1 * torch.randn(C_, 1, k, k, generator=g)).to(dev).requires_grad_(True)
            b = torch.zeros(C_, device=dev, requires_grad=True)
            assert xt.is_contiguous(memory_format=torch.channels_last)
            ref = F.conv2d(xt, w, b, padding=k // 2, groups=C_)
            err = float((T.dwconv(x, w, b, k).permute(0, 3, 1, 2) - ref).abs().max())
            assert err < 1e-3, err
            fw = _alternate({"ours": lambda: T.dwconv(x, w, b, k), "torch": lambda: F.conv2d(xt, w, b, padding=k // 2, groups=C_)})
            yo, yt = T.dwconv(x, w, b, k), F.conv2d(xt, w, b, padding=k // 2, groups=C_)
            bw = _alternate({"ours": lambda: torch.autograd.grad(yo, (x, w, b), dy, retain_graph=True),
                             "torch": lambda: torch.autograd.grad(yt, (xt, w, b), dyt, retain_graph=True)})
            for call, r, moved in (("fwd", fw, 2 * nbytes), ("bwd", bw, 4 * nbytes)):      # fwd: read x, write y; bwd: read dy (dx), read x and dy (dw), write dx
                frac = f"{moved / (statistics.median(r['ours']) * 1e-6) / HBM_PEAK:.2f}" if side >= 28 else "-"
                lines.append(f"   {'dwconv' + str(k):>10} {side:3d}^2x{C_:<3d} {call:>4} | {_fmt(r['ours']):>28} | {_fmt(r['torch']):>28} | "
                             f"{statistics.median(r['ours']) / statistics.median(r['torch']):10.2f} | {frac}")
        ga, be = torch.ones(C_, device=dev, requires_grad=True), torch.zeros(C_, device=dev, requires_grad=True)
        fw = _alternate({"ours": lambda: T.batch_norm_tokens(x, ga, be, 1e-5), "torch": lambda: F.batch_norm(xt, None, None, ga, be, True, 0.0, 1e-5)})
        yo, yt = T.batch_norm_tokens(x, ga, be, 1e-5)[0], F.batch_norm(xt, None, None, ga, be, True, 0.0, 1e-5)
        assert float((yo.permute(0, 3, 1, 2) - yt).abs().max()) < 1e-3
        bw = _alternate({"ours": lambda: torch.autograd.grad(yo, (x, ga, be), dy, retain_graph=True),
                         "torch": lambda: torch.autograd.grad(yt, (xt, ga, be), dyt, retain_graph=True)})
        for call, r, moved in (("fwd", fw, 3 * nbytes), ("bwd", bw, 5 * nbytes)):          # fwd: x twice (statistics, apply), y; bwd: x, dy twice, dx
            frac = f"{moved / (statistics.median(r['ours']) * 1e-6) / HBM_PEAK:.2f}" if side >= 28 else "-"
            lines.append(f"   {'bn_tokens':>10} {side:3d}^2x{C_:<3d} {call:>4} | {_fmt(r['ours']):>28} | {_fmt(r['torch']):>28} | "
                         f"{statistics.median(r['ours']) / statistics.median(r['torch']):10.2f} | {frac}")
    _emit(out, lines)


def step(out):
    import torch
    from copy import deepcopy
    from hpfg_amd.datasets.synthetic import synth_batch
    from hpfg_amd.model import build_model
    from hpfg_amd.train import GraphedStep, HPFGStep
    from hpfg_amd.utils import AttrDict, loadyaml
    dev = torch.device("cuda:0")
    NL, NU, HW = 8, 24, 224
    xl, yl = synth_batch(10, NL, HW, HW, 1, 4, 32)
    xl1, yl1 = synth_batch(12, NL, HW, HW, 1, 4, 32)
    xu, _ = synth_batch(11, NU, HW, HW, 1, 4, 32)
    rep = NU // NL
    a = loadyaml(os.path.join(ROOT, "config", "hpfg_uniformer_plus_30k_224x224_ACDC.yaml"))
    torch.manual_seed(a.seed)
    m1, m2 = (build_model(AttrDict(dict(a, train_crop_size=[HW, HW]))).to(dev) for _ in range(2))
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    st = HPFGStep(m1, m2, em, a)
    cm = st.make_cutmix_mask(NU, (HW, HW), device=dev)
    inputs = [xl.to(dev), yl.to(dev), xl1.repeat(rep, 1, 1, 1).to(dev), yl1.repeat(rep, 1, 1).to(dev), xu.to(dev), cm]
    gs = GraphedStep(st, inputs, warmup=3, alias_inputs=True)
    for i in range(5):
        gs.step(inputs, 10 + i)
    torch.cuda.synchronize()
    it, both = 100, []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(10):
            it += 1
            r = gs.step(inputs, it)
        e1.record()
        torch.cuda.synchronize()
        both.append(((time.perf_counter() - t0) * 1e2, e0.elapsed_time(e1) / 10))
        assert bool(torch.isfinite(r["loss"]))
    ms, dev_ms = [b[0] for b in both], [b[1] for b in both]
    shares = []
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
            fam = next((name for name, pat in FAMILIES if re.search(pat, ev.key)), "other (torch elementwise, copies, patch gather)")
            share[fam] = share.get(fam, 0.0) + t
            total += t
        shares.append(f"   kernel families over 3 replayed steps (torch.profiler kernel records, {total / 3e3:.2f} ms of kernel time per step):")
        for fam, t in sorted(share.items(), key=lambda kv: -kv[1]):
            shares.append(f"     {fam:<48s} {t / 3e3:8.2f} ms/step  {100.0 * t / total:5.1f} %")
    except Exception as e:          # the share is a diagnostic: the step time above stands without it
        shares.append(f"   kernel-family share not recorded: the profiler failed with {type(e).__name__}: {e}")
    _emit(out, ["", f"== (b) replayed HPFG step (one hipGraph), {NL} + {NU} images of {HW} x {HW}, three Uniformer_Plus networks; {torch.cuda.get_device_name(0)}",
                "   per step over blocks of 10 replays, median (min .. max) of 7 blocks: device events | host clock ending in a synchronise",
                f"   uniformer_plus: {statistics.median(dev_ms):8.2f} ms/step ({min(dev_ms):.2f} .. {max(dev_ms):.2f}) | {statistics.median(ms):8.2f} ms/step "
                f"({min(ms):.2f} .. {max(ms):.2f}) = {(NL + NU) / statistics.median(ms) * 1e3:.0f} img/s"] + shares)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ops", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uniformer_timing.txt"))
    a = ap.parse_args()
    (ops if a.mode == "ops" else step)(a.out)
