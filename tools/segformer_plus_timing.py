"""Timings of the SegFormer_Plus feature on one GPU (diagnostics; the benchmark driver has no line for it).

  attn      every attention entry point (forward; backward = dQ + dK/dV + partial sum) at the four MiT-B1 shapes of a 32 x 224 x 224 batch, head
            dim 64, next to the head-dim-32 kernels at the same B, N, M and C (twice the heads: the same FLOPs and bytes) -- alternating blocks
            of launches in one process, device-event time per block, median over the rounds
  launches  the same alternating launches and nothing else: run it under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python
            tools/segformer_plus_timing.py launches` to split the backward into its kernels
  trace     <dir>: per-kernel medians out of that run's *kernel_trace.csv (kernels told apart by name and grid; needs no GPU)
  step      ms per replayed (hipGraph) HPFG step at 8 + 24 images of 224 x 224: three SegFormer_Plus networks (AdamW, the committed config) and,
            beside it in alternating blocks, three U-Net+ networks (SGD) at the same batch

Every mode appends its table to --out (default profiles/segformer_plus_timing.txt).
"""
import argparse
import csv
import glob
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, MKEYS = 32, 49
SHAPES = [(3136, 1), (784, 2), (196, 5), (49, 8)]          # (queries, heads at head dim 64) of the four MiT-B1 stages at 224 x 224
ROUNDS, BLOCK = 9, 20


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def _attn_cases():
    import torch
    from hpfg_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    cases = []
    for N, h64 in SHAPES:
        C_ = 64 * h64
        g = torch.Generator().manual_seed(N)
        q, kv, do = (torch.randn(s, generator=g).to(dev) for s in ((B, N, C_), (B, MKEYS, 2 * C_), (B, N, C_)))
        out, dq, dkv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv)
        for d in (64, 32):
            heads = C_ // d
            scr = torch.empty(lib.hpfg_attn_mfma_scratch_floats(B, N, heads, d), dtype=torch.float32, device=dev)
            keep = (q, kv, do, out, dq, dkv, scr)

            def fwd(N=N, heads=heads, d=d, q=q, kv=kv, out=out):
                L.check(lib.hpfg_attn_mfma_fwd_hd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, MKEYS, heads, d, d ** -0.5, st), "fwd")

            def bwd(N=N, heads=heads, d=d, q=q, kv=kv, do=do, dq=dq, dkv=dkv, scr=scr):
                L.check(lib.hpfg_attn_mfma_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, MKEYS, heads, d, d ** -0.5, st), "bwd")

            cases.append(dict(N=N, C=C_, d=d, heads=heads, fwd=fwd, bwd=bwd, keep=keep))
    return cases


def attn(out, launches_only=False):
    import torch
    cases = _attn_cases()
    res = {}
    for N, h64 in SHAPES:
        pair = [c for c in cases if c["N"] == N]          # [head dim 64, head dim 32]
        for which in ("fwd", "bwd"):
            for c in pair:
                for _ in range(5):
                    c[which]()
            torch.cuda.synchronize()
            for _ in range(ROUNDS):
                for c in pair:                            # alternate the two head dims, block by block
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(BLOCK):
                        c[which]()
                    e1.record()
                    e1.synchronize()
                    res.setdefault((N, which, c["d"]), []).append(e0.elapsed_time(e1) * 1e3 / BLOCK)
    if launches_only:
        return
    import torch
    lines = ["", f"== (a) attention entry points, B = {B}, M = {MKEYS} keys, split-bf16 MFMA kernels (csrc/attn.hip); {torch.cuda.get_device_name(0)}",
             f"   device-event time per launch, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK} launches; bwd = dQ + dK/dV + partial sum",
             f"   {'N':>5} {'C':>4} {'call':>4} | {'head dim 64: heads, us':>34} | {'head dim 32: heads, us':>34} | ratio 64/32"]
    for N, h64 in SHAPES:
        for which in ("fwd", "bwd"):
            a, b = res[(N, which, 64)], res[(N, which, 32)]
            fa = f"{h64:2d}, {statistics.median(a):8.2f} ({min(a):.2f} .. {max(a):.2f})"
            fb = f"{2 * h64:2d}, {statistics.median(b):8.2f} ({min(b):.2f} .. {max(b):.2f})"
            lines.append(f"   {N:5d} {64 * h64:4d} {which:>4} | {fa:>34} | {fb:>34} | {statistics.median(a) / statistics.median(b):.2f}")
    _emit(out, lines)


def trace(out, d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    if len(files) > 1:
        raise SystemExit(f"more than one kernel trace under {d}: {files}")
    durs = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        if not re.search(r"attn_\w+<\d+>", name):
            continue
        wg = [int(row[f"Workgroup_Size_{a}"]) for a in "XYZ"]
        grid = tuple(int(row[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg))          # workgroups (x, heads, images)
        durs.setdefault((re.search(r"attn_\w+<\d+>", name).group(0), grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    blocks = lambda kern, N: (N + 63) // 64 if kern in ("attn_mfma_fwd_kernel", "attn_mfma_dq_kernel") else ((N + 511) // 512 if "dkv_kernel" in kern else 1)
    lines = ["", f"== (a') the same launches per kernel (rocprofv3 kernel trace, median us over all timed launches), B = {B}, M = {MKEYS}",
             f"   {'N':>5} {'C':>4} {'kernel':>22} | {'head dim 64':>11} | {'head dim 32':>11} | ratio 64/32"]
    for N, h64 in SHAPES:
        for kern in ("attn_mfma_fwd_kernel", "attn_mfma_dq_kernel", "attn_mfma_dkv_kernel", "attn_dkv_sum_kernel"):
            t = {}
            for dd, heads in ((64, h64), (32, 2 * h64)):
                v = durs.get((f"{kern}<{dd}>", (blocks(kern, N), heads, B)))
                t[dd] = statistics.median(v) if v else float("nan")
            lines.append(f"   {N:5d} {64 * h64:4d} {kern:>22} | {t[64]:11.2f} | {t[32]:11.2f} | {t[64] / t[32]:.2f}")
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
    runs = {}
    for name, cfg in (("segformer_plus", "hpfg_segformer_plus_30k_224x224_ACDC.yaml"), ("unet_plus", "hpfg_unet_plus_30k_224x224_ACDC.yaml")):
        a = loadyaml(os.path.join(ROOT, "config", cfg))
        a.batch_size, a.unlabel_batch_size = NL, NU
        torch.manual_seed(a.seed)
        blocks = (getattr(a, "model1", a), getattr(a, "model2", a))
        m1, m2 = (build_model(AttrDict(dict(b, train_crop_size=[HW, HW]))).to(dev) for b in blocks)
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
        runs[name] = (gs, inputs, [])
    it = 100
    for _ in range(7):
        for name, (gs, inputs, ms) in runs.items():      # alternate the two step objects, block by block
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(10):
                it += 1
                r = gs.step(inputs, it)
            e1.record()
            torch.cuda.synchronize()
            ms.append(((time.perf_counter() - t0) * 1e2, e0.elapsed_time(e1) / 10))
            assert bool(torch.isfinite(r["loss"]))
    lines = ["", f"== (b) replayed HPFG step (one hipGraph), {NL} + {NU} images of {HW} x {HW}, three networks; {torch.cuda.get_device_name(0)}",
             "   per step over blocks of 10 replays, median (min .. max) of 7 alternating blocks: device events | host clock ending in a synchronise"]
    for name, (_, _, both) in runs.items():
        ms, dev_ms = [b[0] for b in both], [b[1] for b in both]
        lines.append(f"   {name:>15}: {statistics.median(dev_ms):8.2f} ms/step ({min(dev_ms):.2f} .. {max(dev_ms):.2f}) | {statistics.median(ms):8.2f} ms/step "
                     f"({min(ms):.2f} .. {max(ms):.2f}) = {(NL + NU) / statistics.median(ms) * 1e3:.0f} img/s")
    _emit(out, lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["attn", "launches", "trace", "step"])
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segformer_plus_timing.txt"))
    a = ap.parse_args()
    if a.mode == "trace":
        trace(a.out, a.dir)
    elif a.mode == "step":
        step(a.out)
    else:
        attn(a.out, launches_only=a.mode == "launches")
