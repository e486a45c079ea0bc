"""Timings of the 5..16-class range on one GPU (diagnostics; the benchmark driver has no line for it).

  loss   the fused loss (csrc/loss.hip, one kernel family) at 16 x 224 x 224 for C in {2, 4, 8, 9, 12, 16} -- both ends of the range, both
         class strides of the sums layout, 16-byte and scalar accesses, an occupancy edge of the partial-sum kernel (8 -> 9 classes: 6 -> 5
         waves per SIMD): [partial sums + reduction + finalize] and [backward], with a teacher (Mean-Teacher form: 8 labelled + 8 unlabelled
         images, MSE against teacher logits) and without (16 labelled images).  C = 4 is the yardstick of the last column.  Each case is a
         captured hipGraph of BLOCK launches; device-event time per replay, alternating over the cases, median over the rounds; algorithmic
         bytes / time.
  step   ms per replayed (hipGraph) Mean-Teacher step at 8 + 8 images of 224 x 224 for 4, 8 and 9 classes in alternating blocks, and, from
         a second capture with device time stamps around the launches (engine.MarkLog), the launches of decoder.out_conv.

Every mode appends its table to --out (default profiles/multiclass_loss_timing.txt).
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, HW = 16, 224
ROUNDS, BLOCK = 9, 20
LOSS_CLASSES = (2, 4, 8, 9, 12, 16)


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def _loss_case(ncls, teacher):
    import torch
    from hpfg_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(ncls)
    n_lab = N // 2 if teacher else N
    x = torch.randn(N, HW, HW, ncls, generator=g).to(dev)
    t = torch.randn(N, HW, HW, ncls, generator=g).to(dev) if teacher else None
    lab = torch.randint(0, ncls, (n_lab, HW, HW), generator=g).to(torch.uint8).to(dev)
    nblk, nsum = lib.hpfg_loss_blocks(N, HW, HW), lib.hpfg_loss_nsum(ncls)
    partials, sums = torch.empty(nblk * nsum, device=dev), torch.empty(nsum, device=dev)
    outv, dl = torch.empty(8, device=dev), torch.empty_like(x)
    coef = torch.tensor([0.5, 0.5, 0.0, 0.0, 0.1 if teacher else 0.0, 0.0, 0.0, 0.0], device=dev)
    a = L.LossArgs()
    a.logits, a.t_logits, a.labels0, a.labels1 = L.ptr(x), L.ptr(t), L.ptr(lab), None
    a.coef, a.partials, a.sums, a.out, a.dlogits = L.ptr(coef), L.ptr(partials), L.ptr(sums), L.ptr(outv), L.ptr(dl)
    a.N, a.n_lab, a.H, a.W, a.C, a.world = N, n_lab, HW, HW, ncls, 1
    keep = (x, t, lab, partials, sums, outv, dl, coef, a)
    px = N * HW * HW
    rd = px * ncls * 4 + n_lab * HW * HW + ((N - n_lab) * HW * HW * ncls * 4 if teacher else 0)
    graphs = {}
    side = torch.cuda.Stream()
    for which in ("fwd", "bwd"):
        def launch():
            st = torch.cuda.current_stream(dev).cuda_stream
            if which == "fwd":
                L.check(lib.hpfg_seg_loss_partials(C.byref(a), st), "partials")
                L.check(lib.hpfg_seg_loss_finalize(C.byref(a), st), "finalize")
            else:
                L.check(lib.hpfg_seg_loss_bwd(C.byref(a), None, st), "bwd")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                launch()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(BLOCK):
                launch()
        graphs[which] = gr
    return dict(C=ncls, teacher=teacher, graphs=graphs, keep=keep, bytes={"fwd": rd, "bwd": rd + px * ncls * 4}, out=outv)


def loss(out):
    import torch
    cases = [_loss_case(c, t) for t in (True, False) for c in LOSS_CLASSES]
    res = {}
    for which in ("fwd", "bwd"):
        for c in cases:
            c["graphs"][which].replay()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for c in cases:                                # alternate over the cases, replay by replay
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c["graphs"][which].replay()
                e1.record()
                e1.synchronize()
                res.setdefault((c["C"], c["teacher"], which), []).append(e0.elapsed_time(e1) * 1e3 / BLOCK)
    for c in cases:
        assert bool(torch.isfinite(c["out"]).all())
    lines = ["", f"== (a) fused loss kernels, {N} x {HW} x {HW}; {torch.cuda.get_device_name(0)}",
             f"   device-event time per launch: hipGraph of {BLOCK} launches, median (min .. max) of {ROUNDS} alternating replays",
             "   fwd = partial sums + reduction + finalize, bwd = dlogits; bytes = logits (+ teacher logits of the unlabelled half) + labels (+ dlogits)",
             "   C = 4: the yardstick; C % 4 == 0: 16-byte accesses, other C: scalar accesses; C <= 4: 32-float sums rows, above: 104-float rows",
             f"   {'form':>10} {'C':>3} {'call':>4} | {'us':>28} | {'MB':>7} | {'GB/s':>7} | vs C = 4"]
    for teacher in (True, False):
        for which in ("fwd", "bwd"):
            nbytes = {c["C"]: c["bytes"][which] for c in cases if c["teacher"] == teacher}
            base = nbytes[4] / statistics.median(res[(4, teacher, which)]) / 1e3
            for ncls in LOSS_CLASSES:
                v, b = res[(ncls, teacher, which)], nbytes[ncls]
                med = statistics.median(v)
                rate = b / med / 1e3
                lines.append(f"   {'teacher' if teacher else 'no teacher':>10} {ncls:3d} {which:>4} | {med:9.2f} ({min(v):.2f} .. {max(v):.2f}){'':>3} | {b / 1e6:7.2f} | "
                             f"{rate:7.1f} | {rate / base:.2f}")
    _emit(out, lines)


def step(out):
    import torch
    from copy import deepcopy
    from hpfg_amd.datasets.synthetic import synth_batch
    from hpfg_amd.engine import MarkLog
    from hpfg_amd.model import UNet
    from hpfg_amd.train import GraphedStep, MeanTeacherStep
    from hpfg_amd.utils import loadyaml
    dev = torch.device("cuda:0")
    NL = NU = 8
    args = loadyaml(os.path.join(ROOT, "config", "mean_teacher_unet_30k_224x224_ACDC.yaml"))

    def build(ncls, marks):
        torch.manual_seed(1337)
        m = UNet(1, ncls).to(dev)
        ema = deepcopy(m)
        for p in ema.parameters():
            p.requires_grad = False
        m.train()
        ema.train()
        st = MeanTeacherStep(m, ema, args)
        xl, yl = synth_batch(10, NL, HW, HW, 1, ncls, 32)
        xu, _ = synth_batch(11, NU, HW, HW, 1, ncls, 32)
        inputs = [xl.to(dev), yl.to(dev), xu.to(dev)]
        log = None
        if marks:
            for k in range(2):
                st.step(*inputs, k + 1)
            eng = next(iter(m._engines.values()))[0]
            log = eng.marks = MarkLog(dev)

            def reset():
                log.n, log.spans = 0, []
            gs = GraphedStep(st, inputs, warmup=1, alias_inputs=True, before_capture=reset)
        else:
            gs = GraphedStep(st, inputs, warmup=3, alias_inputs=True)
        for i in range(5):
            gs.step(inputs, 10 + i)
        torch.cuda.synchronize()
        return gs, inputs, log

    classes = (4, 8, 9)
    runs = {c: build(c, False) + ([],) for c in classes}
    it = 100
    for _ in range(7):
        for c, (gs, inputs, _, ms) in runs.items():          # alternate the step objects, block by block
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                it += 1
                r = gs.step(inputs, it)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 10)
            assert bool(torch.isfinite(r["loss"]))
    lines = ["", f"== (b) replayed Mean-Teacher step (one hipGraph), {NL} + {NU} images of {HW} x {HW}, bf16x3; {torch.cuda.get_device_name(0)}",
             "   ms per step over blocks of 10 replays (device events), median (min .. max) of 7 alternating blocks"]
    for c, (_, _, _, ms) in runs.items():
        lines.append(f"   {c:2d} classes: {statistics.median(ms):7.3f} ms/step ({min(ms):.3f} .. {max(ms):.3f}) = {(NL + NU) / statistics.median(ms) * 1e3:.0f} img/s")
    runs.clear()
    lines += ["", "== (c) launches that touch decoder.out_conv inside that step (device time stamps around the launch in a second capture, mean of 5",
              "   replays less the calibration bracket); forward: Cout % 4 == 0 takes conv_thin_kernel, 9 classes the generic kernel"]
    for c in classes:
        gs, inputs, log = build(c, True)
        acc = {}
        for r in range(8):
            gs.step(inputs, 50 + r)
            torch.cuda.synchronize()
            if r >= 3:
                for i, (tag, us) in enumerate(log.read_us()):
                    acc.setdefault((i, tag), []).append(us)
        calib = statistics.median(statistics.mean(v) for (_, t), v in acc.items() if t == "calib")
        for (_, tag), v in acc.items():
            if "out_conv" in tag:
                lines.append(f"   {c:2d} classes: {tag:32s} {statistics.mean(v) - calib:7.1f} us")
        del gs, inputs, log
    _emit(out, lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["loss", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiclass_loss_timing.txt"))
    a = ap.parse_args()
    {"loss": loss, "step": step}[a.mode](a.out)
