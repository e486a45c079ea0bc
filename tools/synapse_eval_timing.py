"""Timing of the Synapse evaluation resize on one GPU (diagnostics; the benchmark driver has no line for it).

One synthetic Synapse-sized volume (148 slices of 512 x 512, nine classes) and UNet(1, 9):
  (a) hpfg_amd.val.resize_cubic of the volume to 224 x 224: device time from events, warmed up, median of ROUNDS calls; the bytes the two
      passes move (read the volume, write and read the [S,224,512] intermediate, write the result) and the fraction of 8 TB/s they amount to;
  (b) the reference's route (val.py:243): scipy.ndimage.zoom(order=3) of every slice on the host, then the copy to the device (wall clock);
  (c) test_single_volume_synapse end to end, against the same function fed with slices resized by route (b) (wall clock, synchronised).
The table is appended to --out (default profiles/synapse_eval_timing.txt).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, HW_IN, HW_OUT, NCLS = 148, 512, 224, 9
ROUNDS, HOST_ROUNDS = 30, 3
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synapse_eval_timing.txt"))
    out = ap.parse_args().out
    import numpy as np
    import torch
    from scipy.ndimage import zoom
    from hpfg_amd import val as V
    from hpfg_amd.model import UNet

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    coarse = g.integers(0, NCLS, (S, 8, 8))
    lab = np.kron(coarse, np.ones((HW_IN // 8, HW_IN // 8), dtype=np.int64)).astype(np.uint8)
    img = (lab / (NCLS - 1) + 0.1 * g.standard_normal(lab.shape)).astype(np.float32)
    vol = torch.from_numpy(img).to(dev)
    dst = (HW_OUT, HW_OUT)

    # (a)
    for _ in range(3):
        V.resize_cubic(vol, dst)
    torch.cuda.synchronize()
    ms_a = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = V.resize_cubic(vol, dst)
        e1.record()
        e1.synchronize()
        ms_a.append(e0.elapsed_time(e1))
    a_ms = statistics.median(ms_a)
    moved = 4 * S * (HW_IN * HW_IN + 2 * HW_OUT * HW_IN + HW_OUT * HW_OUT)

    # (b)
    def host_route():
        return torch.from_numpy(np.stack([zoom(sl, (HW_OUT / HW_IN, HW_OUT / HW_IN), order=3) for sl in img])).to(dev)

    ms_b = []
    for _ in range(HOST_ROUNDS):
        t0 = time.perf_counter()
        ref = host_route()
        torch.cuda.synchronize()
        ms_b.append((time.perf_counter() - t0) * 1e3)
    b_ms = statistics.median(ms_b)
    err = float((got - ref).abs().max()) / float(vol.abs().max())

    # (c)
    torch.manual_seed(1)
    net = UNet(1, NCLS).to(dev)
    net.train()
    image, label = torch.from_numpy(img)[None], torch.from_numpy(lab)[None]

    def device_eval():
        return V.test_single_volume_synapse(image, label, net, classes=NCLS, patch_size=dst)

    def host_eval():          # the same function behind the host resize: slices arrive at patch size, the prediction goes back with order 0
        pred = V._resize_nearest(V.predict_volume(host_route(), net, dst), (HW_IN, HW_IN)).contiguous()
        cm = V.confusion_counts(pred, label[0].to(dev), NCLS)
        return [(V.dice_from_counts(cm, c), 0.0) for c in range(1, NCLS)]

    def wall(fn, rounds):
        fn()
        ts = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), r

    c_dev, d_dev = wall(device_eval, 5)
    c_host, d_host = wall(host_eval, HOST_ROUNDS)
    ddice = max(abs(p[0] - q[0]) for p, q in zip(d_dev, d_host))

    lines = [
        f"# synapse_eval_timing: volume [{S},{HW_IN},{HW_IN}] -> {HW_OUT} x {HW_OUT}, {torch.cuda.get_device_name(0)}",
        f"(a) resize_cubic on the device        {a_ms:10.3f} ms  (median of {ROUNDS}, min {min(ms_a):.3f}, max {max(ms_a):.3f}; device events)",
        f"    bytes moved by the two passes     {moved / 1e6:10.1f} MB  -> {moved / (a_ms * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (a_ms * 1e-3) / HBM_BYTES_PER_S:.1f} % of 8 TB/s",
        f"(b) scipy zoom(order=3) + copy        {b_ms:10.1f} ms  (median of {HOST_ROUNDS}, {b_ms / S:.2f} ms per slice; wall clock)",
        f"    (b) / (a)                         {b_ms / a_ms:10.0f} x     max|dev - scipy| = {err:.2e} * max|input|",
        f"(c) test_single_volume_synapse        {c_dev:10.1f} ms  device resize (median of 5, wall clock)",
        f"    the same behind route (b)         {c_host:10.1f} ms  ({c_host / c_dev:.1f} x; max per-class |dice difference| {ddice:.1e})",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
