"""Time of one evaluation of a 2-D image test set (hpfg_amd.val.test_isic: Dice, HD95, Jaccard, ASD of class 1 per batch) through the two
routes of its surface metrics, on the same seeded synthetic test set and the same network (diagnostics; not part of the test suite).
Run it under a limit of its own:  timeout -k 10 900 python tools/image_eval_timing.py

  host    with_hd95=True: val.hd95_host + val.asd_host per batch (scipy erosions and distance transforms of the [B,H,W] masks on this
          machine's cores, three distance transforms per batch), after a copy of the prediction to the host
  device  with_hd95="device": val.surface_metrics_device per batch (csrc/surface.hip: one surface pass, one sort, hpfg_surface_sums)
  none    with_hd95=False: forwards, arg-max and confusion counts only -- what both routes share

The set-up is config/cps_unet_30k_224x224_ISIC.yaml: a U-Net(3, 2) at 224 x 224, --images test images in batches of the config's batch_size
(the last batch short).  The network is trained for --train-iters supervised iterations on the synthetic training images first, so that its
prediction is a set of blobs like a real one, not noise; should it still answer class 1 on under 1 % of the test pixels, the class-1 bias
is moved by the median logit difference (the file says so).  Times are wall times around the whole evaluation with the device idle before
and after, median of --reps runs (host: --host-reps).  Writes --out (default profiles/image_eval_timing.txt).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps, sync):
    out, val = [], None
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        val = fn()
        sync()
        out.append(time.perf_counter() - t0)
    return val, out


def _s(v):
    return f"{statistics.median(v) * 1e3:10.2f} ms ({min(v) * 1e3:.2f} .. {max(v) * 1e3:.2f}, {len(v)} runs)"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_eval_timing.txt"))
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--train-iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()

    import torch
    from hpfg_amd import val as V
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.model import build_model
    from hpfg_amd.train import Supervise
    from hpfg_amd.utils import loadyaml

    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    cfg = loadyaml(os.path.join(ROOT, "config", "cps_unet_30k_224x224_ISIC.yaml"))
    cfg.update(datasets="sup_synthetic", device="cuda:0", total_itrs=a.train_iters, step_size=10 ** 9, synthetic_labeled=64,
               synthetic_test_images=a.images, save_path=None, logger=None)
    dev = torch.device(cfg.device)
    torch.manual_seed(int(cfg.seed))
    model = build_model(cfg).to(dev)
    train_loader, test_loader = build_loader(cfg)
    if a.train_iters > 0:
        Supervise(model, train_loader, None, cfg)
    sync = lambda: torch.cuda.synchronize(dev)          # noqa: E731

    notes = []
    images = torch.cat([i for i, _ in test_loader], 0)
    pred = V.predict_images(images, model)
    frac = float((pred == 1).float().mean())
    if frac < 0.01:
        model.eval()
        with torch.no_grad():
            z = (model.val if hasattr(model, "val") else model)(images[:V.EVAL_BATCH].to(dev).contiguous())
            model.decoder.out_conv.bias.data[1] += float((z[:, 0] - z[:, 1]).median())
        model.train()
        notes.append(f"the trained network answered class 1 on {frac:.2%} of the test pixels: class-1 bias moved by the median logit difference")
        frac = float((V.predict_images(images, model) == 1).float().mean())

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    V.test_isic(model, test_loader, cfg, with_hd95="device")          # warm-up (engines of the full and the padded batch, allocator, sort workspace)
    none, t_none = _timed(lambda: V.test_isic(model, test_loader, cfg), a.reps, sync)
    devv, t_dev = _timed(lambda: V.test_isic(model, test_loader, cfg, with_hd95="device"), a.reps, sync)
    host, t_host = _timed(lambda: V.test_isic(model, test_loader, cfg, with_hd95=True), a.host_reps, sync)
    assert devv[0] > 0.0 and devv[0] == host[0] == none[0] and devv[2] == host[2], (devv, host, none)
    m_none, m_dev, m_host = (statistics.median(t) for t in (t_none, t_dev, t_host))
    batches = [int(i.shape[0]) for i, _ in test_loader]
    lines = ["test_isic over a synthetic 2-D test set: the surface metrics (HD95, ASD) on the host (scipy, this machine's cores) against the device",
             "(csrc/surface.hip), tools/image_eval_timing.py; wall times around the whole evaluation, median (min .. max)", "",
             f"== {a.images} images 3 x 224 x 224 in batches {batches[0]} x {len(batches) - 1} + {batches[-1]}, U-Net(3, 2) after {a.train_iters} supervised "
             f"iterations; {torch.cuda.get_device_name(0)}",
             f"   class 1 predicted on {frac:.1%} of the pixels"] + [f"   note: {n}" for n in notes] + [
             f"   none   (forward, arg-max, confusion counts)   {_s(t_none)}",
             f"   device (with_hd95=\"device\")                   {_s(t_dev)}",
             f"   host   (with_hd95=True)                       {_s(t_host)}",
             f"   surface metrics alone: host {(m_host - m_none) * 1e3:.2f} ms, device {(m_dev - m_none) * 1e3:.2f} ms per evaluation; "
             f"host / device = {(m_host - m_none) / max(m_dev - m_none, 1e-9):.1f}x; whole evaluation host / device = {m_host / m_dev:.1f}x"
             + ("" if m_dev < m_host else "   (the device route is NOT faster here)"),
             f"   (dice, hd95, jac, asd) device: {[round(v, 6) for v in devv]}",
             f"   (dice, hd95, jac, asd) host:   {[round(v, 6) for v in host]}",
             f"   |device - host|: hd95 {abs(devv[1] - host[1]):.2e}, asd {abs(devv[3] - host[3]):.2e} ({abs(devv[3] - host[3]) / np.spacing(host[3]):.0f} ulp)", ""]
    text = "\n".join(lines)
    print(text, end="", flush=True)
    with open(a.out, "w") as f:
        f.write(text)
