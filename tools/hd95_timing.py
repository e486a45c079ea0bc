"""Time of one HD95 evaluation per volume through the two routes of hpfg_amd.val, on the same seeded synthetic volumes (diagnostics; not part
of the test suite).  Run it under a limit of its own:  timeout -k 10 1500 python tools/hd95_timing.py

  host    val.hd95_host per foreground class (scipy erosion + distance_transform_edt over the whole volume, twice per class), on this
          machine's cores: the classes run in worker processes (--workers, forked before the GPU is opened, one class each at a time); the file
          records the wall time of that and the sum of the per-class times, which is what the sequential loop in val.test_single_volume costs
  device  val.hd95_device (csrc/surface.hip + one sort): device-event time around the whole call (it contains its two transfers to the
          host), warmed up, median of several calls; and the same around hpfg_surface_distances alone (compaction + search), from which
          the pair rate is taken: pairs = sum over classes of 2 * n_pred * n_gt surface points

Volumes: ACDC size (10 x 256 x 216, 4 classes), Synapse size (148 x 512 x 512, 9 classes) -- smooth blobs, the prediction a jittered copy of
the truth -- and a worst case: the same Synapse truth against a uniformly random prediction (every voxel a surface voxel).
Writes --out (default profiles/hd95_timing.txt).
"""
import argparse
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("acdc", (10, 256, 216), 4, 20), ("synapse", (148, 512, 512), 9, 7), ("worst", (148, 512, 512), 9, 3)]          # name, shape, classes, timed device calls
HOST_LIMIT = 1200          # seconds for the host route of one case before it is given up


def blobs(shape, ncls, seed, jitter=False):
    """One wobbly ellipsoid per foreground class (later classes overwrite earlier ones); jitter: centres moved by ~3 % of the axis and radii
    scaled by 0.9 .. 1.1, from a second generator -- the 'prediction' of the same organs."""
    g, gj = np.random.default_rng(seed), np.random.default_rng(seed + 1000)
    vol = np.zeros(shape, np.uint8)
    for c in range(1, ncls):
        cen = np.array([g.uniform(0.25, 0.75) * n for n in shape])
        rad = np.array([g.uniform(0.12, 0.25) * n for n in shape])
        ph = g.uniform(0, 2 * np.pi, 2)
        dj, sj = gj.normal(0, 0.03, 3) * np.array(shape), gj.uniform(0.9, 1.1, 3)
        if jitter:
            cen, rad = cen + dj, rad * sj
        rad = np.maximum(rad, 1.0)
        lo = [max(int(cen[k] - 1.3 * rad[k]) - 1, 0) for k in range(3)]
        hi = [min(int(cen[k] + 1.3 * rad[k]) + 2, shape[k]) for k in range(3)]
        z, y, x = (np.arange(lo[k], hi[k], dtype=np.float32) for k in range(3))
        r2 = (((z - cen[0]) / rad[0]) ** 2)[:, None, None] + (((y - cen[1]) / rad[1]) ** 2)[None, :, None] + (((x - cen[2]) / rad[2]) ** 2)[None, None, :]
        wob = 1.0 + 0.2 * np.sin(y / rad[1] * 4 + ph[0])[None, :, None] * np.cos(x / rad[2] * 4 + ph[1])[None, None, :]
        box = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        box[r2 < wob] = c
    return vol


def volumes(name, shape, ncls):
    gt = blobs(shape, ncls, 11)
    pred = np.random.default_rng(12).integers(0, ncls, shape).astype(np.uint8) if name == "worst" else blobs(shape, ncls, 11, jitter=True)
    for c in range(1, ncls):
        assert (gt == c).any() and (pred == c).any(), (name, c)
    return pred, gt


_VOL = {}


def _host_class(job):
    """In a worker: hd95_host of one class; the worker builds the case's volumes itself from the seed (once) and times only the metric."""
    name, shape, ncls, c = job
    from hpfg_amd.val import hd95_host
    if _VOL.get("name") != name:
        _VOL["name"], (_VOL["pred"], _VOL["gt"]) = name, volumes(name, shape, ncls)
    t0 = time.perf_counter()
    v = hd95_host(_VOL["pred"] == c, _VOL["gt"] == c)
    return c, v, time.perf_counter() - t0


def host_route(pool, name, shape, ncls):
    """(values per class, wall seconds, per-class seconds); one class per worker process at a time."""
    pool.map(_host_class, [(name, shape, ncls, 1)] * pool._processes, chunksize=1)          # every worker builds the volumes (and imports) first
    t0 = time.perf_counter()
    res = pool.map_async(_host_class, [(name, shape, ncls, c) for c in range(1, ncls)], chunksize=1).get(timeout=HOST_LIMIT)
    wall = time.perf_counter() - t0
    res.sort()
    return np.array([r[1] for r in res]), wall, [r[2] for r in res]


def device_route(pred, gt, ncls, reps):
    import ctypes
    import torch
    from hpfg_amd import _lib as L
    from hpfg_amd import val as V
    dev = torch.device("cuda:0")
    lib = L.load()
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    s, h, w = pred.shape
    st = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    val = V.hd95_device(p, g, ncls)          # warm-up (allocator, sort workspace, code objects)
    whole = timed(lambda: V.hd95_device(p, g, ncls), reps)
    cdev = torch.empty(L.SURFACE_SEGS, dtype=torch.int32, device=dev)
    L.check(lib.hpfg_surface_counts(L.ptr(p), L.ptr(g), s, h, w, ncls, 3, L.ptr(cdev), st), "surface_counts")
    counts = cdev.cpu().numpy().astype(np.uint32)
    total = int(counts.sum(dtype=np.int64))
    need = lib.hpfg_surface_workspace_bytes(ncls, total)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    search = lambda: L.check(lib.hpfg_surface_distances(L.ptr(p), L.ptr(g), s, h, w, ncls, 3, counts.ctypes.data_as(ctypes.c_void_p), L.ptr(ws), need, st),          # noqa: E731
                             "surface_distances")
    search()
    part = timed(search, reps)
    n = counts.astype(np.int64)
    pairs = int(sum(2 * n[2 * c - 2] * n[2 * c - 1] for c in range(1, ncls)))
    return val, whole, part, n[:2 * (ncls - 1)].reshape(-1, 2), pairs, torch.cuda.get_device_name(0)


def _ms(v):
    return f"{statistics.median(v):10.3f} ms ({min(v):.3f} .. {max(v):.3f}, {len(v)} calls)"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hd95_timing.txt"))
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--cases", default="acdc,synapse,worst")
    a = ap.parse_args()
    cases = [c for c in CASES if c[0] in a.cases.split(",")]
    pool = mp.get_context("fork").Pool(a.workers)          # forked before this process opens the GPU; the workers never touch it
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def emit(lines):
        text = "\n".join(lines) + "\n"
        print(text, end="", flush=True)
        out.write(text)
        out.flush()

    emit(["HD95 of one volume: val.hd95_host (scipy, this machine's cores) against val.hd95_device (csrc/surface.hip), tools/hd95_timing.py",
          "seeded synthetic volumes; device times are device-event times, median (min .. max); the whole route includes its two transfers to the host", ""])
    for name, shape, ncls, reps in cases:
        pred, gt = volumes(name, shape, ncls)
        val, whole, part, n, pairs, gpu = device_route(pred, gt, ncls, reps)
        dev_s = statistics.median(whole) * 1e-3
        emit([f"== {name}: {shape[0]} x {shape[1]} x {shape[2]}, {ncls} classes; {gpu}",
              f"   surface points (pred, gt) per class: {[tuple(int(v) for v in r) for r in n]}",
              f"   pairs searched (both directions): {pairs:.4g}",
              f"   device whole route         {_ms(whole)}",
              f"   device compaction + search {_ms(part)}: {pairs / (statistics.median(part) * 1e-3):.3g} pairs/s",
              f"   hd95 per class (device): {np.round(val, 4).tolist()}"])
        hv, wall, per = host_route(pool, name, shape, ncls)
        seq = sum(per)
        emit([f"   host   per class {[round(t, 2) for t in per]} s: sum {seq:.2f} s (the sequential route); wall with {a.workers} worker processes, "
              f"one class each at a time: {wall:.2f} s",
              f"   host sum / device = {seq / dev_s:.1f}x, host wall / device = {wall / dev_s:.1f}x" + ("" if dev_s < seq else "   (the device route is NOT faster here)"),
              f"   max |device - host| = {np.abs(val - hv).max():.2e}", ""])
    pool.close()
    out.close()
