"""Record the launch schedule of UNetEngine: the MarkLog tags of one eager train-mode forward + backward of UNet(1, 4), for every
regime of REGIMES at every shape of SHAPES, as tests/golden/engine_schedule.json (tests/test_gpu_engine_schedule.py compares against it).

A pull request that changes the schedule on purpose regenerates the file -- the change then shows as a diff of tag lists:

    python tools/record_engine_schedule.py [--out tests/golden/engine_schedule.json]

Only names the engine promises to keep are used (engine attributes set by the tests and bench.py, forward / backward, MarkLog)."""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# 64: levels 64 / 32 / 16 take the thin and fused kernels, levels 8 / 4 the side-tensor path; 80: only level 0 is 16-aligned, odd image count
SHAPES = ((2, 1, 64, 64), (3, 1, 80, 80))

# name -> dict(env: set while the model and its engine are built, that is through the first forward; model / engine: attributes set on them
# (the engine's after a first no_grad forward created it, as tests/test_gpu_dz_side.py sets its switches); cb: backward gets a bucket_cb that
# only records its argument)
REGIMES = {
    "default": {},
    "defer_wgrad": dict(model=dict(defer_wgrad=True)),
    "f32": dict(model=dict(math="f32")),
    "bn_acc_off": dict(engine=dict(bn_acc_on=False)),
    "fused_bwd_off": dict(env=dict(HPFG_FUSED_BWD="0")),
    "upb_fuse_off": dict(engine=dict(upb_fuse=False)),
    "pool_fuse_off": dict(engine=dict(pool_fuse=False)),
    "side_off": dict(engine=dict(dz_side=False, act_side=False)),
    "bucket_cb": dict(cb=True),
    "allreduce": dict(engine=dict(force_sync=True, allreduce=lambda t: t)),      # the data-parallel route on one rank, no process group
}


def shape_key(shape) -> str:
    return "x".join(str(v) for v in shape)


@contextlib.contextmanager
def _environ(values: dict):
    """os.environ with `values` set, restored on exit."""
    saved = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record(regime: str, shape) -> list:
    """Tags of marks.spans, in order, of one eager train-mode forward + backward."""
    import torch
    from hpfg_amd.engine import MarkLog
    from hpfg_amd.model import UNet, reset_dropout_streams

    cfg = REGIMES[regime]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g).to(dev)
    dy = torch.randn(shape[0], 4, shape[2], shape[3], generator=g).to(dev)
    # the engine reads its environment switches when it is constructed, and the model constructs it in its first forward
    with _environ(cfg.get("env", {})):
        reset_dropout_streams()
        torch.manual_seed(7)
        m = UNet(shape[1], 4).to(dev)
        m.train()
        for k, v in cfg.get("model", {}).items():
            setattr(m, k, v)
        with torch.no_grad():
            m(x)
    eng = next(iter(m._engines.values()))[0]
    for k, v in cfg.get("engine", {}).items():
        setattr(eng, k, v)
    log = eng.marks = MarkLog(dev)
    try:
        if cfg.get("cb"):
            seen = []
            logits = eng.forward(x, train=True)
            eng.backward(dy.permute(0, 2, 3, 1).contiguous(), None, seen.append)
            assert seen == [0, 1], seen
            assert logits.shape == (shape[0], shape[2], shape[3], 4)
        else:
            m(x).backward(dy)
        torch.cuda.synchronize()
    finally:
        eng.marks = None
    return [span[0] for span in log.spans]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "engine_schedule.json"))
    args = ap.parse_args()
    table = {shape_key(sh): {name: record(name, sh) for name in REGIMES} for sh in SHAPES}
    for key, regimes in table.items():
        for name, tags in regimes.items():
            print(f"{key} {name}: {len(tags)} launches")
            assert tags, (key, name)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
