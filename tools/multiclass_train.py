"""A short training run of the two Synapse-shaped nine-class configs on the synthetic loaders, through the driver loops:

  sup   config/unet_30k_224x224_Synapse.yaml             -> Supervise(...)
  ict   config/ict-medseg_unet_30k_224x224_Synapse.yaml  -> ICT_MedSeg(...)

--iters iterations, evaluation (test_acdc: Dice of classes 1 .. num_classes - 1) every --every.  Prints the logger's lines and the total loss
as means over windows of 25 iterations.  Checkpoints go to a temporary directory.  profiles/multiclass_training_log.txt is one run of both.
"""
import argparse
import os
import sys
import tempfile
from copy import deepcopy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


class _Log:
    def info(self, msg):
        print("   [logger]", msg, flush=True)

    warning = info


def _args(name, iters, every, tmp):
    from hpfg_amd.utils import loadyaml
    a = loadyaml(os.path.join(ROOT, "config", name))
    a.device = DEV
    a.total_itrs, a.step_size = iters, every
    a.save_path = tmp
    os.makedirs(os.path.join(tmp, "model"), exist_ok=True)
    a.model_save_path = os.path.join(tmp, "model", "model.pth")
    a.ema_model_save_path = os.path.join(tmp, "model", "ema.pth")
    a.logger = _Log()
    return a


def _show(name, log):
    import torch
    log = log.cpu()
    print(f"{name}: {log.numel()} iterations; total loss, mean over windows of 25:")
    print("   " + " ".join(f"{float(log[i:i + 25].mean()):.4f}" for i in range(0, log.numel() - 24, 25)))
    print(f"   first {float(log[0]):.4f}  last {float(log[-1]):.4f}", flush=True)
    assert bool(torch.isfinite(log).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["sup", "ict"])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--every", type=int, default=100)
    o = ap.parse_args()
    import torch
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.model import build_model, reset_dropout_streams
    from hpfg_amd.train import ICT_MedSeg, Supervise
    torch.manual_seed(1)
    reset_dropout_streams()
    with tempfile.TemporaryDirectory() as tmp:
        if o.mode == "sup":
            a = _args("unet_30k_224x224_Synapse.yaml", o.iters, o.every, tmp)
            m = build_model(a).to(DEV)
            train, test = build_loader(a)
            print(f"== Supervise, config/unet_30k_224x224_Synapse.yaml, {a.num_classes} classes, batch {a.batch_size}, "
                  f"total_itrs={o.iters} step_size={o.every}", flush=True)
            _show("Supervise", Supervise(m, train, test, a))
        else:
            a = _args("ict-medseg_unet_30k_224x224_Synapse.yaml", o.iters, o.every, tmp)
            m = build_model(a).to(DEV)
            e = deepcopy(m)
            for p in e.parameters():
                p.requires_grad = False
            lab, unl, test = build_loader(a)
            print(f"== ICT_MedSeg, config/ict-medseg_unet_30k_224x224_Synapse.yaml, {a.num_classes} classes, batch {a.batch_size} + "
                  f"{a.unlabel_batch_size}, total_itrs={o.iters} step_size={o.every}", flush=True)
            _show("ICT_MedSeg", ICT_MedSeg(m, e, lab, unl, test, a))
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
