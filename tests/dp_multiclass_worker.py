"""One data-parallel rank of tests/test_gpu_multiclass_dp.py (a child process: RANK / WORLD_SIZE / MASTER_* in the environment), a sibling of
tests/dp_rank_worker.py at NINE classes: Mean-Teacher steps of the real engine on this rank's shard of a fixed global batch of 4 + 4 images
of 32 x 32 (2 + 2 per rank), global-batch mode (sync_bn), eager.  Saves the loss parts of every step and the final parameters.

    HPFG_TEST_P2P  1 | 0     the BatchNorm / loss sums cross the ranks inside the kernels (peer mailboxes: hpfg_seg_loss_partials_x carries the
                             wide sums) or through host-launched collectives (dp.allreduce_sum(sums))
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hpfg_amd import engine as E  # noqa: E402
from hpfg_amd import parallel  # noqa: E402
from hpfg_amd.datasets.synthetic import synth_batch  # noqa: E402
from hpfg_amd.model import UNet, reset_dropout_streams  # noqa: E402
from hpfg_amd.train import MeanTeacherStep  # noqa: E402
from tests.dp_rank_worker import _frozen, opt_args, take  # noqa: E402

NCLS = 9
N_LAB = N_UNL = 4
SIZE = 32
STEPS = 2


def image_masks(step, who, n_images):
    """Per-IMAGE dropout keep masks of the five encoder dropout sites (as tests/dp_rank_worker.py::image_masks, at this size)."""
    g = torch.Generator().manual_seed(1000 * step + who)
    out = {}
    for lvl in range(5):
        c, h = E.WIDTHS[lvl], SIZE >> lvl
        out[E.enc_prefix(lvl) + ".0"] = (torch.rand(n_images, h, h, c, generator=g) >= E.ENC_DROPOUT[lvl]).to(torch.uint8)
    return out


def run(dev, dp, rank, world, p2p=False):
    torch.manual_seed(5)
    reset_dropout_streams()
    if dp is not None:
        dp.sync_bn, dp.overlap = True, False
        if p2p:
            dp.enable_peer_exchange()
    xl, yl = synth_batch(41, N_LAB, SIZE, SIZE, 1, NCLS, 8)
    xu, _ = synth_batch(42, N_UNL, SIZE, SIZE, 1, NCLS, 8)
    kl, ku = N_LAB // world, N_UNL // world
    il = list(range(rank * kl, (rank + 1) * kl))
    iu = list(range(rank * ku, (rank + 1) * ku))
    idx = il + [N_LAB + i for i in iu]
    m = UNet(1, NCLS).to(dev)
    m.math = "f32"
    ema = _frozen(m)
    m.train()
    st = MeanTeacherStep(m, ema, opt_args(), dp)
    inputs = (xl[il].to(dev), yl[il].to(dev), xu[iu].to(dev))
    losses = []
    for k in range(1, STEPS + 1):
        for net, who in ((m, 0), (ema, 1)):
            net.external_dropout_masks = take(image_masks(k, who, N_LAB + N_UNL), idx, dev)
        losses.append(st.step(*inputs, k, cons_w=0.05)["parts"].cpu().clone())
    torch.cuda.synchronize()
    if dp is not None:
        dp.check_peer_errors()
    return torch.stack(losses), m.flat_params.cpu(), ema.flat_params.cpu()


def main():
    out = sys.argv[1]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dp = parallel.init_from_env(dev, backend="gloo")
    try:
        torch.save(run(dev, dp, dp.rank, dp.world_size, p2p=os.environ.get("HPFG_TEST_P2P", "0") == "1"), f"{out}.rank{dp.rank}")
    finally:
        dp.shutdown()


if __name__ == "__main__":
    main()
