"""GPU, two ranks on one device (gloo between fresh child processes): the data-parallel global-batch mode at NINE classes.  Both paths that
carry the loss sums across the ranks must carry the wide sums (hpfg_loss_nsum(9) floats): the peer mailboxes inside the reduction kernel
(hpfg_seg_loss_partials_x) and the host-launched collective (dp.allreduce_sum(sums)).  Mean-Teacher, 32 x 32, 2 + 2 images per rank:
two ranks on shards == one process on the concatenated batch, losses within 1e-5 (as tests/test_gpu_dp_two_ranks.py)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from tests import dp_multiclass_worker as W
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
LIMIT_S = 240


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(tmp_path, tag, **env_kw):
    """Two rank processes, each under its own `timeout`; both exit statuses are checked, and a non-zero one ends the test."""
    out = str(tmp_path / tag)
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **{k: str(v) for k, v in env_kw.items()})
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(LIMIT_S), sys.executable, "-X", "faulthandler", "-m", "tests.dp_multiclass_worker", out],
                                      cwd=ROOT, env=env))
    try:
        codes = [p.wait(timeout=LIMIT_S + 30) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert codes == [0, 0], codes
    return tuple(torch.load(f"{out}.rank{r}") for r in range(2))


def test_two_ranks_equal_the_global_batch_nine_classes(tmp_path):
    ref = W.run(DEV, None, 0, 1)
    assert torch.isfinite(ref[0]).all() and float(ref[0][:, 5].abs().max()) > 0.0          # the consistency term is live
    for tag, p2p in (("mailbox", 1), ("collective", 0)):          # (the second pair starts only after the first has passed)
        r0, r1 = _two_ranks(tmp_path, tag, HPFG_TEST_P2P=p2p)
        for got in (r0, r1):
            assert maxerr(got[0], ref[0]) < 1e-5, (tag, got[0], ref[0])      # loss parts are normalised by the GLOBAL counts on every rank
            for a, b in zip(got[1:], ref[1:]):
                assert maxerr(a, b) < 1e-5, tag
        assert torch.equal(r0[1], r1[1]) and torch.equal(r0[2], r1[2])
