"""GPU: the Swin-UNet assembly (hpfg_amd/model/swinunet.py) against the reference's fixtures (tools/make_golden_swinunet.py): "net2" forward,
input gradient and every parameter gradient in both math modes, "net3" eval logits; eval == train when all rates are 0; the dropout seed
word under hipGraph capture and across interleaved forwards.  Bound per tensor: 1e-3 max(1, max |reference|), the module rule of
tests/test_gpu_swin.py.  The weights are rebuilt from the recorded seeds; tests/test_swinunet_host.py holds the seeded init to the
reference's hashes."""
import functools
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from hpfg_amd import ops_tokens
from hpfg_amd.model import SwinUnet
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _meta():
    with open(os.path.join(GOLDEN, "swinunet.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"swinunet_{name}.npz"))


def _net(case, **over):
    m = _meta()
    kw = dict(m["net"], norm_layer=partial(nn.LayerNorm, eps=m["norm_eps"]))
    kw.update(depths=(2, 2), num_heads=(1, 2)) if case == "net2" else kw.update(depths=(2, 2, 2), num_heads=(1, 2, 4))
    kw.update(over)
    torch.manual_seed(m["seeds"][case])
    return SwinUnet(**kw).to(DEV)


def _check(what, got, want):
    want = torch.from_numpy(want)
    err, bound = maxerr(got.cpu(), want), 1e-3 * max(1.0, float(want.abs().max()))
    print(f"{what}: {err:.2e} (<= {bound:.2e})")
    assert err <= bound, what


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_net2_forward_and_every_gradient(math):
    z = _fixture("net2")
    net = _net("net2").train()
    net.external_draws = ([tuple(torch.from_numpy(r) for r in pair) for pair in z["net2.draws"]], None)
    x = torch.from_numpy(z["net2.x"]).to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        y = net(x)
        y.backward(torch.from_numpy(z["net2.dy"]).to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    assert y.shape == (2, 4, 56, 56)
    _check(f"net2 {math} y", y.detach(), z["net2.y"])
    _check(f"net2 {math} dx", x.grad, z["net2.dx"])
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == len([k for k in z.files if k.startswith("net2.grad.")])
    for k, g in grads.items():
        assert g is not None, k
        _check(f"net2 {math} grad.{k}", g, z[f"net2.grad.{k}"])


def test_net3_eval_logits():
    z = _fixture("net3")
    net = _net("net3").eval()
    with torch.no_grad():
        y = net(torch.from_numpy(z["net3.x"]).to(DEV))
    _check("net3 y", y, z["net3.y"])


def test_eval_equals_train_when_all_rates_are_zero():
    z = _fixture("net2")
    net = _net("net2", drop_path_rate=0.0)
    x = torch.from_numpy(z["net2.x"]).to(DEV)
    with torch.no_grad():
        assert torch.equal(net.train()(x), net.eval()(x))
    assert int(net.drop_word) == 0          # no dropout: the seed word is never advanced


def _dropout_net():
    return _net("net2", drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.0).train()


def test_forward_forward_backward_uses_the_first_forwards_seed():
    """forward, forward, then backward of the first equals forward + backward done alone, bit for bit: every forward hands its ops its
    own copy of the seed word."""
    z = _fixture("net2")
    net = _dropout_net()
    x, dy = torch.from_numpy(z["net2.x"]).to(DEV), torch.from_numpy(z["net2.dy"]).to(DEV)
    y1 = net(x)
    y2 = net(x)
    assert int(net.drop_word) == 2 and not torch.equal(y1, y2)          # another word, other masks
    y1.backward(dy)
    first = [y1.detach().clone()] + [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    net.drop_word.zero_()
    ya = net(x)
    ya.backward(dy)
    alone = [ya.detach()] + [p.grad for p in net.parameters()]
    for a, b in zip(first, alone):
        assert torch.equal(a, b)


def test_two_networks_and_a_deepcopy_draw_different_masks_for_equal_input():
    """Equal weights, equal input, no drop-path: the eval outputs agree bit for bit, the training outputs differ pairwise -- every instance,
    a deepcopy (the EMA teacher of the HPFG step) included, has a dropout stream of its own."""
    from copy import deepcopy
    z = _fixture("net2")
    a, b = _dropout_net(), _dropout_net()
    c = deepcopy(b)
    x = torch.from_numpy(z["net2.x"]).to(DEV)
    assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), b.state_dict().values()))
    with torch.no_grad():
        ya, yb, yc = a(x), b(x), c(x)
        assert not torch.equal(ya, yb) and not torch.equal(yb, yc) and not torch.equal(ya, yc)
        assert int(a.drop_word) == int(b.drop_word) == int(c.drop_word) == 1
        ea = a.eval()(x)
        assert torch.equal(ea, b.eval()(x)) and torch.equal(ea, c.eval()(x))


def test_captured_dropout_draws_new_masks_every_replay():
    """forward + backward with dropout captured once and replayed twice: each replay equals the eager run from the same seed word, and
    the two replays differ (the word is advanced by a kernel inside the graph)."""
    z = _fixture("net2")
    net = _dropout_net()
    x, dy = torch.from_numpy(z["net2.x"]).to(DEV), torch.from_numpy(z["net2.dy"]).to(DEV)
    params = list(net.parameters())

    def step():
        for t in params:
            t.grad = None
        y = net(x)
        y.backward(dy)
        return [y.detach()] + [t.grad for t in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        outs = step()
    net.drop_word.fill_(100)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in outs])
    assert int(net.drop_word) == 102
    assert not torch.equal(replays[0][0], replays[1][0])
    for k, got in enumerate(replays):
        net.drop_word.fill_(100 + k)
        for a, b in zip(got, step()):
            assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- the HPFG step on three small SwinUnet_Plus ------------------------------------------------------------------------------------------
NECKS = ("dense_projection_high", "dense_projection_head")


def _three():
    """embed 32, depths (2, 2), window 8 at 128 x 128, the factories' rates (dropout 0.1 / 0.1, drop-path 0.2) and norm eps"""
    from copy import deepcopy
    from hpfg_amd.model import SwinUnet_Plus, reset_dropout_streams
    reset_dropout_streams()          # the networks' dropout streams are numbered per instance: equal numbers for the runs that are compared
    kw = dict(in_chans=1, num_classes=4, embed_dim=32, window_size=8, depths=(2, 2), num_heads=(1, 2), mlp_ratio=2., drop_rate=0.1, attn_drop_rate=0.1,
              drop_path_rate=0.2, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    torch.manual_seed(1337)
    m1, m2 = SwinUnet_Plus(**kw).to(DEV), SwinUnet_Plus(**kw).to(DEV)          # the second continues the generator, as in the driver
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    return m1, m2, em


def _hpfg_run(tmp, graph):
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.train import HPFG
    from tests.test_gpu_segformer_plus import _loop_args
    a = _loop_args(tmp, 128, "sgd", model="swinunet_plus", total_itrs=5, step_size=5, hipgraph=graph, log_every=2)
    np.random.seed(3)
    m1, m2, em = _three()
    necks1 = {k: t.detach().clone() for k, t in m1.state_dict().items() if k.startswith(NECKS)}
    torch.manual_seed(11)
    lab, unl, test = build_loader(a)
    log = HPFG(m1, m2, em, lab, unl, test, a)
    torch.cuda.synchronize()
    assert necks1 and all(torch.equal(t, m1.state_dict()[k]) for k, t in necks1.items())          # the first student's necks: never computed, never updated
    assert int(m2.drop_word) > 0 and int(em.drop_word) > 0                                        # the teacher stays in train mode: it drops too
    return log.cpu(), [m.flat_params.detach().cpu().clone() for m in (m1, m2, em)], a


def test_hpfg_loop_on_three_swinunet_plus_graphed_equals_eager_bitwise(tmp_path):
    """The HPFG driver on three small SwinUnet_Plus networks, five iterations: iteration 1 eager, the step captured at iteration 2 and
    replayed for the rest, against the same loop launched eagerly (five eager steps) -- losses finite, and equal bits for the losses and
    every parameter of the three networks."""
    lg, pg, a = _hpfg_run(tmp_path / "g", True)
    le, pe, _ = _hpfg_run(tmp_path / "e", False)
    assert not any("capture unavailable" in ln for ln in a.logger.lines), a.logger.lines
    assert lg.shape == (6,) and torch.isfinite(lg).all()
    assert torch.equal(lg, le), (lg, le)
    assert all(torch.equal(x, y) for x, y in zip(pg, pe))
    assert not torch.equal(pg[1], pg[2])
