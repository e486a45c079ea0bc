"""GPU: the LIDC Swin-UNet (patch 2, window 3 / 4; hpfg_amd/model/swinunet.py on the packed small-window attention of
csrc/attn_window_packed.hip) against the reference's fixtures (tools/make_golden_swinunet_lidc.py): the "dropblock" at window 3 with its recorded
masks and draws, "net2" forward, input gradient and every parameter gradient in both math modes with ``packed`` on and off, "net3" eval logits,
``SupervisedStep`` on the recorded adamW + cosine trace, the captured supervised step against the eager one, ``test_lidc`` on image batches.
Bound per tensor: 1e-3 max(1, max |reference|), the rule of tests/test_gpu_swinunet.py; the trace: |loss error| <= 1e-3 per iteration and that
rule for the final logits, the tolerances tests/test_gpu_swinmae.py applies to its adamW trace.  The weights are rebuilt from the recorded
seeds; tests/test_swinunet_lidc_host.py holds the seeded init to the reference's hashes."""
import functools
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from hpfg_amd import ops_tokens
from hpfg_amd.model import SwinTransformerBlock, SwinUnet, WindowAttention, reset_dropout_streams
from hpfg_amd.utils import AttrDict
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPE = {"net2": dict(window_size=3, depths=(2, 2), num_heads=(1, 2)), "net3": dict(window_size=4, depths=(2, 2, 2), num_heads=(1, 2, 4))}


@functools.lru_cache(maxsize=None)
def _meta():
    with open(os.path.join(GOLDEN, "swinunet_lidc.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def _net(case, packed=True, **over):
    m = _meta()
    kw = dict(m["net"], norm_layer=partial(nn.LayerNorm, eps=m["norm_eps"]), packed=packed, **SHAPE[case])
    kw.update(over)
    torch.manual_seed(m["seeds"][case])
    return SwinUnet(**kw).to(DEV)


def _check(what, got, want):
    want = torch.as_tensor(want)
    err, bound = maxerr(got.detach().cpu(), want), 1e-3 * max(1.0, float(want.abs().max()))
    print(f"{what}: {err:.2e} (<= {bound:.2e})")
    assert err <= bound, what


def _draws(arr):
    return [tuple(torch.from_numpy(r) for r in pair) for pair in arr]


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("packed", [True, False])
def test_dropblock_at_window_3(packed, math):
    """The reference block with drop = attn_drop = 0.1 and drop_path = 0.3 in train mode on four 3 x 3 windows per image, its four recorded
    dropout masks and two drop-path draws replayed: forward and every gradient."""
    z = _fixture("swinunet_lidc_dropblock")
    net = SwinTransformerBlock(32, 1, 3, shift=True, drop=0.1, attn_drop=0.1, drop_path=0.3, allow_dropout=True, packed=packed)
    net.load_state_dict({k[len("dropblock.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("dropblock.sd.")}, strict=True)
    net.external_draws = tuple(torch.from_numpy(r) for r in z["dropblock.draws"])
    net.external_masks = {k[len("dropblock.mask."):]: torch.from_numpy(z[k]).to(DEV) for k in z.files if k.startswith("dropblock.mask.")}
    assert sorted(net.external_masks) == ["attn.attn_drop", "attn.proj_drop", "mlp.drop1", "mlp.drop2"] and net.attn.packed == packed
    net = net.to(DEV).train()
    x = torch.from_numpy(z["dropblock.x"]).to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        y = net(x)
        y.backward(torch.from_numpy(z["dropblock.dy"]).to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == len([k for k in z.files if k.startswith("dropblock.grad.")])
    _check(f"dropblock {math} y", y, z["dropblock.y"])
    _check(f"dropblock {math} dx", x.grad, z["dropblock.dx"])
    for k, g in grads.items():
        assert g is not None, k
        _check(f"dropblock {math} grad.{k}", g, z[f"dropblock.grad.{k}"])


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("packed", [True, False])
def test_net2_forward_and_every_gradient(packed, math):
    z = _fixture("swinunet_lidc_net2")
    net = _net("net2", packed).train()
    assert all(m.packed == packed for m in net.modules() if isinstance(m, WindowAttention))
    net.external_draws = (_draws(z["net2.draws"]), None)
    x = torch.from_numpy(z["net2.x"]).to(DEV).requires_grad_(True)
    ops_tokens.MATH["mode"] = math
    try:
        y = net(x)
        y.backward(torch.from_numpy(z["net2.dy"]).to(DEV))
    finally:
        ops_tokens.MATH["mode"] = None
    assert y.shape == (2, 2, 24, 24)
    _check(f"net2 {math} y", y, z["net2.y"])
    _check(f"net2 {math} dx", x.grad, z["net2.dx"])
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == len([k for k in z.files if k.startswith("net2.grad.")])
    for k, g in grads.items():
        assert g is not None, k
        _check(f"net2 {math} grad.{k}", g, z[f"net2.grad.{k}"])


@pytest.mark.parametrize("packed", [True, False])
def test_net3_eval_logits(packed):
    z = _fixture("swinunet_lidc_net3")
    net = _net("net3", packed).eval()
    with torch.no_grad():
        y = net(torch.from_numpy(z["net3.x"]).to(DEV))
    _check("net3 y", y, z["net3.y"])


def _step(net):
    from hpfg_amd.train import SupervisedStep
    return SupervisedStep(net, AttrDict(dict(_meta()["opt"], device="cuda:0", num_classes=2)))


def test_supervised_step_replays_the_recorded_adamw_cosine_trace():
    from hpfg_amd.utils.optim import FusedAdamW
    z, t = _fixture("swinunet_lidc_net2"), _fixture("trace_swinunet_lidc")
    net = _net("net2").train()
    st = _step(net)
    assert isinstance(st.optimizer, FusedAdamW) and net.flat_params.numel() == sum(p.numel() for p in net.parameters())
    x, label = torch.from_numpy(z["net2.x"]).to(DEV), torch.from_numpy(t["label"]).to(DEV)
    for i in range(3):
        net.external_draws = (_draws(t["draws"][i]), None)
        lr = st._lr(st.optimizer)
        assert abs(lr - float(t["lr"][i])) <= 1e-6 * float(t["lr"][i]), (i, lr, float(t["lr"][i]))
        r = st.step(x, label, i + 1)
        err = abs(float(r["loss"]) - float(t["loss"][i]))
        print(f"trace iteration {i}: lr {lr:.3e} loss {float(r['loss']):.6f} reference {float(t['loss'][i]):.6f} error {err:.2e}")
        assert err <= 1e-3
    net.eval()
    with torch.no_grad():
        _check("final eval logits", net(x), t["logits"])


def test_graphed_supervised_step_equals_eager_and_draws_new_masks():
    """The supervised step on net2 with dropout 0.1 / 0.1 (no drop-path: its draws come from torch's generator, not from the seed word): one
    eager iteration, then the step captured and replayed twice, against three eager iterations -- equal bits for every loss and for the
    parameters after the first replay and after the second; the seed word advanced once per forward, so the second replay drew other masks
    than the first (the eager run it equals used word 3, not word 2)."""
    from hpfg_amd.train import GraphedStep
    z, t = _fixture("swinunet_lidc_net2"), _fixture("trace_swinunet_lidc")
    x, label = torch.from_numpy(z["net2.x"]).to(DEV), torch.from_numpy(t["label"]).to(DEV)
    runs = []
    for graphed in (True, False):
        reset_dropout_streams()          # the networks' dropout streams are numbered per instance: equal numbers for the runs that are compared
        net = _net("net2", drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.0).train()
        st = _step(net)
        losses, params = [st.step(x, label, 1)["loss"].clone()], []          # iteration 1 eager in both runs, as the driver loop does
        runner = GraphedStep(st, [x, label], warmup=0) if graphed else None
        for i in (2, 3):
            r = runner.step([x, label], i) if graphed else st.step(x, label, i)
            losses.append(r["loss"].clone())
            params.append(net.flat_params.detach().clone())
        torch.cuda.synchronize()
        assert int(net.drop_word) == 3
        runs.append((torch.stack(losses).cpu(), [p.cpu() for p in params]))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    # other masks on the second replay: the same weights and input under word 2 and word 3 give different training outputs
    net.drop_word.fill_(1)
    with torch.no_grad():
        y2 = net(x)
        y3 = net(x)
    assert int(net.drop_word) == 3 and not torch.equal(y2, y3)


def test_test_lidc_scores_the_network_on_image_batches():
    """``test_lidc`` (the ``eval_images: "lidc"`` route of the driver loops) on 7 synthetic RGB images in batches of 3 with 2 classes."""
    from hpfg_amd import val as V
    g = torch.Generator().manual_seed(17)
    lab = torch.randint(0, 2, (7, 6, 6), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)
    lab[:, :4, :4] = 1          # class 1 in every batch
    img = (lab.float().unsqueeze(1) + 0.1 * torch.randn(7, 1, 24, 24, generator=g)).expand(7, 3, 24, 24).contiguous()
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(img, lab.to(torch.uint8)), batch_size=3, shuffle=False)
    net = _net("net2").train()
    args = AttrDict(num_classes=2, test_crop_size=(24, 24), device=DEV)
    dice, hd95 = V.test_lidc(net, loader, args, cur_itrs=1, with_hd95="device")
    print(f"test_lidc on the untrained net2: dice {dice:.4f} hd95 {hd95:.4f}")
    assert np.isfinite(dice) and np.isfinite(hd95) and 0.0 <= dice <= 1.0 and hd95 >= 0.0
    assert net.training          # the mode it found
