"""GPU: the Swin-MAE assembly (hpfg_amd/model/swin_mae.py) and its training step against the reference's fixtures
(tools/make_golden_swinmae.py).  The small network replays the recorded masking noise and drop-path draws: the mask must be exact; ``pred``,
the driver's loss, ``forward_loss`` with ``norm_pix_loss`` both ways and the stored gradients are held to the rule tests/test_gpu_swinunet.py
applies to its net2 case, restated here: per tensor 1e-3 max(1, max |reference|), in both math modes.  ``forward`` returns the reference's
``(pred_img, mask_img)``; ``SwinMAEStep`` replays three recorded AdamW iterations; ``GraphedStep(SwinMAEStep)`` equals the eager step bit for
bit under injected noise and draws a new mask of the right size in every replay.  The weights are rebuilt from the recorded seed;
tests/test_swinmae_host.py holds the seeded init to the reference's hashes."""
import functools
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from hpfg_amd import ops_tokens
from hpfg_amd.model import SwinMAE
from hpfg_amd.utils import AttrDict
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_KEYS = ("mask_token", "patch_embed.proj.weight", "decoder_pred.weight", "decoder_pred.bias", "layers.0.blocks.0.attn.qkv.weight",
             "layers.1.blocks.0.attn.qkv.weight", "layers.2.blocks.0.attn.qkv.weight")
GRAD_ROWS4 = ("layers.3.blocks.0.attn.qkv.weight",)          # stored as every fourth row (the file size limit)
OPT = dict(opt="adamW", lr=1e-4, weight_decay=0.05, momentum=0.9, sched="cosine", warmup_epochs=0, warmup_lr=1e-5, min_lr=1e-4, total_itrs=30000,
           step_size=500)          # min_lr = lr: the cosine table stays at the trace's constant 1e-4


@functools.lru_cache(maxsize=None)
def _meta():
    with open(os.path.join(GOLDEN, "swinmae.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def _net(**over):
    m = _meta()
    kw = dict(m["net_kwargs"], norm_layer=partial(nn.LayerNorm, eps=m["norm_eps"]))
    kw.update(depths=tuple(kw["depths"]), num_heads=tuple(kw["num_heads"]))
    kw.update(over)
    torch.manual_seed(m["seeds"]["net"])
    return SwinMAE(**kw).to(DEV).train()


def _draws(arr):
    return [tuple(torch.from_numpy(r) for r in pair) for pair in arr]


def _check(what, got, want):
    want = torch.as_tensor(want)
    err, bound = maxerr(got.detach().cpu(), want), 1e-3 * max(1.0, float(want.abs().max()))
    print(f"{what}: {err:.2e} (<= {bound:.2e})")
    assert err <= bound, what


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_small_network_mask_pred_losses_and_gradients(math):
    z = _fixture("swinmae_net")
    net = _net()
    net.external_noise, net.external_draws = torch.from_numpy(z["noise"]), _draws(z["draws"])
    x = torch.from_numpy(z["x"]).to(DEV)
    ops_tokens.MATH["mode"] = math
    try:
        loss, pred, mask = net.reconstruction_loss(x, with_parts=True)
        loss.backward()
        with torch.no_grad():
            model_loss = net.forward_loss(x, pred, mask, n_masked=x.shape[0] * net.masked_per_image(32))
            counted = net.forward_loss(x, pred, mask)          # counts the mask on the device instead
            net.norm_pix_loss = True
            model_loss_np = net.forward_loss(x, pred, mask)
    finally:
        ops_tokens.MATH["mode"] = None
    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), torch.from_numpy(z["mask"]))
    assert tuple(pred.shape) == (2, 1024, 16) and loss.dim() == 0
    _check(f"{math} pred", pred, z["pred"])
    _check(f"{math} driver loss", loss, z["loss_driver"])
    _check(f"{math} forward_loss", model_loss, z["loss_model"])
    _check(f"{math} forward_loss norm_pix", model_loss_np, z["loss_model_norm_pix"])
    assert torch.equal(model_loss, counted)
    grads = dict(net.named_parameters())
    assert net.pos_embed.grad is None
    for k in GRAD_KEYS:
        _check(f"{math} grad.{k}", grads[k].grad, z[f"grad.{k}"])
    for k in GRAD_ROWS4:
        _check(f"{math} grad_rows4.{k}", grads[k].grad[::4], z[f"grad_rows4.{k}"])


def test_forward_returns_the_references_image_pair():
    z = _fixture("swinmae_net")
    net = _net()
    net.external_noise, net.external_draws = torch.from_numpy(z["noise"]), _draws(z["draws"])
    x = torch.from_numpy(z["x"]).to(DEV)
    with torch.no_grad():
        pred_img, mask_img = net(x)
    assert tuple(pred_img.shape) == tuple(mask_img.shape) == (2, 1, 128, 128) and mask_img.dtype == torch.float32
    mask = torch.from_numpy(z["mask"]).float()
    want = net.unpatchify(mask.unsqueeze(-1).repeat(1, 1, 16))
    assert torch.equal(mask_img.cpu(), want)
    # unpatchify written out: pixel (4 h + p, 4 w + q) of the mask image is token h * 32 + w
    assert torch.equal(want[:, 0], mask.reshape(2, 32, 32).repeat_interleave(4, 1).repeat_interleave(4, 2))
    _check("pred_img", net.patchify(pred_img), z["pred"])


def _step(net):
    from hpfg_amd.train import SwinMAEStep
    return SwinMAEStep(net, AttrDict(dict(OPT, device="cuda:0")))


def test_step_replays_the_recorded_adamw_trace():
    from hpfg_amd.utils.optim import FusedAdamW
    z, t = _fixture("swinmae_net"), _fixture("trace_swinmae")
    net = _net()
    pos = net.pos_embed.detach().clone()
    st = _step(net)
    assert isinstance(st.optimizer, FusedAdamW) and st.optimizer.active_numel == net.flat_params.numel() - net.pos_embed.numel()
    x = torch.from_numpy(z["x"]).to(DEV)
    for i in range(3):
        net.external_noise, net.external_draws = torch.from_numpy(t["noise"][i]), _draws(t["draws"][i])
        r = st.step(x, i + 1)
        err = abs(float(r["loss"]) - float(t["loss"][i]))
        print(f"trace iteration {i}: loss {float(r['loss']):.6f} reference {float(t['loss'][i]):.6f} error {err:.2e}")
        assert err <= 1e-3
    _check("final mask_token", net.mask_token, t["mask_token"])
    assert torch.equal(net.pos_embed, pos), "the frozen pos_embed is neither stepped nor decayed"


def test_graphed_step_equals_eager_bitwise_under_injected_noise():
    from hpfg_amd.train import GraphedStep
    z, t = _fixture("swinmae_net"), _fixture("trace_swinmae")
    x = torch.from_numpy(z["x"]).to(DEV)
    noise = torch.from_numpy(t["noise"][0]).to(DEV)          # a device tensor the captured graph reads in place
    runs = []
    for graphed in (True, False):
        net = _net()
        net.external_noise, net.external_draws = noise, [tuple(d.to(DEV) for d in pair) for pair in _draws(t["draws"][0])]
        st = _step(net)
        losses = [st.step(x, 1)["loss"].clone()]          # iteration 1 eager in both runs, as the driver loop does
        runner = GraphedStep(st, [x], warmup=0) if graphed else None
        for i in (2, 3):
            r = runner.step([x], i) if graphed else st.step(x, i)
            losses.append(r["loss"].clone())
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), net.flat_params.detach().cpu().clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


def test_graph_replays_draw_new_masks_of_the_right_size():
    from hpfg_amd.train import GraphedStep
    z = _fixture("swinmae_net")
    x = torch.from_numpy(z["x"]).to(DEV)
    net = _net()
    st = _step(net)
    torch.manual_seed(5)
    st.step(x, 1)
    runner = GraphedStep(st, [x], warmup=0)
    masks = []
    for i in (2, 3, 4):
        r = runner.step([x], i)
        torch.cuda.synchronize()
        assert torch.isfinite(r["loss"])
        masks.append(r["mask"].cpu().clone())
    ones = 1024 - net.keep_count(32) * 16
    assert ones == 512
    for m in masks:
        assert m.sum(1).tolist() == [ones, ones]
        groups = m.reshape(2, 8, 4, 8, 4)          # whole 4 x 4 groups are removed or kept
        assert torch.equal(groups, groups[:, :, :1, :, :1].expand_as(groups))
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])


def test_swin_mae_loop_trains_from_the_shipped_config_under_one_graph(tmp_path):
    """``"swinmae"`` from config/swinmae_30k_224x224_ACDC.yaml (batch cut to 2 for the test), five iterations under ``Swin_MAE``: iteration 1
    eager, the step captured once at iteration 2, the reference's scalar names logged, the checkpoint written at the evaluation cadence."""
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.model import build_model
    from hpfg_amd.train import Swin_MAE
    from hpfg_amd.utils import loadyaml

    class _Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(str(msg))

        warning = info

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    a = loadyaml(os.path.join(root, "config", "swinmae_30k_224x224_ACDC.yaml"))
    a.update(batch_size=2, synthetic_labeled=4, synthetic_test_volumes=1, total_itrs=4, step_size=2, log_every=2, device="cuda:0", save_path=str(tmp_path),
             logger=_Log())
    torch.manual_seed(a.seed)
    net = build_model(a).to(DEV)
    before = net.flat_params.clone() if hasattr(net, "flat_params") else torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    train_loader, test_loader = build_loader(a)
    log = Swin_MAE(net, train_loader, test_loader, a)
    torch.cuda.synchronize()
    assert not any("capture unavailable" in ln for ln in a.logger.lines), a.logger.lines
    assert log.shape == (5,) and torch.isfinite(log).all() and float(log.min()) > 0.0
    after = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert after.numel() == before.numel() and not torch.equal(after, before)
    ck = torch.load(os.path.join(str(tmp_path), "model", "supervise_model.pth"), map_location="cpu", weights_only=False)
    assert set(ck["model"].keys()) == set(net.state_dict().keys()) and "optimizer" in ck
