"""CPU: the Swin-MAE assembly without a GPU -- ``build_model("swinmae")`` and the small fixture network against the reference's keys, shapes
and seeded-init hashes (tests/golden/swinmae.json, tools/make_golden_swinmae.py), the float64 sin-cos table, the kept-group count, the shipped
config through loadyaml -> build_model -> build_optimizer -> build_lr_scheduler, the constructor's refusals, argument refusals of the new
ops before any launch, the flat-buffer order of a network with a frozen parameter, the ABI."""
import hashlib
import json
import math
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from hpfg_amd import _lib as L
from hpfg_amd.model import SwinMAE, build_model, swin_mae
from hpfg_amd.model.swin_mae import sincos_2d
from hpfg_amd.ops_tokens import mae_keep_count, mae_loss, mae_mask_tokens, mae_window_mask
from hpfg_amd.utils import AttrDict, build_lr_scheduler, build_optimizer, loadyaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("hpfg_mae_window_mask", "hpfg_mae_mask_tokens_fwd", "hpfg_mae_mask_tokens_bwd", "hpfg_mae_mask_tokens_bwd_blocks", "hpfg_mae_loss",
                    "hpfg_mae_loss_blocks")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "swinmae.json")) as f:
        return json.load(f)


def _same_as_reference(sd, want):
    assert set(sd.keys()) == set(want.keys()) and list(sd.keys()) == list(want.keys())
    for k, w in want.items():
        v = sd[k]
        assert list(v.shape) == w["shape"] and str(v.dtype).split(".")[1] == w["dtype"], k
        assert hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() == w["sha256"], k


def _small(meta, **over):
    kw = dict(meta["net_kwargs"], norm_layer=partial(nn.LayerNorm, eps=meta["norm_eps"]))
    kw.update(depths=tuple(kw["depths"]), num_heads=tuple(kw["num_heads"]))
    kw.update(over)
    return SwinMAE(**kw)


def test_build_model_swinmae_is_the_references_network(meta):
    torch.manual_seed(meta["seeds"]["mae224"])
    net = build_model(AttrDict(model="swinmae", in_channels=1, mask_ratio=0.5, num_classes=4, train_crop_size=[224, 224]))
    assert isinstance(net, SwinMAE) and net.mask_ratio == 0.5 and net.in_chans == 1
    _same_as_reference(net.state_dict(), meta["mae224"])
    assert not net.pos_embed.requires_grad and net.mask_token.requires_grad and tuple(net.pos_embed.shape) == (1, 3136, 96)
    assert tuple(net.decoder_pred.weight.shape) == (16, 96) and net.decoder_pred.bias is not None and net.norm_up.eps == 1e-6
    assert not any(k.startswith("skip") for k in net.state_dict())          # no skip connections


def test_small_network_seeded_init_is_the_references(meta):
    torch.manual_seed(meta["seeds"]["net"])
    _same_as_reference(_small(meta).state_dict(), meta["net"])


def test_pos_embed_is_the_float64_sincos_law():
    """The table written out as a law: channel c of token (i, j) of a g x g grid, D channels, omega_k = 10000^(-k / (D / 4)) in float64 --
    [sin(j omega) | cos(j omega) | sin(i omega) | cos(i omega)] (the column coordinate first), rounded to fp32 once."""
    net = swin_mae(in_channels=1, mask_ratio=0.5)
    g, D = 56, 96
    q = D // 4
    want = np.empty((g * g, D), dtype=np.float64)
    omega = 1.0 / 10000 ** (np.arange(q, dtype=np.float64) / q)
    for i in range(g):
        for j in range(g):
            want[i * g + j] = np.concatenate([np.sin(j * omega), np.cos(j * omega), np.sin(i * omega), np.cos(i * omega)])
    table = sincos_2d(D, g)
    # a few float64 ulps of values in [-1, 1] (sin / cos of a scalar and of an array may take different library paths); a float32 table is
    # off by ~1e-6 at the largest arguments
    assert table.dtype == np.float64 and table.shape == want.shape and float(np.abs(table - want).max()) <= 1e-15
    assert torch.equal(net.pos_embed[0], torch.from_numpy(table).float())
    assert math.isclose(float(net.pos_embed[0, 57, 0]), math.sin(1.0), rel_tol=1e-7)          # token (1, 1): column coordinate 1, omega_0 = 1


@pytest.mark.parametrize("d,ratio", [(14, 0.5), (14, 0.75), (14, 0.6), (8, 0.5), (1, 0.5)])
def test_keep_count_is_the_references_python_expression(d, ratio):
    assert mae_keep_count(d, ratio) == int(d ** 2 * (1 - ratio))
    if (d, ratio) == (14, 0.6):
        assert mae_keep_count(d, ratio) == 78          # 196 * 0.4 = 78.4: truncated, not rounded
    if d == 14:
        net = swin_mae(in_channels=1, mask_ratio=ratio)
        assert net.keep_count(56) == mae_keep_count(14, ratio) and net.masked_per_image(56) == 3136 - 16 * mae_keep_count(14, ratio)


def test_shipped_config_builds_model_optimizer_and_scheduler():
    args = loadyaml(os.path.join(ROOT, "config", "swinmae_30k_224x224_ACDC.yaml"))
    assert (args.model, args.opt, args.sched, args.mask_ratio, args.in_channels, args.batch_size) == ("swinmae", "adamW", "cosine", 0.5, 1, 16)
    assert (args.lr, args.weight_decay, args.total_itrs, args.step_size, args.norm_pix_loss) == (0.0001, 0.05, 30000, 500, False)
    net = build_model(args)
    assert isinstance(net, SwinMAE) and net.mask_ratio == 0.5
    opt = build_optimizer(args=args, model=net)          # on the host: torch's AdamW (the device gets FusedAdamW)
    assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 0.05
    sched = build_lr_scheduler(args=args, optimizer=opt)
    sched.step()
    assert 0.0 < opt.param_groups[0]["lr"] <= args.lr


def test_constructor_refuses_what_the_assembly_cannot_run(meta):
    with pytest.raises(ValueError, match="four stages"):
        _small(meta, depths=(2, 2, 2), num_heads=(1, 2, 4))
    with pytest.raises(ValueError, match=r"decoder_embed_dim = 512 must be 8 \* embed_dim = 256"):
        _small(meta, decoder_embed_dim=512)
    with pytest.raises(ValueError, match="masking group"):
        _small(meta, img_size=120, window_size=2)          # token side 30: not divisible by r = 4
    with pytest.raises(ValueError, match="divisible by the window"):
        _small(meta, img_size=160, window_size=4)          # token sides 40 / 20 / 10 / 5: the last is no multiple of 4
    with pytest.raises(ValueError, match="divisible by the window"):
        _small(meta, img_size=112, window_size=7)          # 28 / 14 / 7 / 3.5: the last stage has no whole side
    with pytest.raises(ValueError, match="at most 64 keys"):
        _small(meta, img_size=288, window_size=9)          # what the window kernels refuse
    with pytest.raises(ValueError, match="head dim"):
        _small(meta, num_heads=(2, 2, 4, 8))          # head dim 16
    with pytest.raises(ValueError, match="patch_size"):
        _small(meta, patch_size=8)
    with pytest.raises(ValueError, match="in_chans"):
        _small(meta, in_chans=5)
    with pytest.raises(ValueError, match="mask_ratio"):
        _small(meta, mask_ratio=1.0)
    with pytest.raises(ValueError, match="dropout"):
        _small(meta, drop_rate=0.1)
    with pytest.raises(ValueError, match="norm_layer"):
        _small(meta, norm_layer=None)
    net = _small(meta)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 1, 128, 128))


def test_new_ops_refuse_bad_arguments_before_any_launch():
    """CPU tensors: a ValueError naming the limit (nothing was launched: there is no GPU here), the usual RuntimeError for a supported call."""
    with pytest.raises(ValueError, match="multiple of the group side"):
        mae_window_mask(torch.zeros(1, 4), 9, 4, 1)
    with pytest.raises(ValueError, match="at most 1024"):
        mae_window_mask(torch.zeros(1, 33 * 33), 132, 4, 1)
    with pytest.raises(ValueError, match=r"noise \(1, 5\)"):
        mae_window_mask(torch.zeros(1, 5), 8, 4, 1)
    with pytest.raises(ValueError, match="n_keep = 5"):
        mae_window_mask(torch.zeros(1, 4), 8, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mae_window_mask(torch.zeros(1, 4), 8, 4, 2)
    x, m8, tok = torch.zeros(2, 4, 8), torch.zeros(2, 4, dtype=torch.uint8), torch.zeros(1, 1, 8)
    with pytest.raises(ValueError, match="C = 6"):
        mae_mask_tokens(torch.zeros(2, 4, 6), m8, torch.zeros(6))
    with pytest.raises(ValueError, match="C = 1540"):
        mae_mask_tokens(torch.zeros(1, 1, 1540), m8[:1, :1], torch.zeros(1540))
    with pytest.raises(ValueError, match="mask token"):
        mae_mask_tokens(x, m8, torch.zeros(4))
    with pytest.raises(ValueError, match="uint8"):
        mae_mask_tokens(x, m8.float(), tok)
    with pytest.raises(ValueError, match="8 elements"):
        mae_mask_tokens(x, m8[:1], tok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mae_mask_tokens(x, m8, tok)
    img, pred, m = torch.zeros(2, 1, 8, 8), torch.zeros(2, 4, 16), torch.zeros(2, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="Cin"):
        mae_loss(torch.zeros(2, 4, 80), torch.zeros(2, 5, 8, 8), m, 1.0)
    with pytest.raises(ValueError, match="divisible by the patch"):
        mae_loss(pred, torch.zeros(2, 1, 8, 6), m, 1.0)
    with pytest.raises(ValueError, match=r"pred \(2, 4, 48\)"):
        mae_loss(torch.zeros(2, 4, 48), img, m, 1.0)
    with pytest.raises(ValueError, match="uint8"):
        mae_loss(pred, img, m.bool(), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mae_loss(pred, img, m, 1.0)


def test_frozen_parameters_lie_behind_the_trainable_ones_in_the_flat_buffer(meta):
    """``pos_embed`` is the first entry of ``parameters()`` and never gets a gradient: the flat layout moves it to the end, where an update
    over the leading trainable range leaves it alone.  All-trainable and all-frozen modules keep ``parameters()`` order."""
    from hpfg_amd.utils.optim import flat_order, flatten_parameters
    net = _small(meta)
    ps = list(net.parameters())
    assert ps[0] is net.pos_embed
    order = flat_order(net)
    assert order[-1] is net.pos_embed and order[:-1] == ps[1:]
    flatten_parameters(net)
    n_train = sum(p.numel() for p in ps if p.requires_grad)
    assert net.flat_params.numel() == n_train + net.pos_embed.numel()
    assert net.pos_embed.data_ptr() == net.flat_params[n_train:].data_ptr() and net.mask_token.data_ptr() == net.flat_params.data_ptr()
    lin = nn.Linear(3, 2)
    assert flat_order(lin) == list(lin.parameters())
    for p in lin.parameters():
        p.requires_grad = False
    assert flat_order(lin) == list(lin.parameters())


def test_swinmae_step_refuses_data_parallel(meta):
    from hpfg_amd.train import SwinMAEStep, Swin_MAE          # noqa: F401  (the loop is importable)
    with pytest.raises(NotImplementedError, match="data parallel"):
        SwinMAEStep(_small(meta), AttrDict(), dp=object())


def test_every_new_entry_point_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    assert "model/swin_mae.py:649-710" in src and "model/swin_mae.py:706-709" in src and "model/swin_mae.py:775-791" in src      # the lines they replace
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/hpfg_hip.h"
        assert name in L.PROTOTYPES and hasattr(lib, name), name
    assert lib.hpfg_mae_mask_tokens_bwd_blocks(16) == 1 and lib.hpfg_mae_mask_tokens_bwd_blocks(3136) == 49 and lib.hpfg_mae_mask_tokens_bwd_blocks(10 ** 6) == 512
    assert lib.hpfg_mae_loss_blocks(16, 224, 224, 4) == 196 and lib.hpfg_mae_loss_blocks(3, 16, 16, 4) == 1
    assert lib.hpfg_mae_loss_blocks(1, 18, 16, 4) == -1 and b"mae_loss_blocks" in lib.hpfg_last_error()
    # null pointers and shapes are refused by the library itself before anything is launched
    assert lib.hpfg_mae_window_mask(None, None, 1, 8, 4, 1, None) == -1 and b"mae_window_mask" in lib.hpfg_last_error()
    p = 256          # never dereferenced: the checks below fail first
    assert lib.hpfg_mae_window_mask(p, p, 1, 9, 4, 1, None) == -1 and lib.hpfg_mae_window_mask(p, p, 1, 132, 4, 1, None) == -1
    assert lib.hpfg_mae_window_mask(p, p, 1, 8, 4, 5, None) == -1 and b"n_keep" in lib.hpfg_last_error()
    assert lib.hpfg_mae_mask_tokens_fwd(p, p, p, p, 4, 6, None) == -1 and lib.hpfg_mae_mask_tokens_bwd(p, p, p, p, p, 4, 1540, None) == -1
    assert lib.hpfg_mae_loss(p, p, p, 1.0, 0, p, p, p, 1, 5, 16, 16, 4, None) == -1 and b"channels" in lib.hpfg_last_error()
    assert lib.hpfg_mae_loss(p, p, p, 1.0, 0, p, p, p, 1, 1, 16, 16, 8, None) == -1
