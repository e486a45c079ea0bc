"""CPU: the LIDC Swin-UNet (patch 2, window 3 / 4) without a GPU -- state_dict keys, order, shapes and seeded init of ``get_swinunet_LIDC``
against the reference's hashes (tests/golden/swinunet_lidc.json, tools/make_golden_swinunet_lidc.py), ``build_model("swinunet_lidc")``, the
``packed`` flag of every WindowAttention (the factory's measured per-stage choice), ``patch_size`` in the assembly, the new config, the
refusals of ``window_attention_packed`` before any launch."""
import hashlib
import json
import os
from functools import partial

import pytest
import torch
import torch.nn as nn
import yaml

from hpfg_amd.model import FinalPatchExpanding, SwinUnet, SwinUnet_Plus, WindowAttention, build_model, get_swinunet, get_swinunet_LIDC
from hpfg_amd.model.swinunet import LIDC_PACKED
from hpfg_amd.ops_tokens import window_attention_packed
from hpfg_amd.utils import AttrDict, loadyaml
from oracle.make_golden import REF          # where the fixture tools look for the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_CONFIG = os.path.join(os.environ.get("HPFG_REFERENCE", REF), "config", "swinunet_30k_96x96_LIDC.yaml")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "swinunet_lidc.json")) as f:
        return json.load(f)


def _same_as_reference(sd, want):
    assert list(sd.keys()) == list(want.keys())
    for k, w in want.items():
        v = sd[k]
        assert list(v.shape) == w["shape"] and str(v.dtype).split(".")[1] == w["dtype"], k
        assert hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() == w["sha256"], k


def _attentions(net):
    return [m for m in net.modules() if isinstance(m, WindowAttention)]


@pytest.mark.parametrize("case,side,window", [("lidc96", 96, 3), ("lidc64", 64, 4)])
def test_seeded_factory_is_the_references(meta, case, side, window):
    torch.manual_seed(meta["seeds"][case])
    net = get_swinunet_LIDC(side, in_channels=3, num_classes=2)
    _same_as_reference(net.state_dict(), meta[case])
    att = _attentions(net)
    assert len(att) == 12 + 10 and all(a.window_size == window and a.attn_drop == 0.1 for a in att)
    assert net.encoder.patch_embed.proj.weight.shape == (96, 3, 2, 2) and net.decoder.final_patch_expanding.factor == 2
    assert net.decoder.norm_up.eps == 1e-6 and net.has_dropout and "drop_word" not in net.state_dict()


@pytest.mark.parametrize("case,window,depths,heads", [("net2", 3, (2, 2), (1, 2)), ("net3", 4, (2, 2, 2), (1, 2, 4))])
def test_small_networks_seeded_init_is_the_references(meta, case, window, depths, heads):
    torch.manual_seed(meta["seeds"][case])
    net = SwinUnet(window_size=window, depths=depths, num_heads=heads, norm_layer=partial(nn.LayerNorm, eps=meta["norm_eps"]), packed=True, **meta["net"])
    _same_as_reference(net.state_dict(), meta[case])
    assert all(a.packed for a in _attentions(net))


@pytest.mark.parametrize("crop,window", [([96, 96], 3), (96, 3), ((64, 64), 4)])
def test_build_model_opens_swinunet_lidc(crop, window):
    net = build_model(AttrDict(model="swinunet_lidc", in_channels=3, num_classes=2, train_crop_size=crop))
    assert type(net) is SwinUnet and net.decoder.head.weight.shape[0] == 2
    att = _attentions(net)
    assert all(a.window_size == window for a in att)
    # the factory's per-stage choice (LIDC_PACKED) follows profiles/swinunet_lidc_timing.txt: every stage packed, except the 4 x 4 map of the
    # 64 x 64 network (one 4 x 4 window per image: packing saves no workgroup there and the measured ranges overlap)
    assert LIDC_PACKED == {3: (True, True, True, True), 4: (True, True, True, False)}
    assert [a.packed for a in att].count(False) == (0 if window == 3 else 2)
    for stage, flag in enumerate(LIDC_PACKED[window]):          # encoder stage i and the decoder stage that mirrors it share the flag
        assert all(b.attn.packed == flag for b in net.encoder.layers[stage].blocks)
    for i, up in enumerate(net.decoder.layers_up):
        assert all(b.attn.packed == LIDC_PACKED[window][2 - i] for b in up.blocks)


def test_other_sizes_and_the_old_keys_stay_refused():
    for side in (224, 128, 48):
        with pytest.raises(NotImplementedError):
            get_swinunet_LIDC(side)
        with pytest.raises(NotImplementedError):
            build_model(AttrDict(model="swinunet_lidc", in_channels=3, num_classes=2, train_crop_size=[side, side]))
    with pytest.raises(NotImplementedError):
        get_swinunet(img_size=96)
    with pytest.raises(NotImplementedError):
        build_model(AttrDict(model="swinunet", in_channels=1, num_classes=4, train_crop_size=[224, 224]))


def test_patch_size_and_packed_defaults_change_nothing_existing():
    fin = FinalPatchExpanding(32, patch_size=2)
    assert fin.expand.weight.shape == (4 * 32, 32) and fin.factor == 2 and fin.norm.weight.shape == (32,)
    old = FinalPatchExpanding(32)
    assert old.expand.weight.shape == (16 * 32, 32) and old.factor == 4
    with pytest.raises(ValueError, match="patch_size 3"):
        FinalPatchExpanding(32, patch_size=3)
    net = SwinUnet_Plus(in_chans=1, num_classes=4, embed_dim=32, depths=(2, 2), num_heads=(1, 2))
    assert not any(a.packed for a in _attentions(net)) and net.decoder.final_patch_expanding.factor == 4
    with pytest.raises(ValueError, match="packed=True is for windows 2 .. 4"):
        WindowAttention(32, 7, 1, packed=True)
    mixed = SwinUnet(patch_size=2, in_chans=3, num_classes=2, embed_dim=32, window_size=3, depths=(2, 2), num_heads=(1, 2), packed=(True, False))
    assert [a.packed for a in _attentions(mixed)] == [True, True, False, False, True, True]
    with pytest.raises(ValueError, match="one flag per stage"):
        SwinUnet(patch_size=2, embed_dim=32, window_size=3, depths=(2, 2), num_heads=(1, 2), packed=(True,))


def test_config_loads_and_carries_the_references_keys():
    a = loadyaml(os.path.join(ROOT, "config", "swinunet_30k_96x96_LIDC.yaml"))
    assert (a.model, a.datasets, a.eval_images, a.opt, a.sched) == ("swinunet_lidc", "sup_synthetic", "lidc", "adamW", "cosine")
    assert (a.batch_size, a.in_channels, a.num_classes, a.train_crop_size, a.synthetic_test_images) == (64, 3, 2, [96, 96], 100)
    net = build_model(a)
    assert type(net) is SwinUnet and all(m.window_size == 3 for m in _attentions(net))
    if not os.path.exists(REFERENCE_CONFIG):
        pytest.skip("the reference checkout is absent: its key set is not compared")
    with open(REFERENCE_CONFIG, encoding="utf-8") as f:
        ref = yaml.safe_load(f)
    assert set(ref) <= set(a), sorted(set(ref) - set(a))
    same = [k for k in ref if k not in ("datasets", "data_path", "save_path", "name", "num_workers")]          # the data source is synthetic here
    assert {k: a[k] for k in same} == {k: ref[k] for k in same}


def test_window_attention_packed_refuses_before_any_launch():
    with pytest.raises(ValueError, match="outside 2 .. 4"):
        window_attention_packed(torch.zeros(1, 10, 10, 96), torch.zeros(81, 1), 1, 5, 0, 1.0)
    with pytest.raises(ValueError, match="divisible by the window"):
        window_attention_packed(torch.zeros(1, 10, 10, 96), torch.zeros(25, 1), 1, 3, 0, 1.0)
    with pytest.raises(RuntimeError):          # a CPU tensor: the kernels have no CPU fallback
        window_attention_packed(torch.zeros(1, 9, 9, 96), torch.zeros(25, 1), 1, 3, 0, 1.0)
