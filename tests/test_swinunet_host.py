"""CPU: the Swin-UNet assembly without a GPU -- state_dict keys, order, shapes and seeded init against the reference's hashes
(tests/golden/swinunet.json, tools/make_golden_swinunet.py), ``build_model("swinunet_plus")``, the decoder's drop-path rates, the dropout
opt-in of the block constructors, argument refusals of the new ops before any launch, HPFGStep's refusal of mixed triples, the ABI."""
import hashlib
import json
import os
import re
from functools import partial

import pytest
import torch
import torch.nn as nn

from hpfg_amd import _lib as L
from hpfg_amd.model import (BasicBlock, BasicBlockUp, Mlp, PatchMerging, SwinTransformerBlock, SwinUnet, SwinUnet_Plus, WindowAttention, build_model,
                            get_swinunet, get_swinunet_plus)
from hpfg_amd.ops_tokens import expand_layer_norm, layer_norm, token_dropout, window_attention_dropout
from hpfg_amd.utils import AttrDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("hpfg_ln_px_fwd", "hpfg_ln_px_bwd", "hpfg_ln_px_bwd_blocks", "hpfg_token_dropout", "hpfg_attn_window_drop_fwd",
                    "hpfg_attn_window_drop_bwd", "hpfg_attn_window_drop_elems", "hpfg_attn_window_drop_mask")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(ROOT, "tests", "golden", "swinunet.json")) as f:
        return json.load(f)


def _same_as_reference(sd, want):
    assert list(sd.keys()) == list(want.keys())
    for k, w in want.items():
        v = sd[k]
        assert list(v.shape) == w["shape"] and str(v.dtype).split(".")[1] == w["dtype"], k
        assert hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() == w["sha256"], k


def test_plus224_state_dict_is_the_references(meta):
    torch.manual_seed(meta["seeds"]["plus224"])
    net = get_swinunet_plus(224, in_channels=1, num_classes=4)
    _same_as_reference(net.state_dict(), meta["plus224"])
    assert net.encoder.layers[2].downsample.norm.weight.shape == (1536,) and net.decoder.norm_up.eps == 1e-6
    assert "drop_word" not in net.state_dict() and net.drop_word.dtype == torch.int32
    assert net.backbone_numel() == sum(p.numel() for n, p in net.named_parameters() if n.startswith(("encoder.", "decoder.")))
    seeds = _site_seeds(net)
    assert len(seeds) == 1 + 4 * (12 + 10) and len(set(seeds)) == len(seeds)          # pos_drop + four sites in each of 12 + 10 blocks, no seed twice


@pytest.mark.parametrize("case,depths,heads", [("net2", (2, 2), (1, 2)), ("net3", (2, 2, 2), (1, 2, 4))])
def test_small_networks_seeded_init_is_the_references(meta, case, depths, heads):
    torch.manual_seed(meta["seeds"][case])
    net = SwinUnet(depths=depths, num_heads=heads, norm_layer=partial(nn.LayerNorm, eps=meta["norm_eps"]), **meta["net"])
    _same_as_reference(net.state_dict(), meta[case])


def _site_seeds(net):
    return [net.encoder.pos_drop_seed] + [s for m in net.modules() if hasattr(m, "drop_seeds") for s in m.drop_seeds]


def test_every_network_instance_has_a_dropout_stream_of_its_own(meta):
    """Two networks built after one manual_seed and a deepcopy of one (the EMA teacher) share no layer seed, so they draw independent masks
    for equal input; the base seed comes from the instance counter, not the torch generator: the first network keeps the reference's
    hashes, the copy keeps its source's weights, and restarting the counter reproduces the seeds."""
    from copy import deepcopy
    from hpfg_amd.model import reset_dropout_streams
    kw = dict(depths=(2, 2), num_heads=(1, 2), norm_layer=partial(nn.LayerNorm, eps=meta["norm_eps"]), **meta["net"])

    def three():
        reset_dropout_streams()
        torch.manual_seed(meta["seeds"]["net2"])
        a, b = SwinUnet(**kw), SwinUnet(**kw)
        return a, b, deepcopy(b)

    a, b, c = three()
    _same_as_reference(a.state_dict(), meta["net2"])
    assert all(torch.equal(x, y) for x, y in zip(b.state_dict().values(), c.state_dict().values()))
    assert c.drop_word is not b.drop_word and c.encoder.layers[0] is not b.encoder.layers[0]
    seeds = [_site_seeds(n) for n in (a, b, c)]
    flat = [s for row in seeds for s in row]
    assert len({a.dropout_seed, b.dropout_seed, c.dropout_seed}) == 3 and len(set(flat)) == len(flat) == 3 * (1 + 4 * 6)
    assert [_site_seeds(n) for n in three()] == seeds
    # stages used on their own: the blocks differ from each other
    st = BasicBlock(index=0, embed_dim=32, depths=(2,), num_heads=(1,), drop_rate=0.1, attn_drop_rate=0.1, allow_dropout=True)
    own = [s for m in st.modules() if hasattr(m, "drop_seeds") for s in m.drop_seeds]
    assert len(set(own)) == len(own) == 8


def test_build_model_opens_swinunet_plus_only():
    args = AttrDict(model="swinunet_plus", in_channels=1, num_classes=4, train_crop_size=[224, 224])
    net = build_model(args)
    assert isinstance(net, SwinUnet_Plus) and net.encoder.layers[0].blocks[1].attn.window_size == 7
    assert net.encoder.layers[0].blocks[0].attn.attn_drop == 0.1 and net.encoder.drop_rate == 0.1 and net.has_dropout
    args.train_crop_size = [256, 256]
    assert build_model(args).decoder.layers_up[0].blocks[0].attn.window_size == 8
    args.train_crop_size = [192, 192]
    with pytest.raises(NotImplementedError):
        build_model(args)
    with pytest.raises(NotImplementedError):
        get_swinunet(img_size=192)
    with pytest.raises(NotImplementedError):
        build_model(AttrDict(model="swinunet", in_channels=1, num_classes=4, train_crop_size=[224, 224]))


def test_decoder_drop_path_rates_mirror_the_encoder():
    """BasicBlockUp i takes the slice of encoder stage len(depths) - i - 2 (reference model/swinunet.py:348-354)."""
    depths = (2, 2, 6, 2)
    dpr = [r.item() for r in torch.linspace(0, 0.2, sum(depths))]
    for i, stage in ((0, 2), (1, 1), (2, 0)):
        up = BasicBlockUp(index=i, embed_dim=32, depths=depths, num_heads=(1, 2, 4, 8), drop_path=0.2, patch_expanding=i < 2)
        assert [b.dpr for b in up.blocks] == dpr[sum(depths[:stage]):sum(depths[:stage + 1])]
        assert up.blocks[0].norm1.weight.shape == (32 * 2 ** stage,) and isinstance(up.upsample, nn.Identity) == (i == 2)
    net = get_swinunet(224, in_channels=1)
    assert [b.dpr for b in net.decoder.layers_up[0].blocks] == [b.dpr for b in net.encoder.layers[2].blocks]


def test_constructors_take_dropout_only_with_the_opt_in():
    for make in (lambda **k: WindowAttention(32, 7, 1, attn_drop=0.1, **k), lambda **k: WindowAttention(32, 7, 1, proj_drop=0.2, **k),
                 lambda **k: Mlp(32, 64, drop=0.1, **k), lambda **k: SwinTransformerBlock(32, 1, drop=0.1, attn_drop=0.1, **k),
                 lambda **k: BasicBlock(index=0, embed_dim=32, depths=(2,), num_heads=(1,), drop_rate=0.5, **k),
                 lambda **k: BasicBlockUp(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2), attn_drop_rate=0.5, **k)):
        with pytest.raises(ValueError, match="allow_dropout"):
            make()
        make(allow_dropout=True)
    with pytest.raises(ValueError, match=r"must be in \[0, 1\)"):
        Mlp(32, 64, drop=1.0, allow_dropout=True)
    blk = SwinTransformerBlock(32, 1, drop=0.1, attn_drop=0.2, allow_dropout=True)
    assert (blk.attn.attn_drop, blk.attn.proj_drop, blk.mlp.drop) == (0.2, 0.1, 0.1)
    # norm layers: nn.LayerNorm or a partial of it that sets eps, nothing else
    assert PatchMerging(32, norm_layer=partial(nn.LayerNorm, eps=1e-6)).norm.eps == 1e-6
    with pytest.raises(ValueError, match="norm_layer"):
        PatchMerging(32, norm_layer=partial(nn.LayerNorm, elementwise_affine=False))
    with pytest.raises(ValueError, match="norm_layer"):
        SwinTransformerBlock(32, 1, norm_layer=partial(nn.BatchNorm1d, eps=1e-6))


def test_new_ops_refuse_bad_arguments_before_any_launch():
    """CPU tensors: a ValueError naming the limit (nothing was launched: there is no GPU here), the usual RuntimeError for a supported call."""
    g4, g6 = torch.ones(4), torch.ones(6)
    with pytest.raises(ValueError, match="factor 3"):
        expand_layer_norm(torch.zeros(1, 2, 2, 36), g4, g4, 3, 1e-6)
    with pytest.raises(ValueError, match="C = 1540"):
        expand_layer_norm(torch.zeros(1, 1, 1, 4 * 1540), torch.ones(1540), torch.ones(1540), 2, 1e-6)
    with pytest.raises(ValueError, match="C = 6"):
        layer_norm(torch.zeros(1, 2, 2, 6), g6, g6, 1e-6)
    with pytest.raises(ValueError, match="gamma / beta"):
        expand_layer_norm(torch.zeros(1, 2, 2, 32), g4, g4, 2, 1e-6)
    with pytest.raises(ValueError, match="eps"):
        layer_norm(torch.zeros(1, 2, 2, 4), g4, g4, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        expand_layer_norm(torch.zeros(1, 2, 2, 16), g4, g4, 2, 1e-6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer_norm(torch.zeros(5, 4), g4, g4, 1e-6)          # a [rows, C] matrix is taken at any eps, like the eps 1e-5 route
    with pytest.raises(ValueError, match="multiple of 4"):
        token_dropout(torch.zeros(6), 0.1)
    with pytest.raises(ValueError, match=r"p = 1.0 must be in \[0, 1\)"):
        token_dropout(torch.zeros(8), 1.0)
    with pytest.raises(ValueError, match="mask"):
        token_dropout(torch.zeros(8), 0.1, mask=torch.ones(8))          # not uint8, not on the device
    with pytest.raises(ValueError, match="seed_dev"):
        token_dropout(torch.zeros(8), 0.1, seed_dev=torch.zeros(1, dtype=torch.int32))          # the seed word lives on the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        token_dropout(torch.zeros(8), 0.1)
    qkv, table = torch.zeros(1, 14, 14, 96), torch.zeros(169, 1)
    with pytest.raises(ValueError, match=r"p = -0.1 must be in \[0, 1\)"):
        window_attention_dropout(qkv, table, 1, 7, 0, 1.0, -0.1)
    with pytest.raises(ValueError, match="mask"):
        window_attention_dropout(qkv, table, 1, 7, 0, 1.0, 0.1, mask=torch.ones(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="at most 64 keys"):
        window_attention_dropout(torch.zeros(1, 18, 18, 96), torch.zeros(289, 1), 1, 9, 4, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        window_attention_dropout(qkv, table, 1, 7, 0, 1.0, 0.1)


def test_hpfg_step_refuses_mixed_triples():
    """The kinds are told apart before anything touches a device."""
    from hpfg_amd.model import SegFormer_Plus, UNet_Plus
    from hpfg_amd.train import HPFGStep
    kw = dict(in_chans=1, num_classes=4, embed_dim=32, window_size=8, depths=(2, 2), num_heads=(1, 2))
    sw = [SwinUnet_Plus(**kw) for _ in range(3)]
    with pytest.raises(NotImplementedError, match="mixed SegFormer_Plus / SwinUnet_Plus"):
        HPFGStep(sw[0], SegFormer_Plus(image_size=[128, 128], in_channels=1, num_classes=4), sw[2], AttrDict())
    with pytest.raises(NotImplementedError, match="mixed"):
        HPFGStep(sw[0], sw[1], UNet_Plus(1, 4), AttrDict())
    with pytest.raises(NotImplementedError, match="data parallel"):
        HPFGStep(sw[0], sw[1], sw[2], AttrDict(), dp=object())


def test_every_new_entry_point_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = L.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/hpfg_hip.h"
        assert name in L.PROTOTYPES and hasattr(lib, name), name
    assert lib.hpfg_ln_px_bwd_blocks(30) == lib.hpfg_ln_bwd_blocks(30) and lib.hpfg_ln_px_bwd_blocks(10 ** 6) == 512
    assert lib.hpfg_attn_window_drop_elems(8, 14, 14, 2, 7) == 8 * 4 * 2 * 49 * 49
    assert lib.hpfg_attn_window_drop_elems(1, 15, 14, 1, 7) == -1 and b"attn_window_drop_elems" in lib.hpfg_last_error()
