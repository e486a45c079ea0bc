"""CPU: Uniformer_Plus is constructed like the reference's (tests/golden/uniformer_plus.npz holds the reference's state_dict keys and shapes,
tools/make_golden_uniformer.py), its size rules raise before any launch, build_model opens the key, and the new entry points are declared
and bound."""
import os
import re

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens as T
from hpfg_amd.model import Uniformer_Plus, build_model, uniformer_small
from hpfg_amd.utils import AttrDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hpfg_dwconv_fwd", "hpfg_dwconv_bwd", "hpfg_dwconv_bwd_blocks", "hpfg_bn_tok_stats", "hpfg_bn_tok_apply", "hpfg_bn_tok_bwd")


def _args(side, **kw):
    return AttrDict(model="uniformer_plus", in_channels=1, num_classes=4, train_crop_size=[side, side], **kw)


def test_build_model_returns_uniformer_plus():
    m = build_model(_args(128))
    assert isinstance(m, Uniformer_Plus) and m.side == 128 and not m.skip_necks and m.external_draws is None


@pytest.mark.parametrize("side", [128, 160])
def test_state_dict_keys_and_shapes_are_the_references(side):
    d = np.load(os.path.join(ROOT, "tests", "golden", "uniformer_plus.npz"))
    sd = Uniformer_Plus([side, side], 1, 4).state_dict()
    assert list(sd) == [str(k) for k in d["keys"]]
    assert [list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()] == d["shapes"].tolist()


def test_parameter_order_and_counts():
    d = np.load(os.path.join(ROOT, "tests", "golden", "uniformer_plus.npz"))
    m = Uniformer_Plus([128, 128], 1, 4)
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in d["param_names"]]
    assert sum(p.numel() for p in m.parameters()) == int(d["n_params"])
    lead = [p for part in (m.encoder, m.decoder) for p in part.parameters()]
    assert all(a is b for a, b in zip(lead, m.parameters())) and m.backbone_numel() == sum(p.numel() for p in lead)


def test_uniformer_small_settings():
    enc = uniformer_small(img_size=128, in_chans=1)
    assert enc.depth == [3, 4, 8, 3] and enc.embed_dims == [64, 128, 320, 512]
    blocks = [b for s in range(4) for b in getattr(enc, f"blocks{s + 1}")]
    rates = [b.dpr for b in blocks]
    assert len(blocks) == 18 and rates[0] == 0.0 and abs(rates[-1] - 0.1) < 1e-7 and all(b > a for a, b in zip(rates, rates[1:]))
    assert [b.attn.num_heads for b in enc.blocks3] == [5] * 8 and [b.attn.num_heads for b in enc.blocks4] == [8] * 3
    assert enc.blocks3[0].attn.qkv.bias is not None and enc.blocks3[0].norm1.eps == 1e-6 and enc.patch_embed1.norm.eps == 1e-5
    assert not any("gamma_1" in k for k in enc.state_dict())


def test_a_seed_gives_the_same_weights_twice():
    torch.manual_seed(3)
    a = Uniformer_Plus([128, 128], 1, 4).state_dict()
    torch.manual_seed(3)
    b = Uniformer_Plus([128, 128], 1, 4).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("size,word", [([96, 96], "at least 128"), ([288, 288], "at most 256"), ([224, 192], "square"), ([144, 144], "multiple of 32")])
def test_size_rules_raise_at_construction(size, word):
    with pytest.raises(ValueError, match=word):
        Uniformer_Plus(size, 1, 4)
    with pytest.raises(ValueError, match=word):
        build_model(AttrDict(model="uniformer_plus", in_channels=1, num_classes=4, train_crop_size=size))


@pytest.mark.parametrize("shape,word", [((1, 1, 224, 192), "square"), ((1, 1, 96, 96), "at least 128"), ((1, 1, 288, 288), "at most 256"),
                                        ((1, 1, 128, 128), "built for 224")])
def test_size_rules_raise_in_forward(shape, word):
    m = Uniformer_Plus([224, 224], 1, 4)
    with pytest.raises(ValueError, match=word):
        m(torch.zeros(shape))
    with pytest.raises(ValueError, match=word):
        m.val(torch.zeros(shape))


def test_unbuilt_variants_are_refused():
    from hpfg_amd.model import UniFormer
    with pytest.raises(NotImplementedError, match="conv-stem"):
        UniFormer(img_size=128, conv_stem=True)
    with pytest.raises(NotImplementedError, match="drop_rate"):
        UniFormer(img_size=128, drop_rate=0.1)
    with pytest.raises(NotImplementedError, match="head dim 64"):
        UniFormer(img_size=128, head_dim=32)


def test_new_symbols_are_declared_bound_and_cited():
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in L.PROTOTYPES and hasattr(lib, n), n
    assert "model/uniformer.py" in src
    assert lib.hpfg_version() == L.VERSION


def test_block_count_is_host_arithmetic():
    lib = L.load()
    assert lib.hpfg_dwconv_bwd_blocks(32, 56, 56, 3) == 512 and lib.hpfg_dwconv_bwd_blocks(2, 7, 7, 5) == 2
    assert lib.hpfg_dwconv_bwd_blocks(0, 7, 7, 5) == 0 and lib.hpfg_dwconv_bwd_blocks(2, 7, 7, 4) == 0


def test_ops_refuse_host_tensors():
    x = torch.zeros(1, 4, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.dwconv(x, torch.zeros(8, 1, 3, 3), torch.zeros(8), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.batch_norm_tokens(x, torch.ones(8), torch.zeros(8), 1e-5)
