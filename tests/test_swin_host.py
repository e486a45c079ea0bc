"""CPU: the Swin modules' constructors against the reference's (tests/golden/swin_block.npz, swin_stage.npz written by
tools/make_golden_swin.py): state_dict keys, order, shapes and seeded initial values; every refusal of the window-attention op and of the
modules is raised before anything is launched; build_model still refuses "swinunet"."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hpfg_amd.model import BasicBlock, Mlp, PatchMerging, SwinTransformerBlock, WindowAttention, build_model
from hpfg_amd.ops_tokens import HEAD_DIMS, MAX_WINDOW_KEYS, gelu, patch_merge, window_attention


class AttrDict(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return np.load(os.path.join(golden_dir, "swin_block.npz")), np.load(os.path.join(golden_dir, "swin_stage.npz"))


def _sd(z, case):
    pre = f"{case}.sd."
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def _same_keys_and_shapes(module, want):
    sd = module.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape and str(sd[k].dtype).split(".")[1] == str(v.dtype), k


def test_state_dict_layout_equals_the_reference(fixtures):
    blocks, stage = fixtures
    _same_keys_and_shapes(SwinTransformerBlock(64, 2, 7, shift=True, mlp_ratio=1.0), _sd(blocks, "plain"))
    _same_keys_and_shapes(SwinTransformerBlock(64, 2, 7, shift=True), _sd(stage, "init"))
    _same_keys_and_shapes(SwinTransformerBlock(32, 1, 7, shift=True, drop_path=0.3), _sd(stage, "droppath"))
    want = _sd(stage, "basic")
    _same_keys_and_shapes(BasicBlock(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2)), want)
    assert "blocks.1.attn.relative_position_index" in want and "downsample.reduction.weight" in want
    assert "downsample.reduction.bias" not in want


def test_seeded_init_is_bit_equal(fixtures):
    want = _sd(fixtures[1], "init")
    torch.manual_seed(7)
    sd = SwinTransformerBlock(64, 2, 7, shift=True).state_dict()
    for k, v in want.items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert sd["attn.relative_position_index"].dtype == torch.int64
    # a stage consumes the generator like the reference too: same seed as the fixture's, same weights before the tool scaled the tables
    want = _sd(fixtures[1], "basic")
    torch.manual_seed(13)
    sd = BasicBlock(index=0, embed_dim=32, depths=(2, 2), num_heads=(1, 2)).state_dict()
    for k, v in want.items():
        if not k.endswith("relative_position_bias_table"):
            assert np.array_equal(sd[k].numpy(), v), k
        else:
            assert np.array_equal((sd[k] * 25.0).numpy(), v), k


def test_relative_position_index_is_the_kernel_law():
    """idx = (i1 - i2 + w - 1)(2w - 1) + (j1 - j2 + w - 1), l = i w + j -- what csrc/attn_window.hip computes from the positions"""
    for w in (2, 4, 7, 8):
        idx = WindowAttention(32, w, 1).relative_position_index
        l = torch.arange(w * w)
        i, j = l // w, l % w
        want = (i[:, None] - i[None, :] + w - 1) * (2 * w - 1) + (j[:, None] - j[None, :] + w - 1)
        assert torch.equal(idx, want)


def test_drop_path_rates_follow_the_reference():
    blk = BasicBlock(index=1, embed_dim=32, depths=(2, 2), num_heads=(1, 2), patch_merging=False)
    want = [r.item() for r in torch.linspace(0, 0.1, 4)][2:]
    assert [b.dpr for b in blk.blocks] == want and blk.downsample is None
    assert [b.attn.shift_size for b in blk.blocks] == [0, 3] and blk.blocks[0].attn.num_heads == 2
    assert blk.blocks[0].norm1.weight.shape == (64,)


def test_window_attention_refusals_come_before_any_launch():
    """CPU tensors: a ValueError naming the limit for every unsupported shape (nothing was launched: there is no GPU here), and the
    usual RuntimeError for a supported shape on the CPU"""
    def call(H, W, C, heads, window, shift):
        return window_attention(torch.zeros(1, H, W, 3 * C), torch.zeros((2 * window - 1) ** 2, heads), heads, window, shift, 1.0)

    assert MAX_WINDOW_KEYS == 64 and HEAD_DIMS == (32, 64)
    with pytest.raises(ValueError, match="at most 64 keys"):
        call(18, 18, 32, 1, 9, 4)                                         # window^2 = 81
    with pytest.raises(ValueError, match="divisible by the window 7"):
        call(15, 15, 32, 1, 7, 0)
    with pytest.raises(ValueError, match=r"square \(H == W\), got 14 x 21"):
        call(14, 21, 32, 1, 7, 0)
    with pytest.raises(ValueError, match=r"head dim 48/1 .*\(32, 64\)"):
        call(14, 14, 48, 1, 7, 0)
    with pytest.raises(ValueError, match="head dim"):
        call(14, 14, 64, 3, 7, 0)                                         # heads do not divide C
    with pytest.raises(ValueError, match=r"shift 2 must be 0 or window // 2 = 3"):
        call(14, 14, 32, 1, 7, 2)
    with pytest.raises(ValueError, match="bias_table"):
        window_attention(torch.zeros(1, 14, 14, 96), torch.zeros(169, 2), 1, 7, 0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(14, 14, 32, 1, 7, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gelu(torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        patch_merge(torch.zeros(1, 4, 4, 8))
    with pytest.raises(ValueError, match="even"):
        patch_merge(torch.zeros(1, 5, 4, 8))


def test_modules_refuse_dropout_and_other_layers():
    with pytest.raises(ValueError, match="attn_drop = 0.1"):
        WindowAttention(32, 7, 1, attn_drop=0.1)
    with pytest.raises(ValueError, match="proj_drop = 0.2"):
        WindowAttention(32, 7, 1, proj_drop=0.2)
    with pytest.raises(ValueError, match="drop = 0.1"):
        Mlp(32, 64, drop=0.1)
    with pytest.raises(ValueError, match="drop = 0.1"):
        SwinTransformerBlock(32, 1, drop=0.1)
    with pytest.raises(ValueError, match="attn_drop = 0.1"):
        SwinTransformerBlock(32, 1, attn_drop=0.1)
    with pytest.raises(ValueError, match="drop = 0.5"):
        BasicBlock(index=0, embed_dim=32, depths=(2,), num_heads=(1,), drop_rate=0.5)
    with pytest.raises(ValueError, match="attn_drop = 0.5"):
        BasicBlock(index=0, embed_dim=32, depths=(2,), num_heads=(1,), attn_drop_rate=0.5)
    with pytest.raises(ValueError, match="act_layer"):
        Mlp(32, 64, act_layer=nn.ReLU)
    with pytest.raises(ValueError, match="norm_layer"):
        PatchMerging(32, norm_layer=nn.BatchNorm1d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SwinTransformerBlock(32, 1)(torch.zeros(1, 7, 7, 32))


def test_build_model_still_refuses_swinunet():
    with pytest.raises(NotImplementedError):
        build_model(AttrDict(model="swinunet", in_channels=1, num_classes=4, train_crop_size=[224, 224]))
