"""Host-side contract of the attention over 65 .. 256 keys (no GPU): the C entry points are declared and bound, the two caps, the dispatch
rule, the stage-key arithmetic and the size limit, and the 288 x 288 fixtures hold what the GPU tests read."""
import os
import re

import numpy as np
import pytest

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.model import segformer as seg_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpfg_attn_keys_max", "hpfg_attn_keys_fwd", "hpfg_attn_keys_bwd", "hpfg_attn_keys_scratch_floats")


def test_entry_points_are_declared_cited_and_bound():
    src = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    assert int(re.search(r"#define HPFG_VERSION (\d+)", src).group(1)) == L.VERSION >= 136
    lib = L.load()
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*\w+ %s\(" % name, src, re.S)
        assert m and "model/segformer.py:92-128" in m.group(1), name          # declared, with the reference lines it serves
        assert name in L.PROTOTYPES and hasattr(lib, name)
        assert list(getattr(lib, name).argtypes or []) == list(L.PROTOTYPES[name][1])
    assert lib.hpfg_attn_keys_max() == 256


def test_size_query_and_argument_checks_need_no_device():
    lib = L.load()
    assert lib.hpfg_attn_keys_scratch_floats(1, 1024, 256, 8, 64, 1) == 1024 * 8 + 8 * 4 * 2 * 2 * 64 * 64
    assert lib.hpfg_attn_keys_scratch_floats(1, 1024, 256, 8, 64, 0) == 2 * 8 * 1024 * 256
    assert lib.hpfg_attn_keys_scratch_floats(1, 1024, 257, 8, 64, 1) == -1 and b"256 keys" in lib.hpfg_last_error()
    assert lib.hpfg_attn_keys_scratch_floats(1, 1024, 200, 8, 48, 1) == -1 and b"head dim 48" in lib.hpfg_last_error()
    assert lib.hpfg_attn_keys_fwd(None, None, None, None, 1, 8, 70, 1, 64, 0.125, 1, None) == -1 and b"attn_keys_fwd" in lib.hpfg_last_error()


def test_caps_and_dispatch_rule():
    assert ops_tokens.MAX_KEYS == 64 and ops_tokens.MAX_KEYS_LONG == 256
    for n in range(1, 257):          # a function of the key count alone
        assert ops_tokens.attention_for(n) is (ops_tokens.attention if n <= 64 else ops_tokens.attention_keys)
    assert seg_mod.attention_for is ops_tokens.attention_for


def test_attention_keys_checks_shapes_before_touching_a_device():
    import torch
    with pytest.raises(ValueError, match="at most 256 keys"):
        ops_tokens.attention_keys(torch.zeros(1, 8, 64), torch.zeros(1, 257, 128), 1, 0.125)
    with pytest.raises(ValueError, match="head dim"):
        ops_tokens.attention_keys(torch.zeros(1, 8, 96), torch.zeros(1, 70, 192), 2, 0.1)
    with pytest.raises(ValueError, match="kv"):
        ops_tokens.attention(torch.zeros(1, 8, 64), torch.zeros(1, 65, 128), 1, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_tokens.attention_keys(torch.zeros(1, 8, 64), torch.zeros(1, 70, 128), 1, 0.125)


def test_stage_keys_and_size_limit():
    assert seg_mod.stage_keys(224, 224) == [49] * 4 and seg_mod.stage_keys(256, 256) == [64] * 4
    assert seg_mod.stage_keys(288, 288) == [81] * 4 and seg_mod.stage_keys(384, 384) == [144] * 4
    assert seg_mod.stage_keys(512, 512) == [256] * 4 and seg_mod.stage_keys(512, 256) == [128] * 4
    seg_mod.check_image_size("x", 512, 512)
    for h, w in ((544, 544), (512, 544), (1024, 288)):
        with pytest.raises(ValueError, match="512x512 limit"):
            seg_mod.check_image_size("x", h, w)
    with pytest.raises(ValueError, match="512"):
        seg_mod.SegFormer(image_size=[544, 544], in_channels=1, num_classes=4)


@pytest.mark.parametrize("name,plus", [("segformer_b0_288", False), ("segformer_plus_b1_288", True)])
def test_fixtures_hold_what_the_gpu_tests_read(golden_dir, name, plus):
    path = os.path.join(golden_dir, name + ".npz")
    assert os.path.getsize(path) < 1 << 20
    d = np.load(path)
    s = int(d["logit_stride"])
    assert d["x"].shape == (1, 1, 288, 288) and d["y"].shape == (1, 288, 288)
    n = len(range(0, 288, s))
    assert d[f"eval_logits_s{s}"].shape == d[f"train_logits_s{s}"].shape == (1, 4, n, n)
    assert d["drop_path"].shape == (14, 1) and np.unpackbits(d["dropout_mask"]).size >= 256 and np.isfinite(float(d["loss"]))
    import torch
    from hpfg_amd.model import SegFormer, SegFormer_Plus
    m = (SegFormer_Plus if plus else SegFormer)(image_size=[288, 288], in_channels=1, num_classes=4)
    for k, p in m.named_parameters():
        assert d["g:" + k].shape == (3,), k
    params = dict(m.named_parameters())
    assert len(d["full_grads"]) >= 4
    for k in d["full_grads"]:
        assert d["grad:" + str(k)].shape == tuple(params[str(k)].shape), k
    assert d["oracle_err"].shape == (4,) and float(d["oracle_err"][:2].max()) <= 2e-5          # the oracle agrees with the reference at this size
    if plus:
        assert [d[k].shape for k in ("high_global", "high_dense", "head_global", "head_dense")] == [(1, 128), (1, 128, 16), (1, 128), (1, 128, 16)]
        assert d["neck_weights"].size == 2 * 128 * 17
    del torch
