"""CPU: SegFormer_Plus (MiT-B1 + the two projection necks) -- construction order, state_dict layout and parameter counts against the
oracle (oracle/segformer_ref.py with its DIMS set to B1's at run time) and the reference's own numbers (tests/golden/segformer_plus_b1.npz,
written by tools/make_golden_segformer_plus.py), and the configuration that trains it.  No GPU, no HIP compute calls."""
import os

import numpy as np
import pytest
import torch

from hpfg_amd.model import SegFormer_Plus, build_model
from hpfg_amd.model.segformer import MIT_SETTINGS, MiT
from hpfg_amd.utils import AttrDict, build_lr_scheduler, build_optimizer, loadyaml
from oracle import segformer_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1_DIMS = [64, 128, 320, 512]
NECKS = ("dense_projection_high", "dense_projection_head")


def _build():
    torch.manual_seed(1337)
    return build_model(AttrDict(model="segformer_plus", in_channels=1, num_classes=4, train_crop_size=[128, 128]))


def test_build_model_matches_the_reference_construction(golden_dir, monkeypatch):
    d = np.load(f"{golden_dir}/segformer_plus_b1.npz")
    m = _build()
    assert isinstance(m, SegFormer_Plus) and MIT_SETTINGS["B1"][0] == B1_DIMS
    sd = m.state_dict()
    keys = list(sd.keys())
    assert len(keys) == 208 and keys == [str(k) for k in d["keys"]]          # the reference's keys, in its order
    monkeypatch.setattr(S, "DIMS", B1_DIMS)                                   # the oracle file is B0's; heads, SR ratios and depths are B1's too
    st = S.init_state(1337, 1, 4)
    assert keys[:192] == list(st.keys()) and all(k.startswith(NECKS) for k in keys[192:])
    assert all(torch.equal(sd[k], st[k]) for k in st)                        # backbone: bit-equal, same generator consumption
    for k in keys[192:]:                                                      # the 16 neck tensors follow: the fixture's rows, exactly
        f = sd[k].detach().double().flatten()
        assert list(sd[k].shape) == list(d["neck_shape:" + k]), k
        row = np.concatenate([[float(f.sum()), float(f.abs().sum())], f[:8].numpy()])
        assert np.array_equal(row, d["neck_init:" + k]), (k, row, d["neck_init:" + k])
    n_backbone = sum(p.numel() for n, p in m.named_parameters() if not n.startswith(NECKS))
    assert n_backbone == 13672004 == m.backbone_numel() == int(d["n_backbone"])
    assert sum(p.numel() for p in m.parameters()) == 16570436 == int(d["n_params"])
    # the backbone parameters lead parameters(): what the optimizers' active_numel and the backbone EMA rely on
    lead = 0
    for n, p in m.named_parameters():
        if n.startswith(NECKS):
            break
        lead += p.numel()
    assert lead == n_backbone
    assert callable(m.val) and m.dense_projection_high.mlp["0"].in_features == 512 and m.dense_projection_head.mlp["0"].out_features == 1024


def test_the_oracle_override_is_restored(monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(S, "DIMS", B1_DIMS)
        assert S.init_state(1, 1, 4)["encoder.patch_embed1.proj.weight"].shape[0] == 64
    assert S.DIMS == [32, 64, 160, 256]


def test_yaml_builds_both_students_their_optimizers_and_schedulers():
    a = loadyaml(os.path.join(ROOT, "config", "hpfg_segformer_plus_30k_224x224_ACDC.yaml"))
    assert (a.batch_size, a.unlabel_batch_size, a.opt, a.lr, a.weight_decay, a.sched, a.warmup_epochs) == (8, 24, "adamW", 6e-4, 0.05, "cosine", 1)
    assert (a.consistency, a.consistency_rampup, a.ema_decay, a.datasets, a.seed) == (0.1, 200.0, 0.99, "synthetic", 1337)
    torch.manual_seed(a.seed)
    for block in (getattr(a, "model1", a), getattr(a, "model2", a)):          # a flat file: both students come from the one recipe
        m = build_model(block)
        assert isinstance(m, SegFormer_Plus) and m.decoder.image_size == [224, 224]
        opt = build_optimizer(args=block, model=m)
        assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 0.05
        sch = build_lr_scheduler(args=block, optimizer=opt)
        sch.step()
        assert abs(opt.param_groups[0]["lr"] - 1e-5) < 1e-12                  # the first iteration runs at warmup_lr
        for _ in range(1499):
            sch.step()
        assert abs(opt.param_groups[0]["lr"] - 6e-4) < 1e-12                  # ... and the base rate is reached after one warm-up epoch
    # the SGD alternative the same file names
    sgd = AttrDict(dict(a, opt="sgd", lr=0.01, weight_decay=1e-4, sched="medical", warmup_epochs=0))
    opt = build_optimizer(args=sgd, model=m)
    assert isinstance(opt, torch.optim.SGD)
    sch = build_lr_scheduler(args=sgd, optimizer=opt)
    for _ in range(3):
        sch.step()
    assert 0.0 < opt.param_groups[0]["lr"] < 0.01                             # the polynomial decay has begun


def test_unknown_mit_and_small_images_raise():
    with pytest.raises(NotImplementedError, match="B2"):
        MiT("B2", 1)
    with pytest.raises(NotImplementedError):
        SegFormer_Plus(image_size=[128, 128], in_channels=1, num_classes=4, model_name="B5")
    with pytest.raises(ValueError, match="at least 128"):
        build_model(AttrDict(model="segformer_plus", in_channels=1, num_classes=4, train_crop_size=[64, 64]))
