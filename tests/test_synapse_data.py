"""Synapse data path (reference datasets/Synapse.py:60-153): the directory contract on the host, and -- on the GPU -- build_loader("synapse" /
"sup_synapse") feeding a nine-class supervised step and the driver loops' evaluation hook from such a tree.  The tree is built per test:
npz slices written with numpy, h5 volumes copied from the h5py-written files of tests/golden/acdc_mini."""
import os
import shutil

import numpy as np
import pytest
import torch

from hpfg_amd.datasets import build_loader
from hpfg_amd.datasets.synapse import SynapseFiles
from hpfg_amd.utils import AttrDict

ACDC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acdc_mini")
SLICE_SIZES = [(40, 36), (33, 47), (64, 64), (29, 31), (48, 40), (52, 36)]
VOLUMES = ["patient101_frame01", "patient102_frame01"]


def _slice(k):
    g = np.random.default_rng(100 + k)
    h, w = SLICE_SIZES[k]
    return g.standard_normal((h, w)).astype(np.float32), g.integers(0, 9, (h, w)).astype(np.uint8)


@pytest.fixture()
def synapse_root(tmp_path):
    root = tmp_path / "Synapse"
    (root / "train_npz").mkdir(parents=True)
    (root / "test_vol_h5").mkdir()
    names = [f"case{k // 3:04d}_slice{k % 3:03d}" for k in range(len(SLICE_SIZES))]
    for k, n in enumerate(names):
        img, lab = _slice(k)
        lab[0, 0] = 8
        np.savez(root / "train_npz" / f"{n}.npz", image=img, label=lab)
    for v in VOLUMES:
        shutil.copy(os.path.join(ACDC, "data", v + ".h5"), root / "test_vol_h5" / f"{v}.npy.h5")
    (root / "train.txt").write_text("\n".join(names) + "\n")
    (root / "test_vol.txt").write_text("\n".join(VOLUMES) + "\n")
    return str(root)


def test_directory_contract_and_arrays(synapse_root):
    tr, te = SynapseFiles(synapse_root, "train"), SynapseFiles(synapse_root, "test")
    assert (len(tr), len(te)) == (6, 2)
    assert tr.sample_list[4].endswith("/train_npz/case0001_slice001.npz") and te.sample_list[1].endswith("/test_vol_h5/patient102_frame01.npy.h5")
    for k in range(6):
        img, lab = tr[k]
        want_img, want_lab = _slice(k)
        want_lab[0, 0] = 8
        assert img.dtype == np.float32 and lab.dtype == np.uint8 and np.array_equal(img, want_img) and np.array_equal(lab, want_lab)
    assert int(max(tr[k][1].max() for k in range(6))) == 8
    exp = np.load(os.path.join(ACDC, "expected.npz"))
    for k, v in enumerate(VOLUMES):
        img, lab = te[k]
        assert img.dtype == np.float32 and lab.dtype == np.uint8 and img.shape == lab.shape and img.ndim == 3
        assert np.array_equal(img, exp[f"vol/{v}/image"].astype(np.float32)) and np.array_equal(lab, exp[f"vol/{v}/label"].astype(np.uint8))
    pal = te.label_to_img(np.arange(9, dtype=np.uint8).reshape(3, 3))
    assert pal.shape == (3, 3, 3) and pal.dtype == np.uint8 and len({tuple(c) for c in pal.reshape(-1, 3)}) == 9


def test_other_real_data_keys_still_raise():
    for key in ("lidc", "isic", "sup_lidc", "sup_isic", "sup_building", "nonsense"):
        with pytest.raises(NotImplementedError):
            build_loader(AttrDict(datasets=key))


def _args(root, **kw):
    base = dict(datasets="synapse", data_path=root, in_channels=1, num_classes=9, batch_size=2, unlabel_batch_size=2, train_crop_size=(32, 32),
                test_crop_size=(32, 32), label_num=0.5, device="cuda:0", opt="sgd", lr=0.01, momentum=0.9, weight_decay=1e-4, sched="medical",
                total_itrs=100, step_size=200, warmup_epochs=0, warmup_lr=1e-4, min_lr=1e-6, consistency=0.1, consistency_rampup=200.0, ema_decay=0.99)
    base.update(kw)
    return AttrDict(base)


@pytest.mark.gpu
def test_synapse_loaders_feed_a_step_and_the_loops_evaluation(synapse_root, monkeypatch):
    from hpfg_amd import val as V
    from hpfg_amd.model import UNet
    from hpfg_amd.train import SupervisedStep, _Best
    a = _args(synapse_root)
    torch.manual_seed(3)
    lab, unl, test = build_loader(a)
    assert len(lab.dataset) == 6 and len(lab.indices) == 3 and len(unl.indices) == 3 and sorted(lab.indices + unl.indices) == list(range(6))
    assert len(lab) == 1 and len(unl) == 1 and len(test) == 2
    a4 = _args(synapse_root, label_num=0.4)
    l4, u4, _ = build_loader(a4)
    assert (len(l4.indices), len(u4.indices)) == (2, 4)                   # random_split: int(6 * 0.4) labelled
    for loader in (lab, unl):
        x, y = next(iter(loader))
        assert x.shape == (2, 1, 32, 32) and x.dtype == torch.float32 and x.is_cuda
        assert y.shape == (2, 32, 32) and y.dtype == torch.uint8 and y.is_cuda and int(y.max()) <= 8
    vimg, vlab = next(iter(test))
    assert vimg.shape == vlab.shape and vimg.dim() == 4 and vimg.shape[0] == 1 and vimg.dtype == torch.float32 and vlab.dtype == torch.uint8

    a.datasets = "sup_synapse"
    tr, te = build_loader(a)
    assert len(tr) == 3 and len(te) == 2
    x, y = next(iter(tr))
    m = UNet(1, 9).to("cuda:0")
    m.train()
    st = SupervisedStep(m, a)
    r = st.step(x, y, 1)
    assert torch.isfinite(r["loss"]).all()

    # the loops' evaluation hook goes through test_synapse for the two Synapse keys, through test_acdc otherwise
    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    calls = []
    real_syn, real_acdc = V.test_synapse, V.test_acdc
    monkeypatch.setattr(V, "test_synapse", lambda **kw: calls.append("synapse") or real_syn(**kw))
    monkeypatch.setattr(V, "test_acdc", lambda **kw: calls.append("acdc") or real_acdc(**kw))
    a.logger = Log()
    got = _Best(a, "model")(m, st.optimizer, st.lr_scheduler, te, 200)
    want, _ = real_syn(model=m, test_loader=te, args=_args(synapse_root), cur_itrs=200)
    assert calls == ["synapse"] and got == want and m.training
    assert "model_dice: {:.4f} model_hd95: {:.4f}".format(want, 0.0) in a.logger.lines
    a.datasets = "sup_acdc"
    _Best(a, "model")(m, st.optimizer, st.lr_scheduler, te, 200)
    assert calls == ["synapse", "acdc"]
