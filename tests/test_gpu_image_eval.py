"""GPU: the evaluation of 2-D image test sets (hpfg_amd.val.test_lidc / test_isic, reference val.py:86-151) and the average surface distance
on the device (val.surface_metrics_device: hpfg_surface_sums of csrc/surface.hip) against the project's scipy restatements of medpy,
``val.asd_host`` / ``val.hd95_host``, on the same arrays.

Tolerances.  HD95: 1e-9 absolute, as in test_gpu_hd95.py.  ASD: the device adds the fp64 square roots of a segment exactly (integers) and
the host rounds the mean once, so the whole allowance belongs to the yardstick: numpy's sum of n values, its division and a 1-ulp square
root stay within (n + 2) * 2^-52 * want of the exact mean, n = the surface voxels of the prediction."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from hpfg_amd import val as V
from hpfg_amd.datasets.synthetic import SyntheticVolumes, palette_image
from hpfg_amd.model import UNet, build_model
from hpfg_amd.train import CPS, _Best
from hpfg_amd.utils import AttrDict, loadyaml

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_HD = 1e-9
EMPTY_GT = "The second supplied array does not contain any binary object."


@lru_cache(maxsize=None)
def _blocks(seed, shape, ncls):
    """The label volumes of test_gpu_hd95.py: 5 x 5 coarse labels per slice blown up with np.kron, then cropped."""
    s, h, w = shape
    coarse = np.random.default_rng(seed).integers(0, ncls, (s, 5, 5))
    lab = np.kron(coarse, np.ones((h // 5 + 1, w // 5 + 1), dtype=np.int64))[:, :h, :w].astype(np.uint8)
    lab.setflags(write=False)
    return lab


@lru_cache(maxsize=None)
def _noise(seed, shape, ncls):
    lab = np.random.default_rng(seed).integers(0, ncls, shape).astype(np.uint8)
    lab.setflags(write=False)
    return lab


def _surface_points(mask):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    return int((mask ^ binary_erosion(mask, structure=generate_binary_structure(mask.ndim, 1), iterations=1)).sum())


def _asd_tol(pred_mask, want):
    return (_surface_points(pred_mask) + 2) * 2.0 ** -52 * want


def _device(pred, gt, ncls, ndim=None):
    return V.surface_metrics_device(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), ncls, ndim)


def _check(pred, gt, ncls, what, ndim=None):
    for c in range(1, ncls):
        assert (pred == c).any() and (gt == c).any(), (what, c)          # every class on both sides: no case is vacuous
    hd, asd = _device(pred, gt, ncls, ndim)
    assert hd.dtype == asd.dtype == np.float64 and hd.shape == asd.shape == (ncls - 1,)
    worst = 0.0
    for c in range(1, ncls):
        want, want_hd = V.asd_host(pred == c, gt == c), V.hd95_host(pred == c, gt == c)
        tol = _asd_tol(pred == c, want)
        worst = max(worst, abs(asd[c - 1] - want) / tol)
        assert want > 0.0 and abs(asd[c - 1] - want) <= tol, (what, c, asd[c - 1], want, tol)
        assert abs(hd[c - 1] - want_hd) <= TOL_HD, (what, c, hd[c - 1], want_hd)
    print(f"asd {what}: worst |device - host| = {worst:.3g} of the bound, device {np.round(asd, 4).tolist()}")
    return hd, asd


# S = 1 as 3-D; segments of a handful of points up to a few thousand
@pytest.mark.parametrize("shape", [(1, 9, 7), (2, 8, 8), (3, 17, 13), (7, 33, 29), (5, 70, 66)])
def test_block_volumes(shape):
    _check(_blocks(0, shape, 4), _blocks(100, shape, 4), 4, f"blocks {shape}")


def test_noise_volume():
    _check(_noise(0, (6, 65, 67), 4), _noise(100, (6, 65, 67), 4), 4, "noise (6, 65, 67)")


def test_sixteen_classes():
    _check(_blocks(0, (6, 40, 36), 16), _blocks(100, (6, 40, 36), 16), 16, "16 classes")


def test_long_segments_many_workgroups():
    """About 25 000 points per segment: a hundred workgroups add into the same two words (the launch grid has no cap: one thread per key)."""
    pred, gt = _noise(7, (8, 80, 80), 2), _noise(107, (8, 80, 80), 2)
    assert _surface_points(pred == 1) > 20000
    _check(pred, gt, 2, "two-class noise (8, 80, 80)")


def test_two_d_slice():
    pred, gt = _blocks(1, (1, 31, 27), 4)[0], _blocks(101, (1, 31, 27), 4)[0]
    hd2, asd2 = _check(pred, gt, 4, "2-D slice", ndim=2)
    hd3, asd3 = _check(pred[None], gt[None], 4, "the slice as [1,h,w], ndim 3")
    assert not np.array_equal(asd2, asd3)          # in the plane only the outline is surface; as a one-slice volume every mask voxel is
    two = _device(pred[None], gt[None], 4, ndim=2)
    assert np.array_equal(two[0], hd2) and np.array_equal(two[1], asd2)


@pytest.mark.parametrize("k", [1, 4, 9])
def test_closed_forms(k):
    a, b = np.zeros((3, 12, 14), np.uint8), np.zeros((3, 12, 14), np.uint8)
    a[1, 1, :], b[1, 1 + k, :] = 1, 1          # two parallel one-voxel lines k apart: every distance is k
    hd, asd = _device(a, b, 2)
    assert hd.tolist() == [float(k)] == asd.tolist() and V.asd_host(a == 1, b == 1) == float(k)
    hd, asd = _device(a[1], b[1], 2)           # the same in the plane
    assert hd.tolist() == [float(k)] == asd.tolist()
    hd, asd = _device(a, a, 2)                 # identical masks
    assert hd.tolist() == [0.0] == asd.tolist()


def test_the_reference_rule():
    pred, gt = _noise(0, (4, 19, 23), 4).copy(), _noise(100, (4, 19, 23), 4).copy()
    pred[pred == 2] = 0                                    # class 2 never predicted: 0.0 for both metrics, the others unchanged
    hd, asd = _device(pred, gt, 4)
    assert hd[1] == 0.0 and asd[1] == 0.0
    for c in (1, 3):
        want = V.asd_host(pred == c, gt == c)
        assert asd[c - 1] > 0 and abs(asd[c - 1] - want) <= _asd_tol(pred == c, want)
    gt3 = gt.copy()
    gt3[gt3 == 3] = 0                                      # class 3 predicted but absent from gt: medpy's error
    with pytest.raises(RuntimeError) as e:
        _device(pred, gt3, 4)
    assert str(e.value) == EMPTY_GT
    with pytest.raises(RuntimeError) as e:
        V.asd_host(pred == 3, gt3 == 3)
    assert str(e.value) == EMPTY_GT
    hd, asd = _device(np.zeros_like(gt), gt, 4)            # nothing predicted at all
    assert hd.tolist() == [0.0, 0.0, 0.0] == asd.tolist()
    p = torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="surface_metrics_device"):
        V.surface_metrics_device(p.cpu(), p.cpu(), 4)      # no CPU fallback


def test_two_calls_give_the_same_bits_and_hd95_is_unchanged():
    pred, gt = _noise(0, (6, 65, 67), 4), _noise(100, (6, 65, 67), 4)
    (hd_a, asd_a), (hd_b, asd_b) = _device(pred, gt, 4), _device(pred, gt, 4)
    assert hd_a.tobytes() == hd_b.tobytes() and asd_a.tobytes() == asd_b.tobytes()
    alone = V.hd95_device(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), 4)
    assert alone.tobytes() == hd_a.tobytes()
    pred, gt = _blocks(0, (6, 40, 36), 16), _blocks(100, (6, 40, 36), 16)
    alone = V.hd95_device(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), 16)
    assert alone.tobytes() == _device(pred, gt, 16)[0].tobytes()


# ---- wiring -----------------------------------------------------------------------------------------------------------------------------

class _Images(torch.utils.data.Dataset):
    def __init__(self, images, labels):
        self.images, self.labels = images, labels

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return self.images[i], self.labels[i]

    def label_to_img(self, label):
        return palette_image(label, 2)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


class _Writer:
    def __init__(self):
        self.images = {}

    def add_image(self, tag, img, step, dataformats="CHW"):
        self.images[tag] = (np.asarray(img), step, dataformats)


@pytest.fixture(scope="module")
def loader():
    """7 RGB images of 32 x 32 in batches of 3 (3 + 3 + 1), class 1 in every batch."""
    lab = _blocks(203, (7, 32, 32), 2)
    img = (lab + 0.1 * np.random.default_rng(3).standard_normal(lab.shape)).astype(np.float32)
    images = torch.from_numpy(img).unsqueeze(1).expand(7, 3, 32, 32).contiguous()
    ld = torch.utils.data.DataLoader(_Images(images, torch.from_numpy(lab.copy())), batch_size=3, shuffle=False)
    assert [int(i.shape[0]) for i, _ in ld] == [3, 3, 1] and all(bool((l == 1).any()) for _, l in ld)
    return ld


@pytest.fixture(scope="module")
def model(loader):
    """A 3-channel, 2-class U-Net whose BatchNorm running statistics are not the initial (0, 1): a few train-mode forwards on random data.
    An untrained network answers class 0 everywhere on these images, which would leave nothing to score: the bias of the class-1 logit is
    moved by the median logit difference over the test images, so that about half of their pixels are predicted as class 1."""
    torch.manual_seed(5)
    m = UNet(3, 2).to(DEV)
    m.math = "f32"
    m.train()
    with torch.no_grad():
        for k in range(3):
            m(torch.randn(8, 3, 32, 32, device=DEV) * (1 + k))
        m.eval()
        x = loader.dataset.images.to(DEV)
        z = m(torch.cat([x, x.new_zeros(1, 3, 32, 32)], 0).contiguous())[:7]
        m.decoder.out_conv.bias.data[1] += float((z[:, 0] - z[:, 1]).median())
    m.train()
    return m


def _eval_forward(model, x):
    """An eval-mode forward of one engine batch (zero padded to EVAL_BATCH) and torch's arg-max."""
    was = model.training
    model.eval()
    with torch.no_grad():
        xb = torch.cat([x, x.new_zeros(V.EVAL_BATCH - x.shape[0], *x.shape[1:])], 0).contiguous()
        out = torch.argmax((model.val if hasattr(model, "val") else model)(xb), dim=1)[:x.shape[0]]
    model.train(was)
    return out


def test_predict_images(model, loader):
    images = loader.dataset.images
    model.train()
    p = V.predict_images(images, model)                    # host input, one short engine batch
    assert model.training and p.dtype == torch.uint8 and tuple(p.shape) == (7, 32, 32) and p.device.type == "cuda"
    assert torch.equal(p.long(), _eval_forward(model, images.to(DEV)))
    assert bool((p == 1).any()) and bool((p == 0).any())
    x11 = torch.cat([images, images[:4].flip(0)], 0)       # 11 images: a full engine batch and a padded tail
    p11 = V.predict_images(x11.to(DEV), model)
    assert torch.equal(p11[:8].long(), _eval_forward(model, x11[:8].to(DEV))) and torch.equal(p11[8:].long(), _eval_forward(model, x11[8:].to(DEV)))
    model.eval()
    V.predict_images(images[:1], model)
    assert not model.training                              # the mode it found
    model.train()
    with pytest.raises(ValueError):
        V.predict_images(images[0], model)


def _restated(model, loader):
    """val.py:109-151 in plain numpy / scipy: ``cal`` per batch on (pred == 1), (label == 1) as [B,H,W] arrays, weighted by the batch size,
    over the length of the data set.  Returns the four numbers, the per-batch ASD bounds weighted the same way, and the batches scored."""
    total, tol, scored = [0.0, 0.0, 0.0, 0.0], 0.0, 0
    for img, lab in loader:
        pred = _eval_forward(model, img.to(DEV)).cpu().numpy() == 1
        gt = lab.numpy() == 1
        row = (0, 0, 0, 0)
        if pred.sum() > 0:
            inter = np.count_nonzero(pred & gt)
            row = (2.0 * inter / float(np.count_nonzero(pred) + np.count_nonzero(gt)), V.hd95_host(pred, gt),
                   float(inter) / float(np.count_nonzero(pred | gt)), V.asd_host(pred, gt))
            tol += _asd_tol(pred, row[3]) * img.shape[0]
            scored += 1
        for k in range(4):
            total[k] += row[k] * img.shape[0]
    n = len(loader.dataset)
    return [t / n for t in total], tol / n, scored


def test_isic_and_lidc_routes(model, loader):
    args = AttrDict(num_classes=2, test_crop_size=(32, 32), device=DEV)
    want, asd_tol, scored = _restated(model, loader)
    print(f"image eval: restated (dice, hd95, jac, asd) = {want}, batches with a prediction: {scored}")
    assert scored >= 2 and want[0] > 0 and want[1] > 0 and want[2] > 0 and want[3] > 0          # the network predicts class 1; nothing is vacuous
    host = V.test_isic(model, loader, args, cur_itrs=3, with_hd95=True)
    assert list(host) == want                              # the host route IS the restated arithmetic, ragged batch weighting included
    dev = V.test_isic(model, loader, args, cur_itrs=3, with_hd95="device")
    none = V.test_isic(model, loader, args, cur_itrs=3)
    assert dev[0] == host[0] == none[0] and dev[2] == host[2] == none[2]
    assert none[1] == 0.0 and none[3] == 0.0
    assert abs(dev[1] - host[1]) <= TOL_HD
    # ASD: the per-batch bounds, weighted like the values; plus the roundings of the weighting itself on both sides (3 products, 3 sums and a
    # division each, half an ulp of a partial result that does not exceed the total): 16 ulp of the result is ample
    assert abs(dev[3] - host[3]) <= asd_tol + 16 * np.spacing(host[3])
    for route, full in ((True, host), ("device", dev), (False, none)):
        assert V.test_lidc(model, loader, args, cur_itrs=3, with_hd95=route) == full[:2]
    with pytest.raises(ValueError):
        V.test_isic(model, loader, args, with_hd95="host")
    assert model.training
    # only class 1 is scored, whatever num_classes says
    assert V.test_isic(model, loader, AttrDict(num_classes=4, device=DEV), with_hd95="device") == dev
    # image hooks: the first batch's palette images
    args.writer = _Writer()
    assert V.test_isic(model, loader, args, cur_itrs=9, name="val", with_hd95="device") == dev
    assert sorted(args.writer.images) == ["val/label_pred", "val/label_true"]
    img, step, fmt = args.writer.images["val/label_true"]
    assert img.shape == (32, 3 * 32, 3) and img.dtype == np.uint8 and step == 9 and fmt == "HWC"
    first = next(iter(loader))[1].numpy()
    assert np.array_equal(img, np.concatenate(list(palette_image(first, 2)), axis=1))


def test_a_prediction_against_empty_labels_raises(model, loader):
    images = loader.dataset.images
    assert bool((V.predict_images(images[:3], model) == 1).any())
    empty = torch.utils.data.DataLoader(_Images(images[:3], torch.zeros(3, 32, 32, dtype=torch.uint8)), batch_size=3)
    args = AttrDict(num_classes=2, device=DEV)
    for route in (True, "device"):
        with pytest.raises(RuntimeError) as e:
            V.test_isic(model, empty, args, with_hd95=route)
        assert str(e.value) == EMPTY_GT
    assert V.test_isic(model, empty, args) == (0.0, 0.0, 0.0, 0.0)          # without surface metrics: medpy's dc and jc of a miss


def test_best_logs_the_four_fields(model, loader):
    args = AttrDict(num_classes=2, test_crop_size=(32, 32), device=DEV, eval_images="isic", eval_hd95="device", logger=_Log())
    dice, hd, jac, asd = V.test_isic(model, loader, args, cur_itrs=200, with_hd95="device")
    assert _Best(args, "model")(model, None, None, loader, 200) == dice and model.training
    assert args.logger.lines == ["model_dice: {:.4f} model_hd95: {:.4f} model_jac: {:.4f} model_asd: {:.4f}".format(dice, hd, jac, asd)]
    args.eval_images, args.logger = "lidc", _Log()
    assert _Best(args, "ema")(model, None, None, loader, 200) == dice
    assert args.logger.lines == ["ema_dice: {:.4f} ema_hd95: {:.4f}".format(dice, hd)]
    del args["eval_hd95"]
    args.eval_images, args.logger = "isic", _Log()
    _Best(args, "model")(model, None, None, loader, 200)
    assert args.logger.lines == ["model_dice: {:.4f} model_hd95: {:.4f} model_jac: {:.4f} model_asd: {:.4f}".format(dice, 0.0, jac, 0.0)]


def test_best_without_the_key_logs_the_line_as_before():
    torch.manual_seed(6)
    m = UNet(1, 4).to(DEV)
    m.math = "f32"
    m.train()
    vols = torch.utils.data.DataLoader(SyntheticVolumes(2, 3, (40, 36)), batch_size=1)
    args = AttrDict(num_classes=4, test_crop_size=(32, 32), device=DEV, datasets="acdc", logger=_Log())
    dice, hd = V.test_acdc(m, vols, args, cur_itrs=200)
    assert _Best(args, "model")(m, None, None, vols, 200) == dice
    assert "model_dice: {:.4f} model_hd95: {:.4f}".format(dice, hd) in args.logger.lines
    assert not any("jac" in ln or "asd" in ln for ln in args.logger.lines)


def test_cps_loop_on_the_isic_config(tmp_path):
    """The committed ISIC-shaped configuration shrunk to 32 x 32 and 4 iterations: two evaluations of both networks through test_isic and a
    best-Dice checkpoint of each."""
    from hpfg_amd.datasets import build_loader
    a = loadyaml(os.path.join(ROOT, "config", "cps_unet_30k_224x224_ISIC.yaml"))
    small = dict(total_itrs=4, step_size=2)
    a.update(small, train_crop_size=[32, 32], test_crop_size=[32, 32], batch_size=2, unlabel_batch_size=2, synthetic_labeled=8,
             synthetic_unlabeled=12, synthetic_test_images=5, device="cuda:0", save_path=str(tmp_path), logger=_Log())
    a.model1, a.model2 = AttrDict(dict(a.model1, **small)), AttrDict(dict(a.model2, **small))
    os.makedirs(os.path.join(str(tmp_path), "model"), exist_ok=True)
    for k in ("model1", "model2"):
        a[f"{k}_save_path"] = os.path.join(str(tmp_path), "model", f"{k}.pth")
    assert a.eval_images == "isic" and a.eval_hd95 == "device" and a.in_channels == 3 and a.num_classes == 2
    torch.manual_seed(1337)
    m1, m2 = build_model(a).to(DEV), build_model(a).to(DEV)
    lab, unl, test = build_loader(a)
    assert [int(i.shape[0]) for i, _ in test] == [2, 2, 1] and tuple(next(iter(test))[0].shape) == (2, 3, 32, 32)
    log = CPS(m1, m2, lab, unl, test, a)
    assert log.shape == (a.total_itrs + 1,) and torch.isfinite(log).all()
    for k, m in (("model1", m1), ("model2", m2)):
        lines = [ln for ln in a.logger.lines if ln.startswith(f"{k}_dice")]
        assert len(lines) == 2 and all(f"{k}_hd95" in ln and f"{k}_jac" in ln and f"{k}_asd" in ln for ln in lines), a.logger.lines
        ck = torch.load(a[f"{k}_save_path"], weights_only=False)
        assert set(ck["model"].keys()) == set(m.state_dict().keys()) and ck["cur_itrs"] in (2, 4) and 0.0 < ck["best_dice"] <= 1.0
        assert m.training
