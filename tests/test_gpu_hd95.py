"""GPU: HD95 on the device (hpfg_amd.val.hd95_device: surface extraction and the exact integer nearest-surface search of csrc/surface.hip)
against the project's scipy restatement of medpy's hd95, ``val.hd95_host``, on the same arrays.  The device works in integers and the host
finishes in fp64, so the tolerance is 1e-9 absolute throughout (the rounding of sqrt and of one interpolation on values below 1.5e4),
and equality where a closed form exists."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import val as V
from hpfg_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-9
EMPTY_GT = "The second supplied array does not contain any binary object."


@lru_cache(maxsize=None)
def _blocks(seed, shape, ncls):
    """A label volume built like the evaluation tests' volumes: 5 x 5 coarse labels per slice blown up with np.kron, then cropped."""
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


def _host(pred, gt, ncls):
    """The yardstick, per class, under the reference's rule (val.py:376-387): 0.0 for a class that is never predicted."""
    return np.array([V.hd95_host(pred == c, gt == c) if (pred == c).any() else 0.0 for c in range(1, ncls)])


def _device(pred, gt, ncls, ndim=None):
    return V.hd95_device(torch.from_numpy(np.array(pred)).to(DEV), torch.from_numpy(np.array(gt)).to(DEV), ncls, ndim)


def _check(pred, gt, ncls, what, ndim=None):
    for c in range(1, ncls):
        assert (pred == c).any() and (gt == c).any(), (what, c)          # every class on both sides: no case is vacuous
    got, want = _device(pred, gt, ncls, ndim), _host(pred, gt, ncls)
    print(f"hd95 {what}: max |device - host| = {np.abs(got - want).max():.3e}, host {np.round(want, 4).tolist()}")
    assert got.dtype == np.float64 and got.shape == (ncls - 1,)
    assert np.abs(got - want).max() <= TOL, (what, got, want)


# S = 1 as 3-D; segments of a handful of points; several thousand points per segment: many LDS tiles with ragged last tiles
@pytest.mark.parametrize("shape", [(1, 9, 7), (2, 8, 8), (3, 17, 13), (7, 33, 29), (11, 40, 36), (5, 70, 66)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_block_volumes(seed, shape):
    _check(_blocks(seed, shape, 4), _blocks(seed + 100, shape, 4), 4, f"blocks seed {seed} {shape}")


@pytest.mark.parametrize("shape", [(4, 19, 23), (6, 65, 67)])
def test_noise_volumes(shape):
    _check(_noise(0, shape, 4), _noise(100, shape, 4), 4, f"noise {shape}")


@pytest.mark.parametrize("ncls", [9, 16])
def test_more_classes(ncls):
    _check(_blocks(0, (6, 40, 36), ncls), _blocks(100, (6, 40, 36), ncls), ncls, f"{ncls} classes")


# The two ways a long target segment is walked (csrc/surface.hip: SURF_MIN_BLOCKS = 2048 workgroups per segment, 256 points per tile):
# about 25 600 points per side -> 100 query blocks, the 100 target tiles split over 20 workgroups of 5 tiles each (atomicMin across them);
# about 550 000 points per side -> more than 2048 query blocks, no split, every workgroup streams all 2 100 tiles.
@pytest.mark.parametrize("shape", [(8, 80, 80), (17, 256, 256)])
def test_long_segments_split_and_unsplit(shape):
    pred, gt = _noise(7, shape, 2), _noise(107, shape, 2)
    n = int((pred == 1).sum())
    assert (n > 2048 * 256) == (shape[0] == 17) and n > 20000
    _check(pred, gt, 2, f"two-class noise {shape}")


def test_two_d_and_one_slice_three_d():
    """The same slice has two surfaces: in the plane (ndim 2) only the four in-plane neighbours count, as a one-slice volume (ndim 3) every
    mask voxel is a surface voxel."""
    pred, gt = _blocks(1, (1, 31, 27), 4)[0], _blocks(101, (1, 31, 27), 4)[0]
    _check(pred, gt, 4, "2-D slice", ndim=2)
    _check(pred[None], gt[None], 4, "the slice as [1,h,w], ndim 3")
    two_d = _device(pred, gt, 4)          # a 2-D tensor defaults to ndim 2
    assert np.array_equal(two_d, _device(pred[None], gt[None], 4, ndim=2))          # [1,h,w] with ndim 2: the synapse 2-D branch's form
    assert np.abs(two_d - _host(pred, gt, 4)).max() <= TOL
    assert not np.array_equal(two_d, _device(pred[None], gt[None], 4, ndim=3))      # (the two surfaces do differ on this slice)
    with pytest.raises(L.HipLibraryError, match="2-D"):
        _device(np.stack([pred, pred]), np.stack([gt, gt]), 4, ndim=2)              # ndim 2 needs S = 1


def test_closed_forms():
    a, b = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    a[2:5, 2:5] = 1
    b[2:5, 3:6] = 1
    assert _device(a, b, 2).tolist() == [1.0]
    # one voxel each, 2^2 + 4^2 + 4099^2 = 16801821 apart: above 2^24, where fp32 cannot hold the sum
    a, b = np.zeros((3, 5, 4100), np.uint8), np.zeros((3, 5, 4100), np.uint8)
    a[0, 0, 0] = 1
    b[2, 4, 4099] = 1
    assert _device(a, b, 2).tolist() == [float(np.sqrt(np.float64(16801821)))]
    assert int(np.float32(16801821)) != 16801821
    # a full volume against one voxel: the surface of the full mask is the volume's outer shell (border_value = 0)
    a, b = np.ones((5, 7, 6), np.uint8), np.zeros((5, 7, 6), np.uint8)
    b[2, 3, 2] = 1
    zz, yy, xx = np.meshgrid(np.arange(5), np.arange(7), np.arange(6), indexing="ij")
    shell = (zz == 0) | (zz == 4) | (yy == 0) | (yy == 6) | (xx == 0) | (xx == 5)
    d2 = ((zz - 2) ** 2 + (yy - 3) ** 2 + (xx - 2) ** 2)[shell]
    want = float(np.percentile(np.sqrt(np.concatenate([d2, [d2.min()]]).astype(np.float64)), 95))
    got = _device(a, b, 2)
    assert abs(got[0] - want) <= TOL and abs(got[0] - V.hd95_host(a == 1, b == 1)) <= TOL
    assert np.array_equal(got, _device(b, a, 2))          # symmetric


def test_the_reference_rule_and_foreign_labels():
    pred, gt = _noise(0, (4, 19, 23), 4).copy(), _noise(100, (4, 19, 23), 4).copy()
    pred[pred == 2] = 0                                    # class 2 never predicted: 0.0, no exception, the others unchanged
    got = _device(pred, gt, 4)
    assert got[1] == 0.0 and np.abs(got - _host(pred, gt, 4)).max() <= TOL and got[0] > 0 and got[2] > 0
    gt3 = gt.copy()
    gt3[gt3 == 3] = 0                                      # class 3 predicted but absent from gt: medpy's error, as hd95_host raises it
    with pytest.raises(RuntimeError) as e:
        _device(pred, gt3, 4)
    assert str(e.value) == EMPTY_GT
    with pytest.raises(RuntimeError) as e:
        V.hd95_host(pred == 3, gt3 == 3)
    assert str(e.value) == EMPTY_GT
    assert _device(np.zeros_like(gt), gt, 4).tolist() == [0.0, 0.0, 0.0]          # nothing predicted at all
    # labels >= classes belong to no mask: the background voxels relabelled 255 / 4 / 9 change nothing
    g = np.random.default_rng(5)
    p2, g2 = pred.copy(), gt.copy()
    p2[(pred == 0) & (g.random(pred.shape) < 0.5)] = 255
    g2[(gt == 0) & (g.random(gt.shape) < 0.3)] = 4
    g2[(gt == 0) & (g2 == 0) & (g.random(gt.shape) < 0.3)] = 9
    assert (p2 == 255).sum() > 50 and (g2 == 4).sum() > 50 and (g2 == 9).sum() > 50
    assert np.array_equal(_device(p2, g2, 4), got) and np.abs(got - _host(p2, g2, 4)).max() <= TOL


def test_two_calls_give_the_same_bits():
    pred, gt = _noise(0, (6, 65, 67), 4), _noise(100, (6, 65, 67), 4)
    a, b = _device(pred, gt, 4), _device(pred, gt, 4)
    assert a.tobytes() == b.tobytes()


def test_argument_errors_of_the_python_surface():
    p = torch.zeros((2, 4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        V.hd95_device(p.cpu(), p.cpu(), 4)                # no CPU fallback
    with pytest.raises(ValueError):
        V.hd95_device(p.float(), p.float(), 4)
    with pytest.raises(ValueError):
        V.hd95_device(p, p[:1], 4)
    with pytest.raises(ValueError):
        V.hd95_device(p[0], p[0], 4, ndim=3)


# ---- wiring -----------------------------------------------------------------------------------------------------------------------------

def _image_of(lab, ncls, seed):
    return (lab / (ncls - 1) + 0.1 * np.random.default_rng(seed).standard_normal(lab.shape)).astype(np.float32)


@pytest.fixture(scope="module")
def model():
    """A U-Net whose BatchNorm running statistics are not the initial (0, 1): a few train-mode forwards on random data."""
    torch.manual_seed(5)
    m = UNet(1, 4).to(DEV)
    m.math = "f32"
    m.train()
    with torch.no_grad():
        for k in range(3):
            m(torch.randn(8, 1, 32, 32, device=DEV) * (1 + k))
    return m


def test_single_volume_routes(model):
    lab = _blocks(103, (11, 40, 36), 4)
    img = _image_of(lab, 4, 3)
    it, lt = torch.from_numpy(img), torch.from_numpy(lab.copy())
    p = V.predict_volume(it, model, (32, 32))
    ph = p.cpu().numpy()
    want = _host(ph, lab, 4)
    print(f"hd95 wiring: predicted classes {sorted(set(np.unique(ph).tolist()))}, host {np.round(want, 4).tolist()}")
    assert (want > 0).any()                                # the comparison is not vacuous
    got = V.hd95_device(p, lt.to(DEV), 4)
    assert np.abs(got - want).max() <= TOL
    dev_rows = V.test_single_volume(it[None], lt[None], model, classes=4, patch_size=(32, 32), with_hd95="device")
    host_rows = V.test_single_volume(it[None], lt[None], model, classes=4, patch_size=(32, 32), with_hd95=True)
    none_rows = V.test_single_volume(it[None], lt[None], model, classes=4, patch_size=(32, 32))
    assert [hd for _, hd in dev_rows] == got.tolist() and [hd for _, hd in none_rows] == [0.0] * 3
    assert [d for d, _ in dev_rows] == [d for d, _ in host_rows] == [d for d, _ in none_rows]
    assert np.abs(np.array([hd for _, hd in host_rows]) - want).max() == 0.0
    with pytest.raises(ValueError):
        V.test_single_volume(it[None], lt[None], model, classes=4, patch_size=(32, 32), with_hd95="host")
    assert model.training


def test_single_volume_synapse_routes(model):
    lab = _blocks(103, (5, 40, 36), 4)
    img = _image_of(lab, 4, 3)
    it, lt = torch.from_numpy(img), torch.from_numpy(lab.copy())
    kw = dict(classes=4, patch_size=(32, 32))
    rows = V.test_single_volume_synapse(it[None], lt[None], model, **kw)
    assert [hd for _, hd in rows] == [0.0] * 3             # the default stays 0.0
    p = V.predict_volume(it, model, (32, 32), order=3)
    want = V.hd95_device(p, lt.to(DEV), 4)
    assert (want > 0).any() and np.abs(want - _host(p.cpu().numpy(), lab, 4)).max() <= TOL
    dev_rows = V.test_single_volume_synapse(it[None], lt[None], model, with_hd95="device", **kw)
    assert [hd for _, hd in dev_rows] == want.tolist() and [d for d, _ in dev_rows] == [d for d, _ in rows]
    host_rows = V.test_single_volume_synapse(it[None], lt[None], model, with_hd95=True, **kw)
    assert np.abs(np.array([hd for _, hd in host_rows]) - want).max() <= TOL
    # the 2-D branch ([1,h,w]) measures in the plane
    for seed in (103, 104, 105, 106):                      # the first slice on which the network predicts a foreground class
        lab2 = _blocks(seed, (1, 32, 32), 4)
        i2, l2 = torch.from_numpy(_image_of(lab2, 4, 3)), torch.from_numpy(lab2.copy())
        p2 = V.predict_volume(i2, model, (32, 32))[0]      # forwarded at its own size
        want2 = _host(p2.cpu().numpy(), lab2[0], 4)
        if (want2 > 0).any():
            break
    assert (want2 > 0).any()
    one = V.test_single_volume_synapse(i2, l2, model, with_hd95="device", classes=4, patch_size=(48, 48))
    assert np.abs(np.array([hd for _, hd in one]) - want2).max() <= TOL
    assert np.abs(np.array([hd for _, hd in one]) - V.hd95_device(p2, l2[0].to(DEV), 4, ndim=2)).max() == 0.0
    with pytest.raises(ValueError):
        V.test_single_volume_synapse(it[None], lt[None], model, with_hd95=2, **kw)


@pytest.mark.parametrize("datasets", ["acdc", "synapse"])
def test_best_logs_the_device_hd95(model, datasets):
    from hpfg_amd.datasets.synthetic import SyntheticVolumes
    from hpfg_amd.train import _Best
    from hpfg_amd.utils import AttrDict

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(msg)

    loader = torch.utils.data.DataLoader(SyntheticVolumes(2, 3, (40, 36)), batch_size=1)
    test = V.test_synapse if datasets == "synapse" else V.test_acdc
    args = AttrDict(num_classes=4, test_crop_size=(32, 32), device=DEV, datasets=datasets)
    dice, hd = test(model, loader, args, cur_itrs=200, with_hd95=True)          # the host route is the yardstick
    assert hd > 0.0
    assert test(model, loader, args, cur_itrs=200) == (dice, 0.0)
    dice_d, hd_d = test(model, loader, args, cur_itrs=200, with_hd95="device")
    assert dice_d == dice and abs(hd_d - hd) <= TOL
    args.logger, args.eval_hd95 = Log(), "device"
    assert _Best(args, "model")(model, None, None, loader, 200) == dice
    assert "model_dice: {:.4f} model_hd95: {:.4f}".format(dice, hd) in args.logger.lines
    del args["eval_hd95"]
    args.logger = Log()
    _Best(args, "model")(model, None, None, loader, 200)
    assert "model_dice: {:.4f} model_hd95: {:.4f}".format(dice, 0.0) in args.logger.lines and model.training
