"""CPU: the host side of the 2-D image evaluation (hpfg_amd.val.test_lidc / test_isic): medpy's asd and jc restated, the exact finish of the
device's integer distance sums, the ``eval_images`` key, the image test loader and the ISIC-shaped config."""
import math
import os

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import val as V
from hpfg_amd.datasets import build_loader
from hpfg_amd.train import _Best, eval_images_route
from hpfg_amd.utils import AttrDict, loadyaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY_PRED = "The first supplied array does not contain any binary object."
EMPTY_GT = "The second supplied array does not contain any binary object."


@pytest.mark.parametrize("k", [1, 3, 6])
def test_asd_host_parallel_lines(k):
    a, b = np.zeros((9, 12), bool), np.zeros((9, 12), bool)
    a[1, :], b[1 + k, :] = True, True
    assert V.asd_host(a, b) == float(k) == V.asd_host(b, a) == V.hd95_host(a, b)
    a3, b3 = np.zeros((4, 9, 12), bool), np.zeros((4, 9, 12), bool)          # the same lines in a volume
    a3[2, 1, :], b3[2, 1 + k, :] = True, True
    assert V.asd_host(a3, b3) == float(k)


def test_asd_host_is_one_directional_and_zero_on_identical_masks():
    a, b = np.zeros((10, 10), bool), np.zeros((10, 10), bool)
    a[2:8, 2:8] = True
    b[4, 4] = True
    assert V.asd_host(a, a) == 0.0
    d = np.sqrt(np.array([(y - 4) ** 2 + (x - 4) ** 2 for y in range(2, 8) for x in range(2, 8) if y in (2, 7) or x in (2, 7)], dtype=np.float64))
    assert V.asd_host(a, b) == float(d.mean())          # from the 20 border pixels of the square to the point
    assert V.asd_host(b, a) == 2.0                      # from the point to the nearest border pixel
    assert V.asd_host(a, b) != V.asd_host(b, a)


def test_asd_host_raises_like_medpy_on_an_empty_side():
    a, e = np.zeros((6, 6), bool), np.zeros((6, 6), bool)
    a[2, 2] = True
    with pytest.raises(RuntimeError) as err:
        V.asd_host(e, a)
    assert str(err.value) == EMPTY_PRED
    with pytest.raises(RuntimeError) as err:
        V.asd_host(a, e)
    assert str(err.value) == EMPTY_GT


@pytest.mark.parametrize("n", [1, 7, 1000, 30000])
def test_asd_finish_against_numpy(n):
    """The device adds hi = rint(x 2^19) and lo = (x - hi 2^-19) 2^52 of x = sqrt(d^2) in integers (``asd_limbs`` restates it): the split loses
    nothing, so the finished mean is the correctly rounded mean of the fp64 square roots; numpy's pairwise sum of n values and its division
    stay within (n + 2) 2^-52 of it, relatively."""
    d2 = np.random.default_rng(n).integers(0, 3 * 8191 ** 2 + 1, n)
    hi, lo = V.asd_limbs(d2)
    x = np.sqrt(d2.astype(np.float64))
    assert np.array_equal(hi * 2.0 ** -19 + lo * 2.0 ** -52, x)                      # exact split
    assert int(hi.max()) <= 2 ** 33 and int(np.abs(lo).max()) <= 2 ** 32
    got, want = V.asd_finish(int(hi.sum()), int(lo.sum()), n), float(x.mean())
    assert abs(got - want) <= (n + 2) * 2.0 ** -52 * want
    exact = math.fsum(x.tolist()) / n                                                # one rounding of the sum, one of the division
    assert abs(got - exact) <= np.spacing(exact)
    perm = np.random.default_rng(1).permutation(n)                                   # integer sums: any order, the same bits
    assert V.asd_finish(int(hi[perm].sum()), int(lo[perm].sum()), n) == got


def test_asd_finish_is_exact_on_perfect_squares():
    k = np.random.default_rng(3).integers(0, 8192, 4096)
    hi, lo = V.asd_limbs(k * k)
    assert not lo.any()
    assert V.asd_finish(int(hi.sum()), int(lo.sum()), k.size) == int(k.sum()) / k.size
    assert V.asd_finish(5 << 19, 0, 1) == 5.0 and V.asd_finish(0, 0, 9) == 0.0
    assert V.asd_finish((2 ** 64 - 2 ** 19), -(2 ** 52), 2 ** 31 - 1) == (2 ** 45 - 2) / (2 ** 31 - 1)          # words at the top of their range


def test_jaccard_from_counts():
    cm = np.array([[50, 4, 0], [6, 30, 1], [2, 0, 0]], dtype=np.int64)          # cm[g, p]
    assert V.jaccard_from_counts(cm, 1) == 30 / float(34 + 37 - 30)
    assert V.jaccard_from_counts(cm, 2) == 0.0 / float(1 + 2 - 0)              # predicted, never right
    cm[:, 2] = 0
    assert V.jaccard_from_counts(cm, 2) == 0.0                                 # never predicted: the reference's rule, no division
    pred, gt = np.random.default_rng(0).random((2, 40, 40)) < 0.4
    cm2 = np.array([[(~gt & ~pred).sum(), (~gt & pred).sum()], [(gt & ~pred).sum(), (gt & pred).sum()]])
    assert V.jaccard_from_counts(cm2, 1) == float((pred & gt).sum()) / float((pred | gt).sum())          # medpy jc


def test_eval_images_key_is_validated_before_the_first_iteration():
    assert eval_images_route(AttrDict()) is None and eval_images_route(AttrDict(eval_images=False)) is None
    assert eval_images_route(AttrDict(eval_images="lidc")) == "lidc" and eval_images_route(AttrDict(eval_images="isic")) == "isic"
    for bad in ("acdc", "ISIC", True, 1, ""):
        with pytest.raises(ValueError, match="eval_images"):
            eval_images_route(AttrDict(eval_images=bad))
        with pytest.raises(ValueError, match="eval_images"):
            _Best(AttrDict(eval_images=bad), "model")
    assert _Best(AttrDict(eval_images="isic", eval_hd95="device"), "model").images == "isic"
    assert _Best(AttrDict(), "model").images is None
    assert V.test_lidc.__test__ is False and V.test_isic.__test__ is False


@pytest.mark.parametrize("datasets", ["synthetic", "sup_synthetic"])
def test_image_test_loader_shapes(datasets):
    a = AttrDict(datasets=datasets, in_channels=3, num_classes=2, batch_size=3, unlabel_batch_size=3, train_crop_size=[32, 32],
                 synthetic_labeled=6, synthetic_unlabeled=6, synthetic_test_images=7)
    test = build_loader(a)[-1]
    assert len(test.dataset) == 7 and len(test) == 3 and callable(test.dataset.label_to_img)
    batches = list(test)
    assert [tuple(i.shape) for i, _ in batches] == [(3, 3, 32, 32), (3, 3, 32, 32), (1, 3, 32, 32)]          # the ragged last batch
    assert [tuple(l.shape) for _, l in batches] == [(3, 32, 32), (3, 32, 32), (1, 32, 32)]
    assert all(i.dtype == torch.float32 and l.dtype == torch.uint8 and int(l.max()) <= 1 for i, l in batches)
    again = list(test)
    assert all(torch.equal(i, j) and torch.equal(l, m) for (i, l), (j, m) in zip(batches, again))              # shuffle=False
    assert test.dataset.label_to_img(batches[0][1]).shape == (3, 32, 32, 3)
    del a["synthetic_test_images"]
    image, label = next(iter(build_loader(a)[-1]))                                                             # absent: volumes, as before
    assert tuple(image.shape) == (1, 8, 32, 32) == tuple(label.shape)


def test_isic_config_parses():
    a = loadyaml(os.path.join(ROOT, "config", "cps_unet_30k_224x224_ISIC.yaml"))
    assert a.datasets == "synthetic" and a.eval_images == "isic" and int(a.synthetic_test_images) > 0
    assert a.in_channels == 3 and a.num_classes == 2 and list(a.train_crop_size) == [224, 224] == list(a.test_crop_size)
    assert a.model1.in_channels == 3 and a.model2.num_classes == 2 and a.model1.opt == "sgd" and a.ckpt == "None"
    best = _Best(a, "model1")
    assert best.images == "isic" and best.with_hd95 == "device"
    assert int(a.synthetic_test_images) % int(a.batch_size) != 0          # the committed config exercises the short last batch


def test_the_new_symbol_is_bound():
    assert "hpfg_surface_sums" in L.PROTOTYPES
    lib = L.load()
    assert lib.hpfg_surface_sums(None, 0, 2, None, None, None) == -1 and b"null" in lib.hpfg_last_error()
