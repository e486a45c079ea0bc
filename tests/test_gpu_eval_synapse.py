"""GPU: the Synapse evaluation path of hpfg_amd.val (reference val.py:196-265): every slice reaches the network through the cubic-spline
resize on the device (``resize_cubic``), everything after it is the machinery ``test_single_volume`` already uses."""
import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from hpfg_amd import val as V
from hpfg_amd.model import UNet

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NCLS = 9
MODEL_SEED, VOLUME_SEED = 5, 3          # a pair with which the network predicts several foreground classes (asserted below)


def _volume(seed, s, h, w, ncls=NCLS):
    g = np.random.default_rng(seed)
    coarse = g.integers(0, ncls, (s, 5, 5))
    lab = np.kron(coarse, np.ones((h // 5 + 1, w // 5 + 1), dtype=np.int64))[:, :h, :w].astype(np.uint8)
    img = (lab / (ncls - 1) + 0.1 * g.standard_normal((s, h, w))).astype(np.float32)
    return img, lab


def _trained_like_model(seed):
    """A nine-class U-Net whose BatchNorm running statistics are not the initial (0, 1): a few train-mode forwards on random data."""
    torch.manual_seed(seed)
    m = UNet(1, NCLS).to(DEV)
    m.math = "f32"
    m.train()
    with torch.no_grad():
        for k in range(3):
            m(torch.randn(8, 1, 32, 32, device=DEV) * (1 + k))
    return m


@pytest.fixture(scope="module")
def model():
    return _trained_like_model(MODEL_SEED)


def _dice_rows(pred, lab):
    cm = V.confusion_counts(pred, lab, NCLS)
    return [(V.dice_from_counts(cm, c), 0.0) for c in range(1, NCLS)]


def test_single_volume_synapse_is_the_composition_of_its_pieces(model):
    img, lab = _volume(VOLUME_SEED, 5, 40, 36)
    got = V.test_single_volume_synapse(torch.from_numpy(img)[None], torch.from_numpy(lab)[None], model, classes=NCLS, patch_size=(32, 32))
    x = V.resize_cubic(torch.from_numpy(img).to(DEV), (32, 32))
    at_patch = V.predict_volume(x, model, (32, 32))                       # already at patch size: no resize inside
    pred = V._resize_nearest(at_patch, (40, 36)).contiguous()
    assert got == _dice_rows(pred, torch.from_numpy(lab).to(DEV))          # same kernels on the same batches: bitwise
    assert len(got) == NCLS - 1 and model.training


@pytest.mark.parametrize("shape,patch", [((5, 40, 36), (32, 32)), ((3, 50, 44), (48, 48))])
def test_prediction_matches_the_host_route_through_scipy(model, shape, patch):
    s, h, w = shape
    img, lab = _volume(VOLUME_SEED, s, h, w)
    lab_d = torch.from_numpy(lab).to(DEV)
    pred = V.predict_volume(torch.from_numpy(img), model, patch, order=3)
    host = np.stack([zoom(sl, (patch[0] / h, patch[1] / w), order=3) for sl in img])          # val.py:243
    ref_pred = V._resize_nearest(V.predict_volume(torch.from_numpy(host), model, patch), (h, w)).contiguous()
    p, r = pred.cpu().numpy(), ref_pred.cpu().numpy()
    fg = sorted(set(np.unique(r).tolist()) - {0})
    mism = float((p != r).mean())
    got, want = _dice_rows(pred, lab_d), _dice_rows(ref_pred, lab_d)
    print(f"synapse eval {shape}/{patch}: foreground classes predicted {fg}, mismatch {mism:.2e}, "
          f"max |dice - ref| {max(abs(a[0] - b[0]) for a, b in zip(got, want)):.2e}")
    assert len(fg) >= 2                                                   # the Dice comparison is not vacuous
    assert mism < 2e-3
    for (d, hd), (rd, _) in zip(got, want):
        assert abs(d - rd) < 1e-3 and hd == 0.0


def test_patch_sized_slices_and_single_slices_take_the_no_resize_branch(model):
    img, lab = _volume(1, 3, 32, 32)
    it, lt = torch.from_numpy(img), torch.from_numpy(lab)
    model.train()
    got = V.test_single_volume_synapse(it[None], lt[None], model, classes=NCLS, patch_size=(32, 32))
    assert model.training
    assert got == V.test_single_volume(it[None], lt[None], model, classes=NCLS, patch_size=(32, 32))          # order plays no part without a resize
    # the reference's 2-D branch (val.py:255-260): one slice [1,h,w], forwarded at its own size whatever patch_size says
    one = V.test_single_volume_synapse(it[:1], lt[:1], model, classes=NCLS, patch_size=(48, 48))
    assert one == V.test_single_volume(it[None, :1], lt[None, :1], model, classes=NCLS, patch_size=(32, 32))
    model.eval()
    V.test_single_volume_synapse(it[None], lt[None], model, classes=NCLS, patch_size=(32, 32))
    assert not model.training
    model.train()


def test_synapse_loop_is_the_mean_over_volumes_and_logs_the_reference_images(model):
    from hpfg_amd.datasets.synthetic import SyntheticVolumes
    from hpfg_amd.utils import AttrDict

    class Writer:
        def __init__(self):
            self.images = {}

        def add_image(self, tag, img, step, dataformats="CHW"):
            self.images[tag] = (np.asarray(img), step, dataformats)

    data = SyntheticVolumes(2, 3, (40, 36), ncls=NCLS)
    loader = torch.utils.data.DataLoader(data, batch_size=1)
    w = Writer()
    args = AttrDict(num_classes=NCLS, test_crop_size=(32, 32), writer=w, device=DEV)
    dice, hd = V.test_synapse(model, loader, args, cur_itrs=200, name="model1")
    per = [np.array(V.test_single_volume_synapse(i[None], l[None], model, classes=NCLS, patch_size=(32, 32))) for i, l in data]
    assert abs(dice - float(np.mean((per[0] + per[1]) / 2, axis=0)[0])) < 1e-12 and hd == 0.0 and model.training
    assert set(w.images) == {"model1/Image", "model1/label_pred", "model1/label_true"}
    img, step, fmt = w.images["model1/Image"]
    assert img.shape == (1, 32, 32) and step == 200 and fmt == "CHW"
    image0, label0 = data[0]
    assert np.array_equal(img[0], V._resize_nearest(image0[:1].to(DEV), (32, 32))[0].cpu().numpy())          # the shown slice: order 0 (val.py:215)
    pred0 = V.predict_volume(image0, model, (32, 32), order=3)[0].cpu().numpy()
    assert np.array_equal(w.images["model1/label_pred"][0], data.label_to_img(pred0))
    assert np.array_equal(w.images["model1/label_true"][0], data.label_to_img(label0[0].numpy()))
    assert w.images["model1/label_pred"][0].shape == (40, 36, 3) and w.images["model1/label_pred"][2] == "HWC"
    V.test_synapse(model, loader, AttrDict(num_classes=NCLS, test_crop_size=(32, 32), device=DEV), cur_itrs=1)          # no writer: nothing fails
