"""GPU: the label and batch-mixing kernels of csrc/misc.hip through their hpfg_amd.train wrappers -- argmax_labels (the pseudo-label rule of
CPS / HPFG / CTCT and the CutMix label mix), cutmix_blend, and ICT's mix_samples / softmax_mix -- against plain references on the CPU:
torch.argmax / torch.where exactly, the blends and the mixed softmax in float64 inside bounds derived from the operation count.  Up to 16
classes, odd image sizes, and one case each past the 4096-workgroup cap of the launches (the grid-stride loop's second pass)."""
import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd.train import argmax_labels, cutmix_blend, mix_samples, softmax_mix
from hpfg_amd.utils import BoxMaskGenerator
from tests.helpers import N_BIG_MIX, blend_f64, softmax_mix_f64, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BIG = (1, 1, N_BIG_MIX)          # N, H, W of 4096*256 + 257 pixels: one more than a full pass of 4096 workgroups


def _tied_logits(N, C, H, W, gen):
    """Integer logits in [-2, 2]; at nine pixels in ten one more channel (before or behind the first maximum, or the maximum itself) is
    raised to the maximum, so that most pixels have their maximum more than once.  -> (logits [N,C,H,W], share of pixels with a tie)."""
    x = torch.randint(-2, 3, (N, C, H, W), generator=gen).float()
    mx = x.max(1, keepdim=True).values
    ch = torch.randint(0, C, (N, 1, H, W), generator=gen)
    force = torch.rand(N, 1, H, W, generator=gen) < 0.9
    x = torch.where(force & (torch.arange(C).view(1, C, 1, 1) == ch), mx, x)
    ties = ((x == x.max(1, keepdim=True).values).sum(1) >= 2).float().mean()
    return x, float(ties)


# every class count in both layouts at an odd image size; past the grid cap 2 classes in both layouts and 16 in channels_last
ARGMAX_CASES = ([(C, (3, 37, 53), lay) for C in (1, 2, 4, 9, 16) for lay in ("nchw", "channels_last")]
                + [(2, BIG, "nchw"), (2, BIG, "channels_last"), (16, BIG, "channels_last")])


@pytest.mark.parametrize("C,nhw,layout", ARGMAX_CASES, ids=[f"C{c}-{'grid_cap' if s_ == BIG else '37x53'}-{lay}" for c, s_, lay in ARGMAX_CASES])
def test_argmax_labels_first_maximum_and_label_mix(C, nhw, layout):
    """argmax_labels == torch.argmax(dim=1) on the CPU (the FIRST maximal index) on logits whose maximum is tied at most pixels, and with
    (mix_labels, mix_mask) == where(mask > 0.5, argmax, label): a mask of exactly 0.5 selects the label; labels up to 255.  Both routes of
    the wrapper's layout change: a contiguous NCHW tensor (copied to NHWC) and a channels_last one (viewed)."""
    N, H, W = nhw
    gen = torch.Generator().manual_seed(100 * C + H)
    x, ties = _tied_logits(N, C, H, W, gen)
    assert C == 1 or ties > 0.5, ties            # (one class cannot tie)
    assert x.min() >= -2 and x.max() <= 2
    want = torch.argmax(x, dim=1).to(torch.uint8)
    xd = x.to(DEV)
    if layout == "channels_last":
        xd = xd.to(memory_format=torch.channels_last)
    got = argmax_labels(xd)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W)
    assert torch.equal(got.cpu(), want)
    labels = torch.randint(0, 256, (N, H, W), generator=gen).to(torch.uint8)
    labels[0, 0, :3] = torch.tensor([255, 254, 0], dtype=torch.uint8)
    mask = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])[torch.randint(0, 5, (N, H, W), generator=gen)]
    assert all(float((mask == v).float().mean()) > 0.1 for v in (0.0, 0.25, 0.5, 0.75, 1.0))
    got = argmax_labels(xd, labels.to(DEV), mask.to(DEV))
    assert torch.equal(got.cpu(), torch.where(mask > 0.5, want, labels))


def test_argmax_labels_refusals():
    lib = L.load()
    x = torch.zeros(1, 2, 2, 4, device=DEV)
    out, lab, msk = torch.zeros(4, dtype=torch.uint8, device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV), torch.zeros(4, device=DEV)
    st = stream(DEV)
    assert lib.hpfg_argmax_labels(L.ptr(x), 1, 2, 2, 0, None, None, L.ptr(out), st) == -1
    assert lib.hpfg_argmax_labels(L.ptr(x), 1, 2, 2, 256, None, None, L.ptr(out), st) == -1
    assert lib.hpfg_argmax_labels(L.ptr(x), 1, 2, 2, 4, L.ptr(lab), None, L.ptr(out), st) == -1          # labels without a mask
    assert lib.hpfg_argmax_labels(L.ptr(x), 1, 2, 2, 4, None, L.ptr(msk), L.ptr(out), st) == -1
    assert lib.hpfg_argmax_labels(L.ptr(x), 1, 2, 2, 4, L.ptr(lab), L.ptr(msk), L.ptr(out), st) == 0
    with pytest.raises(L.HipLibraryError):
        argmax_labels(torch.zeros(1, 256, 2, 2, device=DEV))


def _report(what, err, bound):
    ratio = float((err / bound).max())
    print(f"{what}: largest error / bound = {ratio:.3f} (largest error {float(err.max()):.3e})")
    return ratio


@pytest.mark.parametrize("shape", [(4, 3, 37, 53), (1, 1, 9, N_BIG_MIX // 9)], ids=["37x53", "grid_cap"])
def test_cutmix_blend_selects_exactly_and_blends_within_rounding(shape):
    """With a 0/1 mask of BoxMaskGenerator (one [N,1,H,W] mask broadcast over the channels) cutmix_blend == torch.where(mask == 1, b, a)
    bit for bit; with fractional masks |out - (a(1-m) + b m)| <= 3 * 2^-24 * (|a| + |b|) elementwise against float64."""
    N, C_, H, W = shape
    assert (H, W) == (37, 53) or N * C_ * H * W == N_BIG_MIX
    g = torch.Generator().manual_seed(H + W)
    a, b = torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g) * 40
    gen = BoxMaskGenerator(prop_range=(0.25, 0.5), n_boxes=4, random_aspect_ratio=True, prop_by_area=True, within_bounds=True, invert=True)
    mask = gen.generate_params_device(N, (H, W), DEV, rng=np.random.RandomState(5))
    assert tuple(mask.shape) == (N, 1, H, W) and 0.05 < float(mask.mean()) < 0.95 and bool(((mask == 0) | (mask == 1)).all())
    got = cutmix_blend(a.to(DEV), b.to(DEV), mask)
    assert torch.equal(got.cpu(), torch.where(mask.cpu().expand(shape) == 1, b, a))
    frac = torch.rand((N, 1, H, W), generator=g)
    frac[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 0.5, 2.0 ** -24])
    got = cutmix_blend(a.to(DEV), b.to(DEV), frac.to(DEV)).cpu().numpy()
    ref, bound = blend_f64(a.numpy(), b.numpy(), frac.expand(shape).numpy())
    assert _report(f"cutmix_blend {shape}", np.abs(got - ref), bound) <= 1.0


@pytest.mark.parametrize("shape", [(5, 3, 37, 53), (5, 1, 1, 209771)], ids=["37x53", "grid_cap"])
def test_mix_samples_takes_the_factor_of_its_sample(shape):
    """a(1 - f[s]) + b f[s] per sample s within 3 * 2^-24 * (|a| + |b|) of float64; f = 0 gives a and f = 1 gives b bit for bit.  Five samples
    of a size that is no multiple of 256 (and, second case, 5 * 209771 elements: past the grid cap): a factor looked up by anything but
    element / per_sample shows."""
    n, per = shape[0], int(np.prod(shape[1:]))
    assert per % 256 != 0 and (shape[-1] == 53 or n * per > 4096 * 256)
    g = torch.Generator().manual_seed(per % 1000)
    a, b = torch.randn(shape, generator=g) * 3, torch.randn(shape, generator=g) * 40
    f = torch.tensor([0.0, 1.0, 0.3, 0.62, 0.999])
    got = mix_samples(a.to(DEV), b.to(DEV), f.to(DEV)).cpu()
    assert torch.equal(got[0], a[0]) and torch.equal(got[1], b[1])
    ref, bound = blend_f64(a.numpy(), b.numpy(), f.view(n, 1, 1, 1).expand(shape).numpy())
    assert _report(f"mix_samples {shape}", np.abs(got.numpy() - ref), bound) <= 1.0


@pytest.mark.parametrize("C,n,H,W", [(2, 4, 37, 53), (4, 4, 37, 53), (9, 4, 37, 53), (16, 4, 37, 53), (2, 3, 1, N_BIG_MIX // 3)],
                         ids=["C2", "C4", "C9", "C16", "grid_cap"])
def test_softmax_mix_against_float64(C, n, H, W):
    """softmax(t0)(1 - f[s]) + softmax(t1) f[s] against float64, logits randn * 8 with one image row raised by 80 and one lowered by 80 (no
    exp of an unshifted logit survives that): |error| <= (C + 8) * 2^-24 per probability -- a one-ulp expf of a value <= 1, C additions
    for the sum, the division and the mix, each at most 2^-24 of a value <= 1 -- and every pixel's probabilities sum to 1 within
    C * 2^-23.  torch.softmax in float32 on the CPU, mixed in float32, stays inside the same bound on these inputs."""
    assert n * H * W == N_BIG_MIX or (H, W) == (37, 53)
    g = torch.Generator().manual_seed(C * 7 + W % 100)
    t0, t1 = torch.randn(n, C, H, W, generator=g) * 8, torch.randn(n, C, H, W, generator=g) * 8
    if H > 1:
        t0[:, :, 3], t1[:, :, 3] = t0[:, :, 3] + 80, t1[:, :, 3] + 80
        t0[:, :, 11], t1[:, :, 11] = t0[:, :, 11] - 80, t1[:, :, 11] - 80
    else:
        t0[..., :500], t1[..., :500] = t0[..., :500] + 80, t1[..., :500] + 80
        t0[..., 500:1000], t1[..., 500:1000] = t0[..., 500:1000] - 80, t1[..., 500:1000] - 80
    f = torch.tensor([0.0, 1.0, 0.37, 0.81][:n])
    ref = softmax_mix_f64(t0, t1, f)
    bound = (C + 8) * 2.0 ** -24
    w = f.view(n, 1, 1, 1)
    host32 = torch.softmax(t0, 1) * (1 - w) + torch.softmax(t1, 1) * w
    e_host = float((host32.double() - ref).abs().max())
    got = softmax_mix(t0.to(DEV), t1.to(DEV), f.to(DEV))
    assert tuple(got.shape) == (n, C, H, W)
    got = got.cpu().double()
    e = float((got - ref).abs().max())
    print(f"softmax_mix C={C} {n}x{H}x{W}: largest error / bound = {e / bound:.3f} (float32 torch.softmax on the CPU: {e_host / bound:.3f})")
    assert e_host <= bound
    assert torch.isfinite(got).all() and e <= bound
    assert float((got.sum(1) - 1).abs().max()) <= C * 2.0 ** -23


def test_softmax_mix_refuses_more_than_64_classes():
    lib = L.load()
    t = torch.zeros(1, 2, 2, 65, device=DEV)
    f, out = torch.zeros(1, device=DEV), torch.zeros(1, 2, 2, 65, device=DEV)
    assert lib.hpfg_softmax_mix(L.ptr(t), L.ptr(t), L.ptr(f), L.ptr(out), 1, 2, 2, 65, stream(DEV)) == -1
    assert lib.hpfg_softmax_mix(L.ptr(t), L.ptr(t), L.ptr(f), L.ptr(out), 1, 2, 2, 64, stream(DEV)) == 0
    torch.cuda.synchronize()
