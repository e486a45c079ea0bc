"""GPU: hpfg_amd.val.resize_cubic (hpfg_resize_cubic) against scipy.ndimage.zoom(order=3), the resize of the reference's Synapse evaluation
(val.py:243), slice by slice.

Bound: max|dev - scipy| <= 2e-5 * max|input|.  The fp32 restatement of the law differs from scipy (fp64, rounded to fp32) by about
4e-7 * max|input| on the host; the bound leaves ~50x for fused multiply-adds, the summation order of the banded form and the 1e-9 cut of
the prefilter's response, and stays 50x under the project's 1e-3 parity bar.  Inputs are Gaussian + 3.0: a nonzero mean, so that an edge
row that scipy computes cannot pass as zeros and one that scipy zeroes cannot pass by accident."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.ndimage import zoom

from hpfg_amd import _lib as L
from hpfg_amd import val as V

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REL = 2e-5

CASES = [
    ((3, 7, 5), (16, 16)),           # lines shorter than the tap window: the whole closed-form row; upsampling; slice stride
    ((2, 40, 36), (24, 24)),         # downsampling, widths that are no multiple of 64
    ((2, 37, 53), (32, 48)),         # odd sizes (scalar loads), another factor per axis
    ((1, 64, 64), (224, 224)),       # large upsampling
    ((2, 300, 148), (224, 224)),     # one axis down, one up, lines longer than the window, no invalid edge
    ((2, 512, 512), (224, 224)),     # the Synapse case: scipy zeroes output row 223 and column 223
    ((1, 20, 600), (24, 520)),       # more than one 256-column tile in the column pass: each stages only the span of the row it taps
]


def _input(shape, seed=0):
    return (np.random.default_rng(seed).standard_normal(shape) + 3.0).astype(np.float32)


def _scipy(a, dst):
    return np.stack([zoom(sl, (dst[0] / sl.shape[0], dst[1] / sl.shape[1]), order=3) for sl in a])


def _dev(a, dst):
    out = V.resize_cubic(torch.from_numpy(a).to(DEV), dst)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape,dst", CASES)
def test_resize_cubic_matches_scipy(shape, dst):
    a = _input(shape, seed=shape[1])
    ref = _scipy(a, dst)
    got = _dev(a, dst)
    assert got.shape == ref.shape == (shape[0],) + dst and got.dtype == np.float32
    err, amax = float(np.abs(got - ref).max()), float(np.abs(a).max())
    print(f"resize_cubic {shape} -> {dst}: max|dev - scipy| = {err:.3e} = {err / amax:.3e} * max|input|")
    assert err <= REL * amax
    if shape[1:] == (512, 512) and dst == (224, 224):          # the edge quirk, pinned on both sides
        assert (ref[:, 223, :] == 0.0).all() and (ref[:, :, 223] == 0.0).all()
        assert (got[:, 223, :] == 0.0).all() and (got[:, :, 223] == 0.0).all()
        assert (ref[:, :223, :223] > 0.5).any()
    else:
        assert np.abs(ref[:, -1, :]).min() > 0.0 and np.abs(ref[:, :, -1]).min() > 0.0          # no zeroed edge in the reference here


def test_same_size_returns_its_input():
    t = torch.from_numpy(_input((1, 32, 32))).to(DEV)
    assert V.resize_cubic(t, (32, 32)) is t


def test_table_cache_and_scratch_reuse_are_bitwise_stable():
    a, b = _input((2, 40, 36), seed=1), _input((3, 64, 52), seed=2)
    first = _dev(a, (24, 24))
    other = _dev(b, (48, 40))          # another pair of tables, a larger scratch
    again = _dev(a, (24, 24))
    assert np.array_equal(first, again)
    assert float(np.abs(other - _scipy(b, (48, 40))).max()) <= REL * float(np.abs(b).max())


def test_an_axis_shorter_than_two_is_refused_before_any_launch():
    t = torch.ones(2, 1, 8, device=DEV)
    with pytest.raises(ValueError):
        V.resize_cubic(t, (8, 8))
    with pytest.raises(ValueError):
        V.resize_cubic(torch.ones(2, 8, 8, device=DEV), (8, 1))
    lib = L.load()
    assert lib.hpfg_resize_cubic_scratch_bytes(2, 1, 8, 8, 8) == -1 and lib.hpfg_resize_cubic_scratch_bytes(2, 8, 8, 8, 8) == 2 * 8 * 8 * 4
    p = ctypes.c_void_p(256)          # never dereferenced: the argument check returns first
    assert lib.hpfg_resize_cubic(p, 2, 1, 8, p, 8, 8, p, p, p, 1 << 20, None) == -1
    assert b"resize_cubic" in lib.hpfg_last_error()
    assert lib.hpfg_resize_cubic(p, 2, 8, 8, p, 8, 8, p, p, p, 16, None) == -1 and b"scratch" in lib.hpfg_last_error()
    torch.cuda.synchronize()
