"""CPU: the host side of the cubic-spline resize (hpfg_amd.val): the per-axis matrix restates scipy.ndimage.zoom(order=3) (val.py:243), and
the tap tables that hpfg_resize_cubic consumes keep it to below 1e-9."""
import numpy as np
import pytest
from scipy.ndimage import zoom

from hpfg_amd import _lib as L
from hpfg_amd import val as V

SIZES = [((40, 36), (24, 24)), ((37, 53), (32, 48)), ((7, 5), (16, 16)), ((300, 148), (224, 224)), ((512, 512), (224, 224)), ((2, 3), (5, 2))]


@pytest.mark.parametrize("src,dst", SIZES)
def test_axis_matrices_restate_scipy_zoom_order3(src, dst):
    a = np.random.default_rng(7).standard_normal(src) + 3.0
    ref = zoom(a, (dst[0] / src[0], dst[1] / src[1]), order=3)          # fp64 in, fp64 out
    my, _, vy = V._cubic_axis_matrix(src[0], dst[0])
    mx, _, vx = V._cubic_axis_matrix(src[1], dst[1])
    assert np.abs(my @ a @ mx.T - ref).max() <= 1e-12 * np.abs(a).max()
    assert (vy[-1], vx[-1]) == ((False, False) if (src, dst) == ((512, 512), (224, 224)) else (True, True))


@pytest.mark.parametrize("n_in,n_out", [(5, 16), (36, 24), (53, 48), (512, 224), (148, 224)])
def test_tap_tables_are_the_matrix_rows_on_their_windows(n_in, n_out):
    T = L.RESIZE_TAPS
    tab = V._cubic_axis_table(n_in, n_out)
    assert tab.dtype == np.int32 and tab.shape == ((T + 1) * n_out,)
    w, first = tab[:T * n_out].view(np.float32).reshape(n_out, T), tab[T * n_out:]
    m, _, valid = V._cubic_axis_matrix(n_in, n_out)
    assert ((first >= 0) == valid).all() and (first[valid] + min(T, n_in) <= n_in).all()
    dense = np.zeros((n_out, n_in))
    for o in np.nonzero(valid)[0]:
        k = min(T, n_in - first[o])
        dense[o, first[o]:first[o] + k] = w[o, :k]
        assert (w[o, k:] == 0).all()
    assert np.abs(dense - m).max() < 1e-7          # fp32 rounding of weights up to 1.4; the cut itself is asserted < 1e-9 by the builder
    assert (w[~valid] == 0).all()
