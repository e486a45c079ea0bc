"""CPU: the host side of the device HD95 (hpfg_amd.val.hd95_device, csrc/surface.hip): numpy's 95th percentile from two integer order
statistics, the argument checks and the size query of the hpfg_surface_* entry points (none of them reaches the GPU), and the mapping of
the config key ``eval_hd95`` onto the evaluation's ``with_hd95``."""
import ctypes

import numpy as np
import pytest

from hpfg_amd import _lib as L
from hpfg_amd import val as V
from hpfg_amd.train import _Best, eval_hd95_route
from hpfg_amd.utils import AttrDict


def _helper(v):
    k, k1, t = V.hd95_order_stats(len(v))
    return V.hd95_finish(int(v[k]), int(v[k1]), t)


def test_percentile_helper_matches_numpy():
    """Against np.percentile(sqrt(v), 95) for sorted integer arrays; 1e-9: the only difference is fp64 rounding of values below 1.5e4."""
    g = np.random.default_rng(0)
    cases = [np.sort(g.integers(0, 400, n)) for n in range(1, 61)]
    cases += [np.sort(g.integers(0, 1 << 28, int(n), endpoint=True)) for n in g.integers(1, 400, 3000)]
    cases += [np.arange(n, dtype=np.int64) ** 2 for n in (20, 21, 41, 101, 2001)]          # 0.95 (n - 1) a whole number, or nearly
    cases += [np.full(7, 1 << 28), np.zeros(3, np.int64), np.array([0, 1 << 28])]
    worst = 0.0
    for v in cases:
        want = float(np.percentile(np.sqrt(v.astype(np.float64)), 95))
        worst = max(worst, abs(_helper(v) - want))
        k, k1, t = V.hd95_order_stats(len(v))
        assert 0 <= k <= k1 <= len(v) - 1 and k1 - k <= 1 and 0.0 <= t < 1.0
    assert worst <= 1e-9, worst
    assert V.hd95_order_stats(1) == (0, 0, 0.0)
    assert V.hd95_finish(16801821, 16801821, 0.3) == float(np.sqrt(np.float64(16801821)))          # above 2^24: exact in fp64, not in fp32


def _bad_calls(lib):
    """(what, call(S, h, w, C, ndim, null)) of the two launching entry points; every pointer is a dummy the checks never follow."""
    p = ctypes.c_void_p(4096)
    counts = (ctypes.c_uint32 * L.SURFACE_SEGS)()

    def counts_call(S, h, w, C, ndim, null=False):
        return lib.hpfg_surface_counts(None if null else p, p, S, h, w, C, ndim, p, None)

    def dist_call(S, h, w, C, ndim, null=False):
        return lib.hpfg_surface_distances(p, p, S, h, w, C, ndim, None if null else ctypes.cast(counts, ctypes.c_void_p), p, 1 << 20, None)

    return [("surface_counts", counts_call), ("surface_distances", dist_call)]


def test_argument_errors_without_a_gpu():
    lib = L.load()
    for what, call in _bad_calls(lib):
        for args, word in (((3, 8, 8, 4, 3, True), b"null"), ((3, 8, 8, 4, 4), b"ndim"), ((2, 8, 8, 4, 2), b"2-D"), ((3, 8, 8, 1, 3), b"classes"),
                           ((3, 8, 8, 17, 3), b"classes"), ((8193, 8, 8, 4, 3), b"axis"), ((3, 8193, 8, 4, 3), b"axis"), ((3, 8, 8193, 4, 3), b"axis"),
                           ((8192, 8192, 32, 4, 3), b"2^31")):
            assert call(*args) == -1, (what, args)
            msg = lib.hpfg_last_error()
            assert what.encode() in msg and word in msg, (what, args, msg)
    # counts in a segment that no class of C owns, and a workspace that is too small, are refused as well
    counts = (ctypes.c_uint32 * L.SURFACE_SEGS)()
    counts[6] = 1
    p = ctypes.c_void_p(4096)
    assert lib.hpfg_surface_distances(p, p, 3, 8, 8, 4, 3, ctypes.cast(counts, ctypes.c_void_p), p, 1 << 20, None) == -1
    counts[6], counts[0], counts[1] = 0, 100, 100
    assert lib.hpfg_surface_distances(p, p, 3, 8, 8, 4, 3, ctypes.cast(counts, ctypes.c_void_p), p, 256, None) == -1
    assert b"workspace" in lib.hpfg_last_error()
    counts[0] = 3 * 8 * 8 + 1          # more surface points than voxels
    assert lib.hpfg_surface_distances(p, p, 3, 8, 8, 4, 3, ctypes.cast(counts, ctypes.c_void_p), p, 1 << 20, None) == -1
    # nothing to keep: legal, and nothing is launched
    empty = (ctypes.c_uint32 * L.SURFACE_SEGS)()
    assert lib.hpfg_surface_distances(p, p, 3, 8, 8, 4, 3, ctypes.cast(empty, ctypes.c_void_p), p, 256, None) == 0


def test_workspace_size_query():
    """256 bytes of cursors, then keys and points: int32 [n] each, each rounded up to 256 bytes (include/hpfg_hip.h)."""
    lib = L.load()
    assert L.SURFACE_SEGS == 32
    assert lib.hpfg_surface_workspace_bytes(4, 0) == 256
    assert lib.hpfg_surface_workspace_bytes(4, 1) == 256 + 2 * 256
    assert lib.hpfg_surface_workspace_bytes(9, 150000) == 256 + 2 * 600064
    assert lib.hpfg_surface_workspace_bytes(16, (1 << 31) - 1) == 256 + 2 * (1 << 33)
    for c, n in ((1, 10), (17, 10), (4, -1), (4, 1 << 31)):
        assert lib.hpfg_surface_workspace_bytes(c, n) == -1


def test_eval_hd95_key_maps_onto_with_hd95():
    assert eval_hd95_route(AttrDict()) is False
    assert eval_hd95_route(AttrDict(eval_hd95=False)) is False and eval_hd95_route(AttrDict(eval_hd95=None)) is False
    assert eval_hd95_route(AttrDict(eval_hd95="host")) is True
    assert eval_hd95_route(AttrDict(eval_hd95="device")) == "device"
    assert _Best(AttrDict(), "model").with_hd95 is False and _Best(AttrDict(eval_hd95="device"), "model").with_hd95 == "device"
    for bad in ("gpu", True, 1, "Device", ""):
        with pytest.raises(ValueError, match="eval_hd95"):
            _Best(AttrDict(eval_hd95=bad), "model")          # when the loop builds its evaluator, before the first iteration


def test_with_hd95_values():
    assert V._hd95_route(False) is False and V._hd95_route(True) is True and V._hd95_route("device") == "device"
    for bad in ("host", 1, None, "gpu"):
        with pytest.raises(ValueError, match="with_hd95"):
            V._hd95_route(bad)
