"""GPU: the launch schedule of UNetEngine is pinned.

For every regime of tools/record_engine_schedule.py (math mode, where the BatchNorm sums go, each fusion switch, deferred weight gradients,
the data-parallel bucket callback) one eager train-mode forward + backward of UNet(1, 4) must issue the tagged launches of
tests/golden/engine_schedule.json, in that order.  A pull request that changes the schedule on purpose regenerates the file with the tool, and
the change shows as a diff of tag lists.

The second test covers the one thing the schedule cannot: the fused backward kernel's grid is fixed when the backward workspace is
allocated, and a kernel-form option switched afterwards must be refused before the launch (the slab region would have another size)."""
import ctypes as C
import importlib.util
import json
import os

import pytest
import torch

from hpfg_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")

_spec = importlib.util.spec_from_file_location("record_engine_schedule", os.path.join(ROOT, "tools", "record_engine_schedule.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_schedule.json")) as f:
        return json.load(f)


def test_golden_file_covers_every_regime_and_shape(golden):
    assert sorted(golden) == sorted(rec.shape_key(sh) for sh in rec.SHAPES)
    for key, regimes in golden.items():
        assert sorted(regimes) == sorted(rec.REGIMES), key
        assert all(len(tags) > 40 for tags in regimes.values()), key      # 23 convs forward alone
        # the switch that takes a kernel out of the schedule did so: every layer the default schedule hands to the fused thin backward has a
        # weight gradient and -- but for the network's first conv, whose input takes no gradient -- an input gradient of its own instead
        thin = [t.split(":", 1)[1] for t in regimes["default"] if t.startswith("fused_bwd:")]
        off = regimes["fused_bwd_off"]
        assert thin and thin[-1] == "encoder.in_conv.conv_conv.0", (key, thin)
        assert not any(t.startswith("fused_bwd:") for t in off), key
        assert all("wgrad:" + n in off for n in thin) and all("dgrad:" + n in off for n in thin[:-1]), key


@pytest.mark.parametrize("regime", list(rec.REGIMES))
@pytest.mark.parametrize("shape", rec.SHAPES, ids=rec.shape_key)
def test_launch_schedule_equals_the_recorded_one(golden, shape, regime):
    tags = rec.record(regime, shape)
    want = golden[rec.shape_key(shape)][regime]
    assert tags, "the pass recorded no launch"
    assert sum(t.startswith("fwd:") for t in tags) == 23, tags
    first = next((i for i, (a, b) in enumerate(zip(tags, want)) if a != b), min(len(tags), len(want)))
    assert tags == want, f"{len(tags)} launches, {len(want)} recorded; first difference at {first}: {tags[first:first + 3]} != {want[first:first + 3]}"


def _first_layer_grid(n, hw, option):
    """Workgroups hpfg_fused_bwd would launch for the first layer of UNet(1, 4) at n x 1 x hw x hw with HPFG_OPT_FIRST_WGRAD = option."""
    lib = L.load()
    fa = L.FusedBwdArgs()
    fa.xa0.mode, fa.xa0.C, fa.xa0.Hs, fa.xa0.Ws = L.ACT_STRIDED, 1, hw, hw
    fa.d.a0.mode, fa.d.a0.C = L.ACT_DZ, 16
    fa.d.N, fa.d.H, fa.d.W, fa.d.taps, fa.d.math = n, hw, hw, 9, L.MATH_BF16X3
    fa.Cin, fa.CinPad, fa.Cout, fa.CoutPad = 1, 16, 16, 16
    prev = lib.hpfg_set_option(L.OPT_FIRST_WGRAD, option)
    try:
        return lib.hpfg_fused_bwd_grid(C.byref(fa))
    finally:
        lib.hpfg_set_option(L.OPT_FIRST_WGRAD, prev)


def test_fused_backward_refuses_a_grid_other_than_the_allocated_one():
    """The option is switched between the allocation of the backward workspace and a launch: _fused_bwd must raise before the launch, naming
    the layer and both counts -- no kernel runs with a slab region of the wrong size."""
    from hpfg_amd.model import UNet, reset_dropout_streams
    lib = L.load()
    # the first shape at which the two kernel forms differ in their grid (the streaming kernel takes rows of >= 64 pixels only)
    grids = {hw: (_first_layer_grid(2, hw, 0), _first_layer_grid(2, hw, 1)) for hw in (48, 32, 64)}
    hw = next((h for h, (g0, g1) in grids.items() if g0 != g1 and g0 > 0 and g1 > 0), None)
    if hw is None:
        pytest.skip(f"both values of HPFG_OPT_FIRST_WGRAD give the same grid at every shape tried: {grids}")
    reset_dropout_streams()
    torch.manual_seed(5)
    m = UNet(1, 4).to(DEV)
    m.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 1, hw, hw, generator=g).to(DEV)
    dy = torch.randn(2, 4, hw, hw, generator=g).to(DEV)
    m(x).backward(dy)                                   # allocates the backward workspace for the current kernel form
    torch.cuda.synchronize()
    eng = next(iter(m._engines.values()))[0]
    first = eng.order[0].name
    cur = lib.hpfg_set_option(L.OPT_FIRST_WGRAD, 0)     # (returns the value in force)
    lib.hpfg_set_option(L.OPT_FIRST_WGRAD, cur)
    assert eng.fused_grid[first] == grids[hw][1 if cur else 0]
    lib.hpfg_set_option(L.OPT_FIRST_WGRAD, 0 if cur else 1)
    try:
        out = m(x)
        with pytest.raises(RuntimeError, match=r"fused_bwd\[%s\]: %d workgroups, %d weight-gradient slabs allocated"
                           % (first.replace(".", r"\."), grids[hw][0 if cur else 1], grids[hw][1 if cur else 0])):
            out.backward(dy)
    finally:
        lib.hpfg_set_option(L.OPT_FIRST_WGRAD, cur)
        torch.cuda.synchronize()
    # with the option restored the SAME engine trains on (the model hands out an engine whose backward is still owed only when no other is
    # free, so the refused pass is written off first: otherwise a second engine would be built and nothing shown about this one)
    eng.bwd_ready = False
    m(x).backward(dy)
    torch.cuda.synchronize()
    assert [len(pool) for pool in m._engines.values()] == [1] and not eng.bwd_ready
    assert torch.isfinite(m.flat_grads).all()
