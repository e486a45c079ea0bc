"""GPU: the split-bf16 convolution kernels keep their bits.

tools/conv_bits.py runs the chunked 3x3 / 1x1 kernels, the weight gradient, the whole-tile forward kernel, the fused backward kernel and one
U-Net forward + backward on the fixed small cases the suite already argues for, in bf16x3 math; the SHA-256 of every result must equal
tests/golden/conv_bits.json, which was written by the commit BEFORE the kernels' staging phases moved into csrc/stage.h and csrc/tile16.h
(never by the code under test; two runs of that commit gave the same digests).  A digest that differs means an expression of a phase
changed: find it and restore it; a tolerance has no place here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("conv_bits", os.path.join(ROOT, "tools", "conv_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def test_every_result_has_the_recorded_bits(golden_dir):
    with open(os.path.join(golden_dir, "conv_bits.json")) as f:
        want = json.load(f)
    got = bits.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == bits.n_cases()
    diff = {k: [r for r in want[k] if got[k].get(r) != want[k][r]] for k in want if got[k] != want[k]}
    assert not diff, f"results whose bits changed: {diff}"
