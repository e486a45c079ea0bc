"""GPU: the split-bf16 GEMM and attention kernels keep their bits.

tools/dense_bits.py runs hpfg_gemm_bf16x3, its split-K form, hpfg_gemm_tn_bf16x3 and the forward and backward entry points of the three
attention families (the window family also in its dropout form with an explicit mask) on the fixed small cases the suite already argues
for, in bf16x3 math; the SHA-256 of every result must equal tests/golden/dense_bits.json, which was written by commit f4ae714 ("Pin the
GEMM, column-sum and neck kernels to float64 at every edge"), the commit BEFORE the split-bf16 arithmetic moved into csrc/bf16x3.h (never
by the code under test; two runs of that commit's library gave the same digests).  A digest that differs means an expression of the
arithmetic changed: find it and restore it; a tolerance has no place here.

One expression was changed on purpose since: ds_drop_t of csrc/attn_window.h rounds dP .* f on its own, because the contracted form left a
float32 rounding error in a dS that is 0 (tests/test_gpu_attn_window_edges.py holds the result to float64).  The
dqkv and dtable digests of the four "window drop" cases are those of that change; their `out` digests and every other case are still
the run of f4ae714."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("dense_bits", os.path.join(ROOT, "tools", "dense_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def test_every_result_has_the_recorded_bits(golden_dir):
    with open(os.path.join(golden_dir, "dense_bits.json")) as f:
        want = json.load(f)
    got = bits.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == bits.n_cases()
    diff = {k: [r for r in want[k] if got[k].get(r) != want[k][r]] for k in want if got[k] != want[k]}
    assert not diff, f"results whose bits changed: {diff}"
