"""GPU: the attention kernels keep their bits.

tools/attn_bits.py runs forward + backward of ops_tokens.attention, attention_keys and window_attention on a fixed list of small cases in
both math modes; the SHA-256 of every result must equal tests/golden/attn_bits.json, which was written by the commit BEFORE the kernels'
phases moved into csrc/attn_core.h (never by the code under test).  A digest that differs means an expression of a phase changed: find
it and restore it; a tolerance has no place here."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("attn_bits", os.path.join(ROOT, "tools", "attn_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


def test_every_result_has_the_recorded_bits(golden_dir):
    with open(os.path.join(golden_dir, "attn_bits.json")) as f:
        want = json.load(f)
    got = bits.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == 2 * (len(bits.HEAD_DIMS) * (len(bits.ATTENTION) + len(bits.ATTENTION_KEYS)) + len(bits.WINDOW))
    diff = {k: [r for r in want[k] if got[k].get(r) != want[k][r]] for k in want if got[k] != want[k]}
    assert not diff, f"results whose bits changed: {diff}"
