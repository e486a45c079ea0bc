"""GPU: the fused loss keeps the bits it has to keep.

tools/loss_bits.py runs the three loss entry points on a fixed list of small cases (five shapes x C in {2, 3, 4, 5, 8, 9, 16} x five forms) and
records the `sums` row word by word and the SHA-256 of `out` and `dlogits`, the last two from an injected `sums` row.
tests/golden/loss_bits.json was written by the commit BEFORE the two kernel families (C <= 4 and 5 <= C <= 16, csrc/loss.hip and
csrc/loss_wide.hip then) were folded into one, on the GPU, never by the code under test.

  - C >= 5: every word and digest is equal (the kernels are the text they were).
  - every C: the finalize and backward digests are equal (pure functions of their inputs).
  - C <= 4, sums: the whole-numbered entries (cnt0, cnt1, sum mask, Y) are equal; outside the case (3, 1, 24, 24), whose first workgroup
    straddles the label-group boundary at an unaligned offset (another summation order inside it), every entry outside the Z blocks is equal;
    everything else (Z: p * p now enters as one fma, not as a rounded product) lies within 32 * 2^-24 of the recorded value, relative.  All
    these sums have non-negative terms, so any summation path carries a relative error of at most (path length) * 2^-24; the path is the
    product rounding, at most three serial adds per thread, six shuffle levels, three adds across the waves and the final cast: 14 roundings,
    two such results differ by at most 28 * 2^-24, rounded up to 32.  A dropped pixel or a wrong slot is off by 1/576 of a sum or more.
A word outside these rules means an expression changed: find it and restore it."""
import importlib.util
import json
import os
import struct

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("loss_bits", os.path.join(ROOT, "tools", "loss_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

STRADDLED = (3, 1, 24, 24)
REL = 32 * 2.0 ** -24


def _f32(word):
    return struct.unpack("<f", struct.pack("<I", int(word, 16)))[0]


@pytest.fixture(scope="module")
def runs(golden_dir):
    with open(os.path.join(golden_dir, "loss_bits.json")) as f:
        want = json.load(f)
    return want, bits.results()


def test_the_cases_are_the_recorded_ones(runs):
    want, got = runs
    assert sorted(got) == sorted(want)
    unlabelled = sum(1 for s in bits.SHAPES if s[1] < s[0])
    assert len(want) == len(bits.CLASSES) * (len(bits.SHAPES) * len(bits.FORMS) - (len(bits.SHAPES) - unlabelled) * len(bits.NEEDS_UNLABELLED))
    assert len(want) == 154
    for name, ncls, *_ in bits.cases():
        assert len(want[name]["sums"]) == len(got[name]["sums"]) == bits.slots(ncls)["nsum"]


def test_finalize_and_backward_keep_every_bit(runs):
    want, got = runs
    diff = {k: [r for r in ("out", "dlogits") if got[k][r] != want[k][r]] for k in want if any(got[k][r] != want[k][r] for r in ("out", "dlogits"))}
    assert not diff, f"results whose bits changed: {diff}"


def test_sums_above_four_classes_keep_every_bit(runs):
    want, got = runs
    diff = [name for name, ncls, *_ in bits.cases() if ncls >= 5 and got[name]["sums"] != want[name]["sums"]]
    assert not diff, f"sums whose bits changed: {diff}"


def test_sums_up_to_four_classes_move_in_the_z_blocks_alone(runs):
    want, got = runs
    bad, moved = [], 0
    for name, ncls, shape, _, _ in bits.cases():
        if ncls > 4:
            continue
        S = bits.slots(ncls)
        for i, (w, g) in enumerate(zip(want[name]["sums"], got[name]["sums"])):
            if w == g:
                continue
            moved += 1
            exact = i in S["integer"] or (shape != STRADDLED and i not in S["Z"])
            pw, pg = _f32(w), _f32(g)
            if exact or not abs(pg - pw) <= REL * abs(pw):
                bad.append((name, i, w, g, "must be equal" if exact else f"|new - recorded| = {abs(pg - pw):.3e} > {REL:.3e} * |recorded|"))
    print(f"sums words of C <= 4 that differ from the recorded ones: {moved}")
    assert not bad, bad[:20]
