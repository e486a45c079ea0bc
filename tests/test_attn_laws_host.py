"""The float64 laws of the attention kernels (tests/helpers.py: attn_f64, window_attn_f64) against float64 autograd of the written-out
formulas; the input families' conditions; the yardsticks; and the proof that the rule of tests/test_gpu_attn_edges.py -- error at most
8 x the yardstick's own error against the law -- would catch each named way of getting the operation wrong: every mutation of the law
moves some tensor of some case by at least 4 tolerances.  The same for the law with a dropout mask and in the packed tile's view, which
tests/test_gpu_attn_window_edges.py holds the DROP kernels of csrc/attn_window.hip and csrc/attn_window_packed.hip to, and the old hand
bounds of those kernels beside the rule's tolerances.  CPU only."""
import pytest
import torch

from tests import helpers as T

D_ALL = T.ATTN_HEAD_DIMS
ATTN_ALL = [(f, *c) for f in ("unit", "sharp", "offset") for c in T.ATTN_M_EDGES + T.ATTN_N_EDGES] + \
           [(f, *c) for f in ("sharp", "offset") for c in T.ATTN_KEYS_EDGES]
WINDOW_ALL = [(f, *c) for f in ("unit", "sharp", "hot") for c in T.WINDOW_EDGES]


def _rel(a, b):
    return float((a - b).abs().max()) / max(1e-300, float(b.abs().max()))


def _attn_written_out(q, kv, heads, d, scale):
    B, N, C_ = q.shape
    M = kv.shape[1]
    qh = q.reshape(B, N, heads, d).permute(0, 2, 1, 3)
    k, v = kv.reshape(B, M, 2, heads, d).permute(2, 0, 3, 1, 4)
    s = (qh @ k.transpose(-2, -1)) * scale
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, C_), torch.logsumexp(s, -1)


@pytest.mark.parametrize("family,B,N,M,heads,d,scale", [("unit", 2, 65, 33, 2, 32, None), ("sharp", 1, 130, 255, 1, 64, None), ("offset", 2, 65, 17, 2, 32, None),
                                                        ("unit", 2, 65, 33, 2, 64, 0.3), ("unit", 2, 65, 33, 2, 32, 0.0), ("sharp", 1, 513, 49, 1, 32, None)])
def test_attention_law_is_autograd_of_the_formula(family, B, N, M, heads, d, scale):
    c = T.attn_case(family, B, N, M, heads, d, scale)
    qr, kr = c["q"].double().requires_grad_(True), c["kv"].double().requires_grad_(True)
    o, lse = _attn_written_out(qr, kr, heads, d, c["scale"])
    o.backward(c["do"].double())
    out, l64, dq, dkv = c["ref"]
    assert _rel(out, o.detach()) < 1e-13 and float((l64 - lse.detach()).abs().max()) < 1e-12
    if c["scale"] == 0:
        k, v = c["kv"].double().reshape(B, M, 2, heads, d).unbind(2)
        assert _rel(out, v.mean(1, keepdim=True).expand(B, N, heads, d).reshape(B, N, -1)) < 1e-14          # uniform over exactly the M keys
        assert float(dq.abs().max()) == 0.0 and float(dkv.reshape(B, M, 2, -1)[:, :, 0].abs().max()) == 0.0
        assert float(qr.grad.abs().max()) == 0.0
    else:
        assert _rel(dq, qr.grad) < 1e-12
    assert _rel(dkv, kr.grad) < 1e-12


@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("family", ["unit", "hot"])
@pytest.mark.parametrize("B,H,W,w,s,heads", T.WINDOW_EDGES + [(1, 14, 14, 7, 3, 2), (1, 16, 8, 8, 4, 1)])
def test_window_law_is_autograd_of_the_reference_formula(family, B, H, W, w, s, heads, d):
    c = T.window_case(family, B, H, W, w, s, heads, d)
    qr, tr = c["qkv"].double().requires_grad_(True), c["table"].double().requires_grad_(True)
    o = T.window_attn_reference(qr, tr, heads, w, s, c["scale"])
    o.backward(c["do"].double())
    want = T.window_results((o.detach(), qr.grad, tr.grad))
    for name, a, b in zip(T.WINDOW_TENSORS, c["ref"], want):
        assert a.shape == b.shape and _rel(a, b) < 1e-12, name


def test_window_law_takes_another_scale():
    qkv, table, do = T.window_inputs("unit", 1, 8, 12, 4, 1, 2, 32)
    qr, tr = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    o = T.window_attn_reference(qr, tr, 2, 4, 1, 0.3)
    o.backward(do.double())
    for a, b in zip(T.window_attn_f64(qkv, table, do, 2, 4, 1, 0.3), (o.detach(), qr.grad, tr.grad)):
        assert _rel(a, b) < 1e-12


@pytest.mark.parametrize("d", D_ALL)
def test_families_meet_their_conditions_and_yardsticks_are_finite(d):
    """the generators assert the conditions; here every case of the GPU file is generated once"""
    peak = {}
    for family, B, N, M, heads in ATTN_ALL:
        c = T.attn_case(family, B, N, M, heads, d)
        S = T._attn_logits(c["q"], c["kv"], heads, d, c["scale"])
        lo, hi = peak.get(family, (1.0, 0.0))
        peak[family] = (min(lo, float(T._row_max_p(S).median())), max(hi, float(S.abs().max())))
        for m in T.ATTN_MATHS:
            assert all(bool(torch.isfinite(t).all()) for t in c["yard"][m]), (family, B, N, M, heads, m)
            assert all(t > 0 for t in c["tol"][m])
    for family, B, H, W, w, s, heads in WINDOW_ALL:
        c = T.window_case(family, B, H, W, w, s, heads, d)
        for m in T.ATTN_MATHS:
            assert all(bool(torch.isfinite(t).all()) for t in c["yard"][m]), (family, B, H, W, w, s, heads, m)
    for family, (p, top) in peak.items():
        print(f"d={d} {family}: least median row-max P {p:.2f}, largest |logit| {top:.1f}")
    assert peak["offset"][1] > 100 and peak["sharp"][0] >= 0.5


@pytest.mark.parametrize("d", D_ALL)
def test_float32_without_the_max_subtraction_overflows_on_offset(d):
    for B, N, M, heads in T.ATTN_M_EDGES[:3] + T.ATTN_KEYS_EDGES[:1]:
        c = T.attn_case("offset", B, N, M, heads, d)
        bad = T.attn_f64(c["q"], c["kv"], c["do"], heads, d, c["scale"], arith=torch.float32, max_subtract=False)
        assert not bool(torch.isfinite(bad[0]).all())
        good = T.attn_case("unit", B, N, M, heads, d)          # ... and is harmless on unit logits: why the old inputs could not tell
        ok = T.attn_f64(good["q"], good["kv"], good["do"], heads, d, good["scale"], arith=torch.float32, max_subtract=False)
        assert T.worst_ratio((ok[0],), (good["ref"][0],), (good["tol"]["f32"][0],))[0] < 1.0


def _factor(mut, c):
    """by how many tolerances the mutated law misses the law: the lesser of the two math modes' figures"""
    return min(T.worst_ratio(mut, c["ref"], c["tol"][m])[0] for m in T.ATTN_MATHS)


ATTN_MUTATION_CASES = {
    # (not `offset`: a padding key's logit 0 is e^-100 beside its logits; not M = 64: no padding)
    "pad_keys": [(f, *c) for f in ("unit", "sharp") for c in T.ATTN_M_EDGES[:-1]] + [("sharp", *c) for c in T.ATTN_KEYS_EDGES[:3]],
    "dkv_tail": [(f, *c) for f in ("unit", "sharp", "offset") for c in T.ATTN_N_EDGES[-5:]] + [("sharp", *c) for c in T.ATTN_KEYS_EDGES[1:3]],
    "dk_no_scale": [(f, *c) for f in ("unit", "sharp", "offset") for c in T.ATTN_M_EDGES[1::3]],          # (M > 1: one key has dS = 0)
}


@pytest.mark.parametrize("mutation", T.ATTN_MUTATIONS)
def test_attention_mutations_are_caught(mutation):
    best, n_caught, n = 0.0, 0, 0
    for d in D_ALL:
        for family, B, N, M, heads in ATTN_MUTATION_CASES[mutation]:
            c = T.attn_case(family, B, N, M, heads, d)
            f = _factor(T.attn_f64(c["q"], c["kv"], c["do"], heads, d, c["scale"], mutation=mutation), c)
            print(f"{mutation} {family} d={d} B={B} N={N} M={M} heads={heads}: {f:.3g} tolerances")
            best, n_caught, n = max(best, f), n_caught + (f >= 4.0), n + 1
    print(f"{mutation}: caught by {n_caught} of {n} cases, at best {best:.3g} tolerances")
    assert best >= 4.0


def _window_mutation_cases(mutation):
    shifted = [c for c in T.WINDOW_EDGES if c[4] > 0]
    if mutation == "mask_inf":
        return [("hot", *c) for c in T.WINDOW_HOT]
    if mutation == "hw_swap":
        return [(f, *c, d) for f in ("unit", "sharp", "hot") for c in T.WINDOW_EDGES if c[1] != c[2] for d in D_ALL]
    if mutation in ("mask_edge", "roll_sign"):
        return [(f, *c, d) for f in ("unit", "sharp", "hot") for c in shifted if c[3] > 1 for d in D_ALL]
    if mutation == "pad_keys":
        return [(f, *c, d) for f in ("unit", "sharp", "hot") for c in T.WINDOW_EDGES for d in D_ALL]
    return [(f, *c, d) for f in ("unit", "sharp") for c in T.WINDOW_EDGES if c[3] > 1 for d in D_ALL]          # the bias: a 1 x 1 window has one entry


@pytest.mark.parametrize("mutation", T.WINDOW_MUTATIONS)
def test_window_mutations_are_caught(mutation):
    best, n_caught, cases = 0.0, 0, _window_mutation_cases(mutation)
    for family, B, H, W, w, s, heads, d in cases:
        c = T.window_case(family, B, H, W, w, s, heads, d)
        mut = T.window_results(T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation=mutation))
        if mutation == "mask_inf":
            mut, ref, tol = mut[:1], c["ref"][:1], {m: c["tol"][m][:1] for m in T.ATTN_MATHS}          # the family's condition is on `out`
            f = min(T.worst_ratio(mut, ref, tol[m])[0] for m in T.ATTN_MATHS)
        else:
            f = _factor(mut, c)
        print(f"{mutation} {family} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}: {f:.3g} tolerances")
        best, n_caught = max(best, f), n_caught + (f >= 4.0)
    print(f"{mutation}: caught by {n_caught} of {len(cases)} cases, at best {best:.3g} tolerances")
    assert best >= 4.0
    if mutation == "mask_inf":
        assert n_caught == len(cases)          # the condition of the `hot` family, where it was sized


def test_mask_literal_is_invisible_to_unit_logits():
    """what the new families are for: on randn inputs -inf for -100 changes nothing at all"""
    for B, H, W, w, s, heads, d in T.WINDOW_HOT:
        c = T.window_case("unit", B, H, W, w, s, heads, d)
        mut = T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation="mask_inf")
        assert float((mut[0] - c["ref"][0]).abs().max()) == 0.0


def test_emulation_is_the_law_on_operands_bf16_holds_exactly():
    """inputs that are bf16 numbers with lo = 0 and a power-of-two scale: the split loses nothing in the first product, so the emulation's
    error is that of float32 softmax and of re-splitting P / dS (2^-17 relative) only"""
    g = torch.Generator().manual_seed(5)
    B, N, M, heads, d = 1, 40, 33, 2, 64
    q, kv, do = (torch.randn(*s, generator=g).bfloat16().float() for s in ((B, N, heads * d), (B, M, 2 * heads * d), (B, N, heads * d)))
    ref, emu = T.attn_f64(q, kv, do, heads, d, 0.125), T.attn_split_emulation(q, kv, do, heads, d, 0.125)
    for a, b in zip(emu, ref):
        assert _rel(a.double(), b) < 2.0 ** -14


# ---- dropout of the probabilities and the packed tile (the DROP kernels of csrc/attn_window.hip, all of csrc/attn_window_packed.hip) -------
P_PACKED, P_WINDOW = 0.1, 0.5
FAMILIES = ("unit", "sharp", "hot")
SINGLE_ROW = (2, 3, 3, 1, 0, 2)          # L = 1: dS = 0 and the tolerances are the helper's floor; "written and finite" on the GPU, no mutation counts it


def _windows(c):
    return (c[1] // c[3]) * (c[2] // c[3])


def _drop_list(shapes, p):
    return [(f, *c, d, p) for f in FAMILIES for c in shapes for d in D_ALL]


@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("family", ["unit", "hot"])
@pytest.mark.parametrize("B,H,W,w,s,heads,p", [(*c, P_WINDOW) for c in T.WINDOW_EDGES] + [(*c, P_PACKED) for c in T.PACKED_EDGES])
def test_dropout_law_is_autograd_of_the_reference_formula_with_the_mask(family, B, H, W, w, s, heads, p, d):
    c = T.window_drop_case(family, B, H, W, w, s, heads, d, p)
    qr, tr = c["qkv"].double().requires_grad_(True), c["table"].double().requires_grad_(True)
    o = T.window_attn_reference(qr, tr, heads, w, s, c["scale"], drop=(c["mask"], p))
    o.backward(c["do"].double())
    for name, a, b in zip(T.WINDOW_TENSORS, c["ref"], T.window_results((o.detach(), qr.grad, tr.grad))):
        assert a.shape == b.shape and _rel(a, b) < 1e-12, name
    m = c["mask"]
    assert int(m[0, 0, 0].sum()) == 0          # the forced rows: every key dropped (the law's out row is an exact 0) ...
    x = c["ref"][0].reshape(B, H, W, heads, d)[0, s % H, s % W, 0]          # ... position 0 of window 0 is the token (s, s)
    assert float(x.abs().max()) == 0.0
    assert int(m[(0, 0, w * w - 1) if w > 1 else (1, 0, 0)].sum()) == w * w          # ... and every key kept


@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("B,H,W,w,s,heads", T.PACKED_EDGES)
def test_tile_view_is_the_window_law(B, H, W, w, s, heads, d):
    """the exclusion between the windows of a tile is exact: the tile view equals the per-window law, without and with a mask"""
    for family in ("unit", "hot"):
        c, cd = T.window_case(family, B, H, W, w, s, heads, d), T.window_drop_case(family, B, H, W, w, s, heads, d, P_PACKED)
        for ref, drop in ((c["ref"], None), (cd["ref"], (cd["mask"], P_PACKED))):
            tiles = T.window_results(T.window_attn_tiles_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], drop=drop))
            for name, a, b in zip(T.WINDOW_TENSORS, tiles, ref):
                assert _rel(a, b) < 1e-12, (family, name)


def _drop_mutant(c, heads, w, s, mutation):
    return T.window_results(T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation=mutation, drop=(c["mask"], c["p"])))


@pytest.mark.parametrize("mutation", T.WINDOW_DROP_MUTATIONS)
@pytest.mark.parametrize("which", ["packed", "window"])
def test_dropout_mutations_are_caught(which, mutation):
    """f = M, dV from the undropped P, the row sum over the unmasked dP, M[l2][l1]: on PACKED_EDGES at p = 0.1 and on WINDOW_EDGES at p = 0.5"""
    cases = _drop_list(T.PACKED_EDGES, P_PACKED) if which == "packed" else _drop_list([c for c in T.WINDOW_EDGES if c != SINGLE_ROW], P_WINDOW)
    best, n_caught = 0.0, 0
    for family, B, H, W, w, s, heads, d, p in cases:
        c = T.window_drop_case(family, B, H, W, w, s, heads, d, p)
        f = _factor(_drop_mutant(c, heads, w, s, mutation), c)
        print(f"{mutation} p={p} {family} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}: {f:.3g} tolerances")
        best, n_caught = max(best, f), n_caught + (f >= 4.0)
    print(f"{mutation} ({which}, p = {cases[0][-1]}): caught by {n_caught} of {len(cases)} cases, at best {best:.3g} tolerances")
    assert best >= 4.0
    if mutation != "drop_transposed":          # (a mask may be symmetric where it matters; the three factors are wrong in every case)
        assert n_caught == len(cases)


def test_unrounded_masked_dp_is_caught_where_a_row_sits_on_one_key():
    """the mutation of the one kernel fault these cases found (helpers.WINDOW_DROP_ROUNDING): a float32 rounding error of dP .* f left in dS.
    Beside a dS of ordinary size it is rounding; at (3, 2, 2, 2, 1, 1) every other key of a row is behind the mask's -100, dS = 0 up to
    e^-100, and the unit and sharp families there must catch it at both head dims"""
    best, n_caught, n = 0.0, 0, 0
    for p in (0.1, P_WINDOW):
        for family, B, H, W, w, s, heads, d, _ in _drop_list([c for c in T.WINDOW_EDGES if c != SINGLE_ROW], p):
            c = T.window_drop_case(family, B, H, W, w, s, heads, d, p)
            f = _factor(_drop_mutant(c, heads, w, s, T.WINDOW_DROP_ROUNDING), c)
            print(f"{T.WINDOW_DROP_ROUNDING} p={p} {family} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}: {f:.3g} tolerances")
            best, n_caught, n = max(best, f), n_caught + (f >= 4.0), n + 1
            if (B, H, W, w, s, heads) == (3, 2, 2, 2, 1, 1) and family != "hot":          # (hot: logits of tens reach over the -100, dS is not 0)
                assert f >= 4.0, (family, d, p, f)
    print(f"{T.WINDOW_DROP_ROUNDING}: caught by {n_caught} of {n} cases, at best {best:.3g} tolerances")
    assert best >= 4.0


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("mutation", T.PACKED_MUTATIONS)
def test_packed_mutations_are_caught(mutation, drop):
    """tile_leak: every case whose image has more than one window; drop_slot_index: every case whose image has more than one tile"""
    if mutation == "drop_slot_index" and not drop:
        return          # (no mask, nothing to index)
    best, n_caught, n_must, cases = 0.0, 0, 0, [(f, *c, d) for f in FAMILIES for c in T.PACKED_EDGES for d in D_ALL]
    for family, B, H, W, w, s, heads, d in cases:
        c = T.window_drop_case(family, B, H, W, w, s, heads, d, P_PACKED) if drop else T.window_case(family, B, H, W, w, s, heads, d)
        dr = (c["mask"], P_PACKED) if drop else None
        f = _factor(T.window_results(T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation=mutation, drop=dr)), c)
        print(f"{mutation} drop={drop} {family} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}: {f:.3g} tolerances")
        best, n_caught = max(best, f), n_caught + (f >= 4.0)
        nW = _windows((B, H, W, w))
        if nW > (1 if mutation == "tile_leak" else T.ATTN_IMAGE_KEYS // (w * w)):
            n_must += 1
            assert f >= 4.0, (mutation, family, B, H, W, w, s, heads, d, f)
        elif mutation == "tile_leak":
            assert f < 1e-9          # one window: nothing to leak (the float64 sums in another order)
    print(f"{mutation} (dropout mask: {drop}): caught by {n_caught} of {len(cases)} cases ({n_must} have more than one "
          f"{'window' if mutation == 'tile_leak' else 'tile'}), at best {best:.3g} tolerances")
    assert best >= 4.0 and n_caught >= n_must > 0


def test_packed_mask_literal_needs_the_hot_family():
    """the packed kernel writes NEG for another window's keys before the maximum, beside the shift mask's literal -100: on unit logits -inf
    for -100 moves nothing, on the hot family `out` moves by hundreds of tolerances at every shifted packed shape"""
    least = float("inf")
    for B, H, W, w, s, heads in T.PACKED_EDGES:
        if not s:
            continue
        for d in D_ALL:
            c = T.window_case("unit", B, H, W, w, s, heads, d)
            mut = T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation="mask_inf")
            assert float((mut[0] - c["ref"][0]).abs().max()) == 0.0
            c = T.window_case("hot", B, H, W, w, s, heads, d)
            mut = T.window_attn_f64(c["qkv"], c["table"], c["do"], heads, w, s, c["scale"], mutation="mask_inf")
            f = min(T.worst_ratio(mut[:1], c["ref"][:1], c["tol"][m][:1])[0] for m in T.ATTN_MATHS)
            print(f"mask_inf hot d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}: out moves by {f:.3g} tolerances")
            least = min(least, f)
    assert least >= 4.0


@pytest.mark.parametrize("d", D_ALL)
def test_the_rule_is_no_looser_than_the_hand_bounds(d):
    """The packed and dropout GPU files so far hold the kernels to hand constants (helpers.window_hand_bounds).  Per tensor, hand bound /
    rule's tolerance on PACKED_EDGES (unit, bf16x3), without and with the mask: the hand bound is never the tighter one by more than 2 x,
    so holding the kernels to the rule weakens nothing -- and is up to tens of times tighter for the gradients."""
    for p in (0.0, P_PACKED):
        lo, hi = [float("inf")] * 5, [0.0] * 5
        for B, H, W, w, s, heads in T.PACKED_EDGES:
            c = T.window_drop_case("unit", B, H, W, w, s, heads, d, p) if p else T.window_case("unit", B, H, W, w, s, heads, d)
            r = [h / t for h, t in zip(T.window_hand_bounds(B, H, W, w, d, "bf16x3", p), c["tol"]["bf16x3"])]
            print(f"d={d} p={p} B={B} H={H} W={W} w={w} s={s} heads={heads}: hand bound / tolerance  " +
                  "  ".join(f"{n} {x:.2f}" for n, x in zip(T.WINDOW_TENSORS, r)))
            lo, hi = [min(a, x) for a, x in zip(lo, r)], [max(a, x) for a, x in zip(hi, r)]
        print(f"d={d} p={p}: " + "  ".join(f"{n} {a:.2f} .. {b:.2f}" for n, a, b in zip(T.WINDOW_TENSORS, lo, hi)))
        assert min(lo) >= 0.5, lo
