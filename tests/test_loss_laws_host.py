"""CPU: the float64 law of the fused loss (helpers.loss_f64) and of UAMT's entropy (helpers.uncertainty_f64), which
tests/test_gpu_loss_edges.py holds the kernels of csrc/loss.hip and csrc/misc.hip against, checked on a machine without a GPU:
  - against independent float64 restatements: oracle.losses_ref on double inputs, F.cross_entropy(ignore_index=255) and torch autograd of
    their sum, and the reference's own stored outputs (tests/golden/losses.npz, losses_c9.npz);
  - the layout of `sums` against hpfg_loss_nsum and the constants of include/hpfg_hip.h;
  - the tolerance rule (helpers.bound_8x: 8 x the error of the float32 restatement) against five named mistakes: each must miss the law by
    at least 4 x the tolerance wherever the term it changes is active, so that the GPU test cannot pass a kernel that makes one of them."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses_ref
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11          # float64 law against float64 torch: sums of a few thousand O(1) terms
MUT_CLASSES = (2, 3, 6, 7, 13, 16)


def _close(a, b, what, tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err = float((a - b).abs().max())
    assert a.shape == b.shape and err <= tol * max(1.0, float(b.abs().max())), (what, err)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _ce(logits_nchw, lab, C_):
    """ids in [C, 255) count in no term of the cross-entropy: torch refuses them, so they take the ignore value"""
    lab = lab.long()
    return losses_ref.cross_entropy(logits_nchw, torch.where(lab >= C_, torch.full_like(lab, 255), lab))


@pytest.mark.parametrize("shape", H.LOSS_SHAPES)
@pytest.mark.parametrize("C_", [2, 4, 7, 16])
def test_law_matches_oracle_terms_and_autograd(C_, shape):
    N, nl, Hh, W = shape
    c = H.loss_case(C_, *shape)
    K = H.LOSS_K
    x = _nchw(c["logits"].double()).requires_grad_(True)
    tq = torch.softmax(_nchw(c["t_logits"].double()), 1)
    p = torch.softmax(x, 1)
    terms = [_ce(x[:nl], c["labels0"], C_), losses_ref.dice_loss(p[:nl], c["labels0"].long())]
    if nl < N:
        terms += [_ce(x[nl:], c["labels1"], C_), losses_ref.dice_loss(p[nl:], c["labels1"].long()), losses_ref.mse_consistency(p[nl:], tq[nl:])]
    else:
        terms += [torch.zeros((), dtype=torch.float64)] * 3
    total = sum(f * t for f, t in zip((H.f32_exact(v) for v in K), terms))
    total.backward()
    sums, out, dl = H.loss_f64(**H.loss_mode_kwargs(c, "teacher_logits", K), grad_scale=0.5)
    _close(out[0], total.detach(), "total")
    _close(out[1:6], torch.stack([t.detach() for t in terms]), "terms")
    assert float(out[6]) == 0.0 and float(out[7]) == 0.0
    _close(_nchw(dl), 0.5 * x.grad, "dlogits")
    # sums: the oracle's I, Z, Y per group, and F.cross_entropy's sum and count
    S = H.loss_stride(C_)
    for g, (lab, sl) in enumerate(((c["labels0"], slice(0, nl)), (c["labels1"], slice(nl, N)))):
        base = H.LOSS_OFF + g * 3 * S
        if sl.stop == sl.start:
            assert float(sums[2 * g:2 * g + 2].abs().max()) == 0.0 and float(sums[base:base + 3 * S].abs().max()) == 0.0
            continue
        i, z, y = losses_ref.dice_sums(p[sl].detach(), lab.long())
        for k, v in enumerate((i, z, y)):
            _close(sums[base + k * S:base + k * S + C_], v, "IZY"[k])
            assert float(sums[base + k * S + C_:base + (k + 1) * S].abs().sum()) == 0.0
        lab_ = torch.where(lab.long() >= C_, 255, lab.long())
        _close(sums[2 * g], F.cross_entropy(x[sl].detach(), lab_, ignore_index=255, reduction="sum"), "nll")
        assert float(sums[2 * g + 1]) == float((lab_ != 255).sum())
    assert float(sums[6]) == 0.0 and float(sums[7]) == 0.0
    if nl < N:
        _close(sums[4], ((p[nl:].detach() - tq[nl:]) ** 2).sum(), "mse sum")
        assert float(sums[5]) == (N - nl) * Hh * W


@pytest.mark.parametrize("C_", [3, 9])
def test_law_modes_match_plain_torch(C_):
    """Teacher probabilities of the unlabelled images, the masked form, world = 2, and probabilities in: against plain torch float64."""
    shape = H.LOSS_SHAPES[0]
    N, nl, Hh, W = shape
    c = H.loss_case(C_, *shape)
    K = H.LOSS_K_DEAD
    k = [H.f32_exact(v) for v in K]

    def sup(x):
        return k[0] * _ce(x[:nl], c["labels0"], C_) + k[1] * losses_ref.dice_loss(torch.softmax(x[:nl], 1), c["labels0"].long())

    for mode, world in (("teacher_prob_unlab", 1), ("teacher_prob_unlab", 2), ("masked", 1)):
        x = _nchw(c["logits"].double()).requires_grad_(True)
        kw = H.loss_mode_kwargs(c, mode, K)
        # (teacher probabilities: the float32 values the kernel is handed, not their float64 recomputation)
        tq = _nchw(kw["t"].double()) if mode == "teacher_prob_unlab" else torch.softmax(_nchw(c["t_logits"].double()), 1)[nl:]
        d2 = (torch.softmax(x[nl:], 1) - tq) ** 2
        if mode == "masked":
            m = c["mask"].double().unsqueeze(1)
            cons = (m * d2).sum() / (2 * m.sum() + 1e-16)
        else:
            cons = d2.mean() / world
        total = sup(x) + k[4] * cons
        total.backward()
        _, out, dl = H.loss_f64(**kw, world=world)
        _close(out[0], total.detach(), mode), _close(out[5], cons.detach(), mode), _close(_nchw(dl), x.grad, mode)
    # probabilities in: the gradient with respect to them; the softmax's own autograd in front gives that of the logits
    kw = H.loss_mode_kwargs(c, "prob_input", H.LOSS_K)
    x = _nchw(c["logits"].double()).requires_grad_(True)
    pr = torch.softmax(x, 1)
    pr.retain_grad()
    lab = torch.cat([c["labels0"], c["labels1"]]).long()
    total = H.f32_exact(H.LOSS_K[1]) * losses_ref.dice_loss(pr[:nl], lab[:nl]) + H.f32_exact(H.LOSS_K[3]) * losses_ref.dice_loss(pr[nl:], lab[nl:])
    total.backward()
    _, out, dl = H.loss_f64(**dict(kw, logits=torch.softmax(c["logits"].double(), -1)))
    _close(out[0], total.detach(), "prob total"), _close(_nchw(dl), pr.grad, "prob grad")


def test_law_degenerate_groups():
    """A group whose pixels are all ignored: CE 0 where torch's mean is NaN, Dice with I = Y = 0; an all-zero mask: MSE 0, no gradient."""
    c = H.loss_case(6, 3, 1, 24, 24)
    kw = H.loss_mode_kwargs(c, "masked", H.LOSS_K)
    kw["labels0"] = torch.full_like(c["labels0"], 255)
    kw["cons_mask"] = torch.zeros_like(c["mask"])
    sums, out, dl = H.loss_f64(**kw)
    assert float(out[1]) == 0.0 and float(out[5]) == 0.0 and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(out).all())
    assert bool(torch.isnan(F.cross_entropy(_nchw(c["logits"].double())[:1], kw["labels0"].long(), ignore_index=255)))
    _close(out[2], losses_ref.dice_loss(torch.softmax(_nchw(c["logits"].double())[:1], 1), kw["labels0"].long()), "dice0")
    _, _, dl_sup = H.loss_f64(**H.loss_mode_kwargs(dict(c, labels0=kw["labels0"]), "no_teacher", H.LOSS_K))
    assert torch.equal(dl, dl_sup)


def test_law_matches_stored_reference_outputs(golden_dir):
    """The reference's own float32 results: within the error of a float32 evaluation (bound_8x of the law at float32)."""
    for name, C_, key in (("losses", 4, "t_logits"), ("losses_c9", 9, "t_prob")):
        d = np.load(os.path.join(golden_dir, name + ".npz"))
        logits = torch.from_numpy(d["logits"]).permute(0, 2, 3, 1).contiguous()
        lab = torch.from_numpy(d["labels"]).to(torch.uint8)
        t = torch.from_numpy(d[key]).permute(0, 2, 3, 1).contiguous()
        both = lambda **kw: (H.loss_f64(**kw), H.loss_f64(**kw, dtype=torch.float32))

        def scalar(v64, v32, want, what):
            bound = H.bound_8x(v64.reshape(1), v32.reshape(1))
            assert abs(float(v64) - float(want)) <= bound, (name, what, float(v64), float(want), bound)

        (_, o64, _), (_, o32, _) = both(logits=logits, labels0=lab, labels1=None, n_lab=3, coef=(0.5, 0.5, 0, 0, 0))
        scalar(o64[0], o32[0], d["med"], "med"), scalar(o64[1], o32[1], d["ce"], "ce"), scalar(o64[2], o32[2], d["dice"], "dice")
        if C_ == 4:          # losses.npz: teacher logits of the whole batch, the MSE over all three images
            (_, o64, _), (_, o32, _) = both(logits=logits, labels0=None, labels1=None, n_lab=0, coef=(0, 0, 0, 0, 1.0), t=t)
            kw = dict(logits=logits, labels0=lab[:1], labels1=None, n_lab=1, coef=(0.5, 0.5, 0, 0, 0.3), t=t)
        else:                # losses_c9.npz: teacher probabilities of the two unlabelled images
            kw = dict(logits=logits, labels0=lab[:1], labels1=None, n_lab=1, coef=(0.5, 0.5, 0, 0, 0.3), t=t, teacher_is_prob=True, t_unlab_only=True)
            (_, o64, _), (_, o32, _) = both(**dict(kw, coef=(0, 0, 0, 0, 1.0)))
        scalar(o64[5], o32[5], d["mse"], "mse")
        (_, o64, g64), (_, o32, g32) = both(**kw)
        scalar(o64[0], o32[0], d["comp"], "comp")
        want = torch.from_numpy(d["comp_dlogits"]).permute(0, 2, 3, 1).double()
        assert float((g64 - want).abs().max()) <= H.bound_8x(g64, g32), (name, "comp_dlogits")


def test_sums_layout_matches_the_library():
    for C_ in range(2, 17):
        g = H.loss_sum_groups(C_)
        idx = sorted(i for v in g.values() for i in v)
        assert idx == [i for i in range(H.loss_nsum(C_)) if i not in (6, 7)] and set(g) == set(H.LOSS_SUM_GROUPS)
    hdr = open(os.path.join(ROOT, "include", "hpfg_hip.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define\s+(HPFG_LOSS_NSUM(?:_WIDE)?)\s+(\d+)", hdr)}
    assert const == {"HPFG_LOSS_NSUM": H.loss_nsum(4), "HPFG_LOSS_NSUM_WIDE": H.loss_nsum(5)} and H.loss_nsum(16) == H.loss_nsum(5)
    try:
        from hpfg_amd import _lib as L
        lib = L.load()
    except Exception:          # no library on this machine: the header's constants above are the check
        return
    assert [lib.hpfg_loss_nsum(C_) for C_ in range(2, 17)] == [H.loss_nsum(C_) for C_ in range(2, 17)]
    assert L.LOSS_NSUM == H.loss_nsum(4)


@pytest.mark.parametrize("shape", H.LOSS_SHAPES)
@pytest.mark.parametrize("C_", MUT_CLASSES)
def test_tolerance_tells_every_mutation_from_rounding(C_, shape):
    c = H.loss_case(C_, *shape)
    seen = set()
    for K in (H.LOSS_K, H.LOSS_K_DEAD):
        for mode in H.LOSS_MODES:
            kw = H.loss_mode_kwargs(c, mode, K)
            s64, o64, g64 = H.loss_f64(**kw)
            s32, o32, g32 = H.loss_f64(**kw, dtype=torch.float32)
            groups = H.loss_sum_groups(C_)
            for m in H.LOSS_MUTATIONS:
                if not H.loss_mutation_active(m, kw):
                    continue
                seen.add(m)
                sm, om, gm = H.loss_f64(**kw, mutation=m)
                ratios = [abs(float(om[0] - o64[0])) / H.bound_8x(o64[:1], o32[:1]), float((gm - g64).abs().max()) / H.bound_8x(g64, g32)]
                ratios += [float((sm[i] - s64[i]).abs().max()) / H.bound_8x(s64[i], s32[i]) for i in groups.values()]
                print(f"  C={C_} {shape} K1={K[2]} {mode:<20s} {m:<26s} total {ratios[0]:10.1f}  dlogits {ratios[1]:10.1f}  sums {max(ratios[2:]):10.1f}")
                assert max(ratios) >= 4.0, (C_, shape, K, mode, m, ratios)
    assert {"ce_over_all_pixels", "z_skips_ignored", "dice_mean_over_c_minus_1"} <= seen
    if shape[1] < shape[0]:
        assert seen == set(H.LOSS_MUTATIONS)


def test_mutation_activity_rule():
    """A mutation counted as inactive changes nothing: the rule that lets the test above skip a case is itself held to the law."""
    c = H.loss_case(6, *H.LOSS_SHAPES[0])
    for K in (H.LOSS_K, H.LOSS_K_DEAD):
        for mode in H.LOSS_MODES:
            kw = H.loss_mode_kwargs(c, mode, K)
            ref = H.loss_f64(**kw)
            for m in H.LOSS_MUTATIONS:
                if not H.loss_mutation_active(m, kw):
                    got = H.loss_f64(**kw, mutation=m)
                    assert float(got[1][0]) == float(ref[1][0]) and torch.equal(got[2], ref[2]), (mode, m)


@pytest.mark.parametrize("C_", range(1, 9))
def test_uncertainty_law_and_threshold_gap(C_):
    T = 8
    preds = H.uncertainty_case(C_)
    u64 = H.uncertainty_f64(preds, T)
    x = preds.double().permute(0, 3, 1, 2)          # the expression of tests/test_gpu_steps.py, NCHW
    pm = torch.softmax(x, 1).reshape(T, -1, *x.shape[1:]).mean(0)
    _close(u64, -(pm * torch.log(pm + 1e-6)).sum(1), "u")
    bound = H.bound_8x(u64, H.uncertainty_f64(preds, T, torch.float32))
    thr, gap = H.uncertainty_threshold(u64)
    if C_ == 1:          # one class: p = 1 at every pixel, u is the constant -log(1 + 1e-6) and no threshold can split the pixels
        assert gap == 0.0 and float((u64 + np.log1p(1e-6)).abs().max()) < 1e-15
        return
    assert gap >= 100.0 * bound, (C_, gap, bound)
    frac = float((u64 < thr).double().mean())
    assert 0.25 <= frac <= 0.75
