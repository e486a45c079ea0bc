"""GPU parity of the fused loss at 5..16 classes (csrc/loss.hip; 104-float sums rows) against the oracle, CPU autograd and the
reference's own nine-class outputs (tests/golden/losses_c9.npz, tools/make_golden_multiclass.py).  Bounds are those of
tests/test_gpu_loss.py: 1e-5 on loss values, 1e-6 on the MSE, 1e-7 + 1e-4 * max|ref| on gradients.

Shapes: 24 x 24 = 576 and 40 x 28 = 1120 pixels per image are no multiples of the 1024-pixel block of the partial-sum kernel, so blocks
straddle image boundaries and, at (3, 1, 24, 24), the boundary between the two label groups; n_lab == N leaves group 1 empty.  Labels
carry the ignore value 255, one id >= C (matches no class, no cross-entropy: the kernels' rule for C <= 4 as well) and one class that
never occurs."""
import numpy as np
import pytest
import torch

from hpfg_amd.utils import DiceLoss, Med_Sup_Loss, seg_loss
from oracle import losses_ref
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = [0.5, 0.5, 0.2, 0.7, 0.3]
SHAPES = [(3, 1, 24, 24), (2, 2, 40, 28)]


def _coef(v):
    return torch.tensor(list(v) + [0.0] * (8 - len(v)), dtype=torch.float32, device=DEV)


def _ce(logits, lab, C_):
    """Cross-entropy with ids >= C excluded like the ignore value (torch refuses such targets; the kernels count them in no term of CE)."""
    return losses_ref.cross_entropy(logits, torch.where(lab >= C_, torch.full_like(lab, 255), lab))


def _sup(logits, lab, C_, kce, kdice):
    return kce * _ce(logits, lab, C_) + kdice * losses_ref.dice_loss(torch.softmax(logits, 1), lab)


_INPUTS = {}


def _inputs(C_, shape):
    """Seeded inputs of one case, built once: logits, teacher logits, labels of both groups, a 0/1 consistency mask."""
    if (C_, shape) not in _INPUTS:
        N, nl, H, W = shape
        g = torch.Generator().manual_seed(100 * C_ + N)
        logits = 2.0 * torch.randn(N, C_, H, W, generator=g)
        tl = 2.0 * torch.randn(N, C_, H, W, generator=g)
        lab = torch.randint(0, C_ - 1, (N, H, W), generator=g)          # class C-1 never occurs
        lab[0, 0, :5] = 255
        lab[0, 3, 2:9] = C_ + 1                                         # an id >= C that is not the ignore value
        lab[N - 1, H - 1, W - 4:] = 255
        lab[N - 1, 1, 1] = C_
        mask = (torch.rand(N - nl, 1, H, W, generator=g) < 0.6).float()
        assert 255 in lab and (C_ - 1) not in lab and int(((lab >= C_) & (lab != 255)).sum()) > 0
        _INPUTS[(C_, shape)] = (logits, tl, lab[:nl].contiguous(), lab[nl:].contiguous(), mask)
    return _INPUTS[(C_, shape)]


def _check(out, ref, lg, lr, scale=1.0):
    assert abs(float(out[0].detach()) - float(ref.detach())) < 1e-5, (float(out[0].detach()), float(ref.detach()))
    (out[0] * scale).backward()
    ref.backward()
    gref = scale * lr.grad
    err = maxerr(lg.grad.cpu(), gref)
    assert err < 1e-7 + 1e-4 * float(gref.abs().max()), (err, float(gref.abs().max()))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C_", [5, 8, 9, 16])
def test_wide_loss_modes_match_oracle_and_autograd(C_, shape):
    N, nl, H, W = shape
    logits, tl, lab, pseudo, mask = _inputs(C_, shape)
    two = nl < N

    def fresh():
        return logits.clone().requires_grad_(True), logits.to(DEV).requires_grad_(True)

    # two label groups + teacher logits (indexed like the batch)
    lr, lg = fresh()
    ref = _sup(lr[:nl], lab, C_, K[0], K[1])
    if two:
        mse = losses_ref.mse_consistency(torch.softmax(lr[nl:], 1), torch.softmax(tl[nl:], 1))
        ref = ref + _sup(lr[nl:], pseudo, C_, K[2], K[3]) + K[4] * mse
    out = seg_loss(lg, lab.to(DEV), nl, coef=_coef(K), pseudo=pseudo.to(DEV) if two else None, teacher_logits=tl.to(DEV))
    parts = out.detach().cpu()
    assert abs(float(parts[1]) - float(_ce(logits[:nl], lab, C_))) < 1e-5
    assert abs(float(parts[2]) - float(losses_ref.dice_loss(torch.softmax(logits[:nl], 1), lab))) < 1e-5
    if two:
        assert abs(float(parts[3]) - float(_ce(logits[nl:], pseudo, C_))) < 1e-5
        assert abs(float(parts[4]) - float(losses_ref.dice_loss(torch.softmax(logits[nl:], 1), pseudo))) < 1e-5
        assert abs(float(parts[5]) - float(mse.detach())) < 1e-6
    else:
        assert float(parts[3]) == 0.0 and float(parts[4]) == 0.0 and float(parts[5]) == 0.0
    _check(out, ref, lg, lr, scale=2.0)

    # teacher probabilities for the unlabelled images only (ICT's target), no pseudo-labels
    if two:
        tp = torch.softmax(tl[nl:], 1)
        lr, lg = fresh()
        mse = losses_ref.mse_consistency(torch.softmax(lr[nl:], 1), tp)
        ref = _sup(lr[:nl], lab, C_, 0.5, 0.5) + 0.3 * mse
        out = seg_loss(lg, lab.to(DEV), nl, coef=_coef([0.5, 0.5, 0.0, 0.0, 0.3]), teacher_prob=tp.to(DEV))
        assert abs(float(out[5].detach()) - float(mse.detach())) < 1e-6
        _check(out, ref, lg, lr)

        # masked consistency (UAMT's form) on teacher logits of the unlabelled images
        lr, lg = fresh()
        d2 = (torch.softmax(lr[nl:], 1) - torch.softmax(tl[nl:], 1)) ** 2
        cons = (mask * d2).sum() / (2 * mask.sum() + 1e-16)
        ref = _sup(lr[:nl], lab, C_, 0.5, 0.5) + 0.7 * cons
        out = seg_loss(lg, lab.to(DEV), nl, coef=_coef([0.5, 0.5, 0.0, 0.0, 0.7]), teacher_logits=tl[nl:].to(DEV), cons_mask=mask.to(DEV))
        assert abs(float(out[5].detach()) - float(cons.detach())) < 1e-6
        _check(out, ref, lg, lr)

    # probability input: DiceLoss(softmax=False) through torch.softmax autograd, labels of the whole batch
    all_lab = torch.cat([lab, pseudo])
    lr, lg = fresh()
    ref = losses_ref.dice_loss(torch.softmax(lr, 1), all_lab)
    got = DiceLoss(C_)(torch.softmax(lg, 1), all_lab.unsqueeze(1).to(DEV))
    assert abs(float(got.detach()) - float(ref.detach())) < 1e-5
    got.backward()
    ref.backward()
    assert maxerr(lg.grad.cpu(), lr.grad) < 1e-7 + 1e-4 * float(lr.grad.abs().max())
    # and Med_Sup_Loss / DiceLoss(softmax=True), the module surface
    assert abs(float(Med_Sup_Loss(C_)(logits.to(DEV), all_lab.to(DEV))) - float(_sup(logits, all_lab, C_, 0.5, 0.5))) < 1e-5
    assert abs(float(DiceLoss(C_)(logits.to(DEV), all_lab.unsqueeze(1).to(DEV), softmax=True)) - float(ref.detach())) < 1e-5


def test_reference_fixture_nine_classes(golden_dir):
    d = np.load(f"{golden_dir}/losses_c9.npz")
    logits = torch.from_numpy(d["logits"]).to(DEV)
    lab = torch.from_numpy(d["labels"]).to(DEV)
    tp = torch.from_numpy(d["t_prob"]).to(DEV)
    p = torch.softmax(logits, 1)
    assert abs(float(DiceLoss(9)(p, lab.unsqueeze(1))) - float(d["dice"])) < 1e-5
    assert abs(float(DiceLoss(9)(logits, lab.unsqueeze(1), softmax=True)) - float(d["dice"])) < 1e-5
    assert abs(float(Med_Sup_Loss(9)(logits, lab)) - float(d["med"])) < 1e-5
    out = seg_loss(logits, lab, 3, coef=_coef([1.0, 0.0]))
    assert abs(float(out[1]) - float(d["ce"])) < 1e-5
    out = seg_loss(logits, lab[:1], 1, coef=_coef([1.0, 0.0, 0.0, 0.0, 1.0]), teacher_prob=tp)
    assert abs(float(out[5]) - float(d["mse"])) < 1e-6
    lg = logits.clone().requires_grad_(True)
    tot = seg_loss(lg, lab[:1], 1, coef=_coef([0.5, 0.5, 0.0, 0.0, 0.3]), teacher_prob=tp)[0]
    assert abs(float(tot.detach()) - float(d["comp"])) < 1e-5
    tot.backward()
    ref = torch.from_numpy(d["comp_dlogits"])
    assert maxerr(lg.grad.cpu(), ref) < 1e-7 + 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("C_", [7, 9, 13, 16])
def test_two_calls_are_bit_identical(C_):
    logits, tl, lab, pseudo, _ = _inputs(C_, SHAPES[0])
    res = []
    for _ in range(2):
        lg = logits.to(DEV).requires_grad_(True)
        out = seg_loss(lg, lab.to(DEV), 1, coef=_coef(K), pseudo=pseudo.to(DEV), teacher_logits=tl.to(DEV))
        out[0].backward()
        res.append((out.detach().cpu(), lg.grad.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_seventeen_classes_raise_value_error():
    logits = torch.zeros(1, 17, 8, 8, device=DEV)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="16"):
        seg_loss(logits, lab, 1, coef=_coef([0.5, 0.5]))
    with pytest.raises(ValueError, match="16"):
        Med_Sup_Loss(17)(logits, lab)


def test_four_classes_unchanged(golden_dir):
    """C = 4: the composite of tests/test_gpu_loss.py on the reference fixture, value and gradient."""
    d = np.load(f"{golden_dir}/losses.npz")
    logits = torch.from_numpy(d["logits"]).to(DEV)
    tl = torch.from_numpy(d["t_logits"]).to(DEV)
    lab = torch.from_numpy(d["labels"]).to(DEV)
    lg = logits.clone().requires_grad_(True)
    tot = seg_loss(lg, lab[:1], 1, coef=_coef([0.5, 0.5, 0.0, 0.0, 0.3]), teacher_logits=tl)[0]
    assert abs(float(tot.detach()) - float(d["comp"])) < 1e-5
    tot.backward()
    ref = torch.from_numpy(d["comp_dlogits"])
    assert maxerr(lg.grad.cpu(), ref) < 1e-6 + 1e-4 * float(ref.abs().max())
    assert abs(float(Med_Sup_Loss(4)(logits, lab)) - float(d["med"])) < 1e-5
