"""GPU parity of the whole U-Net at 5, 9 and 16 classes (decoder.out_conv beyond four output channels, the fused loss on 104-float sums rows): every
parameter gradient against the CPU oracle under the ensemble control of tests/test_gpu_unet.py::test_backward_all_parameter_gradients,
and the eval-mode logits within 1e-3."""
import numpy as np
import pytest
import torch

from hpfg_amd.datasets.synthetic import synth_batch
from hpfg_amd.model import UNet, reset_dropout_streams
from hpfg_amd.utils import Med_Sup_Loss
from oracle import losses_ref, steps_ref, unet_ref
from tests import trace_replay as R
from tests.helpers import engine_masks, maxerr, state_from_module

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = [(2, 32, 1, 5), (2, 32, 1, 9), (2, 32, 1, 16)]          # (n, hw, in_ch, ncls)


def _engine(m):
    return next(iter(m._engines.values()))[0]


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
@pytest.mark.parametrize("n,hw,in_ch,ncls", CASES)
def test_backward_all_parameter_gradients_multiclass(n, hw, in_ch, ncls, math):
    seed = 40 + ncls
    reset_dropout_streams()
    torch.manual_seed(seed)
    m = UNet(in_ch, ncls).to(DEV)
    m.math = math
    m.train()
    st = state_from_module(m)
    x, lab = synth_batch(100 + seed, n, hw, hw, in_ch, ncls, cell=8)
    out = m(x.to(DEV))
    loss = Med_Sup_Loss(ncls)(out, lab.to(DEV))
    loss.backward()
    masks = engine_masks(_engine(m), m._seed_counter, n, hw, hw)
    names = steps_ref._train_state(st)
    ro = unet_ref.unet_forward(st, x, True, masks)
    rl = losses_ref.med_sup_loss(ro, lab.long())
    rg = steps_ref._grads(rl, st, names)
    assert maxerr(out.detach().cpu(), ro.detach()) < 1e-3
    assert abs(float(loss) - float(rl)) < 1e-4
    # the same control as at <= 4 classes: the device's gradients within 1e-3 + 2x the spread of the oracle ensemble in this math mode
    st0 = {k: v.detach().clone() for k, v in st.items()}
    nominal, ens = R.grad_ensemble(st0, x, lab, masks, math, ncls_loss=ncls)
    live = [k for k in rg if float(rg[k].double().norm()) > 1e-6]
    got = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        got[k] = p.grad.cpu()
    err = {k: R.rel_l2(got[k], rg[k]) for k in live}
    runs = [[R.rel_l2(e[k], rg[k]) for k in live] for e in ens + [nominal]]
    ctl_max, ctl_med = max(max(r) for r in runs), max(float(np.median(r)) for r in runs)
    e_max, e_med = max(err.values()), float(np.median(list(err.values())))
    print(f"ncls {ncls} {math}: grad rel-L2 max {e_max:.3e} (control {ctl_max:.3e}) median {e_med:.3e} (control {ctl_med:.3e})")
    assert e_max < 1e-3 + 2.0 * ctl_max and e_med < 1e-3 + 2.0 * ctl_med, (e_max, ctl_max, e_med, ctl_med, max(err, key=err.get))


@pytest.mark.parametrize("n,hw,in_ch,ncls", CASES)
def test_forward_eval_matches_oracle_multiclass(n, hw, in_ch, ncls):
    torch.manual_seed(40 + ncls)
    m = UNet(in_ch, ncls).to(DEV)
    x, _ = synth_batch(7, n, hw, hw, in_ch, ncls, cell=8)
    m.train()
    with torch.no_grad():
        m(x.to(DEV))            # move the running statistics away from their initial values
    st = state_from_module(m)
    m.eval()
    with torch.no_grad():
        out = m(x.to(DEV))
        ref = unet_ref.unet_forward(st, x, train=False)
    assert out.shape[1] == ncls
    assert maxerr(out.cpu(), ref) < 1e-3
