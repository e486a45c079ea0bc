"""Writes the nine-class fixtures (the reference's Synapse configs: num_classes 9) from the reference's own modules, loaded by path -- arrays only:

  tests/golden/losses_c9.npz      logits [3,9,24,24], labels with ignore rows and all nine ids, teacher probabilities for the two unlabelled
                                  images; the reference's DiceLoss(9), Med_Sup_Loss(9), CE and MSE values and d(composite)/d(logits) from autograd
  tests/golden/trace_sup_c9.npz   four supervised iterations of UNet(1, 9) on 2 images of 32 x 32 (cosine schedule, weight decay 5e-4, as
                                  config/unet_30k_224x224_Synapse.yaml): dropout masks bit-packed, losses, final eval logits
  tests/golden/trace_ict_c9.npz   three ICT iterations of UNet(1, 9) on 2 + 4 images of 32 x 32 (consistency 0.1, ict_alpha 0.2, medical
                                  schedule, weight decay 1e-4, as config/ict-medseg_unet_30k_224x224_Synapse.yaml)

Every value is asserted against the oracle (oracle/losses_ref.py, unet_ref.py, steps_ref.py) before it is written.
Run in the build container, from the repository root:  python -m tools.make_golden_multiclass
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import laws_ref, losses_ref, steps_ref, unet_ref      # noqa: E402
from oracle.make_golden import close, load_reference, pack, synth_batch      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NCLS = 9


def losses_fixture(R):
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(3, NCLS, 24, 24, generator=g)
    lab = torch.randint(0, NCLS, (3, 24, 24), generator=g)
    lab[0, :2] = 255
    lab[2, 5:7, 3:20] = 255
    assert set(range(NCLS)) <= set(lab.unique().tolist())
    t_prob = torch.softmax(2.0 * torch.randn(2, NCLS, 24, 24, generator=g), 1)
    p = torch.softmax(logits, 1)
    v_dice = R.dice.DiceLoss(NCLS)(p, lab.unsqueeze(1))
    v_med = R.med.Med_Sup_Loss(NCLS)(logits, lab)
    v_ce = torch.nn.CrossEntropyLoss(ignore_index=255)(logits, lab)
    v_mse = torch.mean((p[1:] - t_prob) ** 2)
    close(v_dice, losses_ref.dice_loss(p, lab.unsqueeze(1)), 1e-6, "dice")
    close(v_med, losses_ref.med_sup_loss(logits, lab), 1e-6, "med")
    close(v_ce, losses_ref.cross_entropy(logits, lab), 1e-6, "ce")
    close(v_mse, losses_ref.mse_consistency(p[1:], t_prob), 1e-7, "mse")
    # composite: Med_Sup_Loss on image 0 + 0.3 * MSE against the teacher probabilities on images 1..2, and its gradient
    lg = logits.clone().requires_grad_(True)
    comp = R.med.Med_Sup_Loss(NCLS)(lg[:1], lab[:1]) + 0.3 * torch.mean((torch.softmax(lg[1:], 1) - t_prob) ** 2)
    comp.backward()
    lo = logits.clone().requires_grad_(True)
    comp_o = losses_ref.med_sup_loss(lo[:1], lab[:1]) + 0.3 * losses_ref.mse_consistency(torch.softmax(lo[1:], 1), t_prob)
    comp_o.backward()
    close(comp, comp_o, 1e-6, "composite")
    close(lg.grad, lo.grad, 1e-8, "composite gradient")
    np.savez_compressed(os.path.join(OUT, "losses_c9.npz"), logits=logits.numpy(), labels=lab.numpy().astype(np.int64), t_prob=t_prob.numpy(),
                        dice=np.float64(v_dice), med=np.float64(v_med), ce=np.float64(v_ce), mse=np.float64(v_mse),
                        comp=np.float64(comp.item()), comp_dlogits=lg.grad.numpy())
    print("losses_c9.npz written")


def sup_trace(R):
    torch.manual_seed(1337)
    net = R.unet.UNet(1, NCLS)
    st = unet_ref.init_state(1337, 1, NCLS)
    assert all(torch.equal(net.state_dict()[k], st[k]) for k in st)
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=5e-4)
    sch = R.coslr.CosineWarmupLR_Scheduler(opt, warmup_epochs=0, warmup_lr=1e-4, num_epochs=150, base_lr=0.01, final_lr=1e-6, iter_per_epoch=200)
    table = laws_ref.cosine_table(0.01, 0, 1e-4, 1e-6, 200, 150)
    crit = R.med.Med_Sup_Loss(NCLS)
    x, lab = synth_batch(41, 2, 32, 32, 1, NCLS, 8)
    assert lab.unique().tolist() == list(range(NCLS))
    bufs, rl, ol, all_masks = {}, [], [], []
    for k in range(1, 5):
        torch.manual_seed(1000 + k)
        out = net(x)
        loss = crit(out, lab.long())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sch.step()
        rl.append(loss.item())
        torch.manual_seed(1000 + k)
        masks = unet_ref.draw_dropout_masks(2, 32, 32)
        all_masks.append(masks)
        ol.append(steps_ref.supervised_step(st, bufs, x, lab.long(), laws_ref.cosine_lr(k, table), 0.9, 5e-4, masks)["loss"])
    close(rl, ol, 2e-5, "sup c9 trace")
    net.eval()
    with torch.no_grad():
        fin = net(x)
        fo = unet_ref.unet_forward(st, x, train=False)
    close(fin, fo, 2e-4, "sup c9 final logits")
    np.savez_compressed(os.path.join(OUT, "trace_sup_c9.npz"), x=x.numpy(), labels=lab.numpy(), losses=np.array(rl), final_eval_logits=fin.numpy(),
                        oracle_err=np.float64(np.abs(np.array(rl) - np.array(ol)).max()),
                        **{f"it{k}_mask{i}": pack(m) for k, ms in enumerate(all_masks) for i, m in enumerate(ms)})
    print("trace_sup_c9.npz written; reference vs oracle max |d loss| =", float(np.abs(np.array(rl) - np.array(ol)).max()))


def ict_trace(R):
    crit = R.med.Med_Sup_Loss(NCLS)
    torch.manual_seed(1337)
    net = R.unet.UNet(1, NCLS)
    ema = copy.deepcopy(net)
    for p_ in ema.parameters():
        p_.requires_grad = False
    net.train()
    ema.train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    sch = R.medlr.Medical_LR(opt, 0.01, 30000)
    xl, yl = synth_batch(41, 2, 32, 32, 1, NCLS, 8)
    xu, _ = synth_batch(42, 4, 32, 32, 1, NCLS, 8)
    st = unet_ref.init_state(1337, 1, NCLS)
    est = unet_ref.clone_state(st)
    bufs = {}
    cons_w = 0.1 * R.utils.sigmoid_rampup(40, 200.0)
    rng = np.random.RandomState(5)
    rl, ol, mm, mixes = [], [], [], []
    for k in range(1, 4):
        mix = torch.tensor(rng.beta(0.2, 0.2, size=(2, 1, 1, 1)), dtype=torch.float)
        mixes.append(mix.numpy())
        u0, u1 = xu[:2], xu[2:]
        mixed = u0 * (1.0 - mix) + u1 * mix
        torch.manual_seed(3000 + k)
        out = net(torch.cat([xl, mixed], 0))
        soft = torch.softmax(out, 1)
        with torch.no_grad():
            e0 = torch.softmax(ema(u0), dim=1)
            e1 = torch.softmax(ema(u1), dim=1)
            target = e0 * (1.0 - mix) + e1 * mix
        sup = crit(out[:2], yl.long())
        cons = torch.mean((soft[2:] - target) ** 2)
        loss = sup + cons_w * cons
        opt.zero_grad()
        loss.backward()
        opt.step()
        sch.step()
        R.utils.update_ema_variables(net, ema, 0.99, k)
        rl.append([loss.item(), sup.item(), cons.item()])
        torch.manual_seed(3000 + k)
        ms = unet_ref.draw_dropout_masks(4, 32, 32)
        m0 = unet_ref.draw_dropout_masks(2, 32, 32)
        m1 = unet_ref.draw_dropout_masks(2, 32, 32)
        mm.append((ms, m0, m1))
        r = steps_ref.ict_step(st, est, bufs, xl, yl.long(), xu, mix, laws_ref.medical_lr(k, 0.01, 30000), cons_w, laws_ref.ema_alpha(k, 0.99),
                               0.9, 1e-4, ms, m0, m1)
        ol.append([r["loss"], r["sup"], r["cons"]])
    close(rl, ol, 2e-5, "ict c9 trace")
    for k_, v_ in ema.state_dict().items():
        close(v_, est[k_], 1e-5, f"ict c9 ema {k_}")
    err = float(np.abs(np.array(rl) - np.array(ol)).max())
    np.savez_compressed(os.path.join(OUT, "trace_ict_c9.npz"), xl=xl.numpy(), yl=yl.numpy(), xu=xu.numpy(), cons_w=np.float64(cons_w),
                        losses=np.array(rl), mixes=np.stack(mixes), student_logits_last=out.detach().numpy(), target_last=target.numpy(),
                        oracle_err=np.float64(err),
                        **{f"it{k}_{w}{i}": pack(m) for k, trip in enumerate(mm) for w, ml in zip(("s", "a", "b"), trip) for i, m in enumerate(ml)})
    print("trace_ict_c9.npz written; reference vs oracle max |d loss| =", err)


def main():
    torch.set_num_threads(4)
    R = load_reference()
    losses_fixture(R)
    sup_trace(R)
    ict_trace(R)


if __name__ == "__main__":
    main()
