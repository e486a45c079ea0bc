"""Writes the SegFormer_Plus (MiT-B1 + projection necks) fixtures from the reference's own modules, loaded by path -- arrays only:

  tests/golden/segformer_plus_b1.npz          the reference's SegFormer_Plus on a 2 x 1 x 128 x 128 batch after seed 1337: eval / train logits,
                                              both neck outputs, the Med_Sup_Loss value, a (sum, abs-sum, abs-max) row per parameter
                                              gradient, shape + (sum, abs-sum, first 8 values) of the 16 neck tensors at init, and the
                                              drop-path draws / Dropout2d mask of the train-mode forward
  tests/golden/trace_hpfg_segformer_plus.npz  iterations 999, 1000, 1001 of the reference's HPFG loop body (main.py:139-214) on three
                                              SegFormer_Plus networks at 2 + 2 images of 128 x 128, once with SGD + medical and once with
                                              AdamW + warm-up cosine: inputs, CutMix masks, per-iteration draws of all three networks,
                                              learning rates, loss rows and the last iteration's three logit tensors

oracle/segformer_ref.py serves as the B1 yardstick with its DIMS overridden at run time (heads, SR ratios and depths are B1's already);
this script asserts that it reproduces every array of the first file.  Weights are never stored: seeded construction recreates them.
Logit tensors are stored on a fixed pixel stride (the ``_s<stride>`` suffix of their keys) to keep the files small.
Run in the build container, from the repository root:  python -m tools.make_golden_segformer_plus
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

from oracle import losses_ref, segformer_ref as S, unet_ref      # noqa: E402
from oracle.make_golden import _load, close, load_reference, pack, synth_batch      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
B1_DIMS = [64, 128, 320, 512]
NECKS = ("dense_projection_high", "dense_projection_head")
LOGIT_STRIDE, TRACE_STRIDE = 2, 4


def neck_rows(sd):
    """shape and (sum, abs-sum, first 8 values) of every neck tensor of a state dict, in its order."""
    rows = {}
    for k, v in sd.items():
        if k.startswith(NECKS):
            f = v.detach().double().flatten()
            rows["neck_shape:" + k] = np.array(v.shape, dtype=np.int64)
            rows["neck_init:" + k] = np.concatenate([[float(f.sum()), float(f.abs().sum())], f[:8].numpy()])
    return rows


def draws_np(dp, mask):
    """drop-path draws [14, B] (the two branches of the first block draw nothing) and the packed Dropout2d mask [B, 256]"""
    return np.stack([d.reshape(-1).numpy() for d in dp if d is not None]), pack(mask)


def model_fixture(seg, R):
    torch.manual_seed(1337)
    net = seg.SegFormer_Plus(image_size=[128, 128], in_channels=1, num_classes=4, model_name="B1")
    sd = net.state_dict()
    st = S.init_state(1337, 1, 4)
    keys = list(sd.keys())
    assert len(keys) == 208 and keys[:192] == list(st.keys()) and all(k.startswith(NECKS) for k in keys[192:]), "state_dict keys / order differ"
    for k in st:
        close(sd[k], st[k], 0.0, f"init {k}")
    n_backbone = sum(p.numel() for n, p in net.named_parameters() if not n.startswith(NECKS))
    n_total = sum(p.numel() for p in net.parameters())
    assert (n_backbone, n_total) == (13672004, 16570436), (n_backbone, n_total)
    rows = neck_rows(sd)
    for k in keys[192:]:
        st[k] = sd[k].detach().clone()
    x, y = synth_batch(71, 2, 128, 128)
    net.eval()
    with torch.no_grad():
        ev = net.val(x)
        close(ev, S.segformer_forward(st, x, False), 2e-5, "eval logits")
    net.train()
    torch.manual_seed(99)
    out, high, head = net(x)
    loss = R.med.Med_Sup_Loss(4)(out, y.long())
    # the necks take part in the gradient through a fixed linear functional of their outputs (the loss alone never reaches them)
    g = torch.Generator().manual_seed(5)
    wts = [torch.randn(t.shape, generator=g) * 0.01 for t in (*high, *head)]
    total = loss + sum((w * t).sum() for w, t in zip(wts, (*high, *head)))
    total.backward()
    torch.manual_seed(99)
    dp, mask = S.draw_randomness(2)
    names = [k for k in st if st[k].is_floating_point() and "running" not in k]
    for k in names:
        st[k] = st[k].clone().requires_grad_(True)
    taps = {}
    o2 = S.segformer_forward(st, x, True, dp, mask, taps=taps)
    hi2 = unet_ref.projection_neck(st, NECKS[0], taps["stage4"])
    he2 = unet_ref.projection_neck(st, NECKS[1], o2)
    l2 = losses_ref.med_sup_loss(o2, y.long())
    t2 = l2 + sum((w * t).sum() for w, t in zip(wts, (*hi2, *he2)))
    gs = torch.autograd.grad(t2, [st[k] for k in names])
    close(out, o2, 2e-5, "train logits")
    close(loss, l2, 1e-6, "loss")
    for a, b, what in zip((*high, *head), (*hi2, *he2), ("high global", "high dense", "head global", "head dense")):
        close(a, b, 2e-5, what)
    ref_g = dict(net.named_parameters())
    gsum = {}
    for k, g_ in zip(names, gs):
        close(ref_g[k].grad, g_, 2e-5 * max(1.0, float(ref_g[k].grad.abs().max())), f"grad {k}")
        gsum["g:" + k] = np.array([float(ref_g[k].grad.sum()), float(ref_g[k].grad.abs().sum()), float(ref_g[k].grad.abs().max())])
    dpn, maskn = draws_np(dp, mask)
    s = LOGIT_STRIDE
    path = os.path.join(OUT, "segformer_plus_b1.npz")
    np.savez_compressed(path, x=x.numpy(), y=y.numpy(), logit_stride=np.int64(s),
                        **{f"eval_logits_s{s}": ev[..., ::s, ::s].numpy(), f"train_logits_s{s}": out.detach()[..., ::s, ::s].numpy()},
                        high_global=high[0].detach().numpy(), high_dense=high[1].detach().numpy(),
                        head_global=head[0].detach().numpy(), head_dense=head[1].detach().numpy(),
                        neck_weights=np.concatenate([w.flatten().numpy() for w in wts]),
                        loss=np.float64(loss.item()), total=np.float64(total.item()), drop_path=dpn, dropout_mask=maskn,
                        n_backbone=np.int64(n_backbone), n_params=np.int64(n_total), keys=np.array(keys), **rows, **gsum)
    print(f"segformer_plus_b1.npz: {os.path.getsize(path)} bytes; {len(names)} parameter tensors, {n_total} parameters; loss {loss.item():.6f}")


def hpfg_trace(seg, R, variant):
    """main.py:139-214 with model1 = model2's class = SegFormer_Plus, ema_model = deepcopy(model2) (main.py:60-66)."""
    gen = R.utils.BoxMaskGenerator(prop_range=(0.25, 0.5), n_boxes=4, random_aspect_ratio=True, prop_by_area=True, within_bounds=True, invert=True)
    NL, NU, HW, TOTAL = 2, 2, 128, 30000
    torch.manual_seed(1337)
    m1 = seg.SegFormer_Plus(image_size=[HW, HW], in_channels=1, num_classes=4, model_name="B1")
    m2 = seg.SegFormer_Plus(image_size=[HW, HW], in_channels=1, num_classes=4, model_name="B1")
    em = copy.deepcopy(m2)
    for p_ in em.parameters():
        p_.requires_grad = False
    m1.train()
    m2.train()
    em.train()
    if variant == "sgd":
        o1, o2 = (torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4) for m in (m1, m2))
        s1, s2 = (R.medlr.Medical_LR(o, 0.01, TOTAL) for o in (o1, o2))
    else:
        o1, o2 = (torch.optim.AdamW(m.parameters(), lr=6e-4, weight_decay=0.05) for m in (m1, m2))
        s1, s2 = (R.coslr.CosineWarmupLR_Scheduler(o, warmup_epochs=1, warmup_lr=1e-5, num_epochs=TOTAL // 1500, base_lr=6e-4, final_lr=1e-6,
                                                   iter_per_epoch=1500) for o in (o1, o2))
    for _ in range(999 - 1):                           # the schedulers as they stand when iteration 999 begins (no gradient yet: no update)
        o1.step()
        o2.step()
        s1.step()
        s2.step()
    neck0 = {k: v.detach().clone() for k, v in m1.state_dict().items() if k.startswith(NECKS)}
    dense = R.dense.Dense_Loss(NL + NU, torch.device("cpu"))
    ce = torch.nn.CrossEntropyLoss(ignore_index=255)
    dl = R.dice.DiceLoss(4)
    xl, yl = synth_batch(81, NL, HW, HW)
    xl1_, yl1_ = synth_batch(82, NL, HW, HW)
    xu, _ = synth_batch(83, NU, HW, HW)
    rng = np.random.RandomState(3)
    rl, cms, lrs, draws = [], [], [], {}
    for j, cur in enumerate((999, 1000, 1001)):
        rep = NU // NL
        xl1 = xl1_.repeat(rep, 1, 1, 1)
        yl1 = yl1_.repeat(rep, 1, 1).long()
        cm = torch.tensor(gen.generate_params(NU, (HW, HW), rng=rng), dtype=torch.float)
        cms.append(cm)
        mix = torch.cat([xl, xl1 * (1.0 - cm) + xu * cm], 0)
        torch.manual_seed(7000 + j)
        a, _, _ = m1(mix)
        sa_ = torch.softmax(a, 1)
        vol = torch.cat([xl, xu], 0)
        b, h1, h2 = m2(vol)
        sb_ = torch.softmax(b, 1)
        with torch.no_grad():
            eo, eh1, eh2 = em(vol)
            es = torch.softmax(eo.detach(), 1)
        torch.manual_seed(7000 + j)                    # the same draws, in the order model1, model2, teacher
        for w_ in "abt":
            dpn, maskn = draws_np(*S.draw_randomness(NL + NU))
            draws[f"it{j}_{w_}_drop_path"], draws[f"it{j}_{w_}_dropout_mask"] = dpn, maskn
        l1 = 0.5 * (ce(a[:NL], yl.long()) + dl(sa_[:NL], yl.long().unsqueeze(1)))
        l2 = 0.5 * (ce(b[:NL], yl.long()) + dl(sb_[:NL], yl.long().unsqueeze(1)))
        sup = l1 + l2
        con = dense(h1, eh1) + dense(h2, eh2)
        c2 = cm.squeeze(1)
        pseudo = yl1 * (1.0 - c2) + torch.argmax(es[NL:], 1) * c2
        ps = dl(sa_[NL:], pseudo.unsqueeze(1))
        w = 0.1 * R.utils.linear_rampup(cur // 150, 200.0)
        cons2 = 0.0 if cur < 1000 else torch.mean((sb_[NL:] - es[NL:]) ** 2)
        semi = 7 * w * ps + w * cons2 + w * con
        loss = sup + semi
        lrs.append([o1.param_groups[0]["lr"], o2.param_groups[0]["lr"]])
        o1.zero_grad()
        o2.zero_grad()
        loss.backward()
        o1.step()
        o2.step()
        alpha = min(1 - 1 / (cur + 1), 0.99)
        with torch.no_grad():
            for part in ("encoder", "decoder"):
                for pe, pm in zip(getattr(m2, part).parameters(), getattr(m1, part).parameters()):
                    pe.data.mul_(alpha).add_(pm.data, alpha=1 - alpha)
        R.utils.update_ema_variables(m2, em, 0.99, cur)
        s1.step()
        s2.step()
        rl.append([loss.item(), sup.item(), float(semi), ps.item(), con.item(), float(cons2)])
    assert rl[0][5] == 0.0 and rl[1][5] > 0.0
    for k, v in m1.state_dict().items():               # torch skips parameters without a gradient: the first student's necks never move
        if k.startswith(NECKS):
            assert torch.equal(v, neck0[k]), k
    s = TRACE_STRIDE
    d = {"lrs": np.array(lrs), "losses": np.array(rl), f"logits1_last_s{s}": a.detach()[..., ::s, ::s].numpy(),
         f"logits2_last_s{s}": b.detach()[..., ::s, ::s].numpy(), f"t_logits_last_s{s}": eo[..., ::s, ::s].numpy(), **draws}
    shared = dict(xl=xl.numpy(), yl=yl.numpy(), xl1=xl1_.numpy(), yl1=yl1_.numpy(), xu=xu.numpy(), cur_itrs=np.array([999, 1000, 1001]),
                  cutmix=np.stack([pack(c) for c in cms]), logit_stride=np.int64(s))
    return shared, {f"{variant}_{k}": v for k, v in d.items()}


def main():
    torch.set_num_threads(8)
    R = load_reference()
    seg = _load("ref_segformer", "model/segformer.py")
    S.DIMS = B1_DIMS                                   # run-time override: the oracle file itself is not edited
    which = sys.argv[1:] or ["model", "trace"]
    if "model" in which:
        model_fixture(seg, R)
    if "trace" in which:
        out = {}
        for variant in ("sgd", "adamw"):
            shared, d = hpfg_trace(seg, R, variant)
            out.update(shared)
            out.update(d)
            print(variant, "losses", np.array2string(d[f"{variant}_losses"], precision=5))
        path = os.path.join(OUT, "trace_hpfg_segformer_plus.npz")
        np.savez_compressed(path, **out)
        print(f"trace_hpfg_segformer_plus.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
