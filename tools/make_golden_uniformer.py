"""Writes the Uniformer_Plus fixture from the reference's own modules, loaded by path -- arrays only:

  tests/golden/uniformer_plus.npz   the reference's Uniformer_Plus (UniFormer-S + SegFormerHead + projection necks) after seed 1337 on a
                                    2 x 1 x S x S batch, S = 128 (both attention stages at most 64 keys) and S = 160 (stage 3: 100 keys):
                                    eval / train logits, both neck outputs, the loss, the drop-path draws and the Dropout2d mask of the
                                    train-mode forward, a (sum, abs-sum, abs-max) row per parameter gradient, the whole gradient of a few
                                    small named parameters, one stage norm's running statistics after the forward, and the state_dict
                                    keys and shapes.  Keys of a size carry the suffix ``@S``.

  tests/golden/trace_hpfg_uniformer_plus.npz  iterations 999, 1000, 1001 of the reference's HPFG loop body (main.py:139-214) on three
                                    Uniformer_Plus networks at 2 + 2 images of 128 x 128, once with SGD + medical and once with AdamW +
                                    warm-up cosine (the recipe of config/ccnet_uniformer_30k_224x224_ACDC.yaml): inputs, CutMix masks,
                                    per-iteration draws of all three networks in the order they were drawn, learning rates, loss rows
                                    and the last iteration's three logit tensors

The reference's model/uniformer.py imports ``timm``, which is not installed: stand-in modules for the five names it imports are put into
``sys.modules`` first (the recipe SURVEY.md used for ``easydict``): ``trunc_normal_`` is torch's ``nn.init.trunc_normal_`` (a known
deviation: timm's own could not be compared), ``to_2tuple``, ``register_model`` and ``_cfg`` do nothing, and ``DropPath`` applies the law
of the reference's model/segformer.py:23-30 and records its draws.  The Dropout2d mask is read off the head's dropout module (a channel it
zeroed although its input was not zero).  Weights are never stored: seeded construction recreates them.  Logit tensors are stored on a
fixed pixel stride (the ``_s<stride>`` part of their keys).
Run in the build container, from the repository root:  python -m tools.make_golden_uniformer
"""
from __future__ import annotations

import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.make_golden import _load, load_reference, pack, synth_batch      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SEED, DRAW_SEED, LOGIT_STRIDE, TRACE_STRIDE = 1337, 99, 4, 8
NECKS = ("dense_projection_high", "dense_projection_head")
SIDES = (128, 160)
FULL_GRADS = ("encoder.patch_embed1.proj.weight", "encoder.blocks1.0.pos_embed.weight", "encoder.blocks1.0.attn.weight",
              "encoder.blocks1.2.norm1.weight", "encoder.blocks2.3.norm2.bias", "encoder.blocks2.1.attn.bias", "encoder.norm2.weight",
              "encoder.blocks3.0.attn.qkv.bias", "encoder.blocks3.7.pos_embed.weight", "encoder.blocks4.2.norm2.weight", "encoder.norm4.bias",
              "decoder.linear_pred.bias", "decoder.linear_fuse.bn.weight", "dense_projection_high.mlp.2.bias")
DRAWS = []


class DropPath(nn.Module):
    """x / keep * floor(keep + U), one U per sample; p == 0 or eval mode: the identity, nothing drawn.  Records U."""

    def __init__(self, p=None):
        super().__init__()
        self.p = p

    def forward(self, x):
        if self.p == 0. or not self.training:
            return x
        kp = 1 - self.p
        r = torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype)
        DRAWS.append(r.reshape(-1).clone())
        return x.div(kp) * (kp + r).floor()


def stub_timm():
    def mod(name, **names):
        m = types.ModuleType(name)
        m.__dict__.update(names)
        sys.modules[name] = m
        return m
    mod("timm")
    mod("timm.models")
    mod("timm.models.vision_transformer", _cfg=lambda **kw: {})
    mod("timm.models.registry", register_model=lambda f: f)
    mod("timm.models.layers", trunc_normal_=nn.init.trunc_normal_, DropPath=DropPath, to_2tuple=lambda v: v if isinstance(v, tuple) else (v, v))


def fixture(uni, R, side):
    torch.manual_seed(SEED)
    net = uni.Uniformer_Plus(image_size=[side, side], in_channels=1, num_classes=4)
    sd = net.state_dict()
    x, y = synth_batch(70 + side, 2, side, side)
    net.eval()
    with torch.no_grad():
        ev = net.val(x)
    net.train()
    seen = {}
    hook = net.decoder.dropout.register_forward_hook(lambda m, i, o: seen.update(i=i[0].detach().clone(), o=o.detach().clone()))
    DRAWS.clear()
    torch.manual_seed(DRAW_SEED)
    out, high, head = net(x)
    hook.remove()
    zeroed = (seen["o"].abs().sum((2, 3)) == 0) & (seen["i"].abs().sum((2, 3)) > 0)
    mask = (~zeroed).float()                                   # [B, 256]: 1 = kept
    assert 0.75 < float(mask.mean()) < 1.0 and len(DRAWS) == 34, (float(mask.mean()), len(DRAWS))
    loss = R.med.Med_Sup_Loss(4)(out, y.long())
    g = torch.Generator().manual_seed(5)                       # the necks join the gradient through a fixed linear functional of their outputs
    wts = [torch.randn(t.shape, generator=g) * 0.01 for t in (*high, *head)]
    total = loss + sum((w * t).sum() for w, t in zip(wts, (*high, *head)))
    total.backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    s, t = LOGIT_STRIDE, f"@{side}"
    d = {"x" + t: x.numpy(), "y" + t: y.numpy(), f"eval_logits_s{s}" + t: ev[..., ::s, ::s].numpy(),
         f"train_logits_s{s}" + t: out.detach()[..., ::s, ::s].numpy(),
         "high_global" + t: high[0].detach().numpy(), "high_dense" + t: high[1].detach().numpy(),
         "head_global" + t: head[0].detach().numpy(), "head_dense" + t: head[1].detach().numpy(),
         "neck_weights" + t: np.concatenate([w.flatten().numpy() for w in wts]), "loss" + t: np.float64(loss.item()),
         "total" + t: np.float64(total.item()), "drop_path" + t: np.stack([r.numpy() for r in DRAWS]), "dropout_mask" + t: pack(mask),
         "norm1_running_mean" + t: net.encoder.norm1.running_mean.numpy().copy(), "norm1_running_var" + t: net.encoder.norm1.running_var.numpy().copy(),
         "gsum" + t: np.array([[float(v.sum()), float(v.abs().sum()), float(v.abs().max())] for v in grads.values()])}
    for k in FULL_GRADS:
        d[f"grad:{k}" + t] = grads[k].numpy()
    print(f"side {side}: loss {loss.item():.6f}, total {total.item():.6f}, {len(grads)} parameter tensors, kept channels {float(mask.mean()):.3f}")
    return d, sd, list(grads)


class MaskTap:
    """The Dropout2d mask [B, 256] of a network's head at every forward: a channel the module zeroed although its input was not zero."""

    def __init__(self, net):
        self.masks = []
        net.decoder.dropout.register_forward_hook(self)

    def __call__(self, mod, inp, out):
        zeroed = (out.detach().abs().sum((2, 3)) == 0) & (inp[0].detach().abs().sum((2, 3)) > 0)
        self.masks.append((~zeroed).float())


def hpfg_trace(uni, R, variant):
    """main.py:139-214 with model1 = model2's class = Uniformer_Plus, ema_model = deepcopy(model2) (main.py:60-66)."""
    gen = R.utils.BoxMaskGenerator(prop_range=(0.25, 0.5), n_boxes=4, random_aspect_ratio=True, prop_by_area=True, within_bounds=True, invert=True)
    NL, NU, HW, TOTAL = 2, 2, 128, 30000
    torch.manual_seed(SEED)
    m1 = uni.Uniformer_Plus(image_size=[HW, HW], in_channels=1, num_classes=4)
    m2 = uni.Uniformer_Plus(image_size=[HW, HW], in_channels=1, num_classes=4)
    em = copy.deepcopy(m2)
    for p_ in em.parameters():
        p_.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    taps = [MaskTap(m) for m in (m1, m2, em)]
    if variant == "sgd":
        o1, o2 = (torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4) for m in (m1, m2))
        s1, s2 = (R.medlr.Medical_LR(o, 0.01, TOTAL) for o in (o1, o2))
    else:
        o1, o2 = (torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.05) for m in (m1, m2))
        s1, s2 = (R.coslr.CosineWarmupLR_Scheduler(o, warmup_epochs=1, warmup_lr=1e-5, num_epochs=TOTAL // 1500, base_lr=1e-3, final_lr=1e-6,
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
        DRAWS.clear()
        a, _, _ = m1(mix)
        sa_ = torch.softmax(a, 1)
        vol = torch.cat([xl, xu], 0)
        b, h1, h2 = m2(vol)
        sb_ = torch.softmax(b, 1)
        with torch.no_grad():
            eo, eh1, eh2 = em(vol)
            es = torch.softmax(eo.detach(), 1)
        assert len(DRAWS) == 3 * 34 and all(len(t.masks) == j + 1 for t in taps)
        for n_, w_ in enumerate("abt"):                # recorded in the order drawn: model1, model2, teacher
            draws[f"it{j}_{w_}_drop_path"] = np.stack([r.numpy() for r in DRAWS[34 * n_:34 * (n_ + 1)]])
            draws[f"it{j}_{w_}_dropout_mask"] = pack(taps[n_].masks[j])
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
         f"logits2_last_s{s}": b.detach()[..., ::s, ::s].numpy(), f"t_logits_last_s{s}": eo[..., ::s, ::s].numpy(),
         "bn_batches": np.array([int(m.encoder.norm1.num_batches_tracked) for m in (m1, m2, em)]), **draws}
    shared = dict(xl=xl.numpy(), yl=yl.numpy(), xl1=xl1_.numpy(), yl1=yl1_.numpy(), xu=xu.numpy(), cur_itrs=np.array([999, 1000, 1001]),
                  cutmix=np.stack([pack(c) for c in cms]), logit_stride=np.int64(s))
    return shared, {f"{variant}_{k}": v for k, v in d.items()}


def main():
    torch.set_num_threads(8)
    R = load_reference()
    stub_timm()
    uni = _load("ref_uniformer", "model/uniformer.py")
    which = sys.argv[1:] or ["model", "trace"]
    if "trace" in which:
        tr = {}
        for variant in ("sgd", "adamw"):
            shared, d = hpfg_trace(uni, R, variant)
            tr.update(shared)
            tr.update(d)
            print(variant, "losses", np.array2string(d[f"{variant}_losses"], precision=5))
        path = os.path.join(OUT, "trace_hpfg_uniformer_plus.npz")
        np.savez_compressed(path, **tr)
        print(f"trace_hpfg_uniformer_plus.npz: {os.path.getsize(path)} bytes")
    if "model" not in which:
        return
    out = {}
    for side in SIDES:
        d, sd, pnames = fixture(uni, R, side)
        out.update(d)
    out.update(seed=np.int64(SEED), draw_seed=np.int64(DRAW_SEED), logit_stride=np.int64(LOGIT_STRIDE), keys=np.array(list(sd)),
               shapes=np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64), param_names=np.array(pnames),
               n_params=np.int64(sum(v.numel() for k, v in sd.items() if k in set(pnames))))
    path = os.path.join(OUT, "uniformer_plus.npz")
    np.savez_compressed(path, **out)
    print(f"uniformer_plus.npz: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
