"""Writes the SegFormer fixtures above the 64-key boundary from the reference's own modules, loaded by path -- arrays only:

  tests/golden/segformer_b0_288.npz       the reference's SegFormer (MiT-B0) on a 1 x 1 x 288 x 288 batch after seed 1337
  tests/golden/segformer_plus_b1_288.npz  the reference's SegFormer_Plus (MiT-B1 + the two projection necks) on the same batch

At 288 x 288 every stage's attention has (288 / 32)^2 = 81 keys: one full block of 64 and a ragged second one.  Each file holds the input,
eval logits, train logits with the drop-path draws / Dropout2d mask of that forward (stored, so a run can inject them), the Med_Sup_Loss
value, a (sum, abs-sum, abs-max) row per parameter gradient (``g:<name>``) and a handful of whole gradient tensors (``grad:<name>``: the
q / kv / proj weights' neighbours that the attention core feeds directly); the B1 file adds both neck outputs and the weights of the linear
functional through which the necks enter the gradient.  Logits are stored on a pixel stride (``logit_stride``) to keep the files small.

oracle/segformer_ref.py is the yardstick of the device tests; this script asserts that it reproduces every array at this size before
anything is written (for B1 with its DIMS overridden at run time -- the oracle file itself is not edited).  Weights are never stored:
seeded construction recreates them.
Run in the build container, from the repository root:  python -m tools.make_golden_segformer_keys
"""
from __future__ import annotations

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
HW, STRIDE = 288, 4
DIMS = {"B0": [32, 64, 160, 256], "B1": [64, 128, 320, 512]}
NECKS = ("dense_projection_high", "dense_projection_head")
# whole gradient tensors kept: the biases right in front of and behind the attention core of one block per stage, and the spatial-reduction norm
FULL_GRADS = ["encoder.block1.0.attn.q.bias", "encoder.block1.0.attn.kv.bias", "encoder.block2.1.attn.kv.bias", "encoder.block3.0.attn.q.bias",
              "encoder.block3.0.attn.norm.weight", "encoder.block4.1.attn.kv.bias", "encoder.block4.1.attn.proj.bias"]


def fixture(seg, R, name, plus):
    S.DIMS = DIMS[name]
    torch.manual_seed(1337)
    cls = seg.SegFormer_Plus if plus else seg.SegFormer
    net = cls(image_size=[HW, HW], in_channels=1, num_classes=4, model_name=name)
    sd = net.state_dict()
    st = S.init_state(1337, 1, 4)
    keys = list(sd.keys())
    assert keys[:len(st)] == list(st.keys()) and all(k.startswith(NECKS) for k in keys[len(st):]), "state_dict keys / order differ"
    for k in list(st):
        close(sd[k], st[k], 0.0, f"init {k}")
    for k in keys[len(st):]:
        st[k] = sd[k].detach().clone()
    x, y = synth_batch(91, 1, HW, HW)
    net.eval()
    with torch.no_grad():
        ev = net.val(x) if plus else net(x)
        e_ev = close(ev, S.segformer_forward(st, x, False), 2e-5, "eval logits")
    net.train()
    torch.manual_seed(99)
    res = net(x)
    out, necks = (res[0], (*res[1], *res[2])) if plus else (res, ())
    loss = R.med.Med_Sup_Loss(4)(out, y.long())
    g = torch.Generator().manual_seed(5)
    wts = [torch.randn(t.shape, generator=g) * 0.01 for t in necks]      # the necks enter the gradient through a fixed linear functional
    (loss + sum((w * t).sum() for w, t in zip(wts, necks))).backward()
    torch.manual_seed(99)
    dp, mask = S.draw_randomness(1)
    names = [k for k in st if st[k].is_floating_point() and "running" not in k]
    for k in names:
        st[k] = st[k].clone().requires_grad_(True)
    taps = {}
    o2 = S.segformer_forward(st, x, True, dp, mask, taps=taps)
    n2 = (*unet_ref.projection_neck(st, NECKS[0], taps["stage4"]), *unet_ref.projection_neck(st, NECKS[1], o2)) if plus else ()
    l2 = losses_ref.med_sup_loss(o2, y.long())
    gs = torch.autograd.grad(l2 + sum((w * t).sum() for w, t in zip(wts, n2)), [st[k] for k in names])
    e_tr = close(out, o2, 2e-5, "train logits")
    e_loss = close(loss, l2, 1e-6, "loss")
    for a, b, what in zip(necks, n2, ("high global", "high dense", "head global", "head dense")):
        close(a, b, 2e-5, what)
    ref_g = dict(net.named_parameters())
    rows, e_g = {}, 0.0
    for k, g_ in zip(names, gs):
        gr = ref_g[k].grad
        e_g = max(e_g, close(gr, g_, 2e-5 * max(1.0, float(gr.abs().max())), f"grad {k}") / max(1.0, float(gr.abs().max())))
        rows["g:" + k] = np.array([float(gr.sum()), float(gr.abs().sum()), float(gr.abs().max())])
    for k in FULL_GRADS:
        rows["grad:" + k] = ref_g[k].grad.numpy().copy()
    if plus:
        rows.update(high_global=necks[0].detach().numpy(), high_dense=necks[1].detach().numpy(), head_global=necks[2].detach().numpy(),
                    head_dense=necks[3].detach().numpy(), neck_weights=np.concatenate([w.flatten().numpy() for w in wts]))
    fname = "segformer_plus_b1_288.npz" if plus else "segformer_b0_288.npz"
    path = os.path.join(OUT, fname)
    s = STRIDE
    np.savez_compressed(path, x=x.numpy(), y=y.numpy(), logit_stride=np.int64(s),
                        **{f"eval_logits_s{s}": ev[..., ::s, ::s].numpy(), f"train_logits_s{s}": out.detach()[..., ::s, ::s].numpy()},
                        loss=np.float64(loss.item()), drop_path=np.stack([d.reshape(-1).numpy() for d in dp if d is not None]), dropout_mask=pack(mask),
                        full_grads=np.array(FULL_GRADS), oracle_err=np.array([e_ev, e_tr, e_loss, e_g]), **rows)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    print(f"{fname}: {size} bytes; loss {loss.item():.6f}; oracle vs reference: eval logits {e_ev:.2e} train logits {e_tr:.2e} loss {e_loss:.2e} "
          f"gradients / max(1, |g|) {e_g:.2e}")


def main():
    torch.set_num_threads(8)
    R = load_reference()
    seg = _load("ref_segformer", "model/segformer.py")
    fixture(seg, R, "B0", False)
    fixture(seg, R, "B1", True)


if __name__ == "__main__":
    main()
