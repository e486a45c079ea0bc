"""SegFormer_Plus (MiT-B1: head dim 64 attention, 512-channel neck) and the HPFG step on three of them, against
 * the reference's own numbers (tests/golden/segformer_plus_b1.npz, trace_hpfg_segformer_plus.npz: tools/make_golden_segformer_plus.py),
 * the CPU oracle with its DIMS set to B1's at run time (oracle/segformer_ref.py + oracle/unet_ref.projection_neck for the necks).
Logit tensors of the fixtures are stored on a pixel stride (``logit_stride``)."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

from hpfg_amd.model import SegFormer_Plus, build_model
from hpfg_amd.utils import AttrDict, Med_Sup_Loss, loadyaml
from oracle import losses_ref, segformer_ref as S, unet_ref
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B1_DIMS = [64, 128, 320, 512]
NECKS = ("dense_projection_high", "dense_projection_head")


def _draws(dp_rows, mask_bits, B):
    """fixture arrays -> (drop_path_draws, dropout_mask) as SegFormer_Plus.external_draws takes them (the first block draws nothing)"""
    dp = [None, None] + [torch.from_numpy(r.copy()).reshape(B, 1, 1) for r in dp_rows]
    mask = torch.from_numpy(np.unpackbits(mask_bits)[: B * 256].reshape(B, 256, 1, 1).astype(np.float32))
    return dp, mask


def _neck_functional(weights, outs):
    """sum of <w, t> over the four neck outputs: lets the necks take part in a gradient check (the segmentation loss never reaches them)"""
    o, tot = 0, 0.0
    for t in outs:
        w = weights[o:o + t.numel()].view(t.shape)
        o += t.numel()
        tot = tot + (w * t).sum()
    assert o == weights.numel()
    return tot


def test_golden_fixture_parity(golden_dir):
    d = np.load(f"{golden_dir}/segformer_plus_b1.npz")
    s = int(d["logit_stride"])
    torch.manual_seed(1337)
    m = build_model(AttrDict(model="segformer_plus", in_channels=1, num_classes=4, train_crop_size=[128, 128])).to(DEV)
    x, y = torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["y"]).to(DEV)
    m.eval()
    with torch.no_grad():
        ev = m.val(x)
        assert ev.shape == (2, 4, 128, 128)
        e_ev = maxerr(ev[..., ::s, ::s].cpu(), torch.from_numpy(d[f"eval_logits_s{s}"]))
    m.train()
    m.external_draws = _draws(d["drop_path"], d["dropout_mask"], 2)
    out, high, head = m(x)
    assert [tuple(t.shape) for t in (*high, *head)] == [(2, 128), (2, 128, 16), (2, 128), (2, 128, 16)]
    e_tr = maxerr(out.detach()[..., ::s, ::s].cpu(), torch.from_numpy(d[f"train_logits_s{s}"]))
    e_neck = [maxerr(t.detach().cpu(), torch.from_numpy(d[k])) for t, k in zip((*high, *head), ("high_global", "high_dense", "head_global", "head_dense"))]
    loss = Med_Sup_Loss(4)(out, y)
    e_loss = abs(float(loss.detach()) - float(d["loss"]))
    print(f"fixture parity: eval logits {e_ev:.2e} train logits {e_tr:.2e} necks {max(e_neck):.2e} loss {e_loss:.2e}")
    assert e_ev < 1e-3 and e_tr < 1e-3 and max(e_neck) < 1e-3
    assert e_loss < 1e-4
    (loss + _neck_functional(torch.from_numpy(d["neck_weights"]).to(DEV), (*high, *head))).backward()
    worst = 0.0
    for k, p in m.named_parameters():
        ref = d["g:" + k]
        got = np.array([float(p.grad.sum()), float(p.grad.abs().sum()), float(p.grad.abs().max())])
        worst = max(worst, float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max()))))
        assert np.abs(got - ref).max() < 2e-3 * max(1.0, float(np.abs(ref).max())), (k, got, ref)
    print(f"fixture parity: worst gradient row error / max(1, |ref|) {worst:.2e} (< 2e-3)")


@pytest.mark.parametrize("size,B", [(224, 2), (128, 3)])
def test_train_forward_backward_vs_oracle(size, B, monkeypatch):
    """Full-size tokens (3136 / 784 / 196 / 49 queries against 49 keys at 224 x 224, head dim 64 in every stage): logits, loss, both necks and
    every gradient tensor.  Bounds and their reason: tests/test_gpu_segformer.py::test_train_forward_backward_vs_oracle."""
    monkeypatch.setattr(S, "DIMS", B1_DIMS)
    torch.manual_seed(5)
    m = SegFormer_Plus(image_size=[size, size], in_channels=1, num_classes=4).to(DEV)
    st = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(size)
    x = torch.randn(B, 1, size, size, generator=g)
    y = torch.randint(0, 4, (B, size, size), generator=g)
    wts = torch.randn(2 * B * 128 * 17, generator=g) * 0.01
    torch.manual_seed(7)
    dp, mask = S.draw_randomness(B)
    m.train()
    m.external_draws = (dp, mask)
    out, high, head = m(x.to(DEV))
    loss = Med_Sup_Loss(4)(out, y.to(DEV))
    (loss + _neck_functional(wts.to(DEV), (*high, *head))).backward()
    names = [k for k in st if st[k].is_floating_point() and "running" not in k]
    for k in names:
        st[k] = st[k].requires_grad_(True)
    taps = {}
    ro = S.segformer_forward(st, x, True, dp, mask, taps=taps)
    rhigh = unet_ref.projection_neck(st, NECKS[0], taps["stage4"])
    rhead = unet_ref.projection_neck(st, NECKS[1], ro)
    rl = losses_ref.med_sup_loss(ro, y)
    rg = dict(zip(names, torch.autograd.grad(rl + _neck_functional(wts, (*rhigh, *rhead)), [st[k] for k in names])))
    e_logits = maxerr(out.detach().cpu(), ro.detach())
    e_neck = max(maxerr(a.detach().cpu(), b.detach()) for a, b in zip((*high, *head), (*rhigh, *rhead)))
    errs = {k: float((p.grad.cpu().double() - rg[k].double()).norm() / max(1e-5, float(rg[k].double().norm()))) for k, p in m.named_parameters()}
    print(f"{size}^2 x {B}: logits {e_logits:.2e} necks {e_neck:.2e} loss {abs(float(loss.detach()) - float(rl)):.2e} "
          f"grad rel-L2 max {max(errs.values()):.2e} median {np.median(list(errs.values())):.2e}")
    assert e_logits < 1e-3 and e_neck < 1e-3
    assert abs(float(loss.detach()) - float(rl)) < 1e-4
    bad = {k: v for k, v in errs.items() if not v < 1e-2}
    assert not bad, bad
    assert float(np.median(list(errs.values()))) < 5e-3, sorted(((v, k) for k, v in errs.items()), reverse=True)[:20]
    assert maxerr(m.state_dict()["decoder.linear_fuse.bn.running_var"].cpu(), st["decoder.linear_fuse.bn.running_var"]) < 1e-4


def test_small_input_raises_a_clear_error():
    torch.manual_seed(0)
    m = SegFormer_Plus(image_size=[128, 128], in_channels=1, num_classes=4).to(DEV)
    with pytest.raises(ValueError, match="at least 128"):
        m(torch.zeros(1, 1, 64, 64, device=DEV))


OPT = {"sgd": dict(opt="sgd", lr=0.01, momentum=0.9, weight_decay=1e-4, sched="medical", warmup_epochs=0, warmup_lr=1e-4, min_lr=1e-6),
       "adamw": dict(opt="adamW", lr=6e-4, momentum=0.9, weight_decay=0.05, sched="cosine", warmup_epochs=1, warmup_lr=1e-5, min_lr=1e-6)}


def _three(size):
    torch.manual_seed(1337)
    m1 = SegFormer_Plus(image_size=[size, size], in_channels=1, num_classes=4).to(DEV)
    m2 = SegFormer_Plus(image_size=[size, size], in_channels=1, num_classes=4).to(DEV)      # continues the generator, as in the driver
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    return m1, m2, em


@pytest.mark.parametrize("variant", ["sgd", "adamw"])
def test_hpfg_step_trace(golden_dir, variant):
    """HPFGStep on three SegFormer_Plus networks against iterations 999, 1000, 1001 of the reference's loop body (its own modules and
    optimizers), 2 + 2 images of 128 x 128: every loss row to 1e-3; the last iteration's logits of the two students and the teacher to 1e-3
    after SGD steps and to 2e-2 after AdamW steps (Adam's update is lr * sign(g) wherever a gradient is at rounding level: see
    tests/test_gpu_segformer.py::test_ctct_step_trace).  The first student's necks are never computed: their parameters do not move by a
    bit (no gradient -> no update and no weight decay, as in torch); the teacher follows the EMA law of the second student."""
    from hpfg_amd.train import HPFGStep
    from hpfg_amd.utils.optim import FusedAdamW, FusedSGD
    d = np.load(f"{golden_dir}/trace_hpfg_segformer_plus.npz")
    v, s = variant + "_", int(d["logit_stride"])
    m1, m2, em = _three(128)
    args = AttrDict(dict(OPT[variant], batch_size=2, unlabel_batch_size=2, total_itrs=30000, step_size=1500, consistency=0.1, consistency_rampup=200.0,
                         ema_decay=0.99))
    st = HPFGStep(m1, m2, em, args)
    assert isinstance(st.optimizer1, FusedSGD if variant == "sgd" else FusedAdamW) and st.optimizer1.active_numel == m1.backbone_numel() == 13672004
    assert st.optimizer2.active_numel is None
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(int(d["cur_itrs"][0]) - 1):          # the schedulers as they stand when iteration 999 begins
            st.lr_scheduler1.step()
            st.lr_scheduler2.step()
    necks1 = {k: t.detach().clone() for k, t in m1.state_dict().items() if k.startswith(NECKS)}
    necks2 = {k: t.detach().clone() for k, t in m2.state_dict().items() if k.startswith(NECKS)}
    xl, yl, xl1, yl1, xu = (torch.from_numpy(d[k]).to(DEV) for k in ("xl", "yl", "xl1", "yl1", "xu"))
    rows, e_ema = [], 0.0
    for j, cur in enumerate(d["cur_itrs"]):
        assert abs(float(st.optimizer1.param_groups[0]["lr"]) - float(d[v + "lrs"][j, 0])) < 1e-12
        for net, w in ((m1, "a"), (m2, "b"), (em, "t")):      # draw order of the reference's iteration: model1, model2, teacher
            net.external_draws = _draws(d[f"{v}it{j}_{w}_drop_path"], d[f"{v}it{j}_{w}_dropout_mask"], 4)
        cm = torch.from_numpy(np.unpackbits(d["cutmix"][j])[: 2 * 128 * 128].reshape(2, 1, 128, 128).astype(np.float32)).to(DEV)
        t_old = em.flat_params.detach().clone()
        r = st.step(xl, yl, xl1, yl1, xu, cm, int(cur))
        p1, p2 = r["parts1"].cpu(), r["parts2"].cpu()
        sup = 0.5 * float(p1[1]) + 0.5 * float(p1[2]) + 0.5 * float(p2[1]) + 0.5 * float(p2[2])
        rows.append([float(r["loss"]), sup, float(r["loss"]) - sup, float(p1[4]), float(r["contrast"]), float(p2[5]) if cur >= 1000 else 0.0])
        a = min(1.0 - 1.0 / (int(cur) + 1), 0.99)
        e_ema = max(e_ema, maxerr(em.flat_params, a * t_old + (1.0 - a) * m2.flat_params))
    rows, ref = np.array(rows), d[v + "losses"]
    e_logits = [maxerr(r[k][..., ::s, ::s].cpu(), torch.from_numpy(d[f"{v}{n}_s{s}"]))
                for k, n in (("logits1", "logits1_last"), ("logits2", "logits2_last"), ("t_logits", "t_logits_last"))]
    print(f"hpfg trace {variant}: loss rows |diff| max {np.abs(rows - ref).max():.2e} per column {np.abs(rows - ref).max(0)}; "
          f"last logits {e_logits}; teacher vs EMA law {e_ema:.2e}")
    assert np.abs(rows - ref).max() < 1e-3, (rows, ref)
    tol = 1e-3 if variant == "sgd" else 2e-2
    assert max(e_logits) < tol, e_logits
    assert all(torch.equal(t, m1.state_dict()[k]) for k, t in necks1.items())
    assert any(not torch.equal(t, m2.state_dict()[k]) for k, t in necks2.items())
    assert e_ema < 1e-6


def _loop_args(tmp, size, variant, **kw):
    class _Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(str(msg))

        warning = info

    a = AttrDict(dict(OPT[variant], model="segformer_plus", in_channels=1, num_classes=4, datasets="synthetic", batch_size=2, unlabel_batch_size=2,
                      train_crop_size=[size, size], test_crop_size=[size, size], synthetic_labeled=8, synthetic_unlabeled=12, synthetic_test_volumes=1,
                      device="cuda:0", consistency=0.1, consistency_rampup=200.0, ema_decay=0.99, save_path=str(tmp), logger=_Log()))
    a.update(kw)
    os.makedirs(os.path.join(str(tmp), "model"), exist_ok=True)
    for k in ("ema_model", "model1", "model2"):
        a[f"{k}_save_path"] = os.path.join(str(tmp), "model", f"{k}.pth")
    return a


def _hpfg_run(tmp, variant, graph):
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.train import HPFG
    a = _loop_args(tmp, 128, variant, total_itrs=3, step_size=3, hipgraph=graph, log_every=2)
    np.random.seed(3)
    m1, m2, em = _three(128)
    torch.manual_seed(11)
    lab, unl, test = build_loader(a)
    log = HPFG(m1, m2, em, lab, unl, test, a)
    torch.cuda.synchronize()
    return log.cpu(), [m.flat_params.detach().cpu().clone() for m in (m1, m2, em)], a


@pytest.mark.parametrize("variant", ["adamw", "sgd"])
def test_hpfg_loop_graphed_equals_eager_bitwise(tmp_path, variant):
    """The HPFG driver on three SegFormer_Plus networks: iteration 1 eager, the step captured at iteration 2, three replays, one evaluation of
    the three networks in between -- against the same loop launched eagerly, bit for bit (losses and every parameter of the three networks)."""
    lg, pg, a = _hpfg_run(tmp_path / "g", variant, True)
    le, pe, _ = _hpfg_run(tmp_path / "e", variant, False)
    assert not any("capture unavailable" in ln for ln in a.logger.lines), a.logger.lines
    assert lg.shape == (4,) and torch.isfinite(lg).all()
    assert torch.equal(lg, le), (lg, le)
    assert all(torch.equal(x, y) for x, y in zip(pg, pe))


def test_hpfg_from_the_yaml_runs_to_the_end(tmp_path):
    """config/hpfg_segformer_plus_30k_224x224_ACDC.yaml at its real batch (8 + 24 images of 224 x 224, AdamW + warm-up cosine) with total_itrs cut to
    one evaluation period."""
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.train import HPFG
    y = loadyaml(os.path.join(ROOT, "config", "hpfg_segformer_plus_30k_224x224_ACDC.yaml"))
    a = _loop_args(tmp_path, 224, "adamw")
    a.update({k: v for k, v in y.items() if k not in ("save_path",)})
    a.update(total_itrs=3, step_size=3, synthetic_labeled=16, synthetic_unlabeled=48)
    assert (a.batch_size, a.unlabel_batch_size, a.opt, a.model) == (8, 24, "adamW", "segformer_plus")
    torch.manual_seed(a.seed)
    m1, m2 = build_model(a).to(DEV), build_model(a).to(DEV)
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    lab, unl, test = build_loader(a)
    log = HPFG(m1, m2, em, lab, unl, test, a)
    assert log.shape == (a.total_itrs + 1,) and torch.isfinite(log).all(), log
    assert sum("_dice" in ln for ln in a.logger.lines) == 3, a.logger.lines          # one evaluation, three networks
    assert m1.training and m2.training and em.training


def test_mixed_pairs_and_data_parallel_are_refused():
    from hpfg_amd.model import UNet_Plus
    from hpfg_amd.train import HPFGStep
    m1, m2, em = _three(128)
    args = AttrDict(dict(OPT["sgd"], batch_size=2, unlabel_batch_size=2, total_itrs=30000, step_size=1500, consistency=0.1, consistency_rampup=200.0,
                         ema_decay=0.99))
    with pytest.raises(NotImplementedError, match="mixed"):
        HPFGStep(UNet_Plus(1, 4).to(DEV), m2, em, args)
    with pytest.raises(NotImplementedError, match="data parallel"):
        HPFGStep(m1, m2, em, args, dp=object())


def test_draws_are_consumed_in_the_order_model1_model2_teacher(golden_dir):
    """Without external draws the three networks take drop-path factors and Dropout2d masks from the torch device generator, which serves
    its sequence in host call order.  The reference's iteration calls model1, model2, then the teacher (main.py:152-160): (1) the forwards
    are entered in that order and each one advances the generator; (2) a step that draws for itself after a seed equals, bit for bit, a step
    on identical networks that replays draws taken from the same seed in that order."""
    from hpfg_amd.train import HPFGStep
    d = np.load(f"{golden_dir}/trace_hpfg_segformer_plus.npz")
    xl, yl, xl1, yl1, xu = (torch.from_numpy(d[k]).to(DEV) for k in ("xl", "yl", "xl1", "yl1", "xu"))
    cm = torch.from_numpy(np.unpackbits(d["cutmix"][0])[: 2 * 128 * 128].reshape(2, 1, 128, 128).astype(np.float32)).to(DEV)
    args = AttrDict(dict(OPT["sgd"], batch_size=2, unlabel_batch_size=2, total_itrs=30000, step_size=1500, consistency=0.1, consistency_rampup=200.0,
                         ema_decay=0.99))
    gen = torch.cuda.default_generators[0]

    def run(replay):
        nets = _three(128)
        st = HPFGStep(*nets, args)
        order, offsets = [], []

        def note(name):
            def hook(mod, inp):          # (returns None: the inputs pass unchanged)
                order.append(name)
                offsets.append(gen.get_offset())
            return hook

        hooks = [net.register_forward_pre_hook(note(name)) for name, net in zip(("model1", "model2", "teacher"), nets)]
        torch.manual_seed(4242)
        if replay:
            for net in nets:          # model1, model2, teacher: 14 drop-path draws, then the head's channel mask, each
                dp = [None, None] + [torch.rand((4, 1, 1), dtype=torch.float32, device=DEV) for _ in range(14)]
                net.external_draws = (dp, torch.empty(4, 256, 1, 1, device=DEV).bernoulli_(0.9))
        r = st.step(xl, yl, xl1, yl1, xu, cm, 1000)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        return order, offsets + [gen.get_offset()], [r[k].detach().clone() for k in ("loss", "logits1", "logits2", "t_logits")]

    order, offsets, live = run(False)
    assert order == ["model1", "model2", "teacher"], order
    assert all(b > a for a, b in zip(offsets, offsets[1:])), offsets          # every forward consumed draws of its own
    order_r, offsets_r, replayed = run(True)
    assert order_r == order and len(set(offsets_r)) == 1                     # (a replaying forward draws nothing)
    for a, b in zip(live, replayed):
        assert torch.equal(a, b)
