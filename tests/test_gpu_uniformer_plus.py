"""Uniformer_Plus (UniFormer-S + SegFormerHead + the projection necks) against the reference's own numbers: tests/golden/uniformer_plus.npz
(tools/make_golden_uniformer.py), at 128 x 128 (both attention stages at most 64 keys) and 160 x 160 (stage 3: 100 keys, the key-block
kernels), with the recorded drop-path draws and Dropout2d mask replayed through ``external_draws``.  Tolerances are those of
tests/test_gpu_segformer_plus.py for the same quantities: 1e-3 on logits and neck outputs, 1e-4 on the loss, 2e-3 x max(1, |ref|) on the
(sum, abs-sum, abs-max) row of every parameter gradient; the fully recorded gradients get the same relative bound on their largest entry.
The HPFG step on three of them is held against iterations 999, 1000, 1001 of the reference's loop body (trace_hpfg_uniformer_plus.npz, same tool),
and the order in which the three forwards consume the device generator's draws against the reference's call order.
Logit tensors of the fixtures are stored on a pixel stride (``logit_stride``)."""
import numpy as np
import pytest
import torch

from hpfg_amd import ops_tokens
from hpfg_amd.model import build_model
from hpfg_amd.utils import AttrDict, Med_Sup_Loss
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NECK_KEYS = ("high_global", "high_dense", "head_global", "head_dense")


def _draws(dp_rows, mask_bits, B):
    """fixture arrays -> (drop_path_draws, dropout_mask) as Uniformer_Plus.external_draws takes them (the first block draws nothing)"""
    dp = [None, None] + [torch.from_numpy(r.copy()).reshape(B, 1, 1) for r in dp_rows]
    mask = torch.from_numpy(np.unpackbits(mask_bits)[: B * 256].reshape(B, 256, 1, 1).astype(np.float32))
    return dp, mask


def _neck_functional(weights, outs):
    o, tot = 0, 0.0
    for t in outs:
        tot = tot + (weights[o:o + t.numel()].view(t.shape) * t).sum()
        o += t.numel()
    assert o == weights.numel()
    return tot


def _model(d, side):
    torch.manual_seed(int(d["seed"]))
    return build_model(AttrDict(model="uniformer_plus", in_channels=1, num_classes=4, train_crop_size=[side, side])).to(DEV)


@pytest.mark.parametrize("math", ["bf16x3", "f32"])
@pytest.mark.parametrize("side", [128, 160])
def test_golden_fixture_parity(golden_dir, side, math, monkeypatch):
    monkeypatch.setitem(ops_tokens.MATH, "mode", math)
    d = np.load(f"{golden_dir}/uniformer_plus.npz")
    s, t = int(d["logit_stride"]), f"@{side}"
    m = _model(d, side)
    x, y = torch.from_numpy(d["x" + t]).to(DEV), torch.from_numpy(d["y" + t]).to(DEV)
    m.eval()
    with torch.no_grad():
        ev = m.val(x)
        assert ev.shape == (2, 4, side, side)
        assert torch.equal(ev, m(x)[0])                          # val() is forward()[0]
        e_ev = maxerr(ev[..., ::s, ::s].cpu(), torch.from_numpy(d[f"eval_logits_s{s}" + t]))
    assert int(m.encoder.norm1.num_batches_tracked) == 0         # eval mode left the running statistics alone
    m.train()
    m.external_draws = _draws(d["drop_path" + t], d["dropout_mask" + t], 2)
    out, high, head = m(x)
    assert [tuple(v.shape) for v in (*high, *head)] == [(2, 128), (2, 128, 16), (2, 128), (2, 128, 16)]
    e_tr = maxerr(out.detach()[..., ::s, ::s].cpu(), torch.from_numpy(d[f"train_logits_s{s}" + t]))
    e_neck = [maxerr(v.detach().cpu(), torch.from_numpy(d[k + t])) for v, k in zip((*high, *head), NECK_KEYS)]
    loss = Med_Sup_Loss(4)(out, y)
    e_loss = abs(float(loss.detach()) - float(d["loss" + t]))
    e_rm = maxerr(m.encoder.norm1.running_mean.cpu(), torch.from_numpy(d["norm1_running_mean" + t]))
    e_rv = maxerr(m.encoder.norm1.running_var.cpu(), torch.from_numpy(d["norm1_running_var" + t]))
    print(f"fixture parity {side} {math}: eval logits {e_ev:.2e} train logits {e_tr:.2e} necks {max(e_neck):.2e} loss {e_loss:.2e} "
          f"running mean {e_rm:.2e} var {e_rv:.2e}")
    assert e_ev < 1e-3 and e_tr < 1e-3 and max(e_neck) < 1e-3
    assert e_loss < 1e-4
    assert e_rm < 1e-4 and e_rv < 1e-4 and int(m.encoder.norm1.num_batches_tracked) == 1
    (loss + _neck_functional(torch.from_numpy(d["neck_weights" + t]).to(DEV), (*high, *head))).backward()
    worst = 0.0
    for (k, p), ref in zip(m.named_parameters(), d["gsum" + t]):
        got = np.array([float(p.grad.sum()), float(p.grad.abs().sum()), float(p.grad.abs().max())])
        worst = max(worst, float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max()))))
        assert np.abs(got - ref).max() < 2e-3 * max(1.0, float(np.abs(ref).max())), (k, got, ref)
    params = dict(m.named_parameters())
    worst_full = 0.0
    for key in d.files:
        if key.startswith("grad:") and key.endswith(t):
            ref = torch.from_numpy(d[key])
            e = maxerr(params[key[5:-len(t)]].grad.cpu(), ref) / max(1.0, float(ref.abs().max()))
            worst_full = max(worst_full, e)
            assert e < 2e-3, (key, e)
    print(f"fixture parity {side} {math}: worst gradient row error / max(1, |ref|) {worst:.2e}, worst recorded gradient {worst_full:.2e} (< 2e-3)")


def test_train_forward_is_bit_reproducible_and_skip_necks(golden_dir):
    d = np.load(f"{golden_dir}/uniformer_plus.npz")
    m = _model(d, 128)
    x = torch.from_numpy(d["x@128"]).to(DEV)
    m.train()
    m.external_draws = _draws(d["drop_path@128"], d["dropout_mask@128"], 2)
    a, high, _ = m(x)
    m.skip_necks = True
    b, h2, h3 = m(x)
    assert h2 is None and h3 is None and high is not None
    assert torch.equal(a, b)                                     # train-mode BatchNorm uses the batch statistics: the same bits twice


def test_own_draws_come_from_the_device_generator(golden_dir):
    d = np.load(f"{golden_dir}/uniformer_plus.npz")
    m = _model(d, 128)
    x = torch.from_numpy(d["x@128"]).to(DEV)
    m.train()
    torch.manual_seed(5)
    a = m.val(x)
    torch.manual_seed(5)
    b = m.val(x)
    c = m.val(x)
    assert torch.equal(a, b) and not torch.equal(a, c) and bool(torch.isfinite(c).all())
    m.eval()
    state = torch.cuda.get_rng_state(DEV)
    with torch.no_grad():
        m.val(x)
    assert torch.equal(state, torch.cuda.get_rng_state(DEV))     # eval mode draws nothing


def test_wrong_input_size_raises_before_any_launch():
    m = build_model(AttrDict(model="uniformer_plus", in_channels=1, num_classes=4, train_crop_size=[128, 128])).to(DEV)
    with pytest.raises(ValueError, match="built for 128"):
        m(torch.zeros(1, 1, 160, 160, device=DEV))
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(1, 1, 128, 96, device=DEV))


# ---- the HPFG step on three Uniformer_Plus ---------------------------------------------------------------------------------------------------
OPT = {"sgd": dict(opt="sgd", lr=0.01, momentum=0.9, weight_decay=1e-4, sched="medical", warmup_epochs=0, warmup_lr=1e-4, min_lr=1e-6),
       "adamw": dict(opt="adamW", lr=1e-3, momentum=0.9, weight_decay=0.05, sched="cosine", warmup_epochs=1, warmup_lr=1e-5, min_lr=1e-6)}


def _three(size):
    from copy import deepcopy
    from hpfg_amd.model import Uniformer_Plus
    torch.manual_seed(1337)
    m1 = Uniformer_Plus(image_size=[size, size], in_channels=1, num_classes=4).to(DEV)
    m2 = Uniformer_Plus(image_size=[size, size], in_channels=1, num_classes=4).to(DEV)      # continues the generator, as in the driver
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    for m in (m1, m2, em):
        m.train()
    return m1, m2, em


def _loop_args(tmp, size, variant, **kw):
    import os

    class _Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(str(msg))

        warning = info

    a = AttrDict(dict(OPT[variant], model="uniformer_plus", in_channels=1, num_classes=4, datasets="synthetic", batch_size=2, unlabel_batch_size=2,
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
    return log.cpu(), [m.flat_params.detach().cpu().clone() for m in (m1, m2, em)], a, (m1, m2, em)


def test_hpfg_loop_graphed_equals_eager_bitwise(tmp_path):
    """The HPFG driver on three Uniformer_Plus networks (AdamW + warm-up cosine, the config's recipe): iteration 1 eager, the step captured at
    iteration 2, replays, one evaluation of the three networks -- against the same loop launched eagerly, bit for bit (losses, every parameter
    and every BatchNorm running statistic of the three networks)."""
    lg, pg, a, ng = _hpfg_run(tmp_path / "g", "adamw", True)
    le, pe, _, ne = _hpfg_run(tmp_path / "e", "adamw", False)
    assert not any("capture unavailable" in ln for ln in a.logger.lines), a.logger.lines
    assert lg.shape == (4,) and torch.isfinite(lg).all()
    assert torch.equal(lg, le), (lg, le)
    assert all(torch.equal(x, y) for x, y in zip(pg, pe))
    for mg, me in zip(ng, ne):
        bg, be = dict(mg.named_buffers()), dict(me.named_buffers())
        assert all(torch.equal(bg[k], be[k]) for k in bg)
    assert int(ng[1].encoder.norm1.num_batches_tracked) >= 3
    assert ng[0].skip_necks and not ng[1].skip_necks


def test_hpfg_from_the_yaml_runs_to_the_end(tmp_path):
    """config/hpfg_uniformer_plus_30k_224x224_ACDC.yaml at its real batch (8 + 24 images of 224 x 224, AdamW + warm-up cosine) with total_itrs cut
    to one evaluation period."""
    import os
    from copy import deepcopy
    from hpfg_amd.datasets import build_loader
    from hpfg_amd.train import HPFG
    from hpfg_amd.utils import loadyaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    y = loadyaml(os.path.join(root, "config", "hpfg_uniformer_plus_30k_224x224_ACDC.yaml"))
    a = _loop_args(tmp_path, 224, "adamw")
    a.update({k: v for k, v in y.items() if k not in ("save_path",)})
    a.update(total_itrs=3, step_size=3, synthetic_labeled=16, synthetic_unlabeled=48)
    assert (a.batch_size, a.unlabel_batch_size, a.opt, a.model, a.lr) == (8, 24, "adamW", "uniformer_plus", 0.001)
    torch.manual_seed(a.seed)
    m1, m2 = build_model(a).to(DEV), build_model(a).to(DEV)
    em = deepcopy(m2)
    for p in em.parameters():
        p.requires_grad = False
    lab, unl, test = build_loader(a)
    log = HPFG(m1, m2, em, lab, unl, test, a)
    assert log.shape == (a.total_itrs + 1,) and torch.isfinite(log).all(), log
    assert not any("capture unavailable" in ln for ln in a.logger.lines), a.logger.lines
    assert sum("_dice" in ln for ln in a.logger.lines) == 3, a.logger.lines          # one evaluation, three networks
    assert m1.training and m2.training and em.training


def test_mixed_kinds_and_data_parallel_are_refused():
    from hpfg_amd.model import SegFormer_Plus, UNet_Plus
    from hpfg_amd.train import HPFGStep
    m1, m2, em = _three(128)
    args = AttrDict(dict(OPT["sgd"], batch_size=2, unlabel_batch_size=2, total_itrs=30000, step_size=1500, consistency=0.1, consistency_rampup=200.0,
                         ema_decay=0.99))
    with pytest.raises(NotImplementedError, match="mixed .*Uniformer_Plus"):
        HPFGStep(UNet_Plus(1, 4).to(DEV), m2, em, args)
    with pytest.raises(NotImplementedError, match="mixed .*Uniformer_Plus"):
        HPFGStep(m1, SegFormer_Plus(image_size=[128, 128], in_channels=1, num_classes=4).to(DEV), em, args)
    with pytest.raises(NotImplementedError, match="data parallel.*Uniformer_Plus"):
        HPFGStep(m1, m2, em, args, dp=object())


NECKS = ("dense_projection_high", "dense_projection_head")


@pytest.mark.parametrize("variant", ["sgd", "adamw"])
def test_hpfg_step_trace(golden_dir, variant):
    """HPFGStep on three Uniformer_Plus networks against iterations 999, 1000, 1001 of the reference's loop body (its own modules and
    optimizers; tools/make_golden_uniformer.py), 2 + 2 images of 128 x 128, with the bounds tests/test_gpu_segformer_plus.py uses for the same
    quantities: every loss row to 1e-3; the last iteration's logits of the two students and the teacher to 1e-3 after SGD steps and to 2e-2
    after AdamW steps (Adam's update is lr * sign(g) wherever a gradient is at rounding level).  The learning rates are the reference's; the
    first student's necks are never computed, so their parameters do not move by a bit; the teacher follows the EMA law of the second student;
    every network's BatchNorm layers counted the reference's number of batches."""
    from hpfg_amd.train import HPFGStep
    from hpfg_amd.utils.optim import FusedAdamW, FusedSGD
    d = np.load(f"{golden_dir}/trace_hpfg_uniformer_plus.npz")
    v, s = variant + "_", int(d["logit_stride"])
    m1, m2, em = _three(128)
    args = AttrDict(dict(OPT[variant], batch_size=2, unlabel_batch_size=2, total_itrs=30000, step_size=1500, consistency=0.1, consistency_rampup=200.0,
                         ema_decay=0.99))
    st = HPFGStep(m1, m2, em, args)
    assert isinstance(st.optimizer1, FusedSGD if variant == "sgd" else FusedAdamW) and st.optimizer1.active_numel == m1.backbone_numel() == 21558084
    assert st.optimizer2.active_numel is None and st.reference_call_order
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
        assert abs(float(st.optimizer2.param_groups[0]["lr"]) - float(d[v + "lrs"][j, 1])) < 1e-12
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
    assert [int(m.encoder.norm1.num_batches_tracked) for m in (m1, m2, em)] == d[v + "bn_batches"].tolist()


def test_draws_are_consumed_in_the_order_model1_model2_teacher(golden_dir):
    """Without external draws the three networks take drop-path factors and Dropout2d masks from the torch device generator, which serves
    its sequence in host call order.  The reference's iteration calls model1, model2, then the teacher (main.py:152-160): (1) the forwards
    are entered in that order and each one advances the generator; (2) a step that draws for itself after a seed equals, bit for bit, a step
    on identical networks that replays draws taken from the same seed in that order (34 drop-path draws, then the head's mask, each)."""
    from hpfg_amd.train import HPFGStep
    d = np.load(f"{golden_dir}/trace_hpfg_uniformer_plus.npz")
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
            for net in nets:
                dp = [None, None] + [torch.rand((4, 1, 1), dtype=torch.float32, device=DEV) for _ in range(34)]
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


def test_eval_mode_forward_carries_gradients(golden_dir):
    """m.eval(); m(x) without no_grad: the same logits as under no_grad, a finite gradient in every backbone parameter, running statistics
    untouched (the reference allows an eval-mode forward with gradients)."""
    d = np.load(f"{golden_dir}/uniformer_plus.npz")
    m = _model(d, 128)
    x = torch.from_numpy(d["x@128"]).to(DEV)
    m.eval()
    with torch.no_grad():
        ref = m.val(x)
    out = m(x)[0]
    assert torch.equal(out.detach(), ref)
    out.square().mean().backward()
    grads = [p.grad for part in (m.encoder, m.decoder) for p in part.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert float(m.encoder.blocks1[0].norm1.weight.grad.abs().max()) > 0.0 and float(m.encoder.norm4.bias.grad.abs().max()) > 0.0
    assert int(m.encoder.norm1.num_batches_tracked) == 0
