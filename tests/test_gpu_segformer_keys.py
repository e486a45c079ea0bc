"""SegFormer above 256 x 256: every attention of a 288 x 288 input has 81 keys (one full block of 64 and a ragged one, csrc/attn_keys.hip).
 * SegFormer-B0 and SegFormer_Plus-B1 against the reference's own numbers (tests/golden/segformer_b0_288.npz, segformer_plus_b1_288.npz:
   tools/make_golden_segformer_keys.py, which also pins oracle/segformer_ref.py to the reference at this size),
 * one CTCT step at 288 x 288 against the oracle on the host, and captured into a hipGraph against the eager step,
 * at 256 x 256 (64 keys) nothing moves: the <= 64-key op is the one called,
 * sizes whose stage maps exceed 256 keys are refused before any launch.
Bounds: those of tests/test_gpu_segformer.py / tests/test_gpu_segformer_plus.py for the same quantities."""
import numpy as np
import pytest
import torch

from hpfg_amd import ops_tokens
from hpfg_amd.model import SegFormer, SegFormer_Plus, UNet, reset_dropout_streams
from hpfg_amd.model import segformer as seg_mod
from hpfg_amd.utils import AttrDict, Med_Sup_Loss
from oracle import segformer_ref as S
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HW = 288


def _draws(dp_rows, mask_bits, B, dev="cpu"):
    """fixture arrays -> (drop_path_draws, dropout_mask) as external_draws takes them (the first block draws nothing)"""
    dp = [None, None] + [torch.from_numpy(r.copy()).reshape(B, 1, 1).to(dev) for r in dp_rows]
    mask = torch.from_numpy(np.unpackbits(mask_bits)[: B * 256].reshape(B, 256, 1, 1).astype(np.float32)).to(dev)
    return dp, mask


def _neck_functional(weights, outs):
    o, tot = 0, 0.0
    for t in outs:
        tot = tot + (weights[o:o + t.numel()].view(t.shape) * t).sum()
        o += t.numel()
    assert o == weights.numel()
    return tot


@pytest.mark.parametrize("plus", [False, True], ids=["B0", "Plus_B1"])
def test_fixture_parity_at_288(golden_dir, plus):
    d = np.load(f"{golden_dir}/{'segformer_plus_b1_288' if plus else 'segformer_b0_288'}.npz")
    s = int(d["logit_stride"])
    torch.manual_seed(1337)
    m = (SegFormer_Plus if plus else SegFormer)(image_size=[HW, HW], in_channels=1, num_classes=4).to(DEV)
    assert seg_mod.stage_keys(HW, HW) == [81] * 4
    x, y = torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["y"]).to(DEV)
    m.eval()
    with torch.no_grad():
        ev = m.val(x)
        assert ev.shape == (1, 4, HW, HW)
        e_ev = maxerr(ev[..., ::s, ::s].cpu(), torch.from_numpy(d[f"eval_logits_s{s}"]))
    m.train()
    m.external_draws = _draws(d["drop_path"], d["dropout_mask"], 1)
    res = m(x)
    out, necks = (res[0], (*res[1], *res[2])) if plus else (res, ())
    e_tr = maxerr(out.detach()[..., ::s, ::s].cpu(), torch.from_numpy(d[f"train_logits_s{s}"]))
    e_neck = [maxerr(t.detach().cpu(), torch.from_numpy(d[k])) for t, k in zip(necks, ("high_global", "high_dense", "head_global", "head_dense"))]
    loss = Med_Sup_Loss(4)(out, y)
    e_loss = abs(float(loss.detach()) - float(d["loss"]))
    print(f"288 fixture parity ({'Plus-B1' if plus else 'B0'}): eval logits {e_ev:.2e} train logits {e_tr:.2e} necks {max(e_neck, default=0.0):.2e} "
          f"loss {e_loss:.2e}")
    assert e_ev < 1e-3 and e_tr < 1e-3 and max(e_neck, default=0.0) < 1e-3
    assert e_loss < 1e-4
    total = loss + _neck_functional(torch.from_numpy(d["neck_weights"]).to(DEV), necks) if plus else loss
    total.backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = 0.0
    for k, g in grads.items():
        ref = d["g:" + k]
        got = np.array([float(g.sum()), float(g.abs().sum()), float(g.abs().max())])
        worst = max(worst, float(np.abs(got - ref).max() / max(1.0, float(np.abs(ref).max()))))
        assert np.abs(got - ref).max() < 2e-3 * max(1.0, float(np.abs(ref).max())), (k, got, ref)
    # the stored whole tensors: per-tensor relative L2 error, the bound of test_train_forward_backward_vs_oracle
    rel = {}
    for k in d["full_grads"]:
        ref = torch.from_numpy(d["grad:" + str(k)]).double()
        rel[str(k)] = float((grads[str(k)].cpu().double() - ref).norm() / max(1e-5, float(ref.norm())))
    print(f"288 fixture parity: worst gradient row error / max(1, |ref|) {worst:.2e} (< 2e-3); stored tensors rel-L2 max {max(rel.values()):.2e} (< 1e-2)")
    assert max(rel.values()) < 1e-2, rel


def _ctct(draws):
    from hpfg_amd.train import CTCTStep
    torch.manual_seed(1)
    reset_dropout_streams()
    m1, m2 = UNet(1, 4).to(DEV), SegFormer(image_size=[HW, HW], in_channels=1, num_classes=4).to(DEV)
    m1.train()
    m2.train()
    opt = dict(opt="sgd", lr=0.01, momentum=0.9, weight_decay=5e-4, sched="medical", total_itrs=30000, step_size=1500, warmup_epochs=1, warmup_lr=1e-4, min_lr=1e-6)
    a = AttrDict(dict(model1=AttrDict(opt), model2=AttrDict(dict(opt, opt="adamW", lr=0.0008, weight_decay=0.05)), consistency=0.1, consistency_rampup=200.0))
    m2.external_draws = draws
    return CTCTStep(m1, m2, a), m1, m2


def _ctct_batch():
    from hpfg_amd.datasets.synthetic import synth_batch
    xl, yl = synth_batch(31, 1, HW, HW, 1, 4, 32)
    xu, _ = synth_batch(32, 1, HW, HW, 1, 4, 32)
    return xl, yl, xu


def test_ctct_step_at_288_vs_oracle():
    """One CTCT iteration of U-Net + SegFormer-B0 on 1 labelled + 1 unlabelled 288 x 288 image against oracle.steps_ref.ctct_step, with the
    bounds of tests/test_gpu_segformer.py::test_ctct_step_full_size_vs_oracle."""
    from oracle import laws_ref, steps_ref
    from tests.helpers import engine_masks, state_from_module
    torch.manual_seed(77)
    draws = S.draw_randomness(2)
    st, m1, m2 = _ctct(draws)
    s1, s2 = state_from_module(m1), {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
    xl, yl, xu = _ctct_batch()
    w = 0.05
    r = st.step(xl.to(DEV), yl.to(DEV), xu.to(DEV), 1, cons_w=w)
    eng = next(iter(m1._engines.values()))[0]
    masks = engine_masks(eng, m1._seed_counter, 2, HW, HW)
    ro = steps_ref.ctct_step(s1, s2, {}, {}, xl, yl.long(), xu, laws_ref.medical_lr(1, 0.01, 30000), laws_ref.medical_lr(1, 0.0008, 30000), w, 0.9, 5e-4, 0.05,
                             masks, draws)
    p1, p2 = r["parts1"].cpu(), r["parts2"].cpu()
    got = [float(r["loss"]), 0.5 * float(p1[1]) + 0.5 * float(p1[2]), 0.5 * float(p2[1]) + 0.5 * float(p2[2]), float(p1[4]), float(p2[4])]
    ref = [ro["loss"], ro["sup1"], ro["sup2"], ro["ps1"], ro["ps2"]]
    e1, e2 = maxerr(r["logits1"].cpu(), ro["logits1"]), maxerr(r["logits2"].cpu(), ro["logits2"])
    print(f"CTCT step at 288: loss terms {max(abs(x - y) for x, y in zip(got, ref)):.2e} logits1 {e1:.2e} logits2 {e2:.2e} (< 1e-3 each)")
    assert max(abs(x - y) for x, y in zip(got, ref)) < 1e-3, (got, ref)
    assert e1 < 1e-3
    assert e2 < 1e-3
    m2.eval()
    with torch.no_grad():
        ev = m2(xl.to(DEV)).cpu()
        f2 = S.segformer_forward(s2, xl, False)
    assert maxerr(ev, f2) < 2e-2          # after one AdamW step: lr * sign(g) per element (see test_ctct_step_trace)


def test_ctct_step_at_288_graphed_equals_eager_bitwise():
    """attention_keys allocates its scratch by the size query and launches kernels only: the captured step replays the eager step's bits"""
    from hpfg_amd.train import GraphedStep
    torch.manual_seed(77)
    dp, mask = S.draw_randomness(2)
    draws = ([None if t is None else t.to(DEV) for t in dp], mask.to(DEV))          # device tensors: nothing to copy inside the capture
    inputs = [t.to(DEV) for t in _ctct_batch()]

    def run(graphed):
        st, _, _ = _ctct(draws)
        rows = []
        if graphed:
            g = GraphedStep(st, list(inputs), warmup=1, alias_inputs=True)          # (the warm-up is iteration 1, run eagerly)
            step = lambda k: g.step(list(inputs), k, cons_w=0.05)          # noqa: E731
        else:
            st.step(*inputs, 1)
            step = lambda k: st.step(*inputs, k, cons_w=0.05)          # noqa: E731
        for k in range(2, 5):
            r = step(k)
            rows.append(torch.cat([r["loss"].detach().reshape(1), r["parts1"].detach().reshape(-1), r["parts2"].detach().reshape(-1)]).clone())
        torch.cuda.synchronize()
        return torch.stack(rows).cpu()

    eager, graphed = run(False), run(True)
    assert torch.isfinite(eager).all() and float(eager[:, 0].min()) > 0.0
    assert torch.equal(eager, graphed), (eager, graphed)


def test_256_takes_the_64_key_path_and_keeps_its_bits(monkeypatch):
    """At 256 x 256 every stage has exactly 64 keys: attention_for must hand out the <= 64-key op, and the result must be the one of a
    dispatch that knows nothing else."""
    assert seg_mod.stage_keys(256, 256) == [64] * 4
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(1, 1, 256, 256, generator=g).to(DEV), torch.randint(0, 4, (1, 256, 256), generator=g).to(DEV)
    torch.manual_seed(7)
    draws = S.draw_randomness(1)
    real = ops_tokens.attention_for

    def run(dispatch):
        calls = []

        def counted(n_keys):
            fn = dispatch(n_keys)
            calls.append((n_keys, fn.__name__))
            return fn
        monkeypatch.setattr(seg_mod, "attention_for", counted)
        torch.manual_seed(5)
        m = SegFormer(image_size=[256, 256], in_channels=1, num_classes=4).to(DEV)
        m.train()
        m.external_draws = draws
        out = m(x)
        Med_Sup_Loss(4)(out, y).backward()
        return calls, [out.detach()] + [p.grad for p in m.parameters()]

    calls, got = run(real)
    assert len(calls) == 8 and all(c == (64, "attention") for c in calls), calls
    calls_old, want = run(lambda n_keys: ops_tokens.attention)
    assert len(calls_old) == 8
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_sizes_beyond_512_are_refused_before_any_launch():
    with pytest.raises(ValueError, match="512"):
        SegFormer(image_size=[544, 544], in_channels=1, num_classes=4)
    with pytest.raises(ValueError, match="512"):
        SegFormer_Plus(image_size=[544, 544], in_channels=1, num_classes=4)
    torch.manual_seed(0)
    m = SegFormer(image_size=[512, 512], in_channels=1, num_classes=4).to(DEV)          # 256 keys: the largest size served
    with pytest.raises(ValueError, match="512x512 limit"):
        m(torch.zeros(1, 1, 544, 544, device=DEV))
    p = SegFormer_Plus(image_size=[512, 512], in_channels=1, num_classes=4).to(DEV)
    with pytest.raises(ValueError, match="512x512 limit"):
        p(torch.zeros(1, 1, 512, 576, device=DEV))
