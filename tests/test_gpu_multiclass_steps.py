"""GPU: the U-Net step laws at nine classes (the reference's Synapse configs).  SupervisedStep and ICTStep against traces of the
reference's own modules at UNet(1, 9) (tests/golden/trace_sup_c9.npz, trace_ict_c9.npz; tools/make_golden_multiclass.py), Mean-Teacher and
CPS captured into a hipGraph against their eager runs, and the evaluation path at nine classes against the oracle."""
import os
from copy import deepcopy

import numpy as np
import pytest
import torch

from hpfg_amd import engine as E
from hpfg_amd import val as V
from hpfg_amd.datasets.synthetic import synth_batch
from hpfg_amd.model import UNet, reset_dropout_streams
from hpfg_amd.train import CPSStep, GraphedStep, ICTStep, MeanTeacherStep, SupervisedStep
from hpfg_amd.utils import AttrDict
from oracle import eval_ref, laws_ref, steps_ref, unet_ref
from tests import trace_replay as R
from tests.helpers import maxerr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-3
NCLS = 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _opt_args(**kw):
    base = dict(opt="sgd", lr=0.01, momentum=0.9, weight_decay=1e-4, sched="medical", total_itrs=30000, step_size=200, warmup_epochs=0,
                warmup_lr=1e-4, min_lr=1e-6, consistency=0.1, consistency_rampup=200.0, ema_decay=0.99)
    base.update(kw)
    return AttrDict(base)


def _masks(d, key, n, hw):
    out = {}
    for lvl in range(5):
        c, h = E.WIDTHS[lvl], hw >> lvl
        bits = np.unpackbits(d[f"{key}{lvl}"])[: n * c * h * h].reshape(n, c, h, h)
        out[E.enc_prefix(lvl) + ".0"] = torch.from_numpy(bits).permute(0, 2, 3, 1).contiguous().to(DEV)
    return out


# ---- oracle replays of the two nine-class traces (tests/trace_replay.py's replay_sup / replay_ict hold four classes) -------------------
def replay_sup_c9(d, seed=None):
    st, bufs = R.perturb(unet_ref.init_state(1337, 1, NCLS), seed), {}
    table = laws_ref.cosine_table(0.01, 0, 1e-4, 1e-6, 200, 150)
    x, lab = torch.from_numpy(d["x"]), torch.from_numpy(d["labels"]).long()
    losses = [steps_ref.supervised_step(st, bufs, x, lab, laws_ref.cosine_lr(k + 1, table), 0.9, 5e-4, R.unpack_masks(d, f"it{k}_mask", 2, 32))["loss"]
              for k in range(4)]
    with torch.no_grad():
        fin = unet_ref.unet_forward(st, x, train=False)
    return {"losses": np.array(losses), "final_eval_logits": fin}


def replay_ict_c9(d, seed=None):
    st = R.perturb(unet_ref.init_state(1337, 1, NCLS), seed)
    ema, bufs = unet_ref.clone_state(st), {}
    xl, yl, xu = torch.from_numpy(d["xl"]), torch.from_numpy(d["yl"]).long(), torch.from_numpy(d["xu"])
    rows = []
    for k in range(3):
        r = steps_ref.ict_step(st, ema, bufs, xl, yl, xu, torch.from_numpy(d["mixes"][k]), laws_ref.medical_lr(k + 1, 0.01, 30000), float(d["cons_w"]),
                               laws_ref.ema_alpha(k + 1, 0.99), 0.9, 1e-4, R.unpack_masks(d, f"it{k}_s", 4, 32), R.unpack_masks(d, f"it{k}_a", 2, 32),
                               R.unpack_masks(d, f"it{k}_b", 2, 32))
        rows.append([r["loss"], r["sup"], r["cons"]])
    return {"losses": np.array(rows), "student_logits_last": r["logits"]}


_DRIFT = {}


def logit_tol(math, trace, replay, keys):
    """1e-3 in f32; in bf16x3 1e-3 + 2 x the drift of the oracle with emulated split-bf16 products on this trace (as tests/test_gpu_steps.py)."""
    if math == "f32":
        return TOL
    if trace not in _DRIFT:
        d = np.load(os.path.join(GOLDEN, f"trace_{trace}.npz"))
        _DRIFT[trace] = R.emulation_drift(replay, d, list(keys))[0]
    return TOL + 2.0 * _DRIFT[trace]


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
def test_supervised_trace_nine_classes(golden_dir, math):
    d = np.load(f"{golden_dir}/trace_sup_c9.npz")
    torch.manual_seed(1337)
    m = UNet(1, NCLS).to(DEV)
    m.math = math
    m.train()
    st = SupervisedStep(m, _opt_args(weight_decay=5e-4, sched="cosine"))
    x, lab = torch.from_numpy(d["x"]).to(DEV), torch.from_numpy(d["labels"]).to(DEV)
    losses = []
    for k in range(4):
        m.external_dropout_masks = _masks(d, f"it{k}_mask", 2, 32)
        losses.append(st.step(x, lab, k + 1)["loss"])
    losses = torch.stack(losses).cpu().numpy()
    print("sup c9 losses", losses, d["losses"])
    assert np.abs(losses - d["losses"]).max() < TOL, (losses, d["losses"])
    m.eval()
    with torch.no_grad():
        fin = m(x).cpu()
    tol = logit_tol(math, "sup_c9", replay_sup_c9, ["final_eval_logits"])
    err = maxerr(fin, torch.from_numpy(d["final_eval_logits"]))
    print(f"sup c9 {math}: final logits err {err:.3e} (bound {tol:.3e})")
    assert err < tol


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
def test_ict_trace_nine_classes(golden_dir, math):
    d = np.load(f"{golden_dir}/trace_ict_c9.npz")
    torch.manual_seed(1337)
    m = UNet(1, NCLS).to(DEV)
    m.math = math
    ema = deepcopy(m)
    for p in ema.parameters():
        p.requires_grad = False
    m.train()
    ema.train()
    st = ICTStep(m, ema, _opt_args())
    xl, yl, xu = (torch.from_numpy(d[k]).to(DEV) for k in ("xl", "yl", "xu"))
    rows = []
    for k in range(3):
        m.external_dropout_masks = _masks(d, f"it{k}_s", 4, 32)
        ema.external_dropout_masks = [_masks(d, f"it{k}_a", 2, 32), _masks(d, f"it{k}_b", 2, 32)]      # teacher forwards on u0, then u1
        ema._ext_mask_idx = 0
        r = st.step(xl, yl, xu, k + 1, mix_factors=torch.from_numpy(d["mixes"][k]), cons_w=float(d["cons_w"]))
        p = r["parts"].cpu()
        rows.append([float(r["loss"]), 0.5 * float(p[1]) + 0.5 * float(p[2]), float(p[5])])
    print("ict c9 rows", rows, d["losses"])
    assert np.abs(np.array(rows) - d["losses"]).max() < TOL, (rows, d["losses"])
    tol = logit_tol(math, "ict_c9", replay_ict_c9, ["student_logits_last"])
    err = maxerr(r["logits"].cpu(), torch.from_numpy(d["student_logits_last"]))
    print(f"ict c9 {math}: student logits err {err:.3e} (bound {tol:.3e})")
    assert err < tol
    assert maxerr(r["t_prob"].cpu(), torch.from_numpy(d["target_last"])) < TOL


# ---- captured vs eager ------------------------------------------------------------------------------------------------------------------
def _batch():
    xl, yl = synth_batch(41, 2, 32, 32, 1, NCLS, 8)
    xu, _ = synth_batch(42, 2, 32, 32, 1, NCLS, 8)
    return xl.to(DEV), yl.to(DEV), xu.to(DEV)


def _mt():
    torch.manual_seed(3)
    reset_dropout_streams()
    m = UNet(1, NCLS).to(DEV)
    ema = deepcopy(m)
    for p in ema.parameters():
        p.requires_grad = False
    m.train()
    ema.train()
    return MeanTeacherStep(m, ema, _opt_args()), [m, ema]


def _cps():
    torch.manual_seed(3)
    reset_dropout_streams()
    m1, m2 = UNet(1, NCLS).to(DEV), UNet(1, NCLS).to(DEV)
    m1.train()
    m2.train()
    args = _opt_args()
    args.model1, args.model2 = _opt_args(), _opt_args()
    return CPSStep(m1, m2, args), [m1, m2]


def _run(make, graphed, inputs, iters=3, w=0.05):
    st, nets = make()
    losses = []
    if graphed:
        g = GraphedStep(st, list(inputs), warmup=1, alias_inputs=True)          # (the warm-up is iteration 1, run eagerly)
        for k in range(2, iters + 1):
            losses.append(g.step(list(inputs), k, cons_w=w)["loss"].clone())
    else:
        st.step(*inputs, 1)
        for k in range(2, iters + 1):
            losses.append(st.step(*inputs, k, cons_w=w)["loss"].clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), [n_.flat_params.detach().cpu().clone() for n_ in nets]


@pytest.mark.parametrize("make", [_mt, _cps], ids=["mean_teacher", "cps"])
def test_captured_step_equals_eager_nine_classes(make):
    inputs = _batch()
    le, pe = _run(make, False, inputs)
    lg, pg = _run(make, True, inputs)
    assert torch.isfinite(le).all() and float(le.min()) > 0.0
    assert torch.equal(le, lg), (le, lg)                          # the captured step replays the 104-float loss buffers: same bits as eager
    lg2, pg2 = _run(make, True, inputs)
    assert torch.equal(lg, lg2)
    assert all(torch.equal(a, b) for a, b in zip(pg, pg2))        # the captured run twice from the same state: bit-equal parameters
    assert all(maxerr(a, b) < 1e-6 for a, b in zip(pe, pg))


# ---- evaluation -----------------------------------------------------------------------------------------------------------------------
def test_single_volume_nine_classes_matches_oracle():
    torch.manual_seed(5)
    m = UNet(1, NCLS).to(DEV)
    m.math = "f32"
    m.train()
    with torch.no_grad():
        for k in range(3):
            m(torch.randn(8, 1, 32, 32, device=DEV) * (1 + k))
    g = np.random.default_rng(3)
    s, h, w = 7, 40, 36
    coarse = g.integers(0, NCLS, (s, 5, 5))
    lab = np.kron(coarse, np.ones((h // 5 + 1, w // 5 + 1), dtype=np.int64))[:, :h, :w].astype(np.uint8)
    img = (lab / (NCLS - 1) + 0.1 * g.standard_normal((s, h, w))).astype(np.float32)
    got = V.test_single_volume(torch.from_numpy(img)[None], torch.from_numpy(lab)[None], m, classes=NCLS, patch_size=(32, 32))
    state = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref_dice, ref_pred = eval_ref.test_single_volume(img, lab, state, NCLS, (32, 32))
    pred = V.predict_volume(torch.from_numpy(img), m, (32, 32)).cpu().numpy()
    assert len(got) == NCLS - 1
    assert (pred != ref_pred).mean() < 2e-3
    for (d, hd), r in zip(got, ref_dice):
        assert abs(d - r) < 1e-3 and hd == 0.0
