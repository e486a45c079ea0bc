"""CPU: host-side logic of the product (config, factories, schedulers, ramp-ups, CutMix masks, synthetic data, module plumbing,
dropout RNG law) against the oracle / the reference's recorded behaviour.  No GPU, no HIP compute calls."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from hpfg_amd.datasets import build_loader
from hpfg_amd.datasets.synthetic import synth_batch
from hpfg_amd.model import UNet, UNet_Plus, build_model
from hpfg_amd.utils import (AttrDict, BoxMaskGenerator, CosineWarmupLR_Scheduler, Medical_LR, build_lr_scheduler, ema_alpha,
                            get_current_consistency_weight, linear_rampup, loadyaml, sigmoid_rampup)
from oracle import laws_ref, rng_ref, unet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_yaml_configs_parse_with_reference_keys():
    for name in os.listdir(os.path.join(ROOT, "config")):
        a = loadyaml(os.path.join(ROOT, "config", name))
        for k in ("datasets", "num_classes", "train_crop_size", "batch_size", "seed", "total_itrs", "step_size"):
            assert k in a, (name, k)
        assert a.ckpt == "None"            # YAML `ckpt: None` is the STRING "None", as in the reference
        if "model1" in a:
            assert a.model1.opt == "sgd" and isinstance(a.model1, AttrDict)


def test_build_model_keys_and_state_dict_layout():
    torch.manual_seed(1)
    m = build_model(AttrDict(model="unet", in_channels=1, num_classes=4))
    st = unet_ref.init_state(1, 1, 4)
    sd = m.state_dict()
    assert list(sd.keys()) == list(st.keys()) and len(sd) == 136 and len(list(m.parameters())) == 82
    assert all(torch.equal(sd[k], st[k]) for k in st)           # same RNG consumption as the reference constructor
    torch.manual_seed(1)
    mp = build_model(AttrDict(model="unet_plus", in_channels=1, num_classes=4))
    stp = unet_ref.init_state(1, 1, 4, True)
    assert list(mp.state_dict().keys()) == list(stp.keys()) and len(stp) == 152 and len(list(mp.parameters())) == 98
    assert all(torch.equal(mp.state_dict()[k], stp[k]) for k in stp)
    assert hasattr(mp, "encoder") and hasattr(mp, "decoder") and callable(mp.val)
    with pytest.raises(NotImplementedError):
        build_model(AttrDict(model="swinunet", in_channels=1, num_classes=4, train_crop_size=[224, 224]))


def test_flat_parameter_views_deepcopy_and_state_dict_roundtrip():
    torch.manual_seed(3)
    m = UNet(1, 4)
    assert m._is_flat() and m.flat_params.numel() == 1813764 == m.backbone_numel()
    e = copy.deepcopy(m)
    assert e._is_flat() and e.flat_params.data_ptr() != m.flat_params.data_ptr()
    assert torch.equal(e.flat_params, m.flat_params)
    with torch.no_grad():
        m.flat_params.mul_(0.5)
    p = next(m.parameters())
    assert torch.equal(p.detach().reshape(-1), m.flat_params[: p.numel()])          # parameters are views of the flat buffer
    e.load_state_dict(m.state_dict())
    assert e._is_flat() and torch.equal(e.flat_params, m.flat_params)
    mp = UNet_Plus(1, 4)
    assert mp.backbone_numel() == 1813764 and mp.flat_params.numel() == 3663620


def test_cpu_input_is_refused_loudly():
    m = UNet(1, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 1, 32, 32))


def test_schedulers_reproduce_reference_quirks(golden_dir):
    a = json.load(open(f"{golden_dir}/anchors.json"))
    lin = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(lin.parameters(), lr=0.01, momentum=0.9)
    sch = Medical_LR(opt, 0.01, 30000)
    got = []
    for _ in range(6):
        got.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert np.allclose(got, a["medical_lr_first6"], rtol=0, atol=1e-12) and got[0] > 0.01
    opt = torch.optim.SGD(lin.parameters(), lr=0.01, momentum=0.9)
    args = AttrDict(sched="cosine", lr=0.01, warmup_epochs=0, warmup_lr=1e-4, min_lr=1e-6, step_size=200, total_itrs=30000)
    sch = build_lr_scheduler(args, opt)
    assert isinstance(sch, CosineWarmupLR_Scheduler)
    got = []
    for _ in range(6):
        got.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert np.allclose(got, a["cosine_lr_first6"], rtol=0, atol=1e-12)


def test_rampups_ema_alpha_and_box_masks(golden_dir):
    for e in (0, 1, 50, 199, 200, 500):
        assert sigmoid_rampup(e, 200.0) == laws_ref.sigmoid_rampup(e, 200.0)
        assert linear_rampup(e, 200.0) == laws_ref.linear_rampup(e, 200.0)
    assert get_current_consistency_weight(40, AttrDict(consistency=0.1, consistency_rampup=200.0)) == 0.1 * laws_ref.sigmoid_rampup(40, 200.0)
    assert [ema_alpha(s, 0.99) for s in (1, 2, 3, 200)] == [laws_ref.ema_alpha(s, 0.99) for s in (1, 2, 3, 200)]
    d = np.load(f"{golden_dir}/box_masks.npz")
    ref = np.unpackbits(d["masks"])[: int(np.prod(d["shape"]))].reshape(d["shape"])
    gen = BoxMaskGenerator(prop_range=(0.25, 0.5), n_boxes=4, random_aspect_ratio=True, prop_by_area=True, within_bounds=True, invert=True)
    np.random.seed(1)
    got = gen.generate_params(5, (64, 64))
    assert got.shape == (5, 1, 64, 64) and np.array_equal(got.astype(np.uint8), ref)       # the reference's own masks (fixture)


def test_synthetic_loaders_keep_the_batch_contract():
    a = AttrDict(datasets="synthetic", num_classes=4, train_crop_size=[64, 64], batch_size=2, unlabel_batch_size=4, in_channels=1,
                 synthetic_labeled=8, synthetic_unlabeled=16)
    lab, unl, test = build_loader(a)
    x, y = next(iter(lab))
    assert x.shape == (2, 1, 64, 64) and x.dtype == torch.float32 and y.shape == (2, 64, 64) and y.dtype == torch.uint8
    xu, _ = next(iter(unl))
    assert xu.shape == (4, 1, 64, 64) and len(unl) == 4 and len(lab.dataset) == 8
    v, l = next(iter(test))
    assert v.dim() == 4 and v.shape[0] == 1 and l.shape == v.shape
    a2 = AttrDict(datasets="sup_synthetic", num_classes=4, train_crop_size=[32, 32], batch_size=8, in_channels=1)
    tr, te = build_loader(a2)
    assert next(iter(tr))[0].shape == (8, 1, 32, 32)
    with pytest.raises(NotImplementedError):
        build_loader(AttrDict(datasets="lidc"))          # real-data keys outside the hot-path build raise like an unknown key (builder.py:76-77)
    with pytest.raises(NotImplementedError):
        build_loader(AttrDict(datasets="no-such-dataset"))
    x1, y1 = synth_batch(5, 2, 32, 32, 3, 2, 8)
    x2, y2 = synth_batch(5, 2, 32, 32, 3, 2, 8)
    assert torch.equal(x1, x2) and torch.equal(y1, y2) and x1.shape == (2, 3, 32, 32) and int(y1.max()) <= 1


def test_dropout_rng_law_statistics_and_determinism():
    for p in (0.05, 0.1, 0.2, 0.3, 0.5):
        m = rng_ref.keep_mask_nhwc(400000, p, 12345)
        assert abs((1 - m.mean()) - p) < 0.004, p
        assert np.array_equal(m, rng_ref.keep_mask_nhwc(400000, p, 12345))
        assert not np.array_equal(m, rng_ref.keep_mask_nhwc(400000, p, 12346))
    m = rng_ref.keep_mask_nchw(2, 16, 8, 8, 0.3, 7)
    assert m.shape == (2, 16, 8, 8)


def test_local_bn_mode_averages_the_summed_gradient():
    """sync_bn=False: ranks keep their own BatchNorm statistics and loss; the SUM all-reduce of the gradients is turned into the
    mean by the SGD kernel's gradient scale (no extra pass)."""
    from hpfg_amd.train import _StepBase

    class _DP:
        world_size, force_sync, sync_bn = 4, False, False

    class _Opt:
        grad_scale = 1.0

    s = _StepBase.__new__(_StepBase)
    s.dp = _DP()
    o1, o2 = _Opt(), _Opt()
    s._set_grad_scale(o1, o2)
    assert o1.grad_scale == 0.25 and o2.grad_scale == 0.25
    s.dp.sync_bn = True
    o3 = _Opt()
    s._set_grad_scale(o3)
    assert o3.grad_scale == 1.0


def test_eval_zoom_index_is_scipys_mapping():
    """hpfg_amd.val resizes through an index map taken from scipy.ndimage.zoom(order=0) itself (val.py:274,280 semantics)."""
    import numpy as np
    from scipy.ndimage import zoom
    from hpfg_amd import val as V

    g = np.random.default_rng(0)
    for (h, w), (H, W) in (((40, 36), (32, 32)), ((32, 32), (50, 44)), ((17, 23), (64, 48)), ((32, 32), (32, 32)), ((230, 232), (224, 224))):
        a = g.standard_normal((h, w)).astype(np.float32)
        idx = V._zoom_index((h, w), (H, W))
        got = np.where(idx >= 0, a.reshape(-1)[np.maximum(idx, 0)], 0.0).reshape(H, W)
        assert np.array_equal(got, zoom(a, (H / h, W / w), order=0))
    cm = np.array([[5, 1, 0], [2, 4, 0], [1, 1, 0]])
    assert V.dice_from_counts(cm, 1) == 2 * 4 / (6 + 6) and V.dice_from_counts(cm, 2) == 0.0


def test_driver_loop_iteration_law_evaluation_cadence_and_label_cycling():
    """The drivers' shared loop with a stub step: one iteration per unlabelled batch, the labelled loader cycled beside it, the evaluations
    every step_size iterations, and the return once cur_itrs > total_itrs (the reference's law), over more than one epoch."""
    from hpfg_amd.train import _LoopRunner, _with_labels

    class _Step:
        def __init__(self):
            self.calls = []

        def eager_step(self, inputs, cur_itrs, **kw):
            inputs = list(inputs)
            self.calls.append((cur_itrs, [float(t) for t in inputs]))
            return {"parts": torch.tensor([float(cur_itrs), 0.0])}

    args = AttrDict(device="cpu", total_itrs=7, step_size=3, hipgraph=False, log_every=4)
    unlabel = [(torch.tensor(100.0 + i), None) for i in range(3)]
    label = [(torch.tensor(float(i)), torch.tensor(10.0 + i)) for i in range(2)]
    st, evals = _Step(), []
    run = _LoopRunner(st, args, 2, lambda row, h: {"t/loss": row[0]}, ["parts"], lambda: {})

    def best(model, opt, sched, test_loader, cur_itrs, name):
        evals.append((cur_itrs, model, opt, sched, test_loader, name))

    losses = run.drive(unlabel, _with_labels(label, lambda u: [u + 1]), "test", [(best, "m", "o", "s", "model"), (best, "e", "o", "s", "ema")])
    assert [c for c, _ in st.calls] == list(range(1, 9))                      # 7 // 3 + 1 = 3 epochs available; stops at 8 > 7
    assert [x for _, x in st.calls] == [[i % 2, 10 + i % 2, 100 + i % 3, 101 + i % 3] for i in range(8)]
    assert evals == [(k, m, "o", "s", "test", n) for k in (3, 6) for m, n in (("m", "model"), ("e", "ema"))]
    assert losses.tolist() == [float(k) for k in range(1, 9)]
    run.drive(unlabel, _with_labels(label), None, [(best, "m", "o", "s", "model")])
    assert len(evals) == 4                                                   # no test loader: no evaluation


def test_bn_route_truth_table():
    """engine.bn_route over every combination of its six inputs, against the predicates the engine's passes used to spell out at each use."""
    import itertools

    from hpfg_amd import _lib as L
    from hpfg_amd.engine import ACC, ALLREDUCE, EVAL, LOCAL, PEER, bn_route
    n = 0
    for train, math, acc_on, peer, world, force in itertools.product((False, True), (L.MATH_F32, L.MATH_BF16X3), (False, True), (False, True),
                                                                     (1, 2, 8), (False, True)):
        sync = world > 1 or force
        if not train:
            want = EVAL
        elif acc_on and math == L.MATH_BF16X3 and not peer and not sync:
            want = ACC
        elif peer and sync:
            want = PEER
        elif sync:
            want = ALLREDUCE
        else:
            want = LOCAL
        assert bn_route(train, math, acc_on, peer, world, force) == want, (train, math, acc_on, peer, world, force)
        n += 1
    assert n == 96 and len({ACC, LOCAL, ALLREDUCE, PEER, EVAL}) == 5
    assert bn_route(True, L.MATH_BF16X3, True, False, 1, False) == ACC
    assert bn_route(True, L.MATH_BF16X3, True, True, 1, False) == LOCAL          # a peer context without sync: neither exchange nor accumulators
    assert bn_route(True, L.MATH_BF16X3, True, True, 2, False) == PEER and bn_route(True, L.MATH_BF16X3, True, True, 1, True) == PEER
    assert bn_route(True, L.MATH_BF16X3, True, False, 1, True) == ALLREDUCE
    for acc_on, peer, world, force in itertools.product((False, True), (False, True), (1, 2), (False, True)):
        assert bn_route(True, L.MATH_F32, acc_on, peer, world, force) != ACC        # the accumulators serve the bf16x3 kernels only
        assert bn_route(False, L.MATH_BF16X3, acc_on, peer, world, force) == EVAL


def test_desc_table_sub_ranges_alias_the_host_array():
    """engine.DescTable on a CPU tensor: sub(lo, hi) = (device pointer of descriptor lo, host view of [lo, hi) that is NOT a copy, hi - lo)."""
    import ctypes as C

    from hpfg_amd import _lib as L
    from hpfg_amd.engine import DescTable
    descs = (L.SlabDesc * 5)()
    for i, d in enumerate(descs):
        d.S, d.taps, d.Cout = 10 + i, 9, 16
    t = DescTable(descs, torch.device("cpu"))
    sz = C.sizeof(L.SlabDesc)
    assert t.host is descs and t.dev.device.type == "cpu" and t.dev.numel() == 5 * sz
    assert bytes(t.dev.numpy().tobytes()) == bytes(descs)          # the device copy holds the descriptors as built
    base = t.dev.data_ptr()
    for lo, hi in ((0, 5), (1, 4), (3, 5), (2, 3)):
        ptr, host, n = t.sub(lo, hi)
        assert ptr == base + lo * sz and n == hi - lo and len(host) == n and isinstance(host[0], L.SlabDesc)
        assert [d.S for d in host] == [10 + i for i in range(lo, hi)]
    _, host, _ = t.sub(1, 4)
    host[2].S = 77                                   # written through the view ...
    assert descs[3].S == 77                          # ... it shows in the parent array
    descs[1].Cout = 32
    assert host[0].Cout == 32
    assert C.addressof(host) == C.addressof(descs) + sz


def test_acc_encode_reproduces_the_exact_limb_split_of_hpfg_acc_add():
    """tests/helpers.py::acc_encode, the numpy float32 restatement of hpfg_acc_add (csrc/common.h): t = hi + lo * 2^-52 holds EXACTLY for every
    float with |t| >= 2^-29 (and for 0), rint breaks ties to even, |lo| <= 2^51; acc_totals / acc_decode / acc_from_rows agree with it."""
    from fractions import Fraction
    from tests.helpers import ACC_SCALE, acc_decode, acc_encode, acc_from_rows, acc_rows_totals, acc_totals
    rng = np.random.RandomState(5)
    mant = rng.uniform(1.0, 2.0, 4000)
    expo = rng.randint(-29, 40, 4000)
    sign = rng.choice([-1.0, 1.0], 4000)
    ties = [0.5, -0.5, 1.5, 2.5, -1.5, -2.5, 3.5]
    big = [2.0 ** 24, 2.0 ** 24 + 2, -(2.0 ** 24) - 2, 2.0 ** 30 + 128, 3.0 * 2.0 ** 40, -(2.0 ** 62)]
    edge = [0.0, 2.0 ** -29, -(2.0 ** -29), 1.0, -1.0, 0.49999997, 0.50000006, 8388607.5, -8388607.5, 4194303.75]
    t = np.concatenate([sign * mant * 2.0 ** expo, ties, big, edge]).astype(np.float32)
    hi, lo = acc_encode(t)
    assert hi.dtype == np.int64 and lo.dtype == np.int64
    for tv, h, l in zip(t.tolist(), hi.tolist(), lo.tolist()):
        assert Fraction(h) + Fraction(l, ACC_SCALE) == Fraction(tv), (tv, h, l)      # exact, not merely to fp64 rounding
        assert abs(l) <= 2 ** 51, (tv, l)
    np.testing.assert_array_equal(hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -52, t.astype(np.float64))
    got = {tv: (int(h), int(l)) for tv, h, l in zip(ties, *acc_encode(np.float32(ties)))}
    assert got == {0.5: (0, 2 ** 51), -0.5: (0, -(2 ** 51)), 1.5: (2, -(2 ** 51)), 2.5: (2, 2 ** 51), -1.5: (-2, 2 ** 51), -2.5: (-2, -(2 ** 51)),
                   3.5: (4, -(2 ** 51))}
    h, l = acc_encode(np.float32([2.0 ** 24 + 2, 2.0 ** 30 + 128]))
    assert h.tolist() == [2 ** 24 + 2, 2 ** 30 + 128] and l.tolist() == [0, 0]
    # below 2^-29 the low limb drops bits (the documented limit of the split), never more than half a unit of 2^-52
    tiny = np.float32(2.0 ** -30 * 1.2345)
    h, l = acc_encode(tiny)
    assert h == 0 and abs(Fraction(int(l), ACC_SCALE) - Fraction(float(tiny))) <= Fraction(1, 2 * ACC_SCALE)
    # rows -> accumulator tensor -> totals -> float64: integer sums, independent of the shard count
    rows = (rng.randn(21, 2, 5) * 300).astype(np.float32)
    want = acc_rows_totals(rows)
    exact = np.array([[sum(Fraction(float(v)) for v in rows[:, w, c]) for c in range(5)] for w in range(2)], dtype=object)
    for shards in (1, 2, 8):
        acc = acc_from_rows(rows, shards)
        assert tuple(acc.shape) == (shards, 2, 5, 2) and acc.dtype == torch.int64
        tot = acc_totals(acc, 5, shards)
        assert (tot == want).all()
        assert all(Fraction(int(tot[w, c, 0])) + Fraction(int(tot[w, c, 1]), ACC_SCALE) == exact[w, c] for w in range(2) for c in range(5))
        np.testing.assert_array_equal(acc_decode(tot), np.array([[float(exact[w, c]) for c in range(5)] for w in range(2)]))
    assert (acc_from_rows(rows, 8)[1:] != 0).any()      # more than one shard in use
    # 2048 adds of the largest low limb stay inside an int64 word; the Python-integer totals do not wrap beyond it either
    worst = torch.full((8, 2, 1, 2), 2048 * 2 ** 51, dtype=torch.int64)
    assert int(acc_totals(worst, 1, 8)[0, 0, 1]) == 2 ** 65


def test_sgd_ema_restatement_follows_torch_sgd_in_float64():
    """tests/helpers.py::sgd_ema_f32 -- the float32 restatement the GPU test requires hpfg_sgd_step / hpfg_sgd_ema_step / hpfg_ema_update to
    equal bit for bit -- against torch.optim.SGD itself on float64 tensors and a float64 EMA, over five steps with another lr (and EMA
    alpha) each, for every momentum / weight-decay / grad_scale combination of the GPU test: the bit-equality is then a statement about the
    real optimizer, not about the kernel's own expressions.  The bound is derived in helpers.sgd_f64_tolerances (at most 1.3e-5 for the weights
    here: a few ulp of max|w| per step); a flipped weight-decay sign moves a weight by 2 lr wd |w| ~ 2.5e-5 |w| a step, momentum and
    grad_scale swapped by far more."""
    from tests.helpers import N_SMALL, SGD_ALPHAS, SGD_HYPER, SGD_LRS, sgd_case, sgd_ema_f32, sgd_ema_f64, sgd_f64_tolerances
    c = sgd_case(N_SMALL)
    n = N_SMALL
    for mu, wd, gs in SGD_HYPER:
        p32, b32, t32 = sgd_ema_f32(c["p0"], c["g"], c["mom0"], SGD_LRS, mu, wd, gs, t=c["t0"], n_ema=n, alphas=SGD_ALPHAS)
        p64, b64, t64 = sgd_ema_f64(c["p0"], c["g"], c["mom0"], SGD_LRS, mu, wd, gs, c["t0"], SGD_ALPHAS)
        tol_p, tol_b, tol_t = sgd_f64_tolerances(p64, b64, t64, c["g"], wd, gs)
        assert tol_p < 2e-5 and tol_t < 2e-4, (tol_p, tol_t)          # (the bound itself stays at the rounding level: |w| reaches 4, five steps)
        e_p, e_t = np.abs(p32 - p64).max(), np.abs(t32 - t64).max()
        assert e_p <= tol_p and e_t <= tol_t, (mu, wd, gs, e_p, tol_p, e_t, tol_t)
        if mu != 0:
            assert np.abs(b32 - b64).max() <= tol_b, (mu, wd, gs)
        # the mistakes the issue names are far outside: weight-decay sign (where there is decay), momentum and grad_scale swapped
        if wd != 0:
            bad = sgd_ema_f32(c["p0"], c["g"], c["mom0"], SGD_LRS, mu, -wd, gs)[0]
            assert np.abs(bad - p64).max() > 10 * tol_p
        if mu != gs:
            bad = sgd_ema_f32(c["p0"], c["g"], c["mom0"], SGD_LRS, gs, wd, mu)[0]
            assert np.abs(bad - p64).max() > 10 * tol_p
    # a partial teacher slice leaves the rest of the teacher alone; alpha = 0 at the first step makes the slice the fresh student
    p1, _, t1 = sgd_ema_f32(c["p0"], c["g"][:1], c["mom0"], SGD_LRS[:1], 0.9, 5e-4, 0.5, t=c["t0"], n_ema=1001, alphas=(0.0,))
    assert np.array_equal(t1[:1001], p1[:1001]) and np.array_equal(t1[1001:], c["t0"][1001:])


def test_adamw_restatement_passes_the_reference_bound_and_every_mutation_fails_it():
    """The tolerance of tests/test_gpu_optim.py::test_adamw_kernel_trajectory is 8 x the error torch.optim.AdamW in float32 makes against
    torch.optim.AdamW in float64 on the same 40-step trajectory (helpers.adamw_case), per checked step and per buffer.  That bound must
    tell a correct kernel from a subtly wrong one: the numpy float32 restatement of the kernel passes it, and each of the four mistakes
    (t off by one, no sqrt on the second bias correction, eps inside the root, weight decay coupled into the gradient) fails it.
    Measured on the committed trajectory, max|dp| at step 40: reference float32 1.6e-6, restatement 1.6e-6, t+1 1.2e-3, no sqrt 1.2e-1,
    eps inside the root 1.2e-1, coupled decay 3.2e-1."""
    from tests.helpers import ADAMW_CHECKED, ADAMW_MUTATIONS, N_SMALL, adamw_case, adamw_errors, adamw_f32, adamw_within
    c = adamw_case()
    lrs = c["lrs"]
    assert len(set(lrs)) >= len(lrs) - 1 and np.argmax(lrs) in range(5, 20)          # warm-up inside the 40 steps; lr moves at every step
    assert set(c["ref64"]) == set(ADAMW_CHECKED) and all(e > 0 for s in c["ref_err"] for e in c["ref_err"][s])
    mags = np.abs(c["g"]).max(0)
    assert (mags < 1e-7).mean() > 0.05 and (mags > 1e-1).mean() > 0.05               # gradients around eps and around 1
    z = np.zeros(N_SMALL, np.float32)
    ok = adamw_errors(adamw_f32(c["p0"], c["g"], z, z, lrs, checked=ADAMW_CHECKED), c["ref64"])
    assert adamw_within(ok, c["tol"]), (ok, c["tol"])
    for mut in ADAMW_MUTATIONS:
        bad = adamw_errors(adamw_f32(c["p0"], c["g"], z, z, lrs, mutation=mut, checked=ADAMW_CHECKED), c["ref64"])
        assert not adamw_within(bad, c["tol"]), mut
        assert bad[40][0] > 10 * c["tol"][40][0], (mut, bad[40][0], c["tol"][40][0])      # ... by a wide margin in the weights
    # a restart from saved moments continues the same trajectory (what FusedAdamW.load_state_dict relies on)
    a = adamw_f32(c["p0"], c["g"][:6], z, z, lrs[:6])[6]
    b = adamw_f32(a[0], c["g"][6:12], a[1], a[2], lrs[6:12], step0=6)[12]
    whole = adamw_f32(c["p0"], c["g"][:12], z, z, lrs[:12])[12]
    assert all(np.array_equal(x, y) for x, y in zip(b, whole))


def test_mixing_references_and_bounds():
    """helpers.blend_f64 / softmax_mix_f64, the float64 references of the blend and ICT kernels: 0/1 weights select exactly, the bound
    3 * 2^-24 (|a| + |b|) holds for the blend evaluated in float32 on the host, rows of the mixed softmax sum to 1."""
    from tests.helpers import blend_f64, softmax_mix_f64
    r = np.random.RandomState(3)
    a, b = r.randn(4099).astype(np.float32), (r.randn(4099) * 50).astype(np.float32)
    m = r.choice([0.0, 1.0], 4099).astype(np.float32)
    ref, bound = blend_f64(a, b, m)
    assert np.array_equal(ref, np.where(m == 1, b, a).astype(np.float64)) and (bound > 0).all()
    m = r.uniform(0, 1, 4099).astype(np.float32)
    ref, bound = blend_f64(a, b, m)
    got = a * (np.float32(1) - m) + b * m
    assert got.dtype == np.float32 and (np.abs(got - ref) <= bound).all()
    t0, t1 = torch.randn(3, 9, 4, 5) * 8, torch.randn(3, 9, 4, 5) * 8
    out = softmax_mix_f64(t0, t1, [0.0, 1.0, 0.25])
    assert torch.equal(out[0], torch.softmax(t0.double(), 1)[0]) and torch.equal(out[1], torch.softmax(t1.double(), 1)[1])
    assert float((out.sum(1) - 1).abs().max()) < 1e-14


def test_gather_flat_grads_refuses_a_parameter_without_gradient_inside_the_range():
    """torch.optim.AdamW skips a parameter whose .grad is None; the flat AdamW / SGD kernels cannot, and zeros in its place would still decay
    the weight.  No module of the package leaves a parameter of the updated range without a gradient, so gather_flat_grads raises where
    one is met (naming it) instead of packing zeros; past active_numel nothing is looked at or written."""
    from hpfg_amd.utils.optim import flatten_parameters, gather_flat_grads
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    flatten_parameters(net)
    n0 = 7 * 5 + 5
    assert net.flat_params.numel() == n0 + 5 * 3 + 3 and all(p.data_ptr() >= net.flat_params.data_ptr() for p in net.parameters())
    for p in net[0].parameters():
        p.grad = torch.randn_like(p)
    net.flat_grads.fill_(7.0)
    out = gather_flat_grads(net, n0)                       # the second layer has no gradients: outside the range, fine
    assert torch.equal(out[:n0], torch.cat([p.grad.reshape(-1) for p in net[0].parameters()])) and bool((out[n0:] == 7.0).all())
    with pytest.raises(RuntimeError, match=r"1\.weight"):
        gather_flat_grads(net)                             # ... inside it: refused
    net[0].bias.grad = None
    with pytest.raises(RuntimeError, match=r"0\.bias"):
        gather_flat_grads(net, n0)
    with pytest.raises(AssertionError):
        gather_flat_grads(net, n0 - 1)                     # not a parameter boundary
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    assert bool((gather_flat_grads(net) == 1.0).all())


# ---- float64 restatements of the virtual sources (tests/helpers.py) against torch float64 ops, and the split-bf16 error bound ------------------
def test_source_restatements_equal_torch_float64_ops():
    import torch.nn.functional as F
    from hpfg_amd import _lib as L
    from tests import helpers as T
    g = torch.Generator().manual_seed(5)
    N, H, W, C_ = 2, 6, 10, 8
    z, tab = torch.randn(N, H, W, C_, generator=g) * 2 + 0.5, T.bn_table(C_, 4)
    sc, sh = tab[L.BN_SCALE], tab[L.BN_SHIFT]
    y = z.double() * sc.double() + sh.double()
    act = F.leaky_relu(y, T.LEAKY32)
    # bnact: F.leaky_relu, and the keep mask through the oracle's NCHW mask (another indexing path to element pix * C + c)
    v, d = T.bnact_f64(z, sc, sh)
    assert torch.equal(v, act) and float(d.min()) > 0
    v, _ = T.bnact_f64(z, sc, sh, 0.3, 77)
    keep = torch.from_numpy(rng_ref.keep_mask_nchw(N, C_, H, W, 0.3, 77).astype(np.float64)).permute(0, 2, 3, 1)
    assert 0.6 < float(keep.mean()) < 0.8 and torch.equal(v, act * (keep / (1.0 - float(np.float32(0.3)))))
    # pool: F.max_pool2d with indices, its backward
    pv, _ = T.pool_f64(z, sc, sh)
    a_ = T.nchw(act).requires_grad_(True)
    ref, idx = F.max_pool2d(a_, 2, return_indices=True)
    assert torch.equal(T.nchw(pv), ref)
    first = T.pool_argmax(act, 3.0 * T.U24 * (y.abs() + 1))          # (a generous delta: this input is clear of ties)
    yy, xx = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    flat = (2 * yy[None, :, :, None] + first // 2) * W + 2 * xx[None, :, :, None] + first % 2
    assert torch.equal(T.nchw(flat), idx)
    dP = torch.randn(N, H // 2, W // 2, C_, generator=g).double()
    ref.backward(T.nchw(dP))
    assert torch.equal(T.nchw(T.pool_scatter_f64(dP, first)), a_.grad)
    tie = torch.zeros(1, 2, 2, 1, dtype=torch.float64)
    assert int(T.pool_argmax(tie)) == 0                               # first maximum in row-major order
    with pytest.raises(AssertionError, match="max-pool tie"):
        T.pool_argmax(tie, torch.full_like(tie, 1e-9))
    with pytest.raises(AssertionError, match="LeakyReLU tie"):
        T.lrelu_slope(torch.zeros(1, dtype=torch.float64), torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    # up2x / upbwd: F.interpolate(align_corners=True) and its autograd.  The float32 weight law moves a weight by at most 2 u (index): the
    # values by 2 * 2 u (h + w) max|u| on an h x w source
    for h, w in [(1, 1), (3, 10), (7, 7), (5, 17)]:
        u = (torch.randn(N, h, w, C_, generator=g) * 2).double()
        un = T.nchw(u).requires_grad_(True)
        ref = F.interpolate(un, scale_factor=2, mode="bilinear", align_corners=True)
        up, dlt = T.up2x_f64(u)
        tol = 4.0 * T.U24 * (h + w) * float(u.abs().max())
        assert float((T.nchw(up) - ref).abs().max()) <= tol and up.shape == (N, 2 * h, 2 * w, C_) and float(dlt.max()) <= (6.1 + 4 * (h + w)) * T.U24 * float(u.abs().max())
        gup = torch.randn(N, 2 * h, 2 * w, C_, generator=g).double()
        ref.backward(T.nchw(gup))
        gb, _ = T.upbwd_f64(gup)
        assert float((T.nchw(gb) - un.grad).abs().max()) <= 4.0 * T.U24 * (h + w) * 9 * float(gup.abs().max())      # (up to 9 taps of a 3 x 3 footprint carry weight)
        assert abs(float((up * gup).sum() - (u * gb).sum())) <= 1e-12 * float((up.abs() * gup.abs()).sum())            # the exact transpose
    # cat: the two halves side by side
    u = torch.randn(N, H // 2, W // 2, 4, generator=g)
    cv, cd = T.cat_f64(z, sc, sh, u)
    assert torch.equal(cv[..., :C_], act) and torch.equal(cv[..., C_:], T.up2x_f64(u)[0]) and cd.shape == cv.shape
    # dz: F.conv2d autograd through BatchNorm (train mode) + LeakyReLU + Dropout -- dZ = k1 g + k2 z + k3 with the table rows of its batch statistics
    p, seed, eps = 0.3, 123, 1e-5
    gamma, beta = torch.randn(C_, generator=g).double(), torch.randn(C_, generator=g).double()
    zr = T.nchw(z.double()).requires_grad_(True)
    yb = F.batch_norm(zr, None, None, gamma, beta, training=True, eps=eps)
    a = F.leaky_relu(yb, T.LEAKY32) * T.nchw(T.keep_f64((N, H, W, C_), p, seed))
    a.retain_grad()
    w = torch.randn(5, C_, 3, 3, generator=g).double()
    F.conv2d(a, w, None, padding=1).backward(torch.randn(N, 5, H, W, generator=g).double())
    mean, var = z.double().mean((0, 1, 2)), z.double().var((0, 1, 2), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    t64 = torch.zeros(L.BN_ROWS, C_, dtype=torch.float64)
    t64[L.BN_SCALE] = gamma * rstd
    t64[L.BN_SHIFT] = beta - mean * t64[L.BN_SCALE]
    dA = a.grad.permute(0, 2, 3, 1)
    gg = dA * T.keep_f64((N, H, W, C_), p, seed) * torch.where(T.lrelu_slope(z.double(), t64[L.BN_SCALE], t64[L.BN_SHIFT]) == 1.0, 1.0, T.LEAKY32)
    m1, m2 = gg.mean((0, 1, 2)), (gg * (z.double() - mean) * rstd).mean((0, 1, 2))
    t64[L.BN_K1] = gamma * rstd
    t64[L.BN_K2] = -(gamma * rstd * rstd) * m2
    t64[L.BN_K3] = gamma * rstd * (mean * rstd * m2 - m1)
    dzv, dzd = T.dz_f64(z, dA, t64, p, seed)
    assert float((T.nchw(dzv) - zr.grad).abs().max()) <= 1e-12 * float(zr.grad.abs().max()) and float(dzd.min()) >= 0


def _emu(kind, a, w, b=None, g=None):
    """the split-product emulation (oracle.bf16x3_ref: three kept products, fp32 accumulation) of a conv / dgrad / wgrad on float64-derived
    NHWC operands"""
    from oracle import bf16x3_ref
    from tests import helpers as T
    pad = w.shape[-1] // 2
    with bf16x3_ref.math_mode("bf16x3"):
        if kind == "conv":
            return bf16x3_ref.conv2d(T.nchw(a).float(), w, b, padding=pad).permute(0, 2, 3, 1).double()
        if kind == "dgrad":      # (the input gradient alone: no weight gradient is formed)
            xr = torch.zeros(g.shape[0], w.shape[1], g.shape[1], g.shape[2], requires_grad=True)
            bf16x3_ref.conv2d(xr, w, None, padding=pad).backward(T.nchw(g).float())
            return xr.grad.permute(0, 2, 3, 1).double()
        wr = w.clone().requires_grad_(True)
        bf16x3_ref.conv2d(T.nchw(a).float(), wr, None, padding=pad).backward(T.nchw(g).float())
        return wr.grad.double()


def _conv_case_checks():
    """(tag, group, float64 reference, bound, emulated result) of every case of tests/test_gpu_conv_sources.py, from its CPU inputs"""
    from tests import helpers as T
    emu = _emu

    for c in T.FWD3_CASES + [T.FWD3_PERSISTENT] + [k + (None,) for k in T.FWD1_CASES]:
        kind, p, N, H, W, cin, cout = c[:7]
        taps = 9 if len(c) == 8 and c in T.FWD3_CASES + [T.FWD3_PERSISTENT] else 1
        s = T.conv_source(kind, T.case_seed(*c), N, H, W, cin, p)
        w, b = T.adhoc_weights(cin, cout, taps, T.case_seed(*c))
        ref, bound = T.conv_ref_bound(s["v"], s["d"], w, b)
        yield f"fwd{taps} {c}", "A" if taps == 9 else "C", ref, bound, emu("conv", s["v"], w, b)
    for c in T.DGRAD3_CASES + [("plain", 0.0) + k + (None, None) for k in T.DGRAD1_CASES]:
        kind, p, N, H, W, cin, cout = c[:7]
        taps = 9 if c in T.DGRAD3_CASES else 1
        s = T.conv_source(kind, T.case_seed(*c), N, H, W, cout, p)
        w, _ = T.adhoc_weights(cin, cout, taps, T.case_seed(*c))
        ref, bound = T.dgrad_ref_bound(s["v"], s["d"], w)
        if c[-1] == "pool":
            T.pool_epilogue_source(T.pool_epilogue_seed(c), N, H, W, cin)          # (its arg-max guard)
        yield f"dgrad{taps} {c}", "B" if taps == 9 else "C", ref, bound, emu("dgrad", None, w, g=s["v"])
    for c in T.WGRAD_CASES:
        ak, pa, gk, pg, N, H, W, cin, cout, taps = c
        sa = T.conv_source(ak, T.case_seed(*c), N, H, W, cin, pa)
        sg = T.conv_source(gk, T.case_seed(*c) + 1, N, H, W, cout, pg)
        w, _ = T.adhoc_weights(cin, cout, taps, T.case_seed(*c))
        ref, bound = T.wgrad_ref_bound(sa["v"], sa["d"], sg["v"], sg["d"], w.shape)
        yield f"wgrad {c}", "E", ref, bound, emu("wgrad", sa["v"], w, g=sg["v"])
    for c in T.UPBWD_CASES:
        N, H, W, cin, cout = c
        v, d = T.upbwd_f64(torch.randn(N, 2 * H, 2 * W, cout, generator=torch.Generator().manual_seed(T.case_seed(*c))))
        w, _ = T.adhoc_weights(cin, cout, 1, T.case_seed(*c))
        ref, bound = T.dgrad_ref_bound(v, d, w)
        yield f"upbwd dgrad {c}", "C", ref, bound, emu("dgrad", None, w, g=v)
    for kind, p in T.STAGE_CASES:
        c = (kind, p, 3, 10, 34, 64, 64)
        si, sg = T.conv_source(kind, T.case_seed(*c), 3, 10, 34, 64, p), T.conv_source("dz", T.case_seed(*c) + 1, 3, 10, 34, 64, 0.3)
        w, b = T.adhoc_weights(64, 64, 9, T.case_seed(*c))
        ref, bound = T.conv_ref_bound(si["v"], si["d"], w, b)
        yield f"stage fwd {c}", "D", ref, bound, emu("conv", si["v"], w, b)
        ref, bound = T.dgrad_ref_bound(sg["v"], sg["d"], w)
        yield f"stage dgrad {c}", "D", ref, bound, emu("dgrad", None, w, g=sg["v"])
        ref, bound = T.wgrad_ref_bound(si["v"], si["d"], sg["v"], sg["d"], w.shape)
        yield f"stage wgrad {c}", "D", ref, bound, emu("wgrad", si["v"], w, g=sg["v"])


def test_split_product_emulation_stays_within_the_bound_on_every_case():
    """The condition on the inputs of tests/test_gpu_conv_sources.py: oracle.bf16x3_ref.conv2d -- the three kept products with fp32 accumulation
    -- stays within the bound of tests/helpers.py against the float64 convolution for every case (and every guard of the inputs passes)."""
    worst = {}
    for tag, group, ref, bound, got in _conv_case_checks():
        assert bool(torch.isfinite(ref).all()) and float(bound.min()) > 0, tag
        r = float(((got - ref).abs() / bound).max())
        worst[group] = max(worst.get(group, 0.0), r)
        assert r <= 1.0, f"{tag}: the emulation is {r:.3g} x the bound off the float64 result"
    for group in sorted(worst):
        print(f"[conv_sources] {group} (CPU emulation): largest error / bound = {worst[group]:.3g}")


# ---- the cases of tests/test_gpu_tile_edges.py (whole-tile kernels) ------------------------------------------------------------------------
def test_tile_edge_cases_reach_the_kernels_and_the_walk_cases_walk():
    """The launch geometry the GPU tests rely on, from the library's host side: every thin case goes to conv_thin_kernel (a multiple of 8
    rows, not the chunked kernel's count), every fused case has an instantiation, the tile-count edges are what their names say, and in the
    walk cases every workgroup's tile loop runs twice (three times with one workgroup per CU) on an uneven, non-square grid of tiles."""
    import ctypes as C
    from hpfg_amd import _lib as L
    from tests import helpers as T
    lib = L.load()
    seen = set()
    for case in T.THIN_CASES:
        kind, _, N, H, W, _, _, edge = case
        rows = lib.hpfg_conv_stat_rows(C.byref(T.thin_args(case)))
        assert rows > 0 and rows % 8 == 0 and rows != lib.hpfg_conv_stat_rows(C.byref(T.thin_args(case, L.MATH_BF16X3 | T.OLD_KERNEL))), case
        nwork = N * (H // 16) * (W // 16)
        if edge == "walk":
            assert T.walk_conditions(nwork, rows, W // 16, H // 16, T.THIN_INST[kind][2]), (case, rows)
        elif edge:
            assert nwork < rows and (edge == "one") == (nwork == 1), (case, rows)
        seen.add((kind, edge))
    assert seen >= {(k, e) for k in T.THIN_INST for e in ("one", "few", "walk")}
    seen = set()
    for case in T.FUSED_CASES:
        ak, _, gk, _, N, H, W, cin, _, _, edge = case
        grid = lib.hpfg_fused_bwd_grid(C.byref(T.fused_args(case)))
        assert grid > 0, (case, lib.hpfg_last_error())
        inst = [v for v in T.FUSED_INST.values() if v[:3] == (ak, gk, cin)]
        assert len(inst) == 1, case
        nwork = N * (H // 16) * (W // 16)
        if edge == "walk":
            assert T.walk_conditions(nwork, grid, W // 16, H // 16, inst[0][4]), (case, grid)
        elif edge:
            assert nwork < grid and (edge == "one") == (nwork == 1), (case, grid)
        seen.add((ak, gk, cin, edge))
    assert seen >= {v[:3] + (e,) for v in T.FUSED_INST.values() for e in ("one", "few", "walk")}
    assert set(T.QUAD_FUSED) <= set(T.FUSED_CASES)
    for N, H, W, cin, _, _, _ in T.FIRST_CASES:
        assert H % 16 == 0 and W % 16 == 0 and 64 <= W <= 512 and cin in (1, 3)
    assert any(N * H > 768 for N, H, *_ in T.FIRST_CASES) and {c[2] for c in T.FIRST_CASES} >= {64, 80, 272, 512}


def _ratio(got, ref, bound):
    return float(((got - ref).abs() / bound).max())


def test_tile_edge_cases_emulation_stays_within_the_bound():
    """The condition on the inputs of tests/test_gpu_tile_edges.py, as for the chunked kernels above: every source passes its LeakyReLU guard
    (conv_source asserts it), the bounds are positive, and the split-product emulation -- torch float32 for the streaming first-layer kernel,
    which multiplies in fp32 -- stays inside the bound of every case, so the float64 reference alone passes."""
    from tests import helpers as T
    worst = {}

    def within(group, tag, got, ref, bound):
        assert bool(torch.isfinite(ref).all()) and float(bound.min()) > 0, tag
        r = _ratio(got, ref, bound)
        worst[group] = max(worst.get(group, 0.0), r)
        assert r <= 1.0, f"{tag}: the emulation is {r:.3g} x the bound off the float64 result"

    for case in T.THIN_CASES:
        d = T.thin_case(case)
        got = _emu("dgrad", None, d["w"], g=d["s"]["v"]) if case[0] == "dz" else _emu("conv", d["s"]["v"], d["w"], d["b"])
        within("A", f"thin {case}", got, d["ref"], d["bound"])
        assert d["f32"] <= 1.0, case
    for case in T.FUSED_CASES:
        d = T.fused_case(case)
        if d["dx"] is not None:
            within("B", f"fused dX {case}", _emu("dgrad", None, d["w"], g=d["sg"]["v"]), *d["dx"][:2])
        within("B", f"fused dW {case}", _emu("wgrad", d["sa"]["v"], d["w"], g=d["sg"]["v"]), *d["dw"][:2])
    for N, H, W, cin, p in sorted({c[:5] for c in T.FIRST_CASES}):
        d = T.first_case(N, H, W, cin, p)
        assert d["f32"] <= 1.0 and float(d["b_stream"].min()) > 0 and bool((d["b_stream"] < d["b_tile"]).all()), (N, H, W, cin, p)
        w0 = torch.zeros(16, cin, 3, 3)
        within("C", f"first layer {(N, H, W, cin, p)}", _emu("wgrad", d["sx"]["v"], w0, g=d["sg"]["v"]), d["ref"], d["b_tile"])
    for case in T.QUAD_DGRAD:
        kind, p, N, H, W, cin, cout = case[:7]
        s = T.conv_source(kind, T.case_seed(*case), N, H, W, cout, p)
        w, _ = T.adhoc_weights(cin, cout, 9, T.case_seed(*case))
        within("D", f"dgrad {case}", _emu("dgrad", None, w, g=s["v"]), *T.dgrad_ref_bound(s["v"], s["d"], w))
    for case in T.QUAD_WGRAD:
        ak, pa, gk, pg, N, H, W, cin, cout, taps = case
        sa, sg = T.conv_source(ak, T.case_seed(*case), N, H, W, cin, pa), T.conv_source(gk, T.case_seed(*case) + 1, N, H, W, cout, pg)
        w, _ = T.adhoc_weights(cin, cout, taps, T.case_seed(*case))
        within("D", f"wgrad {case}", _emu("wgrad", sa["v"], w, g=sg["v"]), *T.wgrad_ref_bound(sa["v"], sa["d"], sg["v"], sg["d"], w.shape))
    for group in sorted(worst):
        print(f"[tile_edges] {group} (CPU emulation): largest error / bound = {worst[group]:.3g}")


def test_tile_edge_bounds_tell_three_wrong_kernels_apart_on_the_walk_cases():
    """The bounds are tight enough to matter.  Three wrong kernels restated in float64 on the walk cases, each of which must leave the bound:
      halo   the left halo column of one interior tile read as zero -- forward conv and dgrad;
      tile   the pixels of one tile missing from the weight gradient.  The bound grows with (N H W + 2) 2^-24 sum|a||g|, which at the 140 to
             200 thousand pixels of a walk is far more than a unit-scale tile contributes; the walk cases carry one tile of 8 x the amplitude
             (helpers.walk_hot) and it is that tile whose absence must show;
      hi     the hi * lo + lo * hi products dropped (bf16 operands) -- forward conv and dgrad, whose bound is dominated by the split term.  On
             the weight gradient of a walk case the summation term dominates instead and this mutant stays inside: printed, not required."""
    import torch.nn.functional as F
    from torch.nn import grad as G
    from oracle import bf16x3_ref
    from tests import helpers as T
    hi = lambda t: bf16x3_ref.split(t.float())[0].double()
    y0, x0, _ = T.HOT

    def conv(a, w, b):
        return F.conv2d(T.nchw(a), w.double(), None if b is None else b.double(), padding=1).permute(0, 2, 3, 1)

    def dgrad(g, w):
        return F.conv_transpose2d(T.nchw(g), w.double(), padding=1).permute(0, 2, 3, 1)

    def halo_mutant(op, src, n, ref):
        cut = src[n:n + 1].clone()
        cut[0, y0 - 1:y0 + 17, x0 - 1] = 0.0
        mut = ref.clone()
        mut[n, y0:y0 + 16, x0:x0 + 16] = op(cut)[0, y0:y0 + 16, x0:x0 + 16]
        return mut

    for case in [c for c in T.THIN_CASES if c[-1] == "walk"]:
        d, n = T.thin_case(case), case[2] // 2
        v, w = d["s"]["v"], d["w"]
        if case[0] == "dz":
            op, low = (lambda t: dgrad(t, w)), dgrad(hi(v), hi(w))
        else:
            op, low = (lambda t: conv(t, w, d["b"])), conv(hi(v), hi(w), d["b"])
        assert float((op(v[n:n + 1])[0] - d["ref"][n]).abs().max()) <= 1e-9 * float(d["ref"].abs().max())      # (the restatement is the reference's op)
        r_halo, r_hi = _ratio(halo_mutant(op, v, n, d["ref"]), d["ref"], d["bound"]), _ratio(low, d["ref"], d["bound"])
        print(f"[tile_edges] mutants thin {case}: halo {r_halo:.3g}, hi-only {r_hi:.3g} x the bound")
        assert r_halo > 1.0 and r_hi > 1.0, (case, r_halo, r_hi)
    for case in [c for c in T.FUSED_CASES if c[-1] == "walk"]:
        d, n = T.fused_case(case), case[4] // 2
        a, g, w = d["sa"]["v"], d["sg"]["v"], d["w"]
        r_halo = r_hi = float("nan")      # (the first layer has no dX)
        if d["dx"] is not None:
            ref, bound, _ = d["dx"]
            r_halo, r_hi = _ratio(halo_mutant(lambda t: dgrad(t, w), g, n, ref), ref, bound), _ratio(dgrad(hi(g), hi(w)), ref, bound)
            assert r_halo > 1.0 and r_hi > 1.0, (case, r_halo, r_hi)
        ref, bound, _ = d["dw"]
        only = torch.zeros_like(a[n:n + 1])
        only[0, y0:y0 + 16, x0:x0 + 16] = a[n, y0:y0 + 16, x0:x0 + 16]
        r_tile = _ratio(ref - G.conv2d_weight(T.nchw(only), tuple(w.shape), T.nchw(g[n:n + 1]), padding=1), ref, bound)
        r_hi_dw = _ratio(G.conv2d_weight(T.nchw(hi(a)), tuple(w.shape), T.nchw(hi(g)), padding=1), ref, bound)
        print(f"[tile_edges] mutants fused {case}: halo {r_halo:.3g}, hi-only {r_hi:.3g} (dX); missing tile {r_tile:.3g}, hi-only {r_hi_dw:.3g} (dW) x the bound")
        assert r_tile > 1.0, (case, r_tile)
