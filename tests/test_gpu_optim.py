"""GPU: the kernels that write the weights (csrc/misc.hip: hpfg_sgd_step, hpfg_sgd_ema_step, hpfg_ema_update, hpfg_adamw_step) and the
optimizer classes on top of them, against the optimizers' laws -- not against each other.

SGD / EMA are compiled without FMA contraction, so they must equal a numpy float32 restatement of torch.optim.SGD's operation order bit for
bit (tests/helpers.py::sgd_ema_f32; tests/test_host_logic.py holds that restatement against torch.optim.SGD in float64).  AdamW is compared
with torch.optim.AdamW in float64 over 40 steps, inside 8 x the error torch's own float32 AdamW makes on the same trajectory."""
from copy import deepcopy

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd.utils import ema_alpha
from hpfg_amd.utils.optim import FusedAdamW
from tests.helpers import (ADAMW_CHECKED, ADAMW_HP, N_BIG_OPTIM, N_SMALL, SGD_ALPHAS, SGD_HYPER, SGD_LRS, adamw_case, adamw_errors, adamw_f32,
                           adamw_torch, adamw_within, bits_kept as _bits_kept, cosine_warmup_lrs, padded as _padded, sgd_case, sgd_ema_f32, stream)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _same(dev_t, want, n):
    return torch.equal(dev_t[:n].cpu(), torch.from_numpy(want[:n]))


@pytest.mark.parametrize("n", [N_SMALL, N_BIG_OPTIM])
@pytest.mark.parametrize("ema", ["all", "middle", "none"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_and_ema_launches_equal_the_float32_law_bitwise(momentum, ema, n):
    """Five consecutive steps (another lr and EMA alpha each; alpha is 0 at the first, as ema_alpha(0, .)), for momentum in {0, 0.9},
    weight decay in {0, 5e-4} and grad_scale in {1, 0.5, 1/3}: p, the momentum buffer and the teacher equal helpers.sgd_ema_f32 bit for
    bit, through hpfg_sgd_ema_step and through hpfg_sgd_step + hpfg_ema_update.  n = 2048*256 + 257 runs the grid-stride loop a second
    time.  Elements past n, and teacher elements past n_ema, hold a NaN pattern and keep their bits."""
    lib = L.load()
    c = sgd_case(n)
    n_ema = {"all": n, "middle": n // 2 + 77, "none": 0}[ema]
    assert n_ema % 256 != 0 or n_ema == 0
    assert SGD_ALPHAS[0] == ema_alpha(0, 0.99) == 0.0 and SGD_ALPHAS[3] == ema_alpha(3, 0.99)
    st = stream(DEV)
    g_dev = [_padded(c["g"][k]) for k in range(len(SGD_LRS))]
    lr, al = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for mu, wd, gs in (h for h in SGD_HYPER if h[0] == momentum):
        want_p, want_m, want_t = sgd_ema_f32(c["p0"], c["g"], c["mom0"], SGD_LRS, mu, wd, gs, t=c["t0"], n_ema=n_ema, alphas=SGD_ALPHAS)
        for fused in (True, False):
            p, m, t = _padded(c["p0"]), _padded(c["mom0"]), _padded(c["t0"], n_ema)
            for k in range(len(SGD_LRS)):
                lr.fill_(SGD_LRS[k])
                al.fill_(SGD_ALPHAS[k])
                if fused:
                    L.check(lib.hpfg_sgd_ema_step(L.ptr(p), L.ptr(g_dev[k]), L.ptr(m), n, L.ptr(lr), mu, wd, gs, L.ptr(t), n_ema, L.ptr(al), st), "sgd_ema")
                else:
                    L.check(lib.hpfg_sgd_step(L.ptr(p), L.ptr(g_dev[k]), L.ptr(m), n, L.ptr(lr), mu, wd, gs, st), "sgd")
                    if n_ema:
                        L.check(lib.hpfg_ema_update(L.ptr(t), L.ptr(p), n_ema, L.ptr(al), st), "ema")
                if k == 0 and n_ema:      # alpha = 0: the teacher slice IS the fresh student
                    assert torch.equal(t[:n_ema], p[:n_ema]), (mu, wd, gs, fused)
            torch.cuda.synchronize()
            what = (mu, wd, gs, "fused" if fused else "two launches")
            assert _same(p, want_p, n), ("p", what, float((p[:n].cpu() - torch.from_numpy(want_p)).abs().max()))
            assert _same(m, want_m, n), ("momentum", what)
            assert _same(t, want_t, n_ema), ("teacher", what)
            assert _bits_kept(p, n) and _bits_kept(m, n) and _bits_kept(t, n_ema), ("tail", what)


def test_sgd_ema_step_refuses_bad_ranges():
    lib = L.load()
    n = 1000
    p, g, m, t = (torch.zeros(n, device=DEV) for _ in range(4))
    lr, al = torch.full((1,), 0.1, device=DEV), torch.full((1,), 0.5, device=DEV)
    st = stream(DEV)
    assert lib.hpfg_sgd_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), n, L.ptr(lr), 0.9, 0.0, 1.0, L.ptr(t), n + 1, L.ptr(al), st) == -1
    assert lib.hpfg_sgd_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), n, L.ptr(lr), 0.9, 0.0, 1.0, L.ptr(p), n, L.ptr(al), st) == -1
    assert lib.hpfg_sgd_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), n, L.ptr(lr), 0.9, 0.0, 1.0, L.ptr(t), -1, L.ptr(al), st) == -1
    assert lib.hpfg_sgd_ema_step(L.ptr(p), L.ptr(g), L.ptr(m), n, L.ptr(lr), 0.9, 0.0, 1.0, L.ptr(t), n, L.ptr(al), st) == 0
    torch.cuda.synchronize()
    assert not p.any() and not t.any()


def _adamw_launch(lib, p, g, m, v, n, lr, step, hp=ADAMW_HP):
    L.check(lib.hpfg_adamw_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, L.ptr(lr), L.ptr(step), hp["betas"][0], hp["betas"][1], hp["eps"],
                                hp["weight_decay"], hp["grad_scale"], stream(DEV)), "adamw")


def test_adamw_kernel_trajectory():
    """hpfg_adamw_step over 40 steps against torch.optim.AdamW on float64 CPU tensors (betas (0.9, 0.999), eps 1e-8, weight decay 0.05), lr
    from CosineWarmupLR_Scheduler (warm-up inside the 40 steps), grad_scale 0.5, gradient magnitudes spread over 10^U(-8, 0); p, m, v and
    the device step word after steps 1, 2, 3, 10 and 40.  Tolerance per step and buffer: 8 x the error of torch.optim.AdamW in float32 on
    the same trajectory (helpers.adamw_case); test_host_logic.py shows that each of four subtle mistakes fails that bound.

    max|error| against float64 (p, m, v), reference float32 AdamW / this kernel on the MI355X:
      step  1: 2.3e-07 4.5e-09 1.1e-10 / 1.4e-07 4.5e-09 1.1e-10
      step  2: 4.4e-07 7.2e-09 1.2e-10 / 2.5e-07 5.1e-09 1.2e-10
      step  3: 5.7e-07 1.4e-08 1.7e-10 / 3.7e-07 7.9e-09 1.7e-10
      step 10: 1.1e-06 1.2e-08 8.2e-10 / 6.9e-07 4.8e-08 8.2e-10
      step 40: 1.6e-06 2.9e-08 6.8e-09 / 1.3e-06 8.2e-08 6.8e-09
    (Before this test the kernel formed 1 - beta2 from the float32 beta2: 0.00099998713 for 0.001, and every v was 1.3e-5 too small,
    150 x the reference's error at step 1; the betas now reach the kernel as doubles.)"""
    lib = L.load()
    c = adamw_case()
    n = N_SMALL
    p, m, v = _padded(c["p0"]), _padded(np.zeros(n, np.float32)), _padded(np.zeros(n, np.float32))
    lr, step = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    g_all = torch.tensor(c["g"]).to(DEV)
    got = {}
    for k in range(40):
        lr.fill_(c["lrs"][k])
        _adamw_launch(lib, p, g_all[k], m, v, n, lr, step)
        if k + 1 in ADAMW_CHECKED:
            torch.cuda.synchronize()
            assert float(step) == float(k + 1)
            got[k + 1] = tuple(t[:n].cpu().numpy() for t in (p, m, v))
    assert float(step) == 40.0
    err = adamw_errors(got, c["ref64"])
    for s in ADAMW_CHECKED:
        print(f"adamw step {s:2d}: reference float32 " + " ".join(f"{e:.1e}" for e in c["ref_err"][s]) + " / kernel " + " ".join(f"{e:.1e}" for e in err[s]))
    assert adamw_within(err, c["tol"]), (err, c["tol"])
    assert _bits_kept(p, n) and _bits_kept(m, n) and _bits_kept(v, n)


def test_adamw_crosses_the_grid_cap_and_leaves_the_tail():
    """Three steps at n = 2048*256 + 257 (the grid-stride loop runs a second time), lr from the scheduler's warm-up: within 8 x the error of
    torch's float32 AdamW of torch.optim.AdamW in float64, and within the same bound of the numpy float32 restatement of the kernel
    element by element (the two differ by contraction and the device's sqrt / division only): no element of the second pass is skipped
    or written twice.  p, m and v past n keep their bits."""
    lib = L.load()
    n = N_BIG_OPTIM
    r = np.random.RandomState(99)
    p0 = r.randn(n).astype(np.float32)
    g = ((10.0 ** r.uniform(-8.0, 0.0, n))[None, :] * r.randn(3, n)).astype(np.float32)
    lrs = cosine_warmup_lrs(40)[9:12]
    z = np.zeros(n, np.float32)
    ref64 = adamw_torch(p0, g, lrs, torch.float64, checked=(3,))
    ref32 = adamw_torch(p0, g, lrs, torch.float32, checked=(3,))
    tol = {3: tuple(8.0 * float(np.abs(ref32[3][i].astype(np.float64) - ref64[3][i]).max()) for i in range(3))}
    want = adamw_f32(p0, g, z, z, lrs)
    assert adamw_within(adamw_errors(want, ref64), tol)
    p, m, v = _padded(p0), _padded(z), _padded(z)
    lr, step = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for k in range(3):
        lr.fill_(lrs[k])
        _adamw_launch(lib, p, _padded(g[k]), m, v, n, lr, step)
    torch.cuda.synchronize()
    got = {3: tuple(t[:n].cpu().numpy() for t in (p, m, v))}
    err = adamw_errors(got, ref64)
    assert float(step) == 3.0 and adamw_within(err, tol), (err, tol)
    for a, b, t_ in zip(got[3], want[3], tol[3]):
        assert float(np.abs(a.astype(np.float64) - b).max()) <= t_
    assert _bits_kept(p, n) and _bits_kept(m, n) and _bits_kept(v, n)


def _two_linear(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 11)).to(DEV)


def _grads_for(net, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randn(p.shape, generator=g) * 10.0 ** float(torch.empty(1).uniform_(-4, 0, generator=g))).to(DEV) for p in net.parameters()]
            for _ in range(steps)]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _state(opt):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (opt.model.flat_params, opt._m, opt._v, opt._step_dev)]


def test_fused_adamw_active_numel_skips_the_trailing_layer_like_torch():
    """flatten_parameters over two nn.Linear, the second without gradients and past FusedAdamW.active_numel: its weights and moments are not
    touched (torch.optim.AdamW skips a parameter whose .grad is None), while the first layer follows torch.optim.AdamW in float64."""
    net = _two_linear()
    ref = deepcopy(net).double().cpu()
    opt = FusedAdamW(net, lr=1e-2, weight_decay=0.05)
    n0 = sum(p.numel() for p in net[0].parameters())
    opt.active_numel = n0
    opt.grad_scale = 0.5
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=0.05)
    before = net.flat_params.detach().clone()
    grads = _grads_for(net[0], 4, 5)
    for k in range(4):
        _set_grads(list(net[0].parameters()), grads[k])
        for p, g in zip(ref[0].parameters(), grads[k]):
            p.grad = g.double().cpu() * 0.5
        opt.step()
        topt.step()
    flat, m, v, step = _state(opt)
    assert float(step) == 4.0
    assert torch.equal(flat[n0:], before[n0:]) and not m[n0:].any() and not v[n0:].any()
    want = torch.cat([p.detach().reshape(-1) for p in ref[0].parameters()])
    # four steps; a step rounds values no larger than max|w| four times (decay, quotient, product, difference) and the update itself, of size
    # ~lr, carries the ~8 roundings of the moments, the root and the corrections
    u = 2.0 ** -24
    assert float((flat[:n0].double().cpu() - want).abs().max()) <= 4 * (4 * u * float(want.abs().max()) + 8 * u * 1e-2)
    assert all(p.grad is None for p in ref[1].parameters()) and torch.equal(torch.cat([p.detach().reshape(-1) for p in ref[1].parameters()]).float(),
                                                                              before[n0:].cpu())


def test_fused_adamw_resume_is_bit_equal():
    """6 steps, state_dict() into a fresh FusedAdamW on a copy of the weights, 6 more == 12 uninterrupted steps: weights, both moments and
    the device step word, bit for bit."""
    lrs = cosine_warmup_lrs(12)
    net_a = _two_linear(3)
    init = deepcopy(net_a)
    grads = _grads_for(net_a, 12, 8)

    def run(opt, ks):
        for k in ks:
            opt.param_groups[0]["lr"] = lrs[k]
            _set_grads(list(opt.model.parameters()), grads[k])
            opt.step()

    a = FusedAdamW(net_a, lr=lrs[0], weight_decay=0.05)
    run(a, range(12))
    whole = _state(a)
    net_b = deepcopy(init)
    b = FusedAdamW(net_b, lr=lrs[0], weight_decay=0.05)
    run(b, range(6))
    sd = {k_: (v_.detach().clone() if torch.is_tensor(v_) else deepcopy(v_)) for k_, v_ in b.state_dict().items()}
    net_c = deepcopy(init)
    c = FusedAdamW(net_c, lr=lrs[0], weight_decay=0.05)
    with torch.no_grad():
        net_c.flat_params.copy_(net_b.flat_params)
    c.load_state_dict(sd)
    assert float(c._step_dev) == 6.0
    run(c, range(6, 12))
    resumed = _state(c)
    assert float(resumed[3]) == 12.0
    for x, y, name in zip(resumed, whole, ("p", "m", "v", "step")):
        assert torch.equal(x, y), name


def test_fused_adamw_step_replays_in_a_graph_bit_equal_to_eager():
    """One FusedAdamW.step(push_lr=False) captured on a side stream after two warm-up steps and replayed five times, lr written to the device
    word before each replay, equals five eager steps bit for bit (the step count advances on the device inside the graph; the captured
    launches form one chain)."""
    lrs = cosine_warmup_lrs(8)[1:]
    net_g = _two_linear(4)
    net_e = deepcopy(net_g)
    grads = _grads_for(net_g, 7, 9)
    og, oe = FusedAdamW(net_g, lr=lrs[0], weight_decay=0.05), FusedAdamW(net_e, lr=lrs[0], weight_decay=0.05)
    og.grad_scale = oe.grad_scale = 0.5
    for k in range(7):                         # the eager run: 2 + 5 steps
        oe.param_groups[0]["lr"] = lrs[k]
        _set_grads(list(net_e.parameters()), grads[k])
        oe.step()
    want = _state(oe)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(2):
            og.param_groups[0]["lr"] = lrs[k]
            _set_grads(list(net_g.parameters()), grads[k])
            og.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        og.step(push_lr=False)
    for k in range(2, 7):
        _set_grads(list(net_g.parameters()), grads[k])
        og._lr_dev.fill_(lrs[k])
        graph.replay()
    got = _state(og)
    assert float(got[3]) == 7.0
    for x, y, name in zip(got, want, ("p", "m", "v", "step")):
        assert torch.equal(x, y), name
