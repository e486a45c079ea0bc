"""GPU: the fused loss kernels of csrc/loss.hip, entry point by entry point (hpfg_seg_loss_partials, _finalize, _bwd through hpfg_amd._lib),
and the entropy mask of csrc/misc.hip, against the float64 laws of tests/helpers.py (tests/test_loss_laws_host.py holds those against
oracle.losses_ref, torch's float64 ops and the reference's stored outputs) at every class count, mode and dispatch edge.

Conventions.  `partials`, `sums`, `out` and `dlogits` are allocated with a tail and filled with a quiet-NaN bit pattern (helpers.canary_out):
after the launches no element holds the pattern and the tail kept its bits.  `sums`, `out` and `dlogits` must lie within helpers.bound_8x of
the law: 8 x the error the same law makes when it is evaluated in float32 on the CPU, and no less than 4 float32 ulp of the largest
magnitude.  For `sums` the rule holds per entry group (nll, I, Z, mse, mask sum: helpers.loss_sum_groups), so that a large nll hides no small
I; the counts and Y are sums of ones below 2^24 and must be exact, as must the slots 6, 7 and the class slots c >= C (zero).
tests/test_loss_laws_host.py shows that this tolerance tells five named mistakes from rounding by a factor of at least 4.

Every compared tensor prints its error / bound (pytest -s); DESIGN.md (the fused loss) quotes a run on the MI355X per class count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd.utils import seg_loss
from tests import helpers as H
from tests.helpers import bound_8x, bits_kept, canary_ok, canary_out, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BWD_CAP = 4096 * 256          # pixels one pass of loss_bwd_kernel's grid covers


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _coef(v):
    return torch.tensor(list(v) + [0.0] * (8 - len(v)), dtype=torch.float32, device=DEV)


class Run:
    """One partials / finalize / backward sequence on canary buffers.  Keyword arguments as helpers.loss_f64's; grad_scale None passes NULL."""

    def __init__(self, logits, labels0, labels1, n_lab, coef, t=None, teacher_is_prob=False, t_unlab_only=False, cons_mask=None,
                 input_is_prob=False, world=1, grad_scale=None):
        lib = L.load()
        N, Hh, W, C_ = logits.shape
        self.shape, self.C = (N, Hh, W, C_), C_
        self.nblk, self.nsum = lib.hpfg_loss_blocks(N, Hh, W), lib.hpfg_loss_nsum(C_)
        assert self.nsum == H.loss_nsum(C_) and self.nblk == (N * Hh * W + 1023) // 1024
        self.keep = [_dev(logits), _dev(t), _dev(labels0), _dev(labels1), _coef(coef), _dev(cons_mask),
                     None if grad_scale is None else torch.tensor([grad_scale], dtype=torch.float32, device=DEV)]
        self.partials, self.sums, self.out = canary_out(self.nblk * self.nsum), canary_out(self.nsum), canary_out(8)
        self.dlogits = canary_out(N * Hh * W * C_)
        a = self.a = L.LossArgs()
        a.logits, a.t_logits, a.labels0, a.labels1, a.coef, a.cons_mask = (L.ptr(x) for x in self.keep[:6])
        a.partials, a.sums, a.out, a.dlogits = L.ptr(self.partials), L.ptr(self.sums), L.ptr(self.out), L.ptr(self.dlogits)
        a.N, a.n_lab, a.H, a.W, a.C, a.world = N, n_lab, Hh, W, C_, world
        a.input_is_prob, a.teacher_is_prob, a.t_unlab_only = int(input_is_prob), int(teacher_is_prob), int(t_unlab_only)

    def launch(self):
        lib, st = L.load(), stream(DEV)
        L.check(lib.hpfg_seg_loss_partials(C.byref(self.a), st), "seg_loss_partials")
        L.check(lib.hpfg_seg_loss_finalize(C.byref(self.a), st), "seg_loss_finalize")
        L.check(lib.hpfg_seg_loss_bwd(C.byref(self.a), L.ptr(self.keep[6]), st), "seg_loss_bwd")
        torch.cuda.synchronize()
        return self

    def buffers(self):
        return (("partials", self.partials, self.nblk * self.nsum), ("sums", self.sums, self.nsum), ("out", self.out, 8),
                ("dlogits", self.dlogits, int(np.prod(self.shape))))

    def results(self):
        """(sums, out, dlogits) on the CPU after the canary checks."""
        for name, buf, n in self.buffers():
            written, tail = canary_ok(buf, n)
            assert written, f"{name}: elements were never written"
            assert tail, f"{name}: the launch wrote past the end"
        return self.sums[:self.nsum].cpu(), self.out[:8].cpu(), self.dlogits[:int(np.prod(self.shape))].cpu().reshape(self.shape)


def _ratio(tag, name, C_, got, ref64, ref32):
    err = float((got.double() - ref64).abs().max())
    bound = bound_8x(ref64, ref32)
    r = err / bound
    print(f"  RATIO C={C_:<2d} {name:<8s} {tag:<58s} max|err| {err:9.3e}  bound {bound:9.3e}  ratio {r:6.3f}")
    return err, bound


def _compare(tag, run, kw):
    """The run's sums, out and dlogits against the law of the same keyword arguments.  -> (sums, out, dlogits, law64)"""
    law = {k: v for k, v in kw.items() if k != "grad_scale"}
    gs = 1.0 if kw.get("grad_scale") is None else kw["grad_scale"]
    s64, o64, g64 = H.loss_f64(**law, grad_scale=gs)
    s32, o32, g32 = H.loss_f64(**law, grad_scale=gs, dtype=torch.float32)
    sums, out, dl = run.results()
    C_ = run.C
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(out).all()) and bool(torch.isfinite(dl).all()), tag
    fails = []
    groups = H.loss_sum_groups(C_)
    for name in ("cnt", "Y"):          # sums of ones, and the zeros of the class slots c >= C
        assert torch.equal(sums[groups[name]].double(), s64[groups[name]]), (tag, name)
    assert float(sums[6]) == 0.0 and float(sums[7]) == 0.0, tag
    for name in ("nll", "I", "Z", "mse", "mask"):
        i = groups[name]
        err, bound = _ratio(tag, name, C_, sums[i], s64[i], s32[i])
        if err > bound:
            fails.append((name, err, bound))
        assert bool((sums[i][s64[i] == 0] == 0).all()), (tag, name, "a slot that the law leaves at zero")
    for j, name in enumerate(("total", "ce0", "dice0", "ce1", "dice1", "mse_out")):
        err, bound = _ratio(tag, name, C_, out[j:j + 1], o64[j:j + 1], o32[j:j + 1])
        if err > bound:
            fails.append((name, err, bound))
    assert float(out[6]) == 0.0 and float(out[7]) == 0.0, tag
    err, bound = _ratio(tag, "dlogits", C_, dl, g64, g32)
    if err > bound:
        fails.append(("dlogits", err, bound))
    assert not fails, (tag, fails)
    return sums, out, dl, (s64, o64, g64)


def _run_and_compare(tag, kw):
    return _compare(tag, Run(**kw).launch(), kw)


# ---- every class count, both shapes, both coefficient sets, five modes ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", H.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C_", range(2, 17))
def test_every_class_count_and_mode(C_, shape):
    """(3, 1, 24, 24): the group boundary at pixel 576 falls inside the first 1024-pixel block with (pb - p0) % 256 == 64.  (2, 2, 40, 28): blocks
    straddle the image boundary and group 1 is empty.  partials and backward kernels of this C both launch in every mode."""
    N, nl, Hh, W = shape
    assert (nl * Hh * W) % 256 == (64 if nl < N else 192) and (Hh * W) % 1024 != 0
    case = H.loss_case(C_, *shape)
    for K in (H.LOSS_K, H.LOSS_K_DEAD):
        for mode in H.LOSS_MODES:
            kw = H.loss_mode_kwargs(case, mode, K)
            sums, out, dl, _ = _run_and_compare(f"{shape} K1={K[2]} {mode}", kw)
            if nl == N or (mode in ("no_teacher", "prob_input")):
                assert float(out[5]) == 0.0 and float(sums[4]) == 0.0 and float(sums[5]) == 0.0
            if nl == N:
                assert float(out[3]) == 0.0 and float(out[4]) == 0.0


# ---- segment edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 32, 32), (2, 1, 8, 8), (5, 2, 1, 333)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C_", [3, 6])
def test_segment_edges(C_, shape):
    """The boundary on a block edge (1024); 128 pixels for 256 threads; one-row images with a ragged last block (1665 pixels, boundary at 666)."""
    case = H.loss_case(C_, *shape)
    for mode in ("teacher_logits", "masked"):
        _run_and_compare(f"{shape} {mode}", H.loss_mode_kwargs(case, mode))


@pytest.mark.parametrize("C_", [3, 6])
def test_no_labelled_images_and_null_labels0(C_):
    case = H.loss_case(C_, 3, 0, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    assert kw["labels0"] is None and kw["n_lab"] == 0
    sums, out, _, _ = _run_and_compare("n_lab=0", kw)
    assert float(out[1]) == 0.0 and float(out[2]) == 0.0 and float(sums[0]) == 0.0 and float(sums[1]) == 0.0


@pytest.mark.parametrize("C_", [3, 6])
def test_all_labelled_with_a_teacher_present(C_):
    case = H.loss_case(C_, 3, 3, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    assert kw["labels1"] is None and kw["t"] is not None
    sums, out, _, _ = _run_and_compare("n_lab=N teacher", kw)
    assert bool((sums[2:6] == 0).all()) and bool((out[3:6] == 0).all())


@pytest.mark.parametrize("C_", [3, 6, 16])
def test_teacher_without_pseudo_labels(C_):
    """Mean Teacher's shape: group 1 has a consistency target and no labels."""
    case = H.loss_case(C_, 3, 1, 24, 24)
    kw = dict(H.loss_mode_kwargs(case, "teacher_logits"), labels1=None)
    sums, out, _, _ = _run_and_compare("labels1=NULL teacher", kw)
    S = H.loss_stride(C_)
    assert float(out[3]) == 0.0 and float(out[4]) == 0.0 and bool((sums[2:4] == 0).all()) and bool((sums[H.LOSS_OFF + 3 * S:] == 0).all())
    assert float(out[5]) > 0.0


# ---- degenerate groups -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [3, 6])
def test_group_with_every_pixel_ignored(C_):
    case = H.loss_case(C_, 3, 1, 24, 24)
    kw = dict(H.loss_mode_kwargs(case, "teacher_logits"), labels0=torch.full_like(case["labels0"], 255))
    sums, out, dl, _ = _run_and_compare("group 0 all 255", kw)
    S = H.loss_stride(C_)
    assert float(out[1]) == 0.0 and float(sums[0]) == 0.0 and float(sums[1]) == 0.0
    assert bool((sums[H.LOSS_OFF:H.LOSS_OFF + S] == 0).all()) and bool((sums[H.LOSS_OFF + 2 * S:H.LOSS_OFF + 3 * S] == 0).all())      # I and Y
    assert float(out[2]) > 0.0


@pytest.mark.parametrize("C_", [3, 6])
def test_labels_outside_the_classes_only(C_):
    """Ids in [C, 255) match no class and carry no cross-entropy."""
    case = H.loss_case(C_, 3, 1, 24, 24)
    odd = torch.full_like(case["labels1"], C_ + 1)
    odd[:, ::2] = 254
    kw = dict(H.loss_mode_kwargs(case, "teacher_logits"), labels1=odd)
    sums, out, _, _ = _run_and_compare("group 1 ids in [C, 255)", kw)
    assert float(out[3]) == 0.0 and float(sums[2]) == 0.0 and float(sums[3]) == 0.0


@pytest.mark.parametrize("C_", [3, 6])
def test_all_zero_consistency_mask(C_):
    case = H.loss_case(C_, 3, 1, 24, 24)
    kw = dict(H.loss_mode_kwargs(case, "masked"), cons_mask=torch.zeros_like(case["mask"]))
    sums, out, dl, _ = _run_and_compare("mask all zero", kw)
    assert float(out[5]) == 0.0 and float(sums[4]) == 0.0 and float(sums[5]) == 0.0
    _, _, dl_sup = Run(**H.loss_mode_kwargs(case, "no_teacher")).launch().results()
    assert torch.equal(dl, dl_sup)          # the consistency term added exactly 0 to every gradient


# ---- world, grad_scale_dev -------------------------------------------------------------------------------------------------------------------
def _halves(a, b):
    """b == a / 2 bit for bit wherever a is far above the subnormal range (a scaling by a power of two is exact there)."""
    big = a.abs() >= 2.0 ** -100
    return torch.equal(b[big] * 2.0, a[big]) and bool((b[~big].abs() <= a[~big].abs()).all())


@pytest.mark.parametrize("C_", [3, 6])
def test_world_two_halves_the_mse_and_its_gradient(C_):
    case = H.loss_case(C_, 3, 1, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    s1, o1, _, _ = _run_and_compare("world=1", kw)
    s2, o2, _, _ = _run_and_compare("world=2", dict(kw, world=2))
    assert torch.equal(s1, s2) and float(o2[5]) * 2.0 == float(o1[5]) and torch.equal(o1[1:5], o2[1:5])
    only = dict(kw, coef=(0.0, 0.0, 0.0, 0.0, 0.3))          # the MSE alone: its gradient halves exactly
    _, _, g1, _ = _run_and_compare("world=1 mse only", only)
    _, _, g2, _ = _run_and_compare("world=2 mse only", dict(only, world=2))
    assert float(g1.abs().max()) > 0.0 and _halves(g1, g2)


@pytest.mark.parametrize("C_", [3, 6])
def test_grad_scale_device_scalar(C_):
    case = H.loss_case(C_, 3, 1, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    _, _, g_null, _ = _run_and_compare("grad_scale NULL", kw)
    _, _, g_one, _ = _run_and_compare("grad_scale 1.0", dict(kw, grad_scale=1.0))
    _, _, g_half, _ = _run_and_compare("grad_scale 0.5", dict(kw, grad_scale=0.5))
    _run_and_compare("grad_scale 1/3", dict(kw, grad_scale=1.0 / 3.0))
    assert torch.equal(g_null, g_one) and _halves(g_one, g_half)


# ---- saturated logits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [4, 7])
def test_saturated_logits(C_):
    """Logits x 30: expf underflows to 0 for the losing classes (the law goes through logsumexp); everything stays finite and within bound."""
    for shape in H.LOSS_SHAPES:
        case = dict(H.loss_case(C_, *shape))
        case["logits"], case["t_logits"] = case["logits"] * 30.0, case["t_logits"] * 30.0
        assert int((torch.softmax(case["logits"], -1) == 0).sum()) > 0
        for mode in H.LOSS_MODES:
            _run_and_compare(f"{shape} x30 {mode}", H.loss_mode_kwargs(case, mode))


# ---- the backward past its grid cap ----------------------------------------------------------------------------------------------------------
def test_backward_takes_a_second_grid_stride_trip():
    N, nl, Hh, W = 2, 1, 1, 524417
    npix = N * Hh * W
    assert npix == BWD_CAP + 258 and npix > 1048576 and (nl * Hh * W) % 1024 % 256 != 0
    print(f"  backward over {npix} pixels, {(npix + 1023) // 1024} blocks of partial sums")
    case = H.loss_case(2, N, nl, Hh, W)
    run = Run(**H.loss_mode_kwargs(case, "teacher_logits")).launch()
    assert run.nblk == 1025
    _compare("1,048,834 pixels", run, H.loss_mode_kwargs(case, "teacher_logits"))


# ---- argument errors -------------------------------------------------------------------------------------------------------------------------
def _refused(run, calls=("partials", "finalize", "bwd")):
    lib, st = L.load(), stream(DEV)
    fn = {"partials": lambda: lib.hpfg_seg_loss_partials(C.byref(run.a), st), "finalize": lambda: lib.hpfg_seg_loss_finalize(C.byref(run.a), st),
          "bwd": lambda: lib.hpfg_seg_loss_bwd(C.byref(run.a), None, st)}
    for c in calls:
        assert fn[c]() == -1, c
        assert len(lib.hpfg_last_error()) > 0, c
    torch.cuda.synchronize()
    for name, buf, _ in run.buffers():
        assert bits_kept(buf, 0), f"{name} was written by a refused call"


def test_argument_errors_launch_nothing():
    case = H.loss_case(3, 3, 1, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    for C_ in (1, 17):
        run = Run(**kw)
        run.a.C = C_
        _refused(run)
    run = Run(**kw)
    run.a.n_lab = 4
    _refused(run)
    run = Run(**kw)
    run.a.labels0 = None
    _refused(run)
    run = Run(**kw)
    run.a.world = 0
    _refused(run)
    for field, call in (("partials", "partials"), ("out", "finalize"), ("dlogits", "bwd")):
        run = Run(**kw)
        setattr(run.a, field, None)
        _refused(run, (call,))
    _compare("after the refusals", Run(**kw).launch(), kw)          # the library still works


# ---- through seg_loss, the Python surface ----------------------------------------------------------------------------------------------------
def test_seg_loss_layouts_and_errors():
    case = H.loss_case(6, 3, 1, 24, 24)
    kw = H.loss_mode_kwargs(case, "teacher_logits")
    nchw = lambda t: t.permute(0, 3, 1, 2)
    lab0, lab1 = _dev(case["labels0"]), _dev(case["labels1"])
    res = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        lg = nchw(case["logits"]).contiguous(memory_format=fmt).to(DEV).requires_grad_(True)
        tl = nchw(case["t_logits"]).contiguous(memory_format=fmt).to(DEV)
        out = seg_loss(lg, lab0, 1, coef=_coef(H.LOSS_K), pseudo=lab1, teacher_logits=tl)
        out[0].backward()
        res.append((out.detach().cpu(), lg.grad.permute(0, 2, 3, 1).contiguous().cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    _, o64, g64 = H.loss_f64(**kw)
    _, o32, g32 = H.loss_f64(**kw, dtype=torch.float32)
    assert float((res[0][0][:6].double() - o64[:6]).abs().max()) <= bound_8x(o64[:6], o32[:6])
    assert float((res[0][1].double() - g64).abs().max()) <= bound_8x(g64, g32)
    lg = nchw(case["logits"]).contiguous().to(DEV)
    with pytest.raises(ValueError):
        seg_loss(lg, lab0, 1, coef=_coef(H.LOSS_K), pseudo=lab1, teacher_logits=nchw(case["t_logits"])[:1].contiguous().to(DEV))
    with pytest.raises(ValueError):
        seg_loss(lg, lab0, 1, coef=_coef(H.LOSS_K), teacher_logits=lg, cons_mask=torch.ones(2, 1, 24, 23, device=DEV))
    # n_lab = 0 with labels = None
    lg = nchw(case["logits"]).contiguous().to(DEV).requires_grad_(True)
    out = seg_loss(lg, None, 0, coef=_coef(H.LOSS_K), pseudo=_dev(torch.cat([case["labels0"], case["labels1"]])), teacher_logits=nchw(case["t_logits"]).to(DEV))
    out[0].backward()
    kw0 = dict(kw, labels0=None, labels1=torch.cat([case["labels0"], case["labels1"]]), n_lab=0)
    _, o64, g64 = H.loss_f64(**kw0)
    _, o32, g32 = H.loss_f64(**kw0, dtype=torch.float32)
    assert float(abs(out[0].detach().cpu().double() - o64[0])) <= bound_8x(o64[:1], o32[:1])
    assert float((lg.grad.permute(0, 2, 3, 1).cpu().double() - g64).abs().max()) <= bound_8x(g64, g32)


# ---- the entropy mask that feeds cons_mask (csrc/misc.hip) -----------------------------------------------------------------------------------
def _unc_launch(preds, T, S, n_blocks, thr, C_=None, per_block=None):
    lib = L.load()
    n, Hh, W, Cp = preds.shape
    per = per_block if per_block is not None else n // n_blocks
    keep = [_dev(preds[i * per:(i + 1) * per]) if (i + 1) * per <= n else _dev(preds[:per]) for i in range(n_blocks)]
    pb = L.PredBlocks()
    for i, b in enumerate(keep):
        pb.p[i] = L.ptr(b)
    pb.n_blocks, pb.per_block = n_blocks, per
    mask, u = canary_out(S * Hh * W), canary_out(S * Hh * W)
    thr_d = torch.tensor([thr], dtype=torch.float32, device=DEV)
    rc = lib.hpfg_uncertainty_mask(C.byref(pb), T, S, Hh, W, Cp if C_ is None else C_, L.ptr(thr_d), L.ptr(mask), L.ptr(u), stream(DEV))
    torch.cuda.synchronize()
    return rc, mask, u


@pytest.mark.parametrize("C_", range(1, 9))
def test_uncertainty_mask_every_class_count_and_block_split(C_):
    """C = 1 .. 8 at S = 3, 16 x 24 pixels, T = 8, the 24 predictions in 1, 2, 4 and 8 blocks.  The threshold sits in the middle of the widest gap
    of the float64 u in the middle half of its distribution, at least 100 bounds wide: the reference alone decides every pixel.  C = 1 has no
    such gap (p = 1, u is the constant -log(1 + 1e-6) at every pixel): there the threshold is put 1e-3 below and above the constant, equally
    at least 100 bounds away, and the mask must be all zeros and all ones."""
    T, S = 8, 3
    preds = H.uncertainty_case(C_)
    n = S * preds.shape[1] * preds.shape[2]
    u64 = H.uncertainty_f64(preds, T)
    bound = bound_8x(u64, H.uncertainty_f64(preds, T, torch.float32))
    if C_ == 1:
        thresholds = [(-1e-3, 1e-3 - 1e-6), (1e-3, 1e-3)]
    else:
        thresholds = [H.uncertainty_threshold(u64)]
        thresholds[0] = (thresholds[0][0], 0.5 * thresholds[0][1])
    ref_u = None
    for thr, clearance in thresholds:
        assert clearance >= 100.0 * bound and float((u64 - thr).abs().min()) >= 100.0 * bound, (C_, thr, clearance, bound)
        want = (u64 < H.f32_exact(thr)).float().reshape(-1)
        for n_blocks in (1, 2, 4, 8):
            rc, mask, u = _unc_launch(preds, T, S, n_blocks, thr)
            assert rc == 0, L.load().hpfg_last_error()
            for name, buf in (("mask", mask), ("u", u)):
                written, tail = canary_ok(buf, n)
                assert written and tail, (name, n_blocks, written, tail)
            got = u[:n].cpu()
            err = float((got.double().reshape(u64.shape) - u64).abs().max())
            print(f"  RATIO C={C_:<2d} entropy  blocks={n_blocks} thr={thr:.6g}  max|err| {err:9.3e}  bound {bound:9.3e}  ratio {err / bound:6.3f}")
            assert err <= bound, (C_, n_blocks, err, bound)
            assert torch.equal(mask[:n].cpu(), want), (C_, n_blocks, int((mask[:n].cpu() != want).sum()))
            if ref_u is None:
                ref_u = got
            assert torch.equal(got, ref_u)          # the block split is addressing only


def test_uncertainty_mask_argument_errors():
    preds = H.uncertainty_case(8)
    lib = L.load()
    for kw in (dict(n_blocks=1, C_=9), dict(n_blocks=5, per_block=5), dict(n_blocks=4, per_block=5)):
        rc, mask, u = _unc_launch(preds, 8, 3, kw["n_blocks"], 0.5, kw.get("C_"), kw.get("per_block"))
        assert rc == -1 and len(lib.hpfg_last_error()) > 0, kw
        assert bits_kept(mask, 0) and bits_kept(u, 0), kw
