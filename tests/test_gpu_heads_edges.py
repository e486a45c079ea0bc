"""GPU: csrc/heads.hip entry point by entry point through hpfg_amd._lib, and hpfg_amd.utils.Dense_Loss end to end, against the float64
laws of tests/helpers.py ("dense kernels"; tests/test_dense_laws_host.py holds those against torch's float64 ops and autograd and shows
every named mutation caught by the rules used here).

Conventions (those of tests/test_gpu_tokens_edges.py and tests/test_gpu_gemm_edges.py): every output is a canary_out (all of it written,
the tail untouched); an input with a pixel stride above its channel count carries the NaN pattern in the unused floats.  The pooling and
l2norm kernels and Q of NT-Xent lie within bound_8x of the law (8 x the error of torch's float32 CPU op, floor 4 float32 ulp of the law's
largest magnitude).  The NT-Xent value is a difference log(denom_i) - G[i,p(i)] / T of terms as large as 16 / 0.7: its bound is
max(8 x |float32 yardstick - law|, 4 float32 ulp of the largest term).  At n = 1 the law's Q is exactly zero and is compared bit for bit.
A column of l2norm that the clamp holds (or that sits just above it) has a gradient 1e12 times the others': it is compared on its own.

Which test holds which entry point:
  hpfg_neck_pool_fwd   test_neck_pool_forward, test_neck_refusals
  hpfg_neck_pool_bwd   test_neck_pool_backward
  hpfg_l2norm_fwd      test_l2norm_forward_and_backward, test_l2norm_refusals
  hpfg_l2norm_bwd      test_l2norm_forward_and_backward, test_l2norm_refusals
  hpfg_ntxent_rows     test_ntxent_rows, test_ntxent_without_q, test_ntxent_refusals
  (hpfg_gemm_f32_splitk between them: test_dense_loss_end_to_end)

Measured on the MI355X, largest error / bound per family (1.0 is the limit):
  neck pooling    gap 0.24   pool 0.12   dx 0.14
  l2norm          u 0.32   norms 0.22   dx 0.27      zero / tiny column on its own: u 0.11   norms 0.12   dx 0.13
  NT-Xent         loss 0.45   Q 0.30   (Q at n = 1: exactly zero)
  Dense_Loss      value 0.05   dg 0.18   dd 0.18
"""
import pytest
import torch

from hpfg_amd import _lib as L
from tests import helpers as H
from tests.helpers import bits_kept, bound_8x, canary_ok, canary_out, report, stream, within_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return t.contiguous().to(DEV)


# ---- neck pooling --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.POOL_CASES, ids=str)
def test_neck_pool_forward(case):
    """Bins that tile the image (gap from the bin means) and bins that overlap; C = 3 and 5; pstride > C with the NaN pattern in the unused
    floats; channel chunks of grid z with a last chunk of 4 channels (64 slots), of 1 channel (256 slots) and four full chunks; S = 1; a
    bin of 1155 pixels over 64 slots (the four-way unrolled loop and its remainder); the bottleneck's own shape."""
    N, Hh, W, C_, S, ps = case
    lib, st = L.load(), stream(DEV)
    c = H.pool_case(N, Hh, W, C_, S)
    buf = H.nan_filled(N * Hh * W * ps).view(N, Hh, W, ps)
    buf[..., :C_] = c["x"]
    xd = _dev(buf)
    gap, pool = canary_out(N * C_), canary_out(N * S * S * C_)
    L.check(lib.hpfg_neck_pool_fwd(L.ptr(xd), ps, N, Hh, W, C_, S, L.ptr(gap), L.ptr(pool), st), "neck_pool_fwd")
    torch.cuda.synchronize()
    within_bound(f"neck_pool_fwd {case} gap", gap, c["gap"], bound_8x(c["gap"], c["gap32"]))
    within_bound(f"neck_pool_fwd {case} pool", pool, c["pool"], bound_8x(c["pool"], c["pool32"]))


@pytest.mark.parametrize("which", ["gap", "pool", "both"])
@pytest.mark.parametrize("case", H.POOL_CASES, ids=str)
def test_neck_pool_backward(case, which):
    """dgap only, dpool only, both: float64 autograd of the forward law"""
    N, Hh, W, C_, S, _ = case
    lib, st = L.load(), stream(DEV)
    c = H.pool_case(N, Hh, W, C_, S)
    dg = _dev(c["dgap"]) if which != "pool" else None
    dp = _dev(c["dpool"]) if which != "gap" else None
    dx = canary_out(N * Hh * W * C_)
    L.check(lib.hpfg_neck_pool_bwd(L.ptr(dg), L.ptr(dp), N, Hh, W, C_, S, L.ptr(dx), st), "neck_pool_bwd")
    torch.cuda.synchronize()
    law = c["dx_" + which]
    within_bound(f"neck_pool_bwd {case[:5]} {which}", dx, law, bound_8x(law, c["dx32_" + which]))


def test_neck_refusals():
    """-1 with nothing launched: C = 1025, S > H, S > W, pstride < C; the backward without either gradient"""
    lib, st = L.load(), stream(DEV)
    x = torch.zeros(8 * 8 * 1025, device=DEV)
    gap, pool = canary_out(1025), canary_out(16 * 1025)
    p, g, q = L.ptr(x), L.ptr(gap), L.ptr(pool)
    assert lib.hpfg_neck_pool_fwd(p, 1025, 1, 8, 8, 1025, 2, g, q, st) == -1
    assert lib.hpfg_neck_pool_fwd(p, 4, 1, 3, 8, 4, 4, g, q, st) == -1
    assert lib.hpfg_neck_pool_fwd(p, 4, 1, 8, 3, 4, 4, g, q, st) == -1
    assert lib.hpfg_neck_pool_fwd(p, 3, 1, 8, 8, 4, 4, g, q, st) == -1
    assert lib.hpfg_neck_pool_bwd(None, None, 1, 8, 8, 4, 4, g, st) == -1
    torch.cuda.synchronize()
    assert bits_kept(gap, 0) and bits_kept(pool, 0)


# ---- F.normalize ---------------------------------------------------------------------------------------------------------------------------
def _l2norm_compare(name, c, key, buf, layout, scale=1.0):
    G, D, S = c["x"].shape
    law = c[key] * scale
    n = law.numel()
    written, tail = canary_ok(buf, n)
    assert written and tail, f"{name}: output not fully written, or written past its end"
    flat = buf[:n].cpu().double()
    got = flat.view(G, S) if key == "norms" else H.l2norm_unlayout(flat, G, D, S, layout)
    assert bool(torch.isfinite(got).all()), name
    for part, (g_, l_, y_) in enumerate(zip(H.l2norm_parts(c, got), H.l2norm_parts(c, law), H.l2norm_parts(c, c[key + "32"] * scale))):
        err, bound = float((g_ - l_).abs().max()), bound_8x(l_, y_)
        report(f"{name} {key}" + (" (special column)" if c["special"] and part == 0 else ""), err, bound)
        assert err <= bound, (name, key, part, err, bound)


@pytest.mark.parametrize("scale", [None, 3.0])
@pytest.mark.parametrize("layout", H.L2NORM_LAYOUTS)
@pytest.mark.parametrize("special", H.L2NORM_SPECIAL, ids=["plain", "zero_column", "tiny_column"])
@pytest.mark.parametrize("G,D,S", H.L2NORM_CASES)
def test_l2norm_forward_and_backward(G, D, S, special, layout, scale):
    """D below a wave, a multiple of it, one past it, two strides, and 200 (one column, a quarter-filled workgroup); both layouts; scale
    NULL or a device scalar.  zero_column: the clamp (u = 0, norm = 1e-12, dx = scale du / 1e-12).  tiny_column: a norm of 3e-12, where
    x / (norm + eps) would be a quarter short."""
    lib, st = L.load(), stream(DEV)
    c = H.l2norm_case(G, D, S, special)
    sd, ss = (S, 1) if layout == "ds" else (1, D)
    xd, dud = _dev(H.l2norm_layout(c["x"], layout)), _dev(H.l2norm_layout(c["du"], layout))
    u, norms, dx = canary_out(G * D * S), canary_out(G * S), canary_out(G * D * S)
    sc = torch.tensor([scale], device=DEV) if scale is not None else None
    L.check(lib.hpfg_l2norm_fwd(L.ptr(xd), G, D, S, sd, ss, L.ptr(u), L.ptr(norms), st), "l2norm_fwd")
    L.check(lib.hpfg_l2norm_bwd(L.ptr(dud), L.ptr(u), L.ptr(norms), G, D, S, sd, ss, L.ptr(sc), L.ptr(dx), st), "l2norm_bwd")
    torch.cuda.synchronize()
    name = f"l2norm {(G, D, S)} {layout} {special or 'plain'} scale={scale}"
    _l2norm_compare(name, c, "u", u, layout)
    _l2norm_compare(name, c, "norms", norms, layout)
    _l2norm_compare(name, c, "dx", dx, layout, scale or 1.0)
    if special == "zero":
        col = H.l2norm_unlayout(u[:G * D * S].cpu(), G, D, S, layout)[0, :, 0]
        assert not col.any() and float(norms[0].cpu()) == float(torch.tensor(H.L2NORM_EPS, dtype=torch.float32))


def test_l2norm_refusals():
    """(sd, ss) must be (S, 1) or (1, D)"""
    lib, st = L.load(), stream(DEV)
    x = torch.zeros(256, device=DEV)
    out = canary_out(256)
    p, o = L.ptr(x), L.ptr(out)
    for sd, ss in ((1, 1), (3, 8), (8, 3), (2, 1)):
        assert lib.hpfg_l2norm_fwd(p, 2, 8, 3, sd, ss, o, o, st) == -1
        assert lib.hpfg_l2norm_bwd(p, p, p, 2, 8, 3, sd, ss, None, o, st) == -1
    assert lib.hpfg_l2norm_fwd(p, 0, 8, 3, 3, 1, o, o, st) == -1
    torch.cuda.synchronize()
    assert bits_kept(out, 0)


# ---- NT-Xent -------------------------------------------------------------------------------------------------------------------------------
def _ntxent_run(c, with_q=True):
    lib, st = L.load(), stream(DEV)
    n = c["n"]
    gd = _dev(c["G"])
    loss, Q = canary_out(1), canary_out(n * 2 * n) if with_q else None
    L.check(lib.hpfg_ntxent_rows(L.ptr(gd), n, c["T"], L.ptr(loss), L.ptr(Q), st), "ntxent_rows")
    torch.cuda.synchronize()
    return loss, Q


@pytest.mark.parametrize("T_,S", H.NTXENT_T, ids=["T0.7_S16", "T0.07_unit"])
@pytest.mark.parametrize("family", H.NTXENT_FAMILIES)
@pytest.mark.parametrize("n", H.NTXENT_N)
def test_ntxent_rows(n, family, T_, S):
    """n = 1 (denom = pos: loss 0, Q zero), 2, odd 3 and 127, 32, and the limit 2n = 256; teacher rows independent of the student's (loss
    of order log 2n), near copies (loss near 0: the floor of the value's tolerance), and a Gram matrix that is not symmetric (both
    orientations are read as stored: a transposed index shows)."""
    c = H.ntxent_case(family, n, T_, S)
    loss, Q = _ntxent_run(c)
    name = f"ntxent n={n} {family} T={T_}"
    within_bound(name + " loss", loss, c["law"][0].reshape(1), c["tol"][0])
    if n == 1:
        assert all(canary_ok(Q, 2)) and torch.equal(Q[:2].cpu(), torch.zeros(2)), name
    else:
        within_bound(name + " Q", Q, c["law"][1], c["tol"][1])


def test_ntxent_without_q():
    c = H.ntxent_case("independent", 32, 0.7, 16)
    loss, _ = _ntxent_run(c, with_q=False)
    within_bound("ntxent n=32 Q=NULL loss", loss, c["law"][0].reshape(1), c["tol"][0])


def test_ntxent_refusals():
    lib, st = L.load(), stream(DEV)
    g = torch.zeros(4, device=DEV)
    out = canary_out(8)
    for n, T_ in ((0, 0.7), (129, 0.7), (1, 0.0), (1, -0.7)):
        assert lib.hpfg_ntxent_rows(L.ptr(g), n, T_, L.ptr(out), L.ptr(out), st) == -1
    torch.cuda.synchronize()
    assert bits_kept(out, 0)


# ---- Dense_Loss end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position_major", [False, True], ids=["canonical", "position_major"])
@pytest.mark.parametrize("n", H.DENSE_N)
def test_dense_loss_end_to_end(n, position_major):
    """hpfg_amd.utils.Dense_Loss (l2norm, the Gram matrix on hpfg_gemm_f32, NT-Xent, Q U, l2norm backward) against float64 autograd of
    oracle.losses_ref.dense_loss: the value under the NT-Xent value rule, the student gradients under bound_8x.  position_major: the dense
    features live in [n, S, D] memory, as the projection neck produces them."""
    from hpfg_amd.utils import Dense_Loss
    c = H.dense_case(n)

    def put(t):
        if position_major and t.dim() == 3:
            return t.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
        return t.contiguous().to(DEV)
    sg, sd_ = put(c["sg"]).requires_grad_(True), put(c["sd"]).requires_grad_(True)
    assert sd_.permute(0, 2, 1).is_contiguous() == position_major
    loss = Dense_Loss(batch_size=n, temperature=0.7)((sg, sd_), (put(c["tg"]), put(c["td"])))
    dg, dd = torch.autograd.grad(loss, (sg, sd_))
    torch.cuda.synchronize()
    name = f"Dense_Loss n={n} {'position-major' if position_major else 'canonical'}"
    ref, yard = c["ref"], c["yard"]
    err, bound = abs(float(loss) - float(ref[0])), max(8.0 * abs(float(yard[0]) - float(ref[0])), 4.0 * H.ulp32(c["top"]))
    report(name + " value", err, bound)
    assert err <= bound, (name, err, bound)
    for k, got in ((1, dg), (2, dd)):
        err, bound = float((got.cpu().double() - ref[k]).abs().max()), bound_8x(ref[k], yard[k])
        report(name + (" dg" if k == 1 else " dd"), err, bound)
        assert bool(torch.isfinite(got).all()) and err <= bound, (name, k, err, bound)
