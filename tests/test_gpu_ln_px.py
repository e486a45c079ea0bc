"""GPU: hpfg_ln_px_fwd / hpfg_ln_px_bwd (csrc/tokens.hip) -- LayerNorm with eps as an argument, written through the pixel shuffle of the
Swin-UNet patch expanding -- through hpfg_amd._lib, with the conventions of tests/test_gpu_tokens_edges.py: NaN canaries with tails on every
output and on the partial sums, and helpers.bound_8x against the float64 law with eps (tests/helpers_swinunet.py).  Where the old entry
points apply (P = 1, eps 1e-5, C <= 1024) the bits are theirs, and the row map is pure data movement: checked bit for bit against
rearrange of the P = 1 result."""
import pytest
import torch

from hpfg_amd import _lib as L
from tests import helpers_swinunet as S
from tests.helpers import bound_8x, canary_ok, canary_out, chan_affine, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BHW = (2, 3, 5)          # non-square; 30 P^2 rows: the last workgroup of every variant is ragged
CHANNELS = [4, 32, 96, 256, 260, 1024, 1028, 1536]          # every lanes-per-row variant, four float4 per lane, six (above 1024)


def _dev(t):
    return t.contiguous().to(DEV)


def _within(name, buf, ref64, t32):
    n = ref64.numel()
    written, tail = canary_ok(buf, n)
    assert written, f"{name}: elements of the output were never written"
    assert tail, f"{name}: the launch wrote past the end of the output"
    got = buf[:n].cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(got).all()), name
    err, bound = float((got - ref64.double()).abs().max()), bound_8x(ref64, t32.reshape(ref64.shape))
    print(f"  {name:<44s} max|err| {err:9.3e}  bound {bound:9.3e}  ratio {err / bound:6.3f}")
    assert err <= bound, (name, err, bound)


def _launch(x, g, b, dy, P, eps):
    """-> canary buffers (y, mean, rstd, dx, dgb, part), nblk of one forward + backward on the device."""
    lib, st = L.load(), stream(DEV)
    B, Hh, W, PPC = x.shape
    C_ = PPC // (P * P)
    rows = B * Hh * W * P * P
    xd, gd, bd, dyd = _dev(x), _dev(g), _dev(b), _dev(dy)
    y, mean, rstd = canary_out(rows * C_), canary_out(rows), canary_out(rows)
    L.check(lib.hpfg_ln_px_fwd(L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y), L.ptr(mean), L.ptr(rstd), B, Hh, W, P, C_, eps, st), "ln_px_fwd")
    nblk = lib.hpfg_ln_px_bwd_blocks(rows)
    dx, dgb, part = canary_out(rows * C_), canary_out(2 * C_), canary_out(nblk * 2 * C_)
    L.check(lib.hpfg_ln_px_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dgb), L.ptr(dgb[C_:]), L.ptr(part), B, Hh, W, P,
                               C_, st), "ln_px_bwd")
    torch.cuda.synchronize()
    return y, mean, rstd, dx, dgb, part, nblk


def _run(x, P, eps, seed, tag):
    B, Hh, W, PPC = x.shape
    C_ = PPC // (P * P)
    rows = B * Hh * W * P * P
    gen = torch.Generator().manual_seed(seed)
    g, b, dy = chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen), chan_affine((B, Hh * P, W * P, C_), 0, gen)
    xr, gr, br = x.reshape(rows, C_).clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y32, mean32, rstd32 = torch.native_layer_norm(xr, (C_,), gr, br, eps)
    y32.backward(S.px_unshuffle(dy, P).reshape(rows, C_))
    y64, mean64, rstd64 = S.ln_px_f64(x, g, b, P, eps)
    dx64, dg64, db64 = S.ln_px_bwd_f64(x, dy, g, P, eps)
    y, mean, rstd, dx, dgb, part, nblk = _launch(x, g, b, dy, P, eps)
    _within(f"ln_px {tag} y", y, y64, S.px_shuffle(y32.detach().reshape(x.shape), P))
    _within(f"ln_px {tag} mean", mean, mean64, mean32.detach().reshape(-1))
    _within(f"ln_px {tag} rstd", rstd, rstd64, rstd32.detach().reshape(-1))
    _within(f"ln_px {tag} dx", dx, dx64, xr.grad.reshape(x.shape))
    written, tail = canary_ok(part, nblk * 2 * C_)
    assert written and tail, f"ln_px {tag}: partial sums unwritten or written past the scratch"
    _within(f"ln_px {tag} dgamma,dbeta", dgb, torch.stack([dg64, db64]), torch.stack([gr.grad, br.grad]))
    return part, nblk


@pytest.mark.parametrize("C_", CHANNELS)
@pytest.mark.parametrize("P", [1, 2, 4])
def test_ln_px_every_variant_and_factor(P, C_):
    B, Hh, W = BHW
    for eps in (1e-6, 1e-5):
        _run(chan_affine((B, Hh, W, P * P * C_), 100 * C_ + P), P, eps, C_ + P, f"P{P} C{C_} eps{eps:g}")


def test_ln_px_above_the_workgroup_cap():
    """33 120 rows of 4 channels: hpfg_ln_px_bwd_blocks stops at 512 workgroups of whole sweeps (96 rows), so those from 345 on own no rows
    and write zero partial sums."""
    lib = L.load()
    B, Hh, W, P, C_ = 1, 46, 45, 4, 4
    rows = B * Hh * W * P * P
    assert lib.hpfg_ln_px_bwd_blocks(rows) == 512 and (rows + 63) // 64 > 512
    part, nblk = _run(chan_affine((B, Hh, W, P * P * C_), 9), P, 1e-6, 10, f"rows{rows}")
    first_empty = -(-rows // 96)
    assert first_empty == 345 and not part[first_empty * 2 * C_:nblk * 2 * C_].any()


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_ln_px_row_variance_of_the_size_of_eps(eps):
    """x = 3 + 1e-3 randn: the row variance is about 1e-6, so rstd is sqrt(2) off (eps 1e-6) or 3.3 times off (1e-5) when eps is ignored or
    taken as the other value -- far outside the bound."""
    B, Hh, W = BHW
    P, C_ = 2, 96
    x = (3.0 + 1e-3 * torch.randn(B, Hh, W, P * P * C_, generator=torch.Generator().manual_seed(7))).float()
    _run(x, P, eps, 8, f"var~1e-6 eps{eps:g}")


@pytest.mark.parametrize("C_", [c for c in CHANNELS if c <= 1024])
def test_ln_px_identity_map_gives_the_bits_of_ln(C_):
    """P = 1, eps 1e-5, C <= 1024: bit-equal to hpfg_ln_fwd / hpfg_ln_bwd."""
    lib, st = L.load(), stream(DEV)
    B, Hh, W = BHW
    rows = B * Hh * W
    gen = torch.Generator().manual_seed(C_)
    x, g, b, dy = chan_affine((B, Hh, W, C_), 0, gen), chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen), chan_affine((B, Hh, W, C_), 0, gen)
    y, mean, rstd, dx, dgb, _, _ = _launch(x, g, b, dy, 1, 1e-5)
    xd, gd, bd, dyd = _dev(x), _dev(g), _dev(b), _dev(dy)
    y0, mean0, rstd0 = canary_out(rows * C_), canary_out(rows), canary_out(rows)
    L.check(lib.hpfg_ln_fwd(L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(y0), L.ptr(mean0), L.ptr(rstd0), rows, C_, st), "ln_fwd")
    dx0, dgb0, part0 = canary_out(rows * C_), canary_out(2 * C_), canary_out(lib.hpfg_ln_bwd_blocks(rows) * 2 * C_)
    L.check(lib.hpfg_ln_bwd(L.ptr(xd), L.ptr(dyd), L.ptr(gd), L.ptr(mean0), L.ptr(rstd0), L.ptr(dx0), L.ptr(dgb0), L.ptr(dgb0[C_:]), L.ptr(part0), rows, C_,
                            st), "ln_bwd")
    torch.cuda.synchronize()
    for name, a, a0, n in (("y", y, y0, rows * C_), ("mean", mean, mean0, rows), ("rstd", rstd, rstd0, rows), ("dx", dx, dx0, rows * C_),
                           ("dgamma,dbeta", dgb, dgb0, 2 * C_)):
        assert torch.equal(a[:n].view(torch.int32), a0[:n].view(torch.int32)), name


@pytest.mark.parametrize("C_", [32, 260, 1536])
@pytest.mark.parametrize("P", [2, 4])
def test_ln_px_row_map_is_rearrange_of_the_identity_result(P, C_):
    """The map moves rows and changes no arithmetic: y equals rearrange of the P = 1 result of the same rows, and the backward fed dy equals
    the P = 1 backward fed the un-shuffled dy -- bit for bit, dgamma / dbeta included (same rows in the same workgroups)."""
    B, Hh, W = BHW
    eps = 1e-6
    gen = torch.Generator().manual_seed(C_ + P)
    x, g, b = chan_affine((B, Hh, W, P * P * C_), 0, gen), chan_affine((C_,), 0, gen), chan_affine((C_,), 0, gen)
    dy = chan_affine((B, Hh * P, W * P, C_), 0, gen)
    rows = B * Hh * W * P * P
    y, mean, rstd, dx, dgb, _, _ = _launch(x, g, b, dy, P, eps)
    flat = x.reshape(1, 1, rows, C_)          # the same row matrix under the identity map
    y1, mean1, rstd1, dx1, dgb1, _, _ = _launch(flat, g, b, S.px_unshuffle(dy, P).reshape(1, 1, rows, C_), 1, eps)
    n = rows * C_
    want_y = S.px_shuffle(y1[:n].cpu().view(torch.int32).reshape(B, Hh, W, P * P * C_), P)
    assert torch.equal(y[:n].cpu().view(torch.int32).reshape(want_y.shape), want_y)
    assert torch.equal(mean[:rows].view(torch.int32), mean1[:rows].view(torch.int32))
    assert torch.equal(rstd[:rows].view(torch.int32), rstd1[:rows].view(torch.int32))
    assert torch.equal(dx[:n].view(torch.int32), dx1[:n].view(torch.int32))
    assert torch.equal(dgb[:2 * C_].view(torch.int32), dgb1[:2 * C_].view(torch.int32))


def test_ln_px_refusals():
    """C = 1540 (above the six float4 per lane), C = 6 (not a multiple of 4) and P = 3 return -1 with the error text set; nothing is launched."""
    lib, st = L.load(), stream(DEV)
    buf = torch.zeros(4096, device=DEV)
    p = L.ptr(buf)
    for B, Hh, W, P, C_ in ((1, 1, 1, 1, 1540), (1, 1, 1, 1, 6), (1, 1, 1, 3, 8)):
        assert lib.hpfg_ln_px_fwd(p, p, p, p, p, p, B, Hh, W, P, C_, 1e-6, st) == -1
        assert b"ln_px_fwd" in lib.hpfg_last_error()
        assert lib.hpfg_ln_px_bwd(p, p, p, p, p, p, p, L.ptr(buf[C_:]), p, B, Hh, W, P, C_, st) == -1
        assert b"ln_px_bwd" in lib.hpfg_last_error()
    torch.cuda.synchronize()
    assert not buf.any()


def test_layer_norm_op_takes_a_row_matrix_at_any_eps():
    """``ops_tokens.layer_norm`` on [rows, C] at eps 1e-6 (the identity map needs a row count only): the bits of the same rows as a
    [1, 1, rows, C] map, forward and backward."""
    from hpfg_amd.ops_tokens import layer_norm
    gen = torch.Generator().manual_seed(3)
    x, g, b, dy = (chan_affine(s, 0, gen).to(DEV) for s in ((37, 96), (96,), (96,), (37, 96)))
    outs = []
    for shape in ((37, 96), (1, 1, 37, 96)):
        xr, gr, br = (t.clone().requires_grad_(True) for t in (x.reshape(shape), g, b))
        y = layer_norm(xr, gr, br, 1e-6)
        assert y.shape == shape
        y.backward(dy.reshape(shape))
        outs.append([t.reshape(-1) for t in (y.detach(), xr.grad, gr.grad, br.grad)])
    for a, c in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, c)
