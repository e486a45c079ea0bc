"""GPU: the depthwise k x k convolution of csrc/dwconv.hip (hpfg_dwconv_fwd / hpfg_dwconv_bwd through hpfg_amd._lib, and ops_tokens.dwconv)
against the float64 law of tests/helpers_uniformer.py.

The rule is the one of tests/test_gpu_tokens_edges.py: every output, and the partial-sum scratch the finishing reduction reads, is allocated
with a tail and filled with a quiet-NaN bit pattern; after the launch no element of the output holds the pattern and the tail kept its bits;
every value is finite and within 8 x the error torch's own float32 CPU op makes against the float64 law on the same inputs, with a floor of
4 float32 ulp of the law's largest magnitude (helpers.bound_8x).  Inputs carry a per-channel offset in [-3, 3] and scale in [0.25, 4].

A workgroup owns a 16 x 16 pixel tile of 8 channel quads (32 channels): 17 x 33 crosses tile edges on both axes, C = 260 leaves one quad in
the ninth channel slice, and maps below the halo (1 x 1 ... 3 x 3 with k = 5) have taps outside the map at every pixel."""
import pytest
import torch
import torch.nn.functional as F

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens as T
from tests import helpers_uniformer as U
from tests.helpers import bits_kept, bound_8x, canary_ok, canary_out, chan_affine, stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILE = 16


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


def _case(B, Hh, W, C_, k, seed):
    gen = torch.Generator().manual_seed(seed)
    x, dy, other = (chan_affine((B, Hh, W, C_), 0, gen) for _ in range(3))
    wk = (0.6 / k) * chan_affine((k * k, C_), 0, gen)
    bias = 0.3 * chan_affine((C_,), 0, gen)
    return x, dy, other, wk, bias


def _launch(x, dy, other, wk, bias, k, res, add_dy):
    """The raw entry points on canary buffers -> (y, dx, dwk, dbias, partials, nblk)."""
    lib, st = L.load(), stream(DEV)
    B, Hh, W, C_ = x.shape
    n = x.numel()
    xd, dyd, wd, bd = _dev(x), _dev(dy), _dev(wk), _dev(bias)
    rd = {"none": None, "x": xd, "other": _dev(other)}[res]
    nblk = lib.hpfg_dwconv_bwd_blocks(B, Hh, W, k)
    y, dx, dwk, db, part = canary_out(n), canary_out(n), canary_out(k * k * C_), canary_out(C_), canary_out(nblk * (k * k + 1) * C_)
    L.check(lib.hpfg_dwconv_fwd(L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(rd), L.ptr(y), B, Hh, W, C_, k, st), "dwconv_fwd")
    L.check(lib.hpfg_dwconv_bwd(L.ptr(xd), L.ptr(wd), L.ptr(dyd), L.ptr(dx), add_dy, L.ptr(dwk), L.ptr(db), L.ptr(part), B, Hh, W, C_, k, st),
            "dwconv_bwd")
    torch.cuda.synchronize()
    return y, dx, dwk, db, part, nblk


def _run(B, Hh, W, C_, k, res="none", add_dy=0, seed=0):
    x, dy, other, wk, bias = _case(B, Hh, W, C_, k, seed)
    tag = f"k{k} {B}x{Hh}x{W}x{C_} res={res} add_dy={add_dy}"
    xr, br = x.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    wr = wk.t().reshape(C_, 1, k, k).contiguous().requires_grad_(True)
    conv32 = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=k // 2, groups=C_).permute(0, 2, 3, 1)
    conv32.backward(dy)
    radd = {"none": None, "x": x, "other": other}[res]
    y32 = conv32.detach() if radd is None else conv32.detach() + radd
    dx32 = xr.grad + dy if add_dy else xr.grad
    y64 = U.dwconv_k_f64(x, wk, bias, k, radd)
    dx64, dwk64, db64 = U.dwconv_k_bwd_f64(x, wk, dy, k, add_dy=bool(add_dy))
    y, dx, dwk, db, part, nblk = _launch(x, dy, other, wk, bias, k, res, add_dy)
    _within(f"{tag} y", y, y64, y32)
    _within(f"{tag} dx", dx, dx64, dx32)
    written, tail = canary_ok(part, nblk * (k * k + 1) * C_)
    assert written, f"{tag}: partial sums that the finishing reduction reads were never written"
    assert tail, f"{tag}: partial sums written past the scratch"
    _within(f"{tag} dwk", dwk, dwk64, wr.grad.reshape(C_, k * k).t())
    _within(f"{tag} dbias", db, db64, br.grad)
    return nblk


@pytest.mark.parametrize("add_dy", [0, 1])
@pytest.mark.parametrize("res", ["none", "x", "other"])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_residual_and_add_dy_modes(k, res, add_dy):
    _run(2, 17, 33, 64, k, res, add_dy, seed=10 * k + add_dy)


@pytest.mark.parametrize("C_", [4, 260])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_maps_smaller_than_the_halo(k, C_):
    """1 x 1, 1 x 7, 7 x 1, 2 x 2 and 3 x 3: with k = 5 every pixel of each has taps outside the map."""
    for i, (B, Hh, W) in enumerate([(1, 1, 1), (3, 1, 7), (3, 7, 1), (1, 2, 2), (3, 3, 3)]):
        _run(B, Hh, W, C_, k, ("x", "none", "other")[i % 3], i % 2, seed=C_ + i)


@pytest.mark.parametrize("C_", [4, 64, 320, 260])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_tile_edges_and_channel_slices(k, C_):
    """7 x 7 (stage 4), 5 x 9, and 17 x 33 (a second, one-pixel tile on both axes); B = 1 and 3; C = 260: a ragged last channel slice."""
    for i, (B, Hh, W) in enumerate([(1, 7, 7), (3, 7, 7), (3, 5, 9), (1, 17, 33), (3, 17, 33)]):
        _run(B, Hh, W, C_, k, ("x", "other", "none")[i % 3], (i + 1) % 2, seed=7 * C_ + i)


@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_above_the_grid_cap(k):
    """3 x 32 x 1456: 546 tiles on the 512 workgroups hpfg_dwconv_bwd_blocks caps the grid at, and more pixels than 512 tiles of 16 x 16 hold:
    some workgroups walk a second tile in all three kernels."""
    lib = L.load()
    B, Hh, W = 3, 32, 1456
    nblk = lib.hpfg_dwconv_bwd_blocks(B, Hh, W, k)
    assert nblk == 512 and B * -(-Hh // TILE) * -(-W // TILE) > nblk and B * Hh * W > nblk * TILE * TILE
    assert _run(B, Hh, W, 4, k, "x", 1, seed=k) == nblk


def test_dwconv_block_count_follows_the_tiles():
    lib = L.load()
    assert lib.hpfg_dwconv_bwd_blocks(1, 1, 1, 3) == 1 and lib.hpfg_dwconv_bwd_blocks(3, 17, 33, 5) == 3 * 2 * 3
    assert lib.hpfg_dwconv_bwd_blocks(32, 56, 56, 5) == 512 and lib.hpfg_dwconv_bwd_blocks(32, 28, 28, 3) == 128


@pytest.mark.parametrize("B,C_,k", [(2, 8, 4), (2, 8, 7), (2, 6, 3), (0, 8, 3), (2, 8, 1)], ids=["k4", "k7", "C6", "B0", "k1"])
def test_dwconv_refused_arguments_launch_nothing(B, C_, k):
    lib, st = L.load(), stream(DEV)
    n = 2 * 5 * 5 * 8
    src = torch.ones(n + 64, device=DEV)
    y, dx, dwk, db, part = (canary_out(n) for _ in range(5))
    p = L.ptr(src)
    assert lib.hpfg_dwconv_fwd(p, p, p, None, L.ptr(y), B, 5, 5, C_, k, st) == -1
    assert b"dwconv_fwd" in lib.hpfg_last_error()
    assert lib.hpfg_dwconv_bwd(p, p, p, L.ptr(dx), 1, L.ptr(dwk), L.ptr(db), L.ptr(part), B, 5, 5, C_, k, st) == -1
    assert b"dwconv_bwd" in lib.hpfg_last_error()
    torch.cuda.synchronize()
    for t in (y, dx, dwk, db, part):
        assert bits_kept(t, 0)


@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_two_launches_give_the_same_bits(k):
    case = _case(3, 17, 33, 260, k, 5)
    a = _launch(*case, k, "x", 1)
    b = _launch(*case, k, "x", 1)
    for name, u, v in zip(("y", "dx", "dwk", "dbias", "partials"), a[:5], b[:5]):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), name


@pytest.mark.parametrize("res", ["none", "x", "other"])
@pytest.mark.parametrize("k", [3, 5])
def test_dwconv_autograd_equals_the_entry_points(k, res):
    """ops_tokens.dwconv: the [C,1,k,k] parameter, x + dwconv(x) with one gradient for both uses of x, another tensor as the residual."""
    B, Hh, W, C_ = 2, 17, 9, 36
    x, dy, other, wk, bias = _case(B, Hh, W, C_, k, 40 + k)
    y0, dx0, dwk0, db0, _, _ = _launch(x, dy, other, wk, bias, k, res, 1 if res == "x" else 0)
    xd, od, bd = (_dev(t).requires_grad_(True) for t in (x, other, bias))
    wd = _dev(wk.t().reshape(C_, 1, k, k)).requires_grad_(True)
    y = T.dwconv(xd, wd, bd, k, {"none": None, "x": xd, "other": od}[res])
    y.backward(_dev(dy))
    n = x.numel()
    assert torch.equal(y.detach().reshape(-1), y0[:n])
    assert torch.equal(xd.grad.reshape(-1), dx0[:n])
    assert torch.equal(wd.grad.reshape(C_, k * k).t().reshape(-1), dwk0[:k * k * C_])
    assert torch.equal(bd.grad, db0[:C_])
    if res == "other":
        assert torch.equal(od.grad, _dev(dy))
    else:
        assert od.grad is None


def test_dwconv_argument_checks_raise_value_error():
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    w3, b = torch.zeros(8, 1, 3, 3, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="k must be 3 or 5"):
        T.dwconv(x, w3, b, 7)
    with pytest.raises(ValueError, match="weight must be"):
        T.dwconv(x, w3, b, 5)
    with pytest.raises(ValueError, match="C % 4"):
        T.dwconv(torch.zeros(1, 4, 4, 6, device=DEV), w3, b, 3)
    with pytest.raises(ValueError, match="residual"):
        T.dwconv(x, w3, b, 3, torch.zeros(1, 4, 4, 4, device=DEV))
