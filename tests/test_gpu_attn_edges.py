"""The three attention kernel families (csrc/attn.hip, attn_keys.hip, attn_window.hip on csrc/attn_core.h, and the thread-per-query
kernels of csrc/tokens.hip) against the float64 laws of tests/helpers.py, beyond unit logits and at every tile and grid edge.

Rule (helpers.attn_tolerance): per output tensor, max |kernel - law| <= 8 x the largest error the mode's yardstick makes against the law
(torch float32 on the CPU for HPFG_MATH=f32, the split-bf16 emulation of attn_core.h's documented arithmetic for the default mode), and
no less than 4 float32 ulp.  Nothing here is a hand constant; tests/test_attn_laws_host.py shows what the rule catches.
Families: unit (randn), sharp (q, k x 2, x 2.5 above 64 keys: a row's top probability about 0.5 to 0.8, |logit| to 33), offset (+100 on every logit: exp
overflows without the max subtraction, |logit| to 105), hot (windows: q, k x 8, where -inf for the mask's -100 is 650 to 32000 tolerances).
Every case runs both math modes and both head dims through the C entry points on canary buffers (every output element written, nothing
behind it touched, scratch included) and through the autograd op, whose bits must be those of the C entry points.
`pytest -s` prints error / tolerance per tensor."""
import pytest
import torch

from hpfg_amd import _lib as L
from hpfg_amd import ops_tokens
from hpfg_amd.ops_tokens import attention, attention_keys, window_attention
from tests import helpers as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MATH = {"f32": 0, "bf16x3": 1}


def _st():
    return torch.cuda.current_stream(DEV).cuda_stream


def _canaries(bufs):
    torch.cuda.synchronize()
    for name, (t, n) in bufs.items():
        written, tail = T.canary_ok(t, n)
        assert written, f"{name}: an element of the first {n} was not written"
        assert tail, f"{name}: written behind element {n}"


def _through_op(fn, math, args, grads, do):
    leaves = [a.detach().clone().requires_grad_(True) if i in grads else a for i, a in enumerate(args)]
    ops_tokens.MATH["mode"] = math
    try:
        out = fn(*leaves)
        out.backward(do)
    finally:
        ops_tokens.MATH["mode"] = None
    return (out.detach(),) + tuple(leaves[i].grad for i in grads)


def _report(tag, names, got, ref, tol):
    worst, ratios = T.worst_ratio([g.cpu() for g in got], ref, tol)
    print(f"{tag}: " + "  ".join(f"{n} {r:.3f}" for n, r in zip(names, ratios)) + "   (error / tolerance)")
    for n, r in zip(names, ratios):
        assert r < 1.0, f"{n}: {r:.3g} tolerances"


# ---- at most 64 keys: csrc/attn.hip (split-bf16) and the thread-per-query kernels of csrc/tokens.hip (f32) ---------------------------------
def _small(family, B, N, M, heads, d, math, scale=None):
    lib = L.load()
    c = T.attn_case(family, B, N, M, heads, d, scale)
    q, kv, do = (c[k].to(DEV) for k in ("q", "kv", "do"))
    sc, nq, nkv = c["scale"], q.numel(), kv.numel()
    out, dq = T.canary_out(nq), T.canary_out(nq)
    bufs = {"out": (out, nq), "dq": (dq, nq)}
    if math == "bf16x3":
        n_scr = lib.hpfg_attn_mfma_scratch_floats(B, N, heads, d)
        dkv, scr = T.canary_out(nkv), T.canary_out(n_scr)
        bufs.update(dkv=(dkv, nkv), scratch=(scr, n_scr))
        L.check(lib.hpfg_attn_mfma_fwd_hd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, M, heads, d, sc, _st()), "fwd")
        L.check(lib.hpfg_attn_mfma_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, d, sc, _st()), "bwd")
    else:
        n_p = B * heads * N * M
        P, dS = T.canary_out(n_p), T.canary_out(n_p)
        bufs.update(P=(P, n_p), dS=(dS, n_p))
        L.check(lib.hpfg_attn_fwd_hd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, M, heads, d, sc, _st()), "fwd")
        L.check(lib.hpfg_attn_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(P), L.ptr(dS), B, N, M, heads, d, sc, _st()), "bwd")
    _canaries(bufs)
    got = _through_op(attention, math, (q, kv, heads, sc), (0, 1), do)
    assert torch.equal(got[0], out[:nq].view_as(q)) and torch.equal(got[1], dq[:nq].view_as(q))
    if math == "bf16x3":
        assert torch.equal(got[2], dkv[:nkv].view_as(kv))
    ref, tol = c["ref"], c["tol"][math]
    _report(f"<=64 {family} {math} d={d} B={B} N={N} M={M} heads={heads} scale={sc:.4g}", ("out", "dq", "dkv"), got, (ref[0], ref[2], ref[3]),
            (tol[0], tol[2], tol[3]))


@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", ["unit", "sharp", "offset"])
@pytest.mark.parametrize("B,N,M,heads", T.ATTN_M_EDGES)
def test_key_tile_edges(B, N, M, heads, family, d, math):
    """1, 15 / 16 / 17, 31 / 32 / 33, 47 / 48, 63 / 64 keys: both sides of every 16-key tile of the one LDS image"""
    _small(family, B, N, M, heads, d, math)


@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", ["unit", "sharp", "offset"])
@pytest.mark.parametrize("B,N,M,heads", T.ATTN_N_EDGES)
def test_query_grid_edges(B, N, M, heads, family, d, math):
    """both sides of the 64-query forward / dQ workgroup, the 256-query thread-per-query workgroup, the 512-query dK / dV workgroup and
    its 128-query wave step"""
    _small(family, B, N, M, heads, d, math)


@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("B,N,M,heads,scale", T.ATTN_SCALE_CASES)
def test_other_scales(B, N, M, heads, scale, d, math):
    """a scale other than d^-0.5, and scale = 0: uniform probabilities over exactly the M valid keys, dq = dk = 0"""
    _small("unit", B, N, M, heads, d, math, scale)


# ---- 65 to 256 keys: csrc/attn_keys.hip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", ["sharp", "offset"])
@pytest.mark.parametrize("B,N,M,heads", T.ATTN_KEYS_EDGES)
def test_key_blocks(B, N, M, heads, family, d, math):
    lib = L.load()
    c = T.attn_case(family, B, N, M, heads, d)
    q, kv, do = (c[k].to(DEV) for k in ("q", "kv", "do"))
    sc, nq, nkv, nl = c["scale"], q.numel(), kv.numel(), B * heads * N
    n_scr = lib.hpfg_attn_keys_scratch_floats(B, N, M, heads, d, MATH[math])
    out, lse, dq, dkv, scr = T.canary_out(nq), T.canary_out(nl), T.canary_out(nq), T.canary_out(nkv), T.canary_out(n_scr)
    L.check(lib.hpfg_attn_keys_fwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), B, N, M, heads, d, sc, MATH[math], _st()), "fwd")
    L.check(lib.hpfg_attn_keys_bwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, d, sc,
                                   MATH[math], _st()), "bwd")
    _canaries({"out": (out, nq), "lse": (lse, nl), "dq": (dq, nq), "dkv": (dkv, nkv)})
    if math == "bf16x3":          # delta [B heads N], then up to 3 floats that keep the partials 16-byte aligned (nobody's), then the partials
        left = scr[:n_scr].view(torch.int32) == T.NAN_BITS
        left[nl:(nl + 3) // 4 * 4] = False
        assert not bool(left.any()), "scratch: a row's delta or an element of a dK / dV partial was not written"
        assert T.bits_kept(scr, n_scr), "scratch: written behind its end"
    else:
        _canaries({"scratch": (scr, n_scr)})
    got = _through_op(attention_keys, math, (q, kv, heads, sc), (0, 1), do)
    for a, b in zip(got, (out[:nq].view_as(q), dq[:nq].view_as(q), dkv[:nkv].view_as(kv))):
        assert torch.equal(a, b)
    _report(f"keys {family} {math} d={d} B={B} N={N} M={M} heads={heads}", ("out", "lse", "dq", "dkv"),
            (got[0], lse[:nl].view(B, heads, N), got[1], got[2]), c["ref"], c["tol"][math])


# ---- shifted windows: csrc/attn_window.hip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", T.ATTN_MATHS)
@pytest.mark.parametrize("d", T.ATTN_HEAD_DIMS)
@pytest.mark.parametrize("family", ["unit", "sharp", "hot"])
@pytest.mark.parametrize("B,H,W,w,s,heads", T.WINDOW_EDGES)
def test_windows(B, H, W, w, s, heads, family, d, math):
    """rectangular maps (only the C entry points take them), the first and the last shift, every window size, 2 / 3 / 5 workgroups in the
    four slices of the bias-gradient sum; square maps at shift 0 or w // 2 also through window_attention"""
    lib = L.load()
    c = T.window_case(family, B, H, W, w, s, heads, d)
    qkv, table, do = (c[k].to(DEV) for k in ("qkv", "table", "do"))
    sc, no, nqkv, nt = c["scale"], do.numel(), qkv.numel(), table.numel()
    n_scr = lib.hpfg_attn_window_scratch_floats(B, H, W, heads, d, w, MATH[math])
    assert n_scr == B * (H // w) * (W // w) * heads * (2 * w - 1) ** 2
    out, dqkv, dtab, scr = T.canary_out(no), T.canary_out(nqkv), T.canary_out(nt), T.canary_out(n_scr)
    L.check(lib.hpfg_attn_window_fwd(L.ptr(qkv), L.ptr(table), L.ptr(out), B, H, W, heads, d, w, s, sc, MATH[math], _st()), "fwd")
    L.check(lib.hpfg_attn_window_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), B, H, W, heads, d, w, s, sc, MATH[math],
                                     _st()), "bwd")
    _canaries({"out": (out, no), "dqkv": (dqkv, nqkv), "dtable": (dtab, nt), "scratch": (scr, n_scr)})
    got = (out[:no].view_as(do), dqkv[:nqkv].view_as(qkv), dtab[:nt].view_as(table))
    if H == W and s in (0, w // 2):
        for a, b in zip(_through_op(window_attention, math, (qkv, table, heads, w, s, sc), (0, 1), do), got):
            assert torch.equal(a, b)
    _report(f"window {family} {math} d={d} B={B} H={H} W={W} w={w} s={s} heads={heads}", T.WINDOW_TENSORS, T.window_results(got), c["ref"], c["tol"][math])
