"""GPU: csrc/gemm.hip entry point by entry point through hpfg_amd._lib, against the float64 laws of tests/helpers.py ("dense kernels";
tests/test_dense_laws_host.py holds those against torch's float64 ops and shows every named mutation caught by the rules used here).

Conventions (those of tests/test_gpu_tokens_edges.py).  Every output and every scratch buffer is a canary_out: after the launch no output
element holds the NaN pattern, the tail kept its bits and, where ldc > N, so did the gap columns.  Operands with a leading dimension above
their extent carry the same pattern in their gaps (inside the allocation): a kernel that reads a gap element into a product fails the
finiteness check.  Tolerances: the fp32 kernels (hpfg_gemm_f32, its split-K form, col_sum, col_sum2, the db of the tn kernel) lie within
bound_8x of the float64 law, 8 x the error of torch's float32 CPU op; the split-bf16 kernels (hpfg_gemm_bf16x3, its split-K form, the dW
of hpfg_gemm_tn_bf16x3) within bound_8x against torch's float32 result plus bound_8x against the split emulation (helpers._prod3, bias
and C0 added in float64, one rounding).  hpfg_relu_bwd and the structure of the split-K sum are compared bit for bit.

Which test holds which entry point:
  hpfg_gemm_f32            test_gemm_f32_shapes_and_orientations, test_gemm_f32_neither_stride_is_one, test_gemm_epilogue_switches
  hpfg_gemm_f32_splits     test_split_k_geometry_law_and_structure, test_short_k_is_not_split
  hpfg_gemm_f32_splitk     test_split_k_geometry_law_and_structure, test_short_k_is_not_split, test_gemm_epilogue_switches
  hpfg_gemm_bf16x3_ok      test_gemm_bf16x3_shapes_and_orientations, test_gemm_bf16x3_refusals
  hpfg_gemm_bf16x3         test_gemm_bf16x3_shapes_and_orientations, test_gemm_bf16x3_scalar_epilogue, test_gemm_attention_call_shape,
                           test_gemm_epilogue_switches, test_gemm_bf16x3_refusals
  hpfg_gemm_bf16x3_splits  test_split_k_geometry_law_and_structure, test_short_k_is_not_split
  hpfg_gemm_bf16x3_splitk  test_split_k_geometry_law_and_structure, test_short_k_is_not_split, test_gemm_epilogue_switches
  hpfg_gemm_tn_splits      test_gemm_tn_dw_and_db
  hpfg_gemm_tn_bf16x3      test_gemm_tn_dw_and_db, test_gemm_tn_pointer_alone_selects_the_unaligned_kernel, test_gemm_tn_trailing_splits_own_no_rows
  hpfg_col_sum             test_col_sum_and_col_sum2
  hpfg_col_sum_splits      test_col_sum_and_col_sum2, test_col_sum2_at_the_split_cap
  hpfg_col_sum2            test_col_sum_and_col_sum2, test_col_sum2_at_the_split_cap
  hpfg_relu_bwd            test_relu_bwd_is_a_selection

Row splits of hpfg_gemm_tn_bf16x3: while the rows decide the split count (ceil(R / 256)), rounding the rows per split up to 32 never leaves
a split empty (tests/test_dense_laws_host.py checks every R up to 5000); once the cap of 512 splits (or the tile count) decides it, trailing
splits own no rows and must write zero partials: test_gemm_tn_trailing_splits_own_no_rows, (131073, 4, 4), 56 empty splits of 512.

Measured on the MI355X, largest error / bound per family (1.0 is the limit):
  hpfg_gemm_f32             0.37   split-K 0.21
  hpfg_gemm_bf16x3          0.12   split-K 0.12      (of the former 64 x float32 bound: 0.95 and 0.95)
  hpfg_gemm_tn_bf16x3       dW 0.12 (former rule 4.55)   db 0.21
  column sums               col_sum 0.11   col_sum2 0.23
  hpfg_relu_bwd and the split-K structure: equal bit for bit
"""
import pytest
import torch

from hpfg_amd import _lib as L
from tests import helpers as H
from tests.helpers import bits_kept, bound_8x, canary_ok, canary_out, chan_affine, report, stream, within_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FN = {"f32": "hpfg_gemm_f32", "bf16x3": "hpfg_gemm_bf16x3"}


def _dev(t):
    return t.contiguous().to(DEV)


def _gap_kept(buf, rows, n, ldc):
    """the columns [n, ldc) of a [rows][ldc] output still hold the NaN pattern"""
    return ldc == n or bool((buf[:rows * ldc].view(rows, ldc)[:, n:].contiguous().view(torch.int32) == H.NAN_BITS).all())


def _launch(math, a, b, M, N, K, ldc=None, bias=None, C0=None, relu=0, splitk=False, out=None):
    """a, b: (device buffer or pointer, srow, sk) of A (rows = m) and B (rows = n).  -> (out buffer, scratch buffer or None, splits)"""
    lib, st = L.load(), stream(DEV)
    ldc = ldc or N
    if out is None:
        out = canary_out(M * ldc)
    if C0 is not None:
        out[:M * ldc].view(M, ldc)[:, :N] = _dev(C0)
    pa, pb = (t[0] if isinstance(t[0], int) else L.ptr(t[0]) for t in (a, b))
    args = [pa, a[1], a[2], pb, b[2], b[1], L.ptr(out), ldc, M, N, K, L.ptr(bias), int(relu), int(C0 is not None)]
    scratch, splits = None, 1
    if splitk:
        splits = getattr(lib, FN[math] + "_splits")(M, N, K)
        scratch = canary_out(splits * M * N)
        args.append(L.ptr(scratch))
    L.check(getattr(lib, FN[math] + ("_splitk" if splitk else ""))(*args, st), FN[math])
    torch.cuda.synchronize()
    return out, scratch, splits


def _old(math, e):
    """the bound the split-bf16 kernels had before: 64 x torch's float32 error (printed beside the new ratio, not asserted)"""
    return bound_8x(e["law"], e["y32"], 64.0) if math == "bf16x3" else None


def _check(name, out, M, N, ldc, law, bound, old=None):
    written, tail = canary_ok(out[:M * ldc].view(M, ldc)[:, :N].contiguous(), M * N)[0], bits_kept(out, M * ldc)
    assert written, f"{name}: elements of C were never written"
    assert tail and _gap_kept(out, M, N, ldc), f"{name}: the launch wrote into the gap columns or past the end of C"
    got = out[:M * ldc].view(M, ldc)[:, :N].cpu().double()
    assert bool(torch.isfinite(got).all()), f"{name}: not finite (a gap element of an operand was read into a product)"
    err = float((got - law).abs().max())
    report(name, err, bound)
    if old is not None:
        report(name + " [64 x float32 rule]", err, old)
    assert err <= bound, (name, err, bound)
    return got


def _operands(c, oa, ob, pad):
    a, b = H.gemm_operand(c["A"], oa, pad), H.gemm_operand(c["Bt"], ob, pad)
    return (_dev(a[0]),) + a[1:], (_dev(b[0]),) + b[1:]


# ---- shapes x operand orientations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oa,ob", H.GEMM_ORIENTS, ids=["Ak_Bk", "Ak_Bn", "Am_Bk", "Am_Bn"])
@pytest.mark.parametrize("M,N,K", H.GEMM_F32_SHAPES + H.GEMM_BF16_SHAPES)
def test_gemm_f32_shapes_and_orientations(M, N, K, oa, ob):
    """64 x 64 tiles, K chunks of 16: one element, below a tile, exactly a tile, one past / one short of it in each of M, N, K, two row
    tiles of a single column; lda, ldb = extent + 3 with the NaN pattern in the gaps, ldc = N + 3."""
    c = H.gemm_case(M, N, K)
    a, b = _operands(c, oa, ob, 3)
    out, _, _ = _launch("f32", a, b, M, N, K, ldc=N + 3)
    _check(f"gemm_f32 {(M, N, K)} A {oa}-fast B {ob}-fast", out, M, N, N + 3, c["law"], c["tol"]["f32"])


def test_gemm_f32_neither_stride_is_one():
    """A at (sam, sak) = (2 K, 2): the m-fast staging map serves any strides"""
    M, N, K = 65, 63, 17
    c = H.gemm_case(M, N, K)
    a, b = H.gemm_operand(c["A"], "2", 0), H.gemm_operand(c["Bt"], "k", 3)
    out, _, _ = _launch("f32", (_dev(a[0]),) + a[1:], (_dev(b[0]),) + b[1:], M, N, K)
    _check("gemm_f32 (65, 63, 17) A strides (2K, 2)", out, M, N, N, c["law"], c["tol"]["f32"])


@pytest.mark.parametrize("oa,ob", H.GEMM_ORIENTS, ids=["Ak_Bk", "Ak_Bn", "Am_Bk", "Am_Bn"])
@pytest.mark.parametrize("M,N,K", H.GEMM_BF16_SHAPES)
def test_gemm_bf16x3_shapes_and_orientations(M, N, K, oa, ob):
    """128 x 128 tiles, K chunks of 32, both operand images (the plain [row][k] one and the [k][row] one read through the transposing LDS
    read) at ragged tiles; lda, ldb = extent + 4 (the 4-element alignment holds) with the NaN pattern in the gaps, ldc = N + 8."""
    lib = L.load()
    c = H.gemm_case(M, N, K)
    a, b = _operands(c, oa, ob, 4)
    assert lib.hpfg_gemm_bf16x3_ok(L.ptr(a[0]), a[1], a[2], L.ptr(b[0]), b[2], b[1], M, N, K) == 1
    out, _, _ = _launch("bf16x3", a, b, M, N, K, ldc=N + 8)
    _check(f"gemm_bf16x3 {(M, N, K)} A {oa}-fast B {ob}-fast", out, M, N, N + 8, c["law"], c["tol"]["bf16x3"], _old("bf16x3", c))


@pytest.mark.parametrize("M,N,K,ldc", H.GEMM_SCALAR_EPILOGUE)
def test_gemm_bf16x3_scalar_epilogue(M, N, K, ldc):
    """N % 4 != 0 or ldc % 4 != 0 takes the element-wise epilogue (B k-fast: an n-fast B needs N % 4 == 0); ldc = N + 8 the vector one.
    With bias and accumulate, so that the epilogue's reads are covered as well."""
    c = H.gemm_case(M, N, K)
    e = H.gemm_epilogue(c, True, True, True)
    a, b = _operands(c, "k", "k", 4)
    out, _, _ = _launch("bf16x3", a, b, M, N, K, ldc=ldc, bias=_dev(c["bias"]), C0=c["C0"], relu=1)
    _check(f"gemm_bf16x3 {(M, N, K)} ldc={ldc}", out, M, N, ldc, e["law"], e["tol"]["bf16x3"], _old("bf16x3", e))


def test_gemm_attention_call_shape():
    """dV = P^T dO as attention calls it: A m-fast, B n-fast inside a wider row (sbk = 4 N) at an offset base pointer, ldc = 2 N"""
    M, N, K = 132, 64, 36
    c = H.gemm_case(M, N, K)
    a = H.gemm_operand(c["A"], "r", 4)
    wide = H.nan_filled(K * 4 * N).view(K, 4 * N)
    wide[:, N:2 * N] = c["B"]
    wd, ad = _dev(wide.view(-1)), _dev(a[0])
    bptr = wd.data_ptr() + 4 * N
    assert L.load().hpfg_gemm_bf16x3_ok(L.ptr(ad), a[1], a[2], bptr, 4 * N, 1, M, N, K) == 1
    for math in ("f32", "bf16x3"):
        out, _, _ = _launch(math, (ad,) + a[1:], (bptr, 1, 4 * N), M, N, K, ldc=2 * N)
        _check(f"gemm_{math} attention call shape", out, M, N, 2 * N, c["law"], c["tol"][math], _old(math, c))


def test_gemm_bf16x3_refusals():
    """hpfg_gemm_bf16x3_ok == 0 and hpfg_gemm_bf16x3 == -1 with nothing launched (the output keeps the pattern)"""
    lib, st = L.load(), stream(DEV)
    t = torch.zeros(4096, device=DEV)
    p = t.data_ptr()
    out, sink = canary_out(1024), torch.zeros(1024, device=DEV)
    bad = {
        "A offset by one float": (p + 4, 16, 1, p, 1, 16, 8, 8, 16),
        "B offset by one float": (p, 16, 1, p + 4, 1, 16, 8, 8, 16),
        "K % 4 != 0 with a k-fast operand": (p, 20, 1, p, 1, 20, 8, 8, 18),
        "M % 4 != 0 with m-fast A": (p, 1, 8, p, 1, 16, 6, 8, 16),
        "both strides of A != 1": (p, 32, 2, p, 1, 16, 8, 8, 16),
        "both strides of B != 1": (p, 16, 1, p, 2, 32, 8, 8, 16),
    }
    for why, (pa, sam, sak, pb, sbk, sbn, M, N, K) in bad.items():
        assert lib.hpfg_gemm_bf16x3_ok(pa, sam, sak, pb, sbk, sbn, M, N, K) == 0, why
        assert lib.hpfg_gemm_bf16x3(pa, sam, sak, pb, sbk, sbn, L.ptr(out), N, M, N, K, None, 0, 0, st) == -1, why
        assert lib.hpfg_gemm_f32(pa, sam, sak, pb, sbk, sbn, L.ptr(sink), N, M, N, K, None, 0, 0, st) == 0, why          # the fp32 kernel takes them all
    assert lib.hpfg_gemm_bf16x3_splits(8, 8, 512) == 4
    assert lib.hpfg_gemm_bf16x3_splitk(p + 4, 512, 1, p, 1, 512, L.ptr(out), 8, 8, 8, 512, None, 0, 0, L.ptr(sink), st) == -1          # the split form checks too
    assert lib.hpfg_gemm_f32(p, 16, 1, p, 1, 16, L.ptr(out), 7, 8, 8, 16, None, 0, 0, st) == -1                        # ldc < N
    torch.cuda.synchronize()
    assert bits_kept(out, 0)


# ---- the epilogue: act(A B + bias + C0) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [False, True], ids=["unsplit", "splitk"])
@pytest.mark.parametrize("math,shape", [(m, s) for m, ss in H.GEMM_EPILOGUE_SHAPES.items() for s in ss] + [("f32", (132, 68, 516)), ("bf16x3", (132, 68, 516))])
def test_gemm_epilogue_switches(math, shape, splitk):
    """bias in {none, given} x (relu, accumulate) in all four combinations; (1, 1) is relu(A B + bias + C0), which the host test shows
    many tolerances away from relu(A B + bias) + C0 on these inputs.  (132, 68, 516) is where the split-K entry points do split."""
    M, N, K = shape
    c = H.gemm_case(M, N, K)
    a, b = _operands(c, "k", "k", 4)
    bd = _dev(c["bias"])
    for bias in (False, True):
        for relu, acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
            e = H.gemm_epilogue(c, bias, relu, acc)
            out, scratch, splits = _launch(math, a, b, M, N, K, ldc=N + 8, bias=bd if bias else None, C0=c["C0"] if acc else None, relu=relu, splitk=splitk)
            assert scratch is None or bits_kept(scratch, splits * M * N)
            _check(f"gemm_{math}{'_splitk' if splitk else ''} {shape} bias={int(bias)} relu={relu} acc={acc} splits={splits}", out, M, N, N + 8, e["law"], e["tol"][math], _old(math, e))


# ---- split-K -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math,shape", [(m, s) for s, row in H.GEMM_SPLIT_TABLE.items() for m, geo in row.items() if geo], ids=str)
def test_split_k_geometry_law_and_structure(math, shape):
    """The geometry by hpfg_*_splits and the replica; the result against the law; the scratch written for the launched slices only (its
    tail, and the slices beyond the launched count, keep their bits); and the structure bit for bit: the result is the float32
    left-to-right sum ((bias + p_0) + p_1) + ..., then accumulate, then relu, with p_z the unsplit entry point on K-slice z -- no k lost,
    none counted twice, the finishing kernel reading exactly the launched count.  One case runs twice: the same bits."""
    lib = L.load()
    M, N, K = shape
    S, kper, launched, klast = H.GEMM_SPLIT_TABLE[shape][math]
    assert getattr(lib, FN[math] + "_splits")(M, N, K) == S and H.gemm_split_geometry(math, M, N, K) == (S, kper, launched, klast)
    c = H.gemm_case(M, N, K)
    e = H.gemm_epilogue(c, True, True, True)
    bd = _dev(c["bias"])
    for oa, ob in (("k", "k"), ("r", "r")) if math == "f32" or M % 4 == 0 else (("k", "k"),):
        a, b = _operands(c, oa, ob, 4 if K % 4 == 0 else 3)
        out, scratch, splits = _launch(math, a, b, M, N, K, ldc=N + 8, bias=bd, C0=c["C0"], relu=1, splitk=True)
        name = f"gemm_{math}_splitk {shape} A {oa}-fast B {ob}-fast splits={S} launched={launched}"
        assert splits == S
        written, rest = canary_ok(scratch, launched * M * N)
        assert written and rest, f"{name}: the scratch must hold exactly the launched slices"
        got = _check(name, out, M, N, N + 8, e["law"], e["tol"][math], _old(math, e))
        # p_z: the unsplit entry point on slice z of K
        acc32 = c["bias"].expand(M, N).clone()
        for z in range(launched):
            kz = kper if z < launched - 1 else klast
            az = (a[0].data_ptr() + 4 * z * kper * a[2], a[1], a[2])
            bz = (b[0].data_ptr() + 4 * z * kper * b[2], b[1], b[2])
            pz, _, _ = _launch(math, az, bz, M, N, kz)
            assert all(canary_ok(pz, M * N))
            part = pz[:M * N].view(M, N).cpu()
            assert torch.equal(scratch[z * M * N:(z + 1) * M * N].view(M, N).cpu(), part), f"{name}: slice {z} of the scratch is not the product over its k range"
            acc32 = acc32 + part
        want = torch.relu(acc32 + c["C0"])
        assert torch.equal(got.float(), want), f"{name}: not the fixed-order float32 sum of the slices"
        if shape == (132, 68, 516):
            again, _, _ = _launch(math, a, b, M, N, K, ldc=N + 8, bias=bd, C0=c["C0"], relu=1, splitk=True)
            assert torch.equal(again[:M * (N + 8)].view(torch.int32), out[:M * (N + 8)].view(torch.int32)), f"{name}: two runs differ"


@pytest.mark.parametrize("math", ["f32", "bf16x3"])
def test_short_k_is_not_split(math):
    """(64, 64, 255): K < 256 reports one split; the split-K entry point gives the unsplit result and leaves the scratch alone"""
    lib = L.load()
    M, N, K = H.GEMM_UNSPLIT
    assert getattr(lib, FN[math] + "_splits")(M, N, K) == 1
    c = H.gemm_case(M, N, K)
    a, b = _operands(c, "k", "k", 5)
    if math == "bf16x3":          # K = 255 is not a multiple of 4 with k-fast operands: the row-fast images, lda = M + 4
        a, b = _operands(c, "r", "r", 4)
    plain, _, _ = _launch(math, a, b, M, N, K)
    out, scratch, _ = _launch(math, a, b, M, N, K, splitk=True)
    assert bits_kept(scratch, 0)
    _check(f"gemm_{math}_splitk {(M, N, K)} unsplit", out, M, N, N, c["law"], c["tol"][math])
    assert torch.equal(out[:M * N].view(torch.int32), plain[:M * N].view(torch.int32))


# ---- dW = dY^T X, db = column sums of dY ---------------------------------------------------------------------------------------------------
def _tn_run(R, N, K, with_db, x_offset=0):
    lib, st = L.load(), stream(DEV)
    c = H.tn_case(R, N, K)
    S = lib.hpfg_gemm_tn_splits(R, N, K)
    stride = N * K + (N if with_db else 0)
    dw_db, part = canary_out(stride), canary_out(S * stride)
    dyd = _dev(c["dy"])
    xbuf = torch.cat([H.nan_filled(x_offset), c["x"].reshape(-1)]).to(DEV)
    L.check(lib.hpfg_gemm_tn_bf16x3(L.ptr(dyd), xbuf.data_ptr() + 4 * x_offset, L.ptr(dw_db), L.ptr(part), R, N, K, with_db, st), "gemm_tn_bf16x3")
    torch.cuda.synchronize()
    name = f"gemm_tn {(R, N, K)} db={with_db} splits={S}" + (" x offset" if x_offset else "")
    if S > 1:
        written, tail = canary_ok(part, S * stride)
        assert written and tail, f"{name}: partials (every split writes its slice, nothing behind them)"
    else:
        assert bits_kept(part, 0), f"{name}: one split writes straight to dW"
    got = within_bound(name + " dW|db", dw_db, torch.cat([c["dw"].reshape(-1), c["db"]]) if with_db else c["dw"].reshape(-1), float("inf"))
    err = float((got[:N * K].reshape(N, K) - c["dw"]).abs().max())
    report(name + " dW", err, c["tol_dw"])
    report(name + " dW [64 x float32 rule]", err, c["old_dw"])
    assert err <= c["tol_dw"], (name, err, c["tol_dw"])
    if with_db:
        err = float((got[N * K:] - c["db"]).abs().max())
        report(name + " db", err, c["tol_db"])
        assert err <= c["tol_db"], (name, err, c["tol_db"])
    return part, S, stride


@pytest.mark.parametrize("R,N,K,with_db", sorted(H.TN_CASES))
def test_gemm_tn_dw_and_db(R, N, K, with_db):
    """64 x 64 tiles over (N, K), 32 rows per step, rows split over workgroups: one row; below a step; one past it; the unaligned
    instantiation by N and K (300, 5, 7) and by N alone (600, 65, 64); 2 x 3 tiles with db over two n-tiles; 2, 3, 4 and 9 splits (every
    branch of the partial-sum kernel: the paired loop, the odd tail, waves with nothing to add); a last split of one row.  With with_db = 0
    the N floats behind dW are not part of the output: they keep the pattern."""
    S, per, last = H.TN_CASES[(R, N, K, with_db)]
    assert (L.load().hpfg_gemm_tn_splits(R, N, K), *H.tn_geometry(R, N, K)[1:]) == (S, per, last)
    _tn_run(R, N, K, with_db)


def test_gemm_tn_pointer_alone_selects_the_unaligned_kernel():
    """(33, 36, 20) again with x one float off a 16-byte boundary"""
    _tn_run(33, 36, 20, 1, x_offset=1)


def test_gemm_tn_trailing_splits_own_no_rows():
    """(131073, 4, 4): the cap of 512 splits of 288 rows; splits 456 .. 511 own no rows and write zero partials"""
    R, N, K, with_db = H.TN_EMPTY
    part, S, stride = _tn_run(R, N, K, with_db)
    assert S == 512 and not part[456 * stride:512 * stride].any()


# ---- column sums ---------------------------------------------------------------------------------------------------------------------------
def _col_sum_run(R, M, ldx, seed):
    lib, st = L.load(), stream(DEV)
    x = chan_affine((R, M), seed)
    buf = H.nan_filled(R * ldx).view(R, ldx)
    buf[:, :M] = x
    xd = _dev(buf)
    law, y32 = x.double().sum(0), x.sum(0)
    S = lib.hpfg_col_sum_splits(R)
    assert S == H.col_sum_geometry(R)[0]
    out1, out2, scratch = canary_out(M), canary_out(M), canary_out(S * M)
    one_pass = R <= 4096          # hpfg_col_sum: one thread walks a column alone; the cap case is for the two-stage kernel
    if one_pass:
        L.check(lib.hpfg_col_sum(L.ptr(xd), R, M, ldx, L.ptr(out1), st), "col_sum")
    L.check(lib.hpfg_col_sum2(L.ptr(xd), R, M, ldx, L.ptr(out2), L.ptr(scratch), st), "col_sum2")
    torch.cuda.synchronize()
    if S > 1:
        assert all(canary_ok(scratch, S * M)), "col_sum2 partials"
    else:
        assert bits_kept(scratch, 0), "col_sum2 with one split writes straight to out"
    bound = bound_8x(law, y32)
    if one_pass:
        within_bound(f"col_sum R={R} M={M} ldx={ldx}", out1, law, bound)
    within_bound(f"col_sum2 R={R} M={M} ldx={ldx} splits={S}", out2, law, bound)
    return S


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("M", H.COL_SUM_M)
@pytest.mark.parametrize("R", sorted(H.COL_SUM_R))
def test_col_sum_and_col_sum2(R, M, pad):
    assert _col_sum_run(R, M, M + pad, R + M) == H.COL_SUM_R[R]


def test_col_sum2_at_the_split_cap():
    R, M, S = H.COL_SUM_CAP
    assert _col_sum_run(R, M, M, 1) == S


# ---- ReLU backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", H.RELU_BWD_N)
def test_relu_bwd_is_a_selection(n):
    """dy if y > 0 else 0, bit for bit; y holds 0.0, -0.0, a denormal, a negative value, +inf and NaN; dy is updated in place"""
    lib, st = L.load(), stream(DEV)
    y, dy, want = H.relu_bwd_case(n)
    buf = canary_out(n)
    buf[:n] = _dev(dy)
    yd = _dev(y)
    L.check(lib.hpfg_relu_bwd(L.ptr(buf), L.ptr(yd), n, st), "relu_bwd")
    torch.cuda.synchronize()
    assert bits_kept(buf, n)
    assert torch.equal(buf[:n].cpu().view(torch.int32), want.view(torch.int32))
