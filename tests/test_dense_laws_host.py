"""CPU: the float64 laws of the dense kernels (tests/helpers.py, "dense kernels": the GEMM contract, column sums, the neck's adaptive
average pooling, F.normalize, NT-Xent) against torch's own float64 ops and autograd; the Python replicas of the split geometries against
the tables of the issue and, since they are host code, against the library's own hpfg_*_splits; the conditions the GPU tests' inputs have
to meet; and the mutation proof: every named wrong variant of a law moves some output of some case of tests/test_gpu_gemm_edges.py /
tests/test_gpu_heads_edges.py by at least 4 tolerances of that test's own rule."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses_ref
from tests import helpers as T


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _lib():
    from hpfg_amd import _lib as L
    return L.load() if os.path.exists(L.LIB_PATH) else None


# ---- the laws are torch's float64 ops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("relu,acc", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_law_is_addmm_then_relu(bias, relu, acc):
    c = T.gemm_case(65, 63, 17)
    A, B = c["A"].double(), c["B"].double()
    want = torch.addmm(c["bias"].double().expand(65, 63), A, B) if bias else A @ B
    if acc:
        want = want + c["C0"].double()
    if relu:
        want = F.relu(want)
    got = T.gemm_f64(c["A"], c["B"], c["bias"] if bias else None, c["C0"] if acc else None, bool(relu))
    assert got.dtype == torch.float64 and _rel(got, want) <= 1e-12
    # the split emulation is the law on operands bf16 holds exactly
    Ah, Bh = c["A"].bfloat16().float(), c["B"].bfloat16().float()
    assert torch.equal(T.gemm_f64(Ah, Bh, arith="split"), (Ah.double() @ Bh.double()).float())


@pytest.mark.parametrize("case", T.POOL_CASES[:5] + T.POOL_CASES[6:7], ids=str)
def test_pool_law_is_adaptive_avg_pool2d(case):
    N, Hh, W, C_, S, _ = case
    c = T.pool_case(N, Hh, W, C_, S)
    xn = c["x"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gap, pool = F.adaptive_avg_pool2d(xn, 1).reshape(N, C_), F.adaptive_avg_pool2d(xn, S).reshape(N, C_, S * S).transpose(1, 2)
    assert _rel(c["gap"], gap.detach()) <= 1e-12 and _rel(c["pool"], pool.detach()) <= 1e-12
    for which, (a, b) in dict(gap=(c["dgap"], None), pool=(None, c["dpool"]), both=(c["dgap"], c["dpool"])).items():
        out = (gap * a.double()).sum() if a is not None else 0.0
        out = out + ((pool * b.double()).sum() if b is not None else 0.0)
        dx = torch.autograd.grad(out, xn, retain_graph=True)[0].permute(0, 2, 3, 1)
        assert _rel(c["dx_" + which], dx) <= 1e-12, which


@pytest.mark.parametrize("special", T.L2NORM_SPECIAL)
@pytest.mark.parametrize("G,D,S", T.L2NORM_CASES)
def test_l2norm_law_is_normalize_and_its_autograd(G, D, S, special):
    c = T.l2norm_case(G, D, S, special)
    zero = special == "zero"
    x = c["x"].double().requires_grad_(True)
    u = F.normalize(x, dim=1)
    dx = torch.autograd.grad((u * c["du"].double()).sum(), x)[0]
    assert _rel(c["u"], u.detach()) <= 1e-12 and _rel(c["dx"], dx) <= 1e-12
    if special == "tiny":
        assert abs(float(c["norms"][0, 0]) / 3e-12 - 1.0) < 1e-6 and abs(float((c["u"][0, :, 0] ** 2).sum()) - 1.0) < 1e-6
    if zero:          # the clamp: u = 0, norm = 1e-12, dx = du / 1e-12
        assert not c["u"][0, :, 0].any() and float(c["norms"][0, 0]) == T.L2NORM_EPS
        assert _rel(c["dx"][0, :, 0], c["du"][0, :, 0].double() / T.L2NORM_EPS) <= 1e-12
    for layout in T.L2NORM_LAYOUTS:
        assert torch.equal(T.l2norm_unlayout(T.l2norm_layout(c["x"], layout), G, D, S, layout), c["x"])


@pytest.mark.parametrize("T_,S", T.NTXENT_T)
@pytest.mark.parametrize("n", [1, 2, 3, 32])
def test_ntxent_law_is_autograd_of_the_reference_formula(n, T_, S):
    """value, Q and the l2norm backward together: d loss / d (student features) = l2norm_bwd(Q U)"""
    g = torch.Generator().manual_seed(n + S)
    a = torch.randn(n, 8, S, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(n, 8, S, generator=g, dtype=torch.float64)
    Tf = T.f32_exact(T_)
    want = losses_ref.nt_xent(a, b, Tf)
    da = torch.autograd.grad(want, a)[0]
    (ua, na), (ub, _) = T.l2norm_f64(a.detach()), T.l2norm_f64(b)
    U = torch.cat([ua.flatten(1), ub.flatten(1)])
    loss, Q, _ = T.ntxent_f64(U @ U.t(), n, T_)
    assert abs(float(loss) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    dU = (Q @ U).reshape(n, 8, S)
    assert _rel(T.l2norm_bwd_f64(dU, ua, na), da) <= 1e-11
    # and Q is the symmetrised gradient with respect to the matrix itself, both orientations read as stored
    Gm = (U @ U.t() * (1.0 + 1e-3 * torch.randn(2 * n, 2 * n, generator=g, dtype=torch.float64))).requires_grad_(True)
    dG = torch.autograd.grad(T.ntxent_f64(Gm, n, T_)[0], Gm)[0]
    assert _rel(T.ntxent_f64(Gm.detach(), n, T_)[1], (dG + dG.t())[:n]) <= 1e-12


def test_dense_case_is_the_reference_formula():
    c = T.dense_case(3)
    a, b = c["sg"].double().requires_grad_(True), c["sd"].double().requires_grad_(True)
    v = 0.5 * (losses_ref.nt_xent(a, c["tg"].double(), 0.7) + losses_ref.nt_xent(b, c["td"].double(), 0.7))
    assert abs(float(v) - float(c["ref"][0])) <= 1e-12 and c["top"] > 0


# ---- geometry replicas --------------------------------------------------------------------------------------------------------------------
def test_split_geometries_reproduce_the_tables():
    lib = _lib()
    for (M, N, K), row in T.GEMM_SPLIT_TABLE.items():
        for math, want in row.items():
            if want is None:
                assert K % 4 != 0          # the split-bf16 kernels refuse a k-fast operand with K % 4 != 0
                continue
            assert T.gemm_split_geometry(math, M, N, K) == want, (math, M, N, K)
            kper, launched = want[1], want[2]
            assert kper % 32 == 0 or math == "f32"          # slices start at multiples of 32 floats: the bf16x3 alignment holds
            assert (launched - 1) * kper < K <= launched * kper
    for math in T.GEMM_TILE:
        assert T.gemm_split_geometry(math, *T.GEMM_UNSPLIT)[0] == 1
    for (R, N, K, _), want in T.TN_CASES.items():
        assert T.tn_geometry(R, N, K) == want, (R, N, K)
    assert sorted({T.tn_geometry(R, N, K)[0] for R, N, K, _ in T.TN_CASES}) == [1, 2, 3, 4, 9]
    for R, S in T.COL_SUM_R.items():
        assert T.col_sum_geometry(R)[0] == S
    assert T.col_sum_geometry(T.COL_SUM_CAP[0]) == (256, 513)
    if lib is not None:          # host functions of the library: no device needed
        for (M, N, K) in list(T.GEMM_SPLIT_TABLE) + [T.GEMM_UNSPLIT, (1568, 32, 2048), (100352, 256, 256)]:
            assert lib.hpfg_gemm_f32_splits(M, N, K) == T.gemm_split_geometry("f32", M, N, K)[0]
            assert lib.hpfg_gemm_bf16x3_splits(M, N, K) == T.gemm_split_geometry("bf16x3", M, N, K)[0]
        for R, N, K, _ in T.TN_CASES:
            assert lib.hpfg_gemm_tn_splits(R, N, K) == T.tn_geometry(R, N, K)[0]
        for R in list(T.COL_SUM_R) + [T.COL_SUM_CAP[0]]:
            assert lib.hpfg_col_sum_splits(R) == T.col_sum_geometry(R)[0]


def test_which_row_splits_can_be_empty():
    """hpfg_gemm_tn_bf16x3: while the rows decide the split count (splits = ceil(R / 256)) the rounding of the rows per split to 32 never
    leaves the last split without rows; once the tile count or the cap of 512 decides it, trailing splits can own no rows and must
    contribute zeros -- T.TN_EMPTY is the smallest such case.  hpfg_col_sum2 rounds to whole rows: never empty."""
    for R in list(range(1, 5000)) + [131072]:
        S, per, last = T.tn_geometry(R, 4, 4)
        assert S == -(-R // 256) and 1 <= last <= per, R
    R, N, K, _ = T.TN_EMPTY
    S, per, last = T.tn_geometry(R, N, K)
    assert (S, per, -(-R // per)) == (512, 288, 456) and last < 0
    for R in list(range(1, 3000)) + [131073, 10 ** 6 + 7]:
        S, per = T.col_sum_geometry(R)
        assert (S - 1) * per < R <= S * per


# ---- the conditions of the GPU tests' inputs ----------------------------------------------------------------------------------------------
def test_ragged_shapes_are_ragged_where_they_claim():
    assert (65 % 64, 63 % 64, 17 % 16) != (0, 0, 0) and all(v % t for v, t in zip((65, 63, 273), (64, 64, 16)))
    assert all(v % 128 for v in (132, 124)) and 36 % 32 and 28 % 32 and 260 % 128 and 68 % 32
    for M, N, K in T.GEMM_BF16_SHAPES:
        assert M % 4 == 0 and N % 4 == 0 and K % 4 == 0          # every orientation is eligible
    assert [c[1] % 4 != 0 or c[3] % 4 != 0 for c in T.GEMM_SCALAR_EPILOGUE] == [True, True, True, False]
    for (R, N, K, with_db), (S, per, last) in T.TN_CASES.items():
        assert per % 32 == 0
    assert T.TN_CASES[(257, 68, 132, 1)][0] == 2 and 68 > 64 and 132 > 128          # db over two n-tiles, 2 x 3 tiles
    for N, Hh, W, C_, S, ps in T.POOL_CASES:
        assert S <= Hh and S <= W and ps >= C_ and C_ <= 1024
    assert [c[3] % 256 for c in T.POOL_CASES[3:6]] == [4, 1, 0]
    y0, y1 = T.pool_bins(70, 2)[0]
    x0, x1 = T.pool_bins(66, 2)[0]
    assert (y1 - y0) * (x1 - x0) == 1155 and 1155 // 64 >= 4 and (1155 % (4 * 64)) != 0          # the unrolled loop and its remainder
    assert T.pool_bins(7, 4) == [(0, 2), (1, 4), (3, 6), (5, 7)]          # overlapping bins


@pytest.mark.parametrize("math,shape", [(m, s) for m, ss in T.GEMM_EPILOGUE_SHAPES.items() for s in ss])
def test_epilogue_case_separates_the_two_orders(math, shape):
    c = T.gemm_case(*shape)
    for bias in (False, True):
        e = T.gemm_epilogue(c, bias, True, True)
        wrong = T.gemm_f64(c["A"], c["B"], c["bias"] if bias else None, c["C0"], True, mutation="relu_before_accumulate")
        assert float((wrong - e["law"]).abs().max()) >= 100.0 * e["tol"][math]


@pytest.mark.parametrize("T_,S", T.NTXENT_T)
@pytest.mark.parametrize("family", T.NTXENT_FAMILIES)
@pytest.mark.parametrize("n", T.NTXENT_N)
def test_ntxent_yardstick_is_finite_and_families_meet_their_conditions(n, family, T_, S):
    c = T.ntxent_case(family, n, T_, S)
    assert np.isfinite(float(c["yard"][0])) and bool(torch.isfinite(c["yard"][1]).all())
    assert abs(float(c["G"][0, 0]) - S) < (1e-2 if family == "nonsymmetric" else 1e-5) * S
    loss = float(c["law"][0])
    if family == "near_copy":
        assert c["tol"][0] >= 4.0 * T.ulp32(S / T_ * 0.99)          # the floor comes from the terms, not from the result
        assert abs(loss) < 0.05 if S == 16 else loss <= float(T.ntxent_case("independent", n, T_, S)["law"][0])
    elif n >= 2:
        assert loss > 0.3 * np.log(2 * n)
    if family == "nonsymmetric":
        assert float((c["G"] - c["G"].t()).abs().max()) > 1e-5
    if n == 1:
        assert not c["law"][1].any()          # denom = pos: Q is exactly zero


def test_sum_minus_diagonal_is_no_yardstick():
    """why the float32 yardstick masks: at S = 16 the diagonal term e^(16 / 0.7) swallows the row sum"""
    c = T.ntxent_case("independent", 3, 0.7, 16)
    E = torch.exp(c["G"] / np.float32(0.7))
    assert not bool(torch.isfinite(-torch.log(torch.exp(c["G"][0, 3] / np.float32(0.7)) / (E.sum(1) - E.diag())[0])))


# ---- the mutation proof -------------------------------------------------------------------------------------------------------------------
def _gemm_mutation_cases(mutation):
    if mutation in ("split_chunk_doubled", "bias_per_split"):
        return [(s, m) for s, row in T.GEMM_SPLIT_TABLE.items() for m, geo in row.items() if geo]
    if mutation in ("lo_hi_dropped", "hi_hi_only"):
        return [(s, "bf16x3") for s in T.GEMM_BF16_SHAPES] + [(s, "bf16x3") for s, row in T.GEMM_SPLIT_TABLE.items() if row["bf16x3"]]
    if mutation == "relu_before_accumulate":
        return [(s, m) for m, ss in T.GEMM_EPILOGUE_SHAPES.items() for s in ss]
    return [(s, "f32") for s in T.GEMM_F32_SHAPES] + [(s, "bf16x3") for s in T.GEMM_BF16_SHAPES]


@pytest.mark.parametrize("mutation", T.GEMM_MUTATIONS)
def test_gemm_mutations_are_caught(mutation):
    best = {}
    for shape, math in _gemm_mutation_cases(mutation):
        c = T.gemm_case(*shape)
        epi = mutation in ("bias_per_split", "relu_before_accumulate")
        e = T.gemm_epilogue(c, epi, epi, epi)
        kper = T.gemm_split_geometry(math, *shape)[1]
        kw = dict(bias=c["bias"], C0=c["C0"], relu=True) if epi else {}
        f = float((T.gemm_f64(c["A"], c["B"], mutation=mutation, kper=kper, **kw) - e["law"]).abs().max()) / e["tol"][math]
        print(f"{mutation} {math} {shape}: {f:.3g} tolerances")
        best[math] = max(best.get(math, 0.0), f)
    assert best and min(best.values()) >= 4.0, best          # caught under the rule of every kernel family it applies to


def test_old_rule_against_the_new_one():
    """The figures of DESIGN.md: the split emulation's own error against the 64 x float32 bound the split-bf16 kernels had, and against
    the sum of the two yardsticks they have now."""
    for shape in ((8, 8, 264), (65, 63, 273), (132, 68, 516)):
        c = T.gemm_case(*shape)
        own = float((c["ysplit"].double() - c["law"]).abs().max())
        old, new = T.bound_8x(c["law"], c["y32"], 64.0), c["tol"]["bf16x3"]
        print(f"{shape}: emulation error {own:.3g}, 64 x float32 bound {old:.3g} (ratio {own / old:.3g}), new bound {new:.3g} (ratio {own / new:.3g})")
        assert own / new <= 0.126          # its own 8 x term alone admits it eight times over


@pytest.mark.parametrize("mutation", T.TN_MUTATIONS)
def test_tn_mutations_are_caught(mutation):
    best = 0.0
    for (R, N, K, with_db), (S, per, last) in T.TN_CASES.items():
        if mutation == "db_first_tile_only" and not with_db:
            continue
        c = T.tn_case(R, N, K)
        dw, db = T.tn_mutant(c, mutation, per)
        f = float((dw - c["dw"]).abs().max()) / c["tol_dw"]
        if with_db:
            f = max(f, float((db - c["db"]).abs().max()) / c["tol_db"])
        print(f"{mutation} {(R, N, K)}: {f:.3g} tolerances")
        best = max(best, f)
    assert best >= 4.0


@pytest.mark.parametrize("mutation", T.POOL_MUTATIONS)
def test_pool_mutations_are_caught(mutation):
    best = 0.0
    for N, Hh, W, C_, S, _ in T.POOL_CASES:
        c = T.pool_case(N, Hh, W, C_, S)
        if mutation == "bwd_divides_by_hw":
            f = max(float((T.neck_pool_bwd_f64(a, b, N, Hh, W, C_, S, mutation) - c["dx_" + w]).abs().max()) / T.bound_8x(c["dx_" + w], c["dx32_" + w])
                    for w, (a, b) in dict(pool=(None, c["dpool"]), both=(c["dgap"], c["dpool"])).items())
        else:
            gap, pool = T.neck_pool_f64(c["x"], S, mutation)
            f = max(float((gap - c["gap"]).abs().max()) / T.bound_8x(c["gap"], c["gap32"]),
                    float((pool - c["pool"]).abs().max()) / T.bound_8x(c["pool"], c["pool32"]))
        print(f"{mutation} {(N, Hh, W, C_, S)}: {f:.3g} tolerances")
        best = max(best, f)
    assert best >= 4.0


@pytest.mark.parametrize("mutation", T.L2NORM_MUTATIONS)
def test_l2norm_mutations_are_caught(mutation):
    """x / (norm + eps) shows only on a column whose norm is of the size of eps: the `tiny` column (added for this mutation)."""
    best = 0.0
    for G, D, S in T.L2NORM_CASES:
        for special in T.L2NORM_SPECIAL:
            c = T.l2norm_case(G, D, S, special)
            u, norms = T.l2norm_f64(c["x"], mutation)
            dx = T.l2norm_bwd_f64(c["du"], c["u"], c["norms"], mutation=mutation)
            f = 0.0
            for name, got in (("u", u), ("norms", norms), ("dx", dx)):
                for g_, law, y32 in zip(T.l2norm_parts(c, got), T.l2norm_parts(c, c[name]), T.l2norm_parts(c, c[name + "32"])):
                    f = max(f, float((g_ - law).abs().max()) / T.bound_8x(law, y32))
            print(f"{mutation} {(G, D, S)} {special}: {f:.3g} tolerances")
            best = max(best, f)
    assert best >= 4.0


@pytest.mark.parametrize("mutation", T.NTXENT_MUTATIONS)
def test_ntxent_mutations_are_caught(mutation):
    best, by_family = 0.0, {}
    for T_, S in T.NTXENT_T:
        for family in T.NTXENT_FAMILIES:
            for n in T.NTXENT_N:
                c = T.ntxent_case(family, n, T_, S)
                loss, Q, _ = T.ntxent_f64(c["G"], n, T_, mutation)
                f = max(abs(float(loss) - float(c["law"][0])) / c["tol"][0], float((Q - c["law"][1]).abs().max()) / c["tol"][1] if n > 1 else 0.0)
                print(f"{mutation} {family} n={n} T={T_}: {f:.3g} tolerances")
                best = max(best, f)
                by_family[family] = max(by_family.get(family, 0.0), f)
    assert best >= 4.0, by_family
