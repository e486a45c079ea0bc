"""CPU: the float64 laws of the first conv and the stand-alone backward kernels (tests/helpers.py, "the first conv and the stand-alone
backward kernels") against torch's own float64 ops and autograd; the same laws in torch float32 inside the derived bounds on every case of
tests/test_gpu_standalone_edges.py (a case that fails this is wrongly chosen, not the kernel); the Python replicas of the launch
geometries against the counts the case comments claim and, since they are host code, against the library's own functions; and the mutation
proof: every named wrong variant of a law moves some output of some GPU case by at least 4 bounds."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import helpers as T


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _lib():
    from hpfg_amd import _lib as L
    return L.load() if os.path.exists(L.LIB_PATH) else None


# ---- the laws are torch's float64 ops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 17, 31, 3), (1, 5, 40, 2), (1, 1, 1, 4)], ids=str)
def test_first_conv_law_is_conv2d_without_the_split_term(case):
    c = T.first_fwd_case(*case)
    want = F.conv2d(T.nchw(c["x"].double()), c["w"].double(), c["b"].double(), padding=1).permute(0, 2, 3, 1)
    assert c["ref"].dtype == torch.float64 and _rel(c["ref"], want) <= 1e-12
    assert torch.equal(T.first_fwd_f64(c["x"].double(), c["w"], c["b"]), c["ref"])
    _, with_split = T.conv_ref_bound(c["x"].double(), torch.zeros_like(c["x"], dtype=torch.float64), c["w"], c["b"])
    S = (with_split - c["bound"]) / (3.0 * 2.0 ** -16)          # the split term is exactly what split=False leaves out
    T_ = 9 * case[3] + 1
    assert _rel(c["bound"], (T_ + 2) * T.U24 * S) <= 1e-9 and float((with_split / c["bound"]).min()) > 20          # 1 + 768 / (T + 2)


@pytest.mark.parametrize("case", [(1, 1, 1, 4), (2, 1, 7, 8), (2, 7, 1, 8), (2, 2, 2, 4), (1, 5, 6, 12), (1, 9, 7, 256)], ids=str)
def test_upbwd_law_is_autograd_of_interpolate(case):
    """to 1e-6 relative: the law forms its weights in fp32 like the kernels, f = ratio * index to 2^-24 f -- the cases with at most 9 source rows
    and columns, where that is below the tolerance"""
    N, Hl, Wl, C_ = case
    c = T.upbwd_case(*case)
    u = torch.zeros(N, C_, Hl, Wl, dtype=torch.float64, requires_grad=True)
    F.interpolate(u, scale_factor=2, mode="bilinear", align_corners=True).backward(T.nchw(c["g"].double()))
    assert _rel(c["ref"], u.grad.permute(0, 2, 3, 1)) <= 1e-6
    assert torch.equal(T.upbwd_mutant(c["g"], None, T.upbwd_geometry(*case)), c["ref"])


def test_the_gather_window_is_wider_than_any_weight_reaches():
    """hpfg_up_taps looks at outputs 2 lo - 2 .. 2 lo + 4; with the law's fp32 weights an output outside 2 lo - 1 .. 2 lo + 2 never reads source lo, for every
    admitted table size -- the variant window_one_short therefore loses 2 lo + 2, the last that counts"""
    reach = [T.up2x_window_reach(Lo) for Lo in (1, 2, 3, 4, 5, 7, 16, 25, 64, 255, 256, 511)]
    assert max(r[0] for r in reach) == 2 and min(r[1] for r in reach) == -1


@pytest.mark.parametrize("case", [c for c in T.POOLBWD_CASES if c[3] <= 64 and not c[4]], ids=str)
def test_pool_scatter_law_is_autograd_of_max_pool2d(case):
    c = T.poolbwd_case(*case)
    a = T.nchw(c["a"]).requires_grad_(True)
    F.max_pool2d(a, 2).backward(T.nchw(c["dP"].double()))
    assert torch.equal(T.pool_scatter_f64(c["dP"], c["first"]), a.grad.permute(0, 2, 3, 1))
    assert torch.equal(c["done"], c["base"] + a.grad.permute(0, 2, 3, 1).float())


def test_channel_sum_and_slab_laws_are_sums():
    c = T.chansum_case(5000, 16, 24)
    assert _rel(c["ref"], c["buf"].double().reshape(5000, 24)[:, :16].sum(0)) <= 1e-12
    c = T.chansum_case(*T.CHANSUM_OFFSET)
    npix, C_, ps, off = T.CHANSUM_OFFSET
    assert _rel(c["ref"], c["buf"].double()[off:].reshape(npix, ps)[:, :C_].sum(0)) <= 1e-12
    for layer in T.SLAB_LAYERS:
        taps, cin, cip, cout, cop = layer
        c = T.slab_case(layer, 17)
        assert c["ref"].shape == (cout, cin, taps) and bool(torch.isfinite(c["ref"]).all())
        want = torch.nan_to_num(c["slab"].double()).sum(0)[:, :cin, :cout]
        for co, ci, tap in ((0, 0, 0), (cout - 1, cin - 1, taps - 1)):
            assert abs(float(c["ref"][co, ci, tap] - want[tap, ci, co])) <= 1e-12
        assert bool(torch.isnan(c["slab"][:, :, cin:]).all()) and bool(torch.isnan(c["slab"][:, :, :, cout:]).all())


def test_bwd_sums_law_is_the_batchnorm_backward_of_autograd():
    """sum g and sum g xhat of bwd_sums_f64 are dbeta and dgamma of a float64 BatchNorm + LeakyReLU (+ dropout) chain with the table's statistics"""
    N, H, W, C_, p = T.BNBWD_CASES[1]
    c = T.bnbwd_case(N, H, W, C_, p)
    s = c["s"]
    tab = s["tab"].double()
    gamma = torch.ones(C_, dtype=torch.float64, requires_grad=True)
    beta = torch.zeros(C_, dtype=torch.float64, requires_grad=True)
    xh = (s["z"].double() - tab[T.L.BN_MEAN]) * tab[T.L.BN_RSTD]
    y = s["z"].double() * tab[T.L.BN_SCALE] + tab[T.L.BN_SHIFT]          # the slope is decided by the table's affine map
    slope = torch.where(y > 0, 1.0, T.LEAKY32)
    out = (xh * gamma + beta) * slope * T.keep_f64(s["z"].shape, p, s["dseed"])
    out.backward(s["dA"].double())
    assert _rel(c["val"][0], beta.grad) <= 1e-12 and _rel(c["val"][1], gamma.grad) <= 1e-12


# ---- the reference alone stays within the bound: the same law in torch float32 on the CPU ------------------------------------------------
def test_float32_reference_is_within_every_bound():
    worst = {}

    def note(group, ratio, what):
        assert ratio <= 1.0, f"{group} {what}: torch float32 is {ratio:.3g} x the bound off -- the case is wrongly chosen"
        worst[group] = max(worst.get(group, 0.0), ratio)

    for case in T.FIRST_FWD_CASES:
        c = T.first_fwd_case(*case)
        note("first conv", c["f32"], case)
        if T.first_fwd_stats(case[1], case[2]):
            out32 = F.conv2d(T.nchw(c["x"]), c["w"], c["b"], padding=1).permute(0, 2, 3, 1)
            rows = torch.stack([out32.reshape(-1, 16).sum(0), (out32 * out32).reshape(-1, 16).sum(0)])
            note("first conv sums", T.fwd_sums_ratio(rows.double(), out32), case)
    for case in T.UPBWD_SUMS_CASES:
        c = T.upbwd_case(*case)
        note("upsample backward", c["f32"], case)
        if T.upbwd_sums_admitted(case[3]):
            dU = c["ref"].float()
            val, bound = T.upbwd_sums_f64(dU, T.upbwd_geometry(*case))
            note("upsample backward sums", float(((dU.reshape(-1, case[3]).sum(0).double() - val).abs() / bound).max()), case)
    for case in T.CHANSUM_CASES + (T.CHANSUM_OFFSET,):
        note("channel sums", T.chansum_case(*case)["f32"], case)
    for layer in T.SLAB_LAYERS:
        for S in T.SLAB_S:
            note("slab reduce", T.slab_case(layer, S)["f32"], (layer, S))
    for layer in T.SLAB_CAP_LAYERS:
        note("slab reduce", T.slab_case(layer, T.SLAB_CAP_S)["f32"], layer)
    for case in T.BNBWD_CASES:
        note("bn backward sums", T.bnbwd_case(*case)["f32"], case)
    for case in T.POOLBWD_CASES:
        c = T.poolbwd_case(*case)
        C_ = case[3]
        g32 = c["g64"].float()
        xh = (c["z"] - c["tab"][T.L.BN_MEAN]) * c["tab"][T.L.BN_RSTD]
        f32 = torch.stack([g32.reshape(-1, C_).sum(0), (g32 * xh).reshape(-1, C_).sum(0)])
        note("pooled backward sums", float(((f32.double() - c["val"]).abs() / c["bound"]).max()), case)
    for group in sorted(worst):
        print(f"[standalone laws] {group}: torch float32 on the CPU reaches {worst[group]:.3g} x the bound")


# ---- geometry replicas --------------------------------------------------------------------------------------------------------------------
def test_geometry_replicas_give_the_counts_the_cases_claim():
    assert T.first_fwd_geometry(33, 32, 256) == (1024, 1056) and T.first_fwd_geometry(23, 40, 250) == (1024, 1104)
    assert T.first_fwd_geometry(2, 16, 16) == (2, 2) and T.first_fwd_geometry(1, 32, 48) == (6, 6) and T.first_fwd_geometry(1, 5, 40) == (3, 3)
    geo = {c: T.upbwd_geometry(*c) for c in T.UPBWD_SA_CASES}
    g = geo[(1, 16, 30, 16)]
    assert (g["total"], g["blocks"], g["nxcd"], g["gx"], g["span"]) == (1920, 8, 8, 1, 256) and 7 * g["span"] < g["total"] < 8 * g["span"]
    g = geo[(1, 13, 25, 48)]
    assert (g["total"], g["blocks"], g["nxcd"], g["gx"], g["span"], g["trips"]) == (3900, 16, 8, 2, 512, 1)
    g = geo[(1, 20, 23, 20)]
    assert (g["total"], g["blocks"], g["nxcd"]) == (2300, 9, 1)
    g = geo[(3, 64, 64, 128)]
    assert (g["total"], g["blocks"], g["nxcd"], g["gx"], g["span"], g["trips"]) == (393216, 1024, 8, 128, 49152, 2)
    assert g["span"] // 256 == 192          # rows of a span on 128 workgroups: one and a half trips each
    for c in ((1, 1, 511, 4), (1, 511, 1, 4)):
        assert c[1] + c[2] == T.UPB_MAXDIM
    assert T.UPBWD_REFUSED[1] + T.UPBWD_REFUSED[2] == T.UPB_MAXDIM + 1
    assert [c for c in T.UPBWD_SUMS_C if not T.upbwd_sums_admitted(c)] == [48]
    assert not any(T.upbwd_sums_admitted(c) for c in (12, 20, 260)) and all(T.upbwd_sums_admitted(c) for c in (4, 8, 16, 32, 64, 128, 256))
    cs = {c: T.chansum_geometry(*c) for c in T.CHANSUM_CASES}
    g = cs[(100, 64, 64)]
    assert (g["blocks"], g["busy"], g["blocks"] - g["busy"]) == (25, 7, 18)
    g = cs[(1000, 12, 12)]
    assert g["vec"] and g["lanes"] == 85 and 85 * 3 == 255
    assert cs[(300, 256, 256)]["lanes"] == 4 and cs[(5000, 16, 24)]["vec"] and not cs[(5000, 16, 18)]["vec"]
    assert all(not cs[(5000, c, c)]["vec"] for c in (1, 2, 3, 5, 9, 255))
    g = cs[(8197, 256, 256)]
    assert (g["blocks"], g["vec"], g["trips"], g["sweep"]) == (512, True, 2, 8192)
    g = cs[(65539, 2, 2)]
    assert (g["blocks"], g["vec"], g["trips"], g["sweep"]) == (512, False, 2, 65536)
    assert all(g["trips"] == 1 for c, g in cs.items() if c[0] <= 5000 and c[1] != 255) and cs[(5000, 255, 255)]["trips"] == 10
    assert T.chansum_geometry(0, 4, 4)["blocks"] == 0 and T.chansum_geometry(5, 0, 4)["blocks"] == 0 and T.chansum_geometry(5, 257, 257)["blocks"] == 0
    assert T.slab_grid(T.SLAB_CAP_LAYERS) == (2048, 2) and T.slab_grid(T.SLAB_LAYERS) == (36, 1)
    assert {t * cip * cop % 4 != 0 for t, _, cip, _, cop in T.SLAB_LAYERS} == {True, False}          # both paths
    assert min(t * cip * cop for t, _, cip, _, cop in T.SLAB_LAYERS) < 64
    assert T.bn_bwd_blocks(1, 2, 2, 4) == 1 and T.bn_bwd_blocks(2, 3, 5, 1024) == 2 and T.bn_bwd_blocks(3, 12, 16, 64) == 3
    assert T.bn_bwd_pool_blocks(3, 6, 8, 1024) == 72 and T.bn_bwd_pool_blocks(1, 1, 1, 4) == 1


def test_geometry_replicas_are_the_librarys_host_functions():
    lib = _lib()
    if lib is None:          # (host code of the library: compared wherever it is built, as in tests/test_dense_laws_host.py)
        return
    for N, H, W, _ in T.FIRST_FWD_CASES:
        assert lib.hpfg_conv_first_rows(N, H, W) == T.first_fwd_geometry(N, H, W)[0]
    for c in T.UPBWD_SUMS_CASES + (T.UPBWD_REFUSED,):
        assert lib.hpfg_upsample2x_bwd_blocks(*c) == T.upbwd_geometry(*c)["blocks"], c
    for npix, C_, ps in T.CHANSUM_CASES + ((0, 4, 4), (5, 0, 4), (5, 257, 257)):
        assert lib.hpfg_channel_sum_blocks(npix, C_) == T.chansum_geometry(npix, C_, ps)["blocks"], (npix, C_)
    for N, H, W, C_, _ in T.BNBWD_CASES:
        assert lib.hpfg_bn_bwd_blocks(N, H, W, C_) == T.bn_bwd_blocks(N, H, W, C_)
    for N, H2, W2, C_, _ in T.POOLBWD_CASES:
        assert lib.hpfg_bn_bwd_pool_blocks(N, H2 // 2, W2 // 2, C_) == T.bn_bwd_pool_blocks(N, H2 // 2, W2 // 2, C_)
        assert lib.hpfg_bn_bwd_blocks(N, H2, W2, C_) == T.bn_bwd_blocks(N, H2, W2, C_)


# ---- the mutation proof -------------------------------------------------------------------------------------------------------------------
def _first_mutant_ratio(mutation):
    if mutation == "stats_over_partial_tiles":          # the case is the refusal the GPU file pins: were it launched, the sums would be these
        N, H, W = T.FIRST_FWD_REFUSED_STATS
        x = T.conv_source("plain", 5, N, H, W, 1)["z"].double()
        w, b = T.adhoc_weights(1, 16, 9, 5)
        (val, bound), (mut, _) = T.first_sums_f64(x, w, b), T.first_sums_f64(x, w, b, mutation)
        return T.mutation_ratio(mut, val, bound)
    cases = [(33, 32, 256, 1)] if mutation == "second_tile_skipped" else [(2, 16, 16, 1), (2, 17, 31, 3), (1, 1, 1, 4)]
    worst = 0.0
    for case in cases:
        c = T.first_fwd_case(*case)
        worst = max(worst, T.mutation_ratio(T.first_fwd_f64(c["x"].double(), c["w"], c["b"], mutation), c["ref"], c["bound"]))
    return worst


def _upbwd_mutant_ratio(mutation):
    worst = 0.0
    for case in ((2, 2, 2, 4), (1, 16, 30, 16), (1, 13, 25, 48)) + (((3, 64, 64, 128),) if mutation == "sums_of_first_trip_only" else ()):
        c, geo = T.upbwd_case(*case), T.upbwd_geometry(*case)
        if mutation == "sums_of_first_trip_only":
            if T.upbwd_sums_admitted(case[3]):
                (val, bound), (mut, _) = T.upbwd_sums_f64(c["ref"], geo), T.upbwd_sums_f64(c["ref"], geo, mutation)
                worst = max(worst, T.mutation_ratio(mut, val, bound))
        else:
            worst = max(worst, T.mutation_ratio(T.upbwd_mutant(c["g"], mutation, geo), c["ref"], c["bound"]))
    return worst


def _chansum_mutant_ratio(mutation):
    worst = 0.0
    for case in T.CHANSUM_CASES:
        c, geo = T.chansum_case(*case), T.chansum_geometry(*case)
        worst = max(worst, T.mutation_ratio(T.chansum_f64(c["g"], geo, mutation)[0], c["ref"], c["bound"]))
    return worst


def _slab_mutant_ratio(mutation):
    worst = 0.0
    for layer in T.SLAB_LAYERS:
        for S in T.SLAB_S:
            c = T.slab_case(layer, S)
            worst = max(worst, T.mutation_ratio(T.slab_reduce_f64(c["slab"], layer, mutation)[0], c["ref"], c["bound"]))
    return worst


def _poolbwd_mutant_ratio(mutation):
    worst = 0.0
    for case in T.POOLBWD_CASES:
        if case[3] > 64:
            continue
        c = T.poolbwd_case(*case)
        done, sums = T.poolbwd_mutant(c, mutation)
        worst = max(worst, T.mutation_ratio(done, c["done"], 0.0), T.mutation_ratio(sums, c["val"], c["bound"]))
    return worst


_PROOFS = dict(first=_first_mutant_ratio, upbwd=_upbwd_mutant_ratio, chansum=_chansum_mutant_ratio, slab=_slab_mutant_ratio,
               poolbwd=_poolbwd_mutant_ratio)


@pytest.mark.parametrize("group,mutation", [(g, m) for g, ms in T.STANDALONE_MUTATIONS.items() for m in ms])
def test_every_wrong_variant_is_at_least_four_bounds_off(group, mutation):
    ratio = _PROOFS[group](mutation)
    print(f"[standalone laws] {group} {mutation}: {ratio:.3g} x the bound")
    assert ratio >= 4.0, f"{mutation}: no case moves by 4 bounds ({ratio:.3g}) -- a case is missing"


def test_single_faults_are_caught_case_by_case():
    """the cases that exist for one fault each do catch it on their own"""
    c, geo = T.chansum_case(*T.CHANSUM_IDLE), T.chansum_geometry(*T.CHANSUM_IDLE)
    assert T.mutation_ratio(T.chansum_f64(c["g"], geo, "idle_rows_not_zero")[0], c["ref"], c["bound"]) >= 4
    for case in ((8197, 256, 256), (65539, 2, 2)):          # the second trip of either loop
        c, geo = T.chansum_case(*case), T.chansum_geometry(*case)
        assert T.mutation_ratio(T.chansum_f64(c["g"], geo, "last_trip_dropped")[0], c["ref"], c["bound"]) >= 4, case
    for S in T.SLAB_S:                                      # every S above 16 loses a slab of its own
        c = T.slab_case(T.SLAB_LAYERS[0], S)
        r = T.mutation_ratio(T.slab_reduce_f64(c["slab"], T.SLAB_LAYERS[0], "slab_lane_16_dropped")[0], c["ref"], c["bound"])
        assert (r >= 4) == (S > 16), S
    for layer in T.SLAB_LAYERS:                             # the scalar path's tail in every layer that takes it
        per = layer[0] * layer[2] * layer[4]
        c = T.slab_case(layer, 17)
        r = T.mutation_ratio(T.slab_reduce_f64(c["slab"], layer, "scalar_path_quad_tail_dropped")[0], c["ref"], c["bound"])
        assert (r >= 4) == (per % 4 != 0), layer
    c = T.poolbwd_case(*T.POOLBWD_CASES[-1])                # ties on purpose: only there does the tie rule show
    assert T.POOLBWD_CASES[-1][4] and int(c["tied"].sum()) == 2
    assert T.mutation_ratio(T.poolbwd_mutant(c, "last_max_wins")[0], c["done"], 0.0) == float("inf")
    c = T.poolbwd_case(*T.POOLBWD_CASES[1])
    assert T.mutation_ratio(T.poolbwd_mutant(c, "last_max_wins")[0], c["done"], 0.0) == 0.0
    for case in ((1, 16, 30, 16), (1, 13, 25, 48)):         # either XCD case loses its last span
        c, geo = T.upbwd_case(*case), T.upbwd_geometry(*case)
        assert T.mutation_ratio(T.upbwd_mutant(c["g"], "last_xcd_span_dropped", geo), c["ref"], c["bound"]) >= 4, case
