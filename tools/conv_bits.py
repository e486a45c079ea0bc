"""SHA-256 of every result of the split-bf16 convolution kernels on a fixed list of small cases: the guard that a change to their staging code
(csrc/stage.h and the four kernel families built on it: conv_bf16_kernel.h, conv_thin_kernel.h, fused_bwd_kernel.h, wgrad_bf16_kernel.h)
keeps every bit.

The cases are the ones the suite already argues for, with inputs from the same seeded generators, in bf16x3 math:
  chunked / wgrad  the lists of tests/helpers.py (FWD3_CASES, FWD3_PERSISTENT, DGRAD3_CASES with their epilogues, FWD1_CASES, DGRAD1_CASES,
                   UPBWD_CASES, STAGE_CASES, WGRAD_CASES) through AdHocConv, set up as tests/test_gpu_conv_sources.py sets them up
  thin             CASES and the two 64 -> 32 dgrad cases of tests/test_gpu_conv_thin.py, and two sources whose coefficients come from the
                   producer's sum accumulators (HpfgAct.bn_acc, as tests/test_gpu_bn_acc.py FWD_CONSUMERS)
  fused            CASES of tests/test_gpu_fused_bwd.py
  unet             one U-Net forward + backward at 2 x 64 x 64 in train mode (dropout on) through the default routes: the one case that runs
                   the concat source inside all four families with the engine's own strides
For each the digest of the raw bytes of every result: out, out2, the rows of stat_partials the launch reports, stage_out, side_sums, dw, dX,
logits, parameter gradients.  Writes one JSON object {case: {result: digest}} to --out.

To compare two trees, run this same file in each (a fresh process per tree) and compare the two JSON files; tests/golden/conv_bits.json is
the run of the commit before the staging phases were shared, and tests/test_gpu_conv_bits.py compares against it.  Needs a GPU: there is no
fallback."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THIN_DGRAD = [(2, 32, 48, 0.0), (5, 48, 32, 0.2)]                                          # test_gpu_conv_thin.py: N, H, W, p of the 64 -> 32 layer
THIN_ACC = [(2, 32, 32, 16, 16, "bnact", 8, 16, 48), (2, 32, 32, 16, 16, "cat", 2, 0, 16)]      # test_gpu_bn_acc.py FWD_CONSUMERS, the thin rows
UNET = (2, 64, 64)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _id(case):
    return "-".join("x" if v is None else str(v) for v in case)


def _rows(part, rows, cpad):
    return _sha(part.view(-1, 2, cpad)[:rows])


def _chunked(res):
    """groups A .. E of tests/test_gpu_conv_sources.py"""
    import torch
    from hpfg_amd import _lib as L
    from tests import helpers as T
    from tests import test_gpu_conv_sources as S
    B16, DEV, NAN = L.MATH_BF16X3, S.DEV, float("nan")

    def forward(name, case, taps):
        kind, p, N, H, W, cin, cout, opt = case
        seed = T.case_seed(*case)
        s = T.conv_source(kind, seed, N, H, W, cin, p)
        with S._narrow(opt):
            layer = T.AdHocConv(cin, cout, taps, DEV, seed=seed, hw=(H, W))
            a0, a1, keep = S._device_source(s, H, W)
            out, part = layer.conv(a0, a1, N, H, W, stats=True, math=B16, out_pstride=cout + S.OPAD, out_coff=S.OOFF)
            torch.cuda.synchronize()
        res[f"{name} {_id(case)}"] = {"out": _sha(S._interior(out, cout, S.OOFF)[0]), "stat_partials": _rows(part, layer.rows, layer.cout_pad)}

    for case in T.FWD3_CASES + [T.FWD3_PERSISTENT]:
        forward("fwd3", case, 9)
    for case in T.FWD1_CASES:
        forward("fwd1", case + (None,), 1)

    for case in T.DGRAD3_CASES:
        kind, p, N, H, W, cin, cout, opt, epi = case
        seed = T.case_seed(*case)
        s = T.conv_source(kind, seed, N, H, W, cout, p)
        r = res[f"dgrad3 {_id(case)}"] = {}
        with S._narrow(opt):
            layer = T.AdHocConv(cin, cout, 9, DEV, seed=seed, hw=(H, W))
            g0, _, keep = S._device_source(s, H, W)
            if epi == "split":
                half = cin // 2
                out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=half + S.OPAD, out_coff=S.OOFF, out_split=half,
                                    out2_pstride=cin + S.O2PAD, out2_coff=S.O2OFF)
                r["out"], r["out2"] = _sha(S._interior(out, half, S.OOFF)[0]), _sha(S._interior(layer.out2, cin - half, S.O2OFF)[0])
            elif epi == "pool":      # the max-pool backward in the epilogue, in place on bwd_of.aux
                be = T.pool_epilogue_source(T.pool_epilogue_seed(case), N, H, W, cin)
                bo, _, bkeep = S._device_source(be, 2 * H, 2 * W)
                _, part = layer.conv(g0, None, N, H, W, stats=True, dgrad=True, math=B16, bwd_stats=2, bwd_of=bo, out_pstride=cin + S.OPAD,
                                     out_coff=S.OOFF)
                torch.cuda.synchronize()
                r["out"], r["stat_partials"] = _sha(S._interior(bkeep[2], cin, S.AOFF)[0]), _rows(part, layer.rows, layer.cin_pad)
            else:
                out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + S.OPAD, out_coff=S.OOFF)
                r["out"] = _sha(S._interior(out, cin, S.OOFF)[0])
                if epi == "stats1":
                    below = T.conv_source("dz", seed + 1, N, H, W, cin, 0.3)
                    bo, _, bkeep = S._device_source(below, H, W)
                    out1, part = layer.conv(g0, None, N, H, W, stats=True, dgrad=True, math=B16, bwd_stats=1, bwd_of=bo,
                                            out_pstride=cin + S.OPAD, out_coff=S.OOFF)
                    torch.cuda.synchronize()
                    r["out stats1"], r["stat_partials"] = _sha(S._interior(out1, cin, S.OOFF)[0]), _rows(part, layer.rows, layer.cin_pad)
            torch.cuda.synchronize()

    for case in T.DGRAD1_CASES:
        N, H, W, cin, cout = case
        seed = T.case_seed(*(("plain", 0.0) + case + (None, None)))
        s = T.conv_source("plain", seed, N, H, W, cout)
        layer = T.AdHocConv(cin, cout, 1, DEV, seed=seed, hw=(H, W))
        g0, _, keep = S._device_source(s, H, W)
        out, _ = layer.conv(g0, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + S.OPAD, out_coff=S.OOFF)
        torch.cuda.synchronize()
        res[f"dgrad1 {_id(case)}"] = {"out": _sha(S._interior(out, cin, S.OOFF)[0])}

    for case in T.UPBWD_CASES:
        N, H, W, cin, cout = case
        seed = T.case_seed(*case)
        gup = torch.randn(N, 2 * H, 2 * W, cout, generator=torch.Generator().manual_seed(seed))
        layer = T.AdHocConv(cin, cout, 1, DEV, seed=seed, hw=(H, W))
        gb, gptr = S._wide(gup)
        a = L.Act()
        a.z, a.mode, a.C, a.Hs, a.Ws, a.pstride = gptr, L.ACT_UPBWD, cout, H, W, cout + S.PADC
        rows = N * ((H + 7) // 8) * ((W + 7) // 8)
        stage = torch.full((N, H, W, cout), NAN, device=DEV)
        side = torch.full((rows, cout), NAN, device=DEV)
        out, _ = layer.conv(a, None, N, H, W, dgrad=True, math=B16, out_pstride=cin + S.OPAD, out_coff=S.OOFF, stage_out=stage, side_sums=side)
        torch.cuda.synchronize()
        res[f"upbwd {_id(case)}"] = {"out": _sha(S._interior(out, cin, S.OOFF)[0]), "stage_out": _sha(stage), "side_sums": _sha(side)}

    for kind, p in T.STAGE_CASES:
        N, H, W, Cc = 3, 10, 34, 64
        seed = T.case_seed(kind, p, N, H, W, Cc, Cc)
        si, sg = T.conv_source(kind, seed, N, H, W, Cc, p), T.conv_source("dz", seed + 1, N, H, W, Cc, 0.3)
        layer = T.AdHocConv(Cc, Cc, 9, DEV, seed=seed, hw=(H, W))
        a0, a1, keep = S._device_source(si, H, W)
        g0, _, gkeep = S._device_source(sg, H, W)
        r, stage = {}, {}
        for name, src, dgrad in (("input", (a0, a1), False), ("dZ", (g0, None), True)):
            buf = torch.full((N, H, W, Cc), NAN, device=DEV)
            out, _ = layer.conv(src[0], src[1], N, H, W, dgrad=dgrad, math=B16, stage_out=buf)
            torch.cuda.synchronize()
            r[f"stage_out {name}"], r[f"out {name}"], stage[name] = _sha(buf), _sha(out), buf
        dw = layer.wgrad(S._split_act(stage["input"], Cc, H, W), None, S._split_act(stage["dZ"], Cc, H, W), N, H, W, math=B16, slab_nan=True)
        torch.cuda.synchronize()
        r["dw"] = _sha(dw)
        res[f"stage {kind}-{p}"] = r

    for case in T.WGRAD_CASES:
        ak, pa, gk, pg, N, H, W, cin, cout, taps = case
        seed = T.case_seed(*case)
        sa, sg = T.conv_source(ak, seed, N, H, W, cin, pa), T.conv_source(gk, seed + 1, N, H, W, cout, pg)
        layer = T.AdHocConv(cin, cout, taps, DEV, seed=seed, hw=(H, W))
        a0, a1, keep = S._device_source(sa, H, W)
        g0, _, gkeep = S._device_source(sg, H, W)
        dw = layer.wgrad(a0, a1, g0, N, H, W, math=B16, slab_nan=True)
        torch.cuda.synchronize()
        res[f"wgrad {_id(case)}"] = {"dw": _sha(dw)}


def _thin_source(ak, g, N, H, W, cin, p, seed):
    """the layer input of a case of test_gpu_conv_thin.py / test_gpu_fused_bwd.py: (a0, a1, raw z, table, keep-alive)"""
    import torch
    from hpfg_amd import _lib as L
    from tests.test_gpu_fused_bwd import DEV, _bnact
    from tests.test_gpu_kernels import _bn_table
    if ak == "bnact":
        z, tab = torch.randn(N, H, W, cin, generator=g).to(DEV), _bn_table(cin, 3).to(DEV)
        return _bnact(z, tab, cin, H, W, p=p, seed=seed), None, z, tab, ()
    if ak == "pool":
        z, tab = torch.randn(N, 2 * H, 2 * W, cin, generator=g).to(DEV), _bn_table(cin, 3).to(DEV)
        return _bnact(z, tab, cin, 2 * H, 2 * W, mode=L.ACT_BNACT_POOL), None, z, tab, ()
    c2 = cin // 2
    z, tab = torch.randn(N, H, W, c2, generator=g).to(DEV), _bn_table(c2, 3).to(DEV)
    ud = torch.randn(N, H // 2, W // 2, c2, generator=g).to(DEV)
    a1 = L.Act()
    a1.z, a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = L.ptr(ud), L.ACT_UP2X, c2, H // 2, W // 2, c2
    return _bnact(z, tab, c2, H, W), a1, z, tab, (ud,)


def _thin(res):
    """the whole-tile forward kernel: a bf16x3 launch of an eligible layer takes it (rows = a multiple of 8 workgroups)"""
    import numpy as np
    import torch
    from hpfg_amd import _lib as L
    from tests import helpers as T
    from tests import test_gpu_bn_acc as A
    from tests import test_gpu_conv_thin as TH
    from tests.test_gpu_fused_bwd import _dz
    from tests.test_gpu_kernels import _bn_table
    B16, DEV = L.MATH_BF16X3, TH.DEV
    for case in TH.CASES:
        N, H, W, cin, cout, ak, p = case
        g = torch.Generator().manual_seed(H * 5 + cin + cout)
        layer = T.AdHocConv(cin, cout, 9, DEV, seed=cin * 3 + cout, hw=(H, W))
        a0, a1, z, tab, keep = _thin_source(ak, g, N, H, W, cin, p, 55)
        stats = cout % 16 == 0
        out, part = layer.conv(a0, a1, N, H, W, stats=stats, math=B16)
        torch.cuda.synchronize()
        r = res[f"thin {_id(case)}"] = {"out": _sha(out)}
        if stats:
            assert layer.rows % 8 == 0
            r["stat_partials"] = _rows(part, layer.rows, layer.cout_pad)
    for case in THIN_DGRAD:
        N, H, W, p = case
        g = torch.Generator().manual_seed(H + W)
        layer = T.AdHocConv(64, 32, 9, DEV, seed=4, hw=(H, W))
        zo, dA = torch.randn(N, H, W, 32, generator=g).to(DEV), torch.randn(N, H, W, 32, generator=g).to(DEV)
        tabo = _bn_table(32, 11).to(DEV)
        out, _ = layer.conv(_dz(zo, tabo, dA, 32, H, W, p=p, seed=21), None, N, H, W, dgrad=True, math=B16)
        torch.cuda.synchronize()
        res[f"thin dgrad {_id(case)}"] = {"out": _sha(out)}
    for case in THIN_ACC:
        N, H, W, cs, cout, kind, shards, coff, stride = case
        g = torch.Generator().manual_seed(H + cs + cout + coff)
        cin = 2 * cs if kind == "cat" else cs
        layer = T.AdHocConv(cin, cout, 9, DEV, seed=cs + cout, hw=(H, W))
        z = A._randn(g, N, H, W, cs)
        gamma, beta = torch.randn(stride, generator=g), torch.randn(stride, generator=g)
        rows = np.asarray(A._chunk_rows(A._randn(g, N * 4, stride), N))
        rows[:, :, coff:coff + cs] = A._chunk_rows(z.reshape(-1, cs), N)
        zd, gd, bd, acc = z.to(DEV), gamma.to(DEV), beta.to(DEV), T.acc_from_rows(rows, shards).to(DEV)
        tab = torch.full((L.BN_ROWS, stride), float("nan"), device=DEV)
        a0 = L.Act()
        a0.z, a0.bn, a0.mode, a0.C, a0.Hs, a0.Ws, a0.pstride = L.ptr(zd), L.ptr(tab), L.ACT_BNACT, cs, H, W, cs
        a0.bn_stride, a0.bn_coff = stride, coff
        a0.bn_acc, a0.bn_gamma, a0.bn_beta, a0.bn_count, a0.bn_eps, a0.bn_shards = L.ptr(acc), L.ptr(gd), L.ptr(bd), float(N * H * W), A.EPS, shards
        a1 = None
        if kind == "cat":
            ud = A._randn(g, N, H // 2, W // 2, cs).to(DEV)
            a1 = L.Act()
            a1.z, a1.mode, a1.C, a1.Hs, a1.Ws, a1.pstride = L.ptr(ud), L.ACT_UP2X, cs, H // 2, W // 2, cs
        out, part = layer.conv(a0, a1, N, H, W, stats=True, math=B16)
        torch.cuda.synchronize()
        assert layer.rows % 8 == 0
        res[f"thin bn_acc {_id(case)}"] = {"out": _sha(out), "stat_partials": _rows(part, layer.rows, layer.cout_pad)}


def _fused(res):
    import torch
    from tests import helpers as T
    from tests import test_gpu_fused_bwd as FB
    from tests.test_gpu_kernels import _bn_table
    DEV = FB.DEV
    for k, case in enumerate(FB.CASES):
        N, H, W, cin, cout, ak, gk, p_in, p_out = case
        g = torch.Generator().manual_seed(H * 7 + cin * 3 + cout)
        layer = T.AdHocConv(cin, cout, 9, DEV, seed=cin + cout, hw=(H, W))
        xa0, xa1, zi, tabi, keep = _thin_source(ak, g, N, H, W, cin, p_in, 77)
        if gk == "dz":
            zo, dA = torch.randn(N, H, W, cout, generator=g).to(DEV), torch.randn(N, H, W, cout, generator=g).to(DEV)
            tabo = _bn_table(cout, 11).to(DEV)
            gsrc = FB._dz(zo, tabo, dA, cout, H, W, p=p_out, seed=99)
        else:
            dl = torch.randn(N, H, W, cout, generator=g).to(DEV)
            gsrc = T.plain_act(dl, cout, H, W)
        bwd_of = FB._dz(zi, tabi, None, cin, H, W, p=p_in, seed=77) if ak == "bnact" else None
        split = cin // 2 if (ak == "cat" and cin == 32) else 0
        dx, dw, part = FB._fused(layer, xa0, xa1, gsrc, N, H, W, bwd_of=bwd_of, split=split)
        r = res[f"fused {k} {_id(case)}"] = {"dw": _sha(dw)}      # (the index: the list holds the concat case twice)
        if split:
            r["dX"], r["dX2"] = _sha(dx[0]), _sha(dx[1])
        else:
            r["dX"] = _sha(dx)
        if part is not None:
            r["stat_partials"] = _sha(part)


def _unet(res):
    import torch
    from hpfg_amd.model import UNet, reset_dropout_streams
    dev = torch.device("cuda:0")
    N, H, W = UNET
    reset_dropout_streams()
    torch.manual_seed(3)
    m = UNet(1, 4).to(dev)
    m.train()
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(N, 1, H, W, generator=g).to(dev), torch.randn(N, 4, H, W, generator=g).to(dev)
    out = m(x)
    out.backward(dy)
    torch.cuda.synchronize()
    r = res[f"unet {N}x{H}x{W} {m.math}"] = {"logits": _sha(out)}
    for name, p in m.named_parameters():
        r[f"grad {name}"] = _sha(p.grad)


def digests(unet=True):
    """{case name: {result name: sha256 hex}} of every case, computed on cuda:0"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_bits: no GPU; nothing computed")
    res = {}
    _chunked(res)
    _thin(res)
    _fused(res)
    if unet:
        _unet(res)
    torch.cuda.synchronize()
    return res


def n_cases():
    from tests import helpers as T
    from tests import test_gpu_conv_thin as TH
    from tests import test_gpu_fused_bwd as FB
    lists = (T.FWD3_CASES, [T.FWD3_PERSISTENT], T.DGRAD3_CASES, T.FWD1_CASES, T.DGRAD1_CASES, T.UPBWD_CASES, T.STAGE_CASES, T.WGRAD_CASES,
             TH.CASES, THIN_DGRAD, THIN_ACC, FB.CASES, [UNET])
    return sum(len(l) for l in lists)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="the JSON file to write (keep it out of the tracked tree)")
    a = ap.parse_args()
    r = digests()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"conv_bits: {len(r)} cases -> {a.out}")
