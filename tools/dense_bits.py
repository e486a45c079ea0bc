"""SHA-256 of every result of the split-bf16 GEMM and attention entry points on a fixed list of small cases: the guard that a change to
their arithmetic (csrc/bf16x3.h: the hi / lo split, the transposing LDS read, the three-issue product) or to the kernels built on it
(csrc/gemm.hip, csrc/attn_frag.h, csrc/attn_core.h, attn.hip, attn_keys.hip, attn_window.hip) keeps every bit.

The cases come from the lists the suite already argues for, with inputs from the same seeded generators, in bf16x3 math, straight through
the C entry points:
  gemm         hpfg_gemm_bf16x3 on tests/helpers.GEMM_BF16_SHAPES (one tile, ragged last tiles in M, N and K, three row tiles) in the four
               operand orientations (k-fast: the plain fragment read; row-fast: the transposing read), and GEMM_SCALAR_EPILOGUE with bias,
               accumulate and ReLU
  gemm_splitk  hpfg_gemm_bf16x3_splitk on the bf16x3 rows of GEMM_SPLIT_TABLE, both orientations, with the scratch slices it launched
  gemm_tn      hpfg_gemm_tn_bf16x3 on the rows of TN_CASES up to 600 rows (with and without with_db, the aligned and the unaligned
               instantiation, 1, 2 and 3 row splits) and (33, 36, 20) with x one float off a 16-byte boundary
  attn         hpfg_attn_mfma_fwd_hd / _bwd_hd at 1, 17 and 64 keys, and past one and two dK / dV workgroups of queries
  attn_keys    hpfg_attn_keys_fwd / _bwd at 33, 64, 65, 255 and 256 keys
  window       hpfg_attn_window_fwd / _bwd: a window of 7 with and without shift, a rectangular map, the last shift, a window of 1; and the
               _drop_ forms with an explicit mask on the first two
each attention case at head dims 32 and 64.  Writes one JSON object {case: {result: digest}} to --out.

To compare two trees, run this same file in each (a fresh process per tree) and compare the two JSON files; tests/golden/dense_bits.json
is the run of the commit before the arithmetic moved into csrc/bf16x3.h (but for the dqkv / dtable digests of the window drop cases, see
the test's docstring), and tests/test_gpu_dense_bits.py compares against it.  Needs a GPU: there is no fallback."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD_DIMS = (32, 64)
TN_MAX_ROWS = 600
TN_OFFSET = [(33, 36, 20, 1), (33, 36, 20, 0)]          # x one float off a 16-byte boundary: the unaligned kernel by the pointer alone
# (family, B, N, M, heads) of tests/helpers.ATTN_M_EDGES / ATTN_N_EDGES
ATTENTION = [("unit", 2, 65, 1, 2), ("sharp", 2, 65, 17, 2), ("unit", 2, 65, 64, 2), ("sharp", 1, 257, 49, 1), ("unit", 1, 513, 49, 1)]
# M below, at and above one key block (ATTN_SCALE_CASES' shape, ATTN_M_EDGES, ATTN_KEYS_EDGES)
ATTENTION_KEYS = [("unit", 2, 65, 33, 2), ("unit", 2, 65, 64, 2), ("sharp", 1, 65, 65, 1), ("sharp", 1, 130, 255, 1), ("sharp", 1, 64, 256, 1)]
# (B, H, W, window, shift, heads): WINDOW_HOT's 14 x 14 map, one unshifted window of 7, and three of WINDOW_EDGES
WINDOW = [(1, 14, 14, 7, 3, 2), (1, 7, 7, 7, 0, 1), (1, 8, 12, 4, 1, 2), (5, 7, 7, 7, 6, 1), (2, 3, 3, 1, 0, 2)]
WINDOW_DROP = WINDOW[:2]
DROP_P = 0.25
BF16X3 = 1          # HPFG_MATH_BF16X3


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _gemm(res):
    import torch
    from hpfg_amd import _lib as L
    from tests import helpers as H
    lib, dev = L.load(), torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(name, M, N, K, oa, ob, ldc, epilogue, splitk):
        c = H.gemm_case(M, N, K)
        a, b = H.gemm_operand(c["A"], oa, 4), H.gemm_operand(c["Bt"], ob, 4)
        ad, bd = a[0].to(dev), b[0].to(dev)
        assert lib.hpfg_gemm_bf16x3_ok(L.ptr(ad), a[1], a[2], L.ptr(bd), b[2], b[1], M, N, K) == 1
        out = torch.zeros(M, ldc, device=dev)
        bias = c["bias"].to(dev) if epilogue else None
        if epilogue:
            out[:, :N] = c["C0"].to(dev)
        args = [L.ptr(ad), a[1], a[2], L.ptr(bd), b[2], b[1], L.ptr(out), ldc, M, N, K, L.ptr(bias), int(epilogue), int(epilogue)]
        r = res[name] = {}
        if splitk:
            S, kper, launched, klast = H.GEMM_SPLIT_TABLE[(M, N, K)]["bf16x3"]
            assert lib.hpfg_gemm_bf16x3_splits(M, N, K) == S
            scratch = torch.zeros(S * M * N, device=dev)
            L.check(lib.hpfg_gemm_bf16x3_splitk(*args, L.ptr(scratch), st), name)
            r["partials"] = _sha(scratch[:launched * M * N])
        else:
            L.check(lib.hpfg_gemm_bf16x3(*args, st), name)
        torch.cuda.synchronize()
        r["C"] = _sha(out[:, :N])

    for M, N, K in H.GEMM_BF16_SHAPES:
        for oa, ob in H.GEMM_ORIENTS:
            run(f"gemm {M}x{N}x{K} A {oa}-fast B {ob}-fast", M, N, K, oa, ob, N + 8, False, False)
    for M, N, K, ldc in H.GEMM_SCALAR_EPILOGUE:
        run(f"gemm {M}x{N}x{K} ldc={ldc} bias relu accumulate", M, N, K, "k", "k", ldc, True, False)
    for M, N, K in _split_shapes():
        for oa, ob in (("k", "k"), ("r", "r")):
            run(f"gemm_splitk {M}x{N}x{K} A {oa}-fast B {ob}-fast", M, N, K, oa, ob, N + 8, True, True)

    for R, N, K, with_db, off in _tn_cases():
        c = H.tn_case(R, N, K)
        S = lib.hpfg_gemm_tn_splits(R, N, K)
        stride = N * K + (N if with_db else 0)
        dw_db, part = torch.zeros(stride, device=dev), torch.zeros(S * stride, device=dev)
        dyd = c["dy"].contiguous().to(dev)
        xbuf = torch.cat([torch.zeros(off), c["x"].reshape(-1)]).to(dev)
        name = f"gemm_tn {R}x{N}x{K} db={with_db}" + (" x offset" if off else "")
        L.check(lib.hpfg_gemm_tn_bf16x3(L.ptr(dyd), xbuf.data_ptr() + 4 * off, L.ptr(dw_db), L.ptr(part), R, N, K, with_db, st), name)
        torch.cuda.synchronize()
        res[name] = {"dw_db": _sha(dw_db), "partials": _sha(part)}


def _split_shapes():
    from tests import helpers as H
    return [s for s, row in H.GEMM_SPLIT_TABLE.items() if row["bf16x3"]]


def _tn_cases():
    from tests import helpers as H
    return [k + (0,) for k in sorted(H.TN_CASES) if k[0] <= TN_MAX_ROWS] + [k + (1,) for k in TN_OFFSET]


def _attention(res):
    import torch
    from hpfg_amd import _lib as L
    from tests import helpers as H
    lib, dev = L.load(), torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    for d in HEAD_DIMS:
        for family, B, N, M, heads in ATTENTION:
            q, kv, do = (t.to(dev) for t in H.attn_inputs(family, B, N, M, heads, d))
            out, dq, dkv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(kv)
            scr = torch.zeros(lib.hpfg_attn_mfma_scratch_floats(B, N, heads, d), device=dev)
            sc = d ** -0.5
            L.check(lib.hpfg_attn_mfma_fwd_hd(L.ptr(q), L.ptr(kv), L.ptr(out), B, N, M, heads, d, sc, st), "attn fwd")
            L.check(lib.hpfg_attn_mfma_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, d, sc, st), "attn bwd")
            torch.cuda.synchronize()
            res[f"attn {family} d{d} B{B} N{N} M{M} h{heads}"] = {"out": _sha(out), "dq": _sha(dq), "dkv": _sha(dkv)}
        for family, B, N, M, heads in ATTENTION_KEYS:
            q, kv, do = (t.to(dev) for t in H.attn_inputs(family, B, N, M, heads, d))
            out, dq, dkv, lse = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(kv), torch.zeros(B * heads * N, device=dev)
            scr = torch.zeros(lib.hpfg_attn_keys_scratch_floats(B, N, M, heads, d, BF16X3), device=dev)
            sc = d ** -0.5
            L.check(lib.hpfg_attn_keys_fwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), B, N, M, heads, d, sc, BF16X3, st), "attn_keys fwd")
            L.check(lib.hpfg_attn_keys_bwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scr), B, N, M, heads, d, sc,
                                           BF16X3, st), "attn_keys bwd")
            torch.cuda.synchronize()
            res[f"attn_keys {family} d{d} B{B} N{N} M{M} h{heads}"] = {"out": _sha(out), "lse": _sha(lse), "dq": _sha(dq), "dkv": _sha(dkv)}
        for case in WINDOW + [c + (DROP_P,) for c in WINDOW_DROP]:
            B, Hh, W, w, s, heads = case[:6]
            p = case[6] if len(case) > 6 else 0.0
            qkv, table, do = (t.to(dev) for t in H.window_inputs("unit", B, Hh, W, w, s, heads, d))
            out, dqkv, dtab = torch.zeros_like(do), torch.zeros_like(qkv), torch.zeros_like(table)
            scr = torch.zeros(lib.hpfg_attn_window_scratch_floats(B, Hh, W, heads, d, w, BF16X3), device=dev)
            sc = d ** -0.5
            geo = (B, Hh, W, heads, d, w, s, sc, BF16X3)
            if p:
                g = torch.Generator().manual_seed(1000 * Hh + 10 * w + s + d)
                n = lib.hpfg_attn_window_drop_elems(B, Hh, W, heads, w)
                mask = (torch.rand(n, generator=g) >= p).to(torch.uint8).to(dev)
                L.check(lib.hpfg_attn_window_drop_fwd(L.ptr(qkv), L.ptr(table), L.ptr(out), *geo, p, 0, None, L.ptr(mask), st), "window drop fwd")
                L.check(lib.hpfg_attn_window_drop_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), *geo, p, 0, None,
                                                      L.ptr(mask), st), "window drop bwd")
            else:
                L.check(lib.hpfg_attn_window_fwd(L.ptr(qkv), L.ptr(table), L.ptr(out), *geo, st), "window fwd")
                L.check(lib.hpfg_attn_window_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtab), L.ptr(scr), *geo, st), "window bwd")
            torch.cuda.synchronize()
            res[f"window{' drop' if p else ''} d{d} B{B} H{Hh} W{W} w{w} s{s} h{heads}"] = {"out": _sha(out), "dqkv": _sha(dqkv), "dtable": _sha(dtab)}


def digests():
    """{case name: {result name: sha256 hex}} of every case, computed on cuda:0"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dense_bits: no GPU; nothing computed")
    res = {}
    _gemm(res)
    _attention(res)
    torch.cuda.synchronize()
    return res


def n_cases():
    from tests import helpers as H
    gemm = len(H.GEMM_BF16_SHAPES) * len(H.GEMM_ORIENTS) + len(H.GEMM_SCALAR_EPILOGUE) + 2 * len(_split_shapes()) + len(_tn_cases())
    return gemm + len(HEAD_DIMS) * (len(ATTENTION) + len(ATTENTION_KEYS) + len(WINDOW) + len(WINDOW_DROP))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="the JSON file to write (keep it out of the tracked tree)")
    a = ap.parse_args()
    r = digests()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"dense_bits: {len(r)} cases -> {a.out}")
