"""Timings of the attention over up to 256 keys (csrc/attn_keys.hip) on one GPU, and the measured errors of its parity test (diagnostics).

  attn    device time of forward and backward (dQ + dK/dV + partial sum) of hpfg_attn_keys_* at the four MiT-B1 stages of one 512 x 512 image
          (N = 16384 / 4096 / 1024 / 256 queries, 256 keys, 1 / 2 / 5 / 8 heads, head dim 64); beside each the <= 64-key kernels
          (hpfg_attn_mfma_*_hd) at the same stage of a 224 x 224 image (49 keys); and 64 keys through both entry points at equal shapes.
          Alternating blocks of launches in one process, device-event time per block, median over the rounds.
  errors  <log>: copies the error lines that tests/test_gpu_attn_keys.py prints (pytest -s) out of a log of that run (needs no GPU).

Every mode appends to --out (default profiles/attn_keys_timing.txt).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 64
STAGES_512 = [(16384, 1), (4096, 2), (1024, 5), (256, 8)]          # (queries, heads) of MiT-B1 at 512 x 512: 256 keys
STAGES_224 = [(3136, 1), (784, 2), (196, 5), (49, 8)]              # ... at 224 x 224: 49 keys
BOTH_64 = [(4096, 2), (256, 8)]                                    # 64 keys (the 256 x 256 stages 2 and 4) through both entry points
ROUNDS, BLOCK = 9, 20


def _emit(out, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(text)


def _case(lib, L, new, N, M, heads):
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    C_, scale = heads * D, D ** -0.5
    g = torch.Generator().manual_seed(N + M)
    q, kv, do = (torch.randn(s, generator=g).to(dev) for s in ((1, N, C_), (1, M, 2 * C_), (1, N, C_)))
    out, dq, dkv, lse = torch.empty_like(q), torch.empty_like(q), torch.empty_like(kv), torch.empty(heads * N, device=dev)
    p = L.ptr
    if new:
        scr = torch.empty(lib.hpfg_attn_keys_scratch_floats(1, N, M, heads, D, 1), device=dev)
        fwd = lambda: L.check(lib.hpfg_attn_keys_fwd(p(q), p(kv), p(out), p(lse), 1, N, M, heads, D, scale, 1, st), "fwd")          # noqa: E731
        bwd = lambda: L.check(lib.hpfg_attn_keys_bwd(p(q), p(kv), p(out), p(lse), p(do), p(dq), p(dkv), p(scr), 1, N, M, heads, D, scale, 1, st), "bwd")          # noqa: E731
    else:
        scr = torch.empty(lib.hpfg_attn_mfma_scratch_floats(1, N, heads, D), device=dev)
        fwd = lambda: L.check(lib.hpfg_attn_mfma_fwd_hd(p(q), p(kv), p(out), 1, N, M, heads, D, scale, st), "fwd")          # noqa: E731
        bwd = lambda: L.check(lib.hpfg_attn_mfma_bwd_hd(p(q), p(kv), p(do), p(dq), p(dkv), p(scr), 1, N, M, heads, D, scale, st), "bwd")          # noqa: E731
    fwd()          # the backward of the new entry points reads out and lse
    return dict(fwd=fwd, bwd=bwd, keep=(q, kv, do, out, dq, dkv, lse, scr))


def _time_pair(pair):
    """{which: ([us of case 0 per round], [us of case 1 per round])}: the two cases alternate block by block"""
    import torch
    res = {}
    for which in ("fwd", "bwd"):
        for c in pair:
            for _ in range(5):
                c[which]()
        torch.cuda.synchronize()
        rows = ([], [])
        for _ in range(ROUNDS):
            for c, r in zip(pair, rows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BLOCK):
                    c[which]()
                e1.record()
                e1.synchronize()
                r.append(e0.elapsed_time(e1) * 1e3 / BLOCK)
        res[which] = rows
    return res


def _fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):.2f} .. {max(v):.2f})"


def attn(out):
    import torch
    from hpfg_amd import _lib as L
    lib = L.load()
    lines = ["", f"== attention entry points, one image, head dim {D}, split-bf16 MFMA kernels; {torch.cuda.get_device_name(0)}",
             f"   device-event time per launch in us, median (min .. max) of {ROUNDS} alternating blocks of {BLOCK} launches; bwd = dQ + dK/dV + partial sum",
             "", "   (a) MiT-B1 stages: 512 x 512 through hpfg_attn_keys_* (256 keys) | 224 x 224 through hpfg_attn_mfma_*_hd (49 keys)",
             f"   {'heads':>5} {'call':>4} | {'N':>6} {'keys: 256, us':>30} | {'N':>5} {'keys: 49, us':>30} | ratio | (N M) ratio"]
    for (n5, h), (n2, _) in zip(STAGES_512, STAGES_224):
        r = _time_pair([_case(lib, L, True, n5, 256, h), _case(lib, L, False, n2, 49, h)])
        for which in ("fwd", "bwd"):
            a, b = r[which]
            lines.append(f"   {h:5d} {which:>4} | {n5:6d} {_fmt(a):>30} | {n2:5d} {_fmt(b):>30} | {statistics.median(a) / statistics.median(b):5.2f} | "
                         f"{n5 * 256 / (n2 * 49):6.1f}")
    lines += ["", "   (b) 64 keys through both entry points (the forward gives the same bits)",
              f"   {'heads':>5} {'call':>4} | {'N':>6} {'hpfg_attn_keys_*, us':>30} | {'hpfg_attn_mfma_*_hd, us':>30} | ratio"]
    for n, h in BOTH_64:
        r = _time_pair([_case(lib, L, True, n, 64, h), _case(lib, L, False, n, 64, h)])
        for which in ("fwd", "bwd"):
            a, b = r[which]
            lines.append(f"   {h:5d} {which:>4} | {n:6d} {_fmt(a):>30} | {_fmt(b):>30} | {statistics.median(a) / statistics.median(b):5.2f}")
    _emit(out, lines)


def errors(out, log):
    import re
    pat = re.compile(r"^[.FEsx]*((?:keys|wide|bitwise forward) .*\d\]?)")          # (pytest -q -s puts its progress marks in front of a test's output)
    rows = [m.group(1) for m in map(pat.match, open(log)) if m]
    if not rows:
        raise SystemExit(f"no error lines of tests/test_gpu_attn_keys.py in {log}")
    _emit(out, ["", "== measured errors of tests/test_gpu_attn_keys.py against the fp64 reference on the CPU (max abs; the bound in brackets), and the",
                "   error of the same formula in plain fp32 PyTorch on the CPU on the same inputs"] + ["   " + r for r in rows])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["attn", "errors"])
    ap.add_argument("log", nargs="?")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_keys_timing.txt"))
    a = ap.parse_args()
    if a.mode == "errors":
        errors(a.out, a.log)
    else:
        attn(a.out)
