"""SHA-256 of every result of the three attention ops on a fixed list of small cases: the guard that a change to the attention kernels
(csrc/attn_core.h and the three files built on it) keeps every bit.

For each case: inputs from numpy.random.default_rng(seed), forward + backward through ops_tokens.attention / attention_keys /
window_attention in both math modes, and the digest of the raw bytes of out, dq, dkv (window: out, dqkv, dtable).  The cases are the smallest
ones where each phase of the kernels can go wrong (ATTENTION, ATTENTION_KEYS, WINDOW below).  Writes one JSON object {case: {result: digest}} to --out.

To compare two trees, run this same file in each (a fresh process per tree) and compare the two JSON files; tests/golden/attn_bits.json is
the run of the commit before the phases were shared, and tests/test_gpu_attn_bits.py compares against it.  Needs a GPU: there is no fallback.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEAD_DIMS = (32, 64)
MATHS = ("bf16x3", "f32")
# (B, N, M, heads): one key and one partial query tile; a ragged key tile and the second trip of a wave's query loop; all 64 keys and more
# than Q_PER_BLOCK queries (two dK / dV workgroups and the partial sum)
ATTENTION = [(2, 10, 1, 2), (1, 130, 49, 2), (1, 600, 64, 1)]
# one key in the second block; ragged queries; four blocks with the last ragged and two query blocks; four full blocks
ATTENTION_KEYS = [(1, 10, 65, 1), (2, 130, 81, 2), (1, 600, 200, 1), (1, 33, 256, 2)]
# (B, H, window, shift, heads, head dim): 49 keys with padding and mask; 16 keys; all 64 keys; one unshifted window
WINDOW = [(2, 14, 7, 3, 2, 32), (1, 8, 4, 2, 3, 32), (1, 16, 8, 4, 1, 64), (1, 7, 7, 0, 1, 64)]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _rand(rng, *shape):
    import torch
    return torch.from_numpy(rng.standard_normal(shape, dtype="float32"))


def _token_case(fn, B, N, M, heads, d, seed, dev):
    import numpy as np
    rng = np.random.default_rng(seed)
    C_ = heads * d
    q, kv, do = _rand(rng, B, N, C_), _rand(rng, B, M, 2 * C_), _rand(rng, B, N, C_)
    qd, kd = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    out = fn(qd, kd, heads, d ** -0.5)
    out.backward(do.to(dev))
    return {"out": _sha(out), "dq": _sha(qd.grad), "dkv": _sha(kd.grad)}


def _window_case(B, H, w, s, heads, d, seed, dev):
    import numpy as np
    from hpfg_amd.ops_tokens import window_attention
    rng = np.random.default_rng(seed)
    C_ = heads * d
    qkv, table, do = _rand(rng, B, H, H, 3 * C_), _rand(rng, (2 * w - 1) ** 2, heads), _rand(rng, B, H, H, C_)      # a non-zero bias table
    qd, td = qkv.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
    out = window_attention(qd, td, heads, w, s, d ** -0.5)
    out.backward(do.to(dev))
    return {"out": _sha(out), "dqkv": _sha(qd.grad), "dtable": _sha(td.grad)}


def digests():
    """{case name: {result name: sha256 hex}} of every case in both math modes, computed on cuda:0"""
    import torch
    from hpfg_amd import ops_tokens
    if not torch.cuda.is_available():
        raise SystemExit("attn_bits: no GPU; nothing computed")
    dev = torch.device("cuda:0")
    res, seed = {}, 0
    try:
        for math in MATHS:
            ops_tokens.MATH["mode"] = math
            for name, fn, shapes in (("attention", ops_tokens.attention, ATTENTION), ("attention_keys", ops_tokens.attention_keys, ATTENTION_KEYS)):
                for d in HEAD_DIMS:
                    for B, N, M, heads in shapes:
                        seed += 1
                        res[f"{name} {math} d{d} B{B} N{N} M{M} h{heads}"] = _token_case(fn, B, N, M, heads, d, seed, dev)
            for B, H, w, s, heads, d in WINDOW:
                seed += 1
                res[f"window_attention {math} B{B} H{H} w{w} s{s} h{heads} d{d}"] = _window_case(B, H, w, s, heads, d, seed, dev)
    finally:
        ops_tokens.MATH["mode"] = None
    torch.cuda.synchronize()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="the JSON file to write (keep it out of the tracked tree)")
    a = ap.parse_args()
    r = digests()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"attn_bits: {len(r)} cases -> {a.out}")
