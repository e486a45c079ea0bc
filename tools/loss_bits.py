"""Every bit of the fused segmentation loss (csrc/loss.hip) on a fixed list of small cases: the guard that a change to the loss kernels keeps
what it has to keep.

For each case: inputs from numpy.random.default_rng(seed); the C entry points are called through _lib with an L.LossArgs (as
tools/multiclass_timing.py does), so that `sums` can be read and injected.  Recorded per case:
  sums     the row after hpfg_seg_loss_partials, as float32 hex words (hpfg_loss_nsum(C) of them)
  out      SHA-256 of the 8 floats after hpfg_seg_loss_finalize
  dlogits  SHA-256 after hpfg_seg_loss_bwd
Finalize and backward run on an INJECTED sums row, filled from the case's seed (the same in every tree), so the two are pinned on their own,
whatever the partial sums of the tree under test are.

Cases: SHAPES x CLASSES x FORMS, less the forms that need an unlabelled image where the shape has none.  Labels carry the ignore value 255,
one id >= C and one class that never occurs (as tests/test_gpu_loss_wide.py builds them).  Writes one JSON object {case: {result: value}} to
--out.

To compare two trees, run this same file in each (a fresh process per tree); tests/golden/loss_bits.json is the run of the commit before
the two kernel families were folded into one, and tests/test_gpu_loss_bits.py compares against it.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (N, n_lab, H, W): 576 pixels per image, block 0 straddles the label-group boundary at an unaligned offset; boundary at 256, straddled at an
# aligned offset; boundary on a block edge, five blocks; no second group, ragged last block; no first group
SHAPES = [(3, 1, 24, 24), (3, 1, 16, 16), (5, 2, 32, 32), (2, 2, 40, 28), (2, 0, 16, 16)]
CLASSES = (2, 3, 4, 5, 8, 9, 16)
# teacher logits indexed like the batch, with pseudo-labels | teacher probabilities of the unlabelled part only | masked consistency (0/1 mask)
# on teacher logits of the unlabelled part | probability input | no labels1, teacher logits indexed like the batch
FORMS = ("teacher_logits", "teacher_prob_unlab", "masked", "prob_input", "no_labels1")
NEEDS_UNLABELLED = ("teacher_prob_unlab", "masked", "no_labels1")          # (an empty teacher / mask tensor has no device pointer to pass)
COEF = [0.5, 0.5, 0.2, 0.7, 0.3, 0.0, 0.0, 0.0]
GSCALE = 1.5


def cases():
    """[(name, C, shape, form, seed)] in a fixed order; the seed is the position in the full product, skipped combinations included"""
    res, seed = [], 0
    for shape in SHAPES:
        for ncls in CLASSES:
            for form in FORMS:
                seed += 1
                if form in NEEDS_UNLABELLED and shape[1] == shape[0]:
                    continue
                res.append((f"N{shape[0]} lab{shape[1]} {shape[2]}x{shape[3]} C{ncls} {form}", ncls, shape, form, seed))
    return res


def slots(ncls):
    """indices into a sums row: 0 nll0, 1 cnt0, 2 nll1, 3 cnt1, 4 mse, 5 sum mask, then 8 + g * 3 * S + k * S + c for group g, k = 0 / 1 / 2
    = I (sum p t) / Z (sum p p) / Y (sum t t), class stride S = 4 up to four classes and 16 above"""
    S = 4 if ncls <= 4 else 16
    blk = {k: [8 + g * 3 * S + i * S + c for g in range(2) for c in range(ncls)] for i, k in enumerate("IZY")}
    return dict(nsum=8 + 6 * S, integer=[1, 3, 5] + blk["Y"], **blk)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _softmax(x):
    import numpy as np
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype("float32")


def _case(lib, L, dev, ncls, shape, form, seed):
    import numpy as np
    import torch
    N, nl, H, W = shape
    rng = np.random.default_rng(seed)
    logits = (2.0 * rng.standard_normal((N, H, W, ncls))).astype("float32")
    tl = (2.0 * rng.standard_normal((N, H, W, ncls))).astype("float32")
    lab = rng.integers(0, max(ncls - 1, 1), (N, H, W)).astype("uint8")          # class C-1 never occurs
    lab[0, 0, :5] = 255
    lab[0, 3, 2:9] = ncls + 1                                                   # an id >= C that is not the ignore value
    lab[N - 1, H - 1, W - 4:] = 255
    lab[N - 1, 1, 1] = ncls
    mask = (rng.random((N - nl, H, W)) < 0.6).astype("float32")
    S = slots(ncls)
    inj = np.zeros(S["nsum"], "float32")          # a plausible row: positive sums, whole-numbered counts
    inj[[0, 2, 4]] = rng.uniform(1.0, 300.0, 3)
    inj[[1, 3, 5]] = rng.integers(50, 2000, 3)
    for k in "IZY":
        inj[S[k]] = rng.uniform(0.5, 400.0, 2 * ncls)
    inj = inj.astype("float32")

    if form == "prob_input":
        logits = _softmax(logits)
    x = torch.from_numpy(logits).to(dev)
    lab0 = torch.from_numpy(lab[:nl].copy()).to(dev) if nl > 0 else None
    lab1 = torch.from_numpy(lab[nl:].copy()).to(dev) if nl < N and form not in ("teacher_prob_unlab", "masked", "no_labels1") else None
    unlab_only = form in ("teacher_prob_unlab", "masked")
    t_np = tl[nl:] if unlab_only else tl
    if form == "teacher_prob_unlab":
        t_np = _softmax(t_np)
    t = torch.from_numpy(np.ascontiguousarray(t_np)).to(dev)
    cm = torch.from_numpy(mask).to(dev) if form == "masked" else None
    nblk, nsum = lib.hpfg_loss_blocks(N, H, W), lib.hpfg_loss_nsum(ncls)
    assert nsum == S["nsum"]
    partials = torch.full((nblk * nsum,), float("nan"), device=dev)
    sums = torch.full((nsum,), float("nan"), device=dev)
    outv = torch.full((8,), float("nan"), device=dev)
    dl = torch.full_like(x, float("nan"))
    coef = torch.tensor(COEF, device=dev)
    gs = torch.tensor([GSCALE], device=dev)
    a = L.LossArgs()
    a.logits, a.t_logits, a.labels0, a.labels1 = L.ptr(x), L.ptr(t), L.ptr(lab0), L.ptr(lab1)
    a.coef, a.partials, a.sums, a.out, a.dlogits = L.ptr(coef), L.ptr(partials), L.ptr(sums), L.ptr(outv), L.ptr(dl)
    a.N, a.n_lab, a.H, a.W, a.C, a.world = N, nl, H, W, ncls, 1
    a.input_is_prob = 1 if form == "prob_input" else 0
    a.teacher_is_prob = 1 if form == "teacher_prob_unlab" else 0
    a.t_unlab_only = 1 if unlab_only and nl > 0 else 0
    a.cons_mask = L.ptr(cm)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.hpfg_seg_loss_partials(C.byref(a), st), "partials")
    torch.cuda.synchronize()
    words = [f"{int(w):08x}" for w in sums.cpu().numpy().view("uint32")]
    sums.copy_(torch.from_numpy(inj))
    L.check(lib.hpfg_seg_loss_finalize(C.byref(a), st), "finalize")
    L.check(lib.hpfg_seg_loss_bwd(C.byref(a), L.ptr(gs), st), "bwd")
    torch.cuda.synchronize()
    return {"sums": words, "out": _sha(outv), "dlogits": _sha(dl)}


def results():
    """{case name: {"sums": [hex words], "out": sha256, "dlogits": sha256}} of every case, computed on cuda:0"""
    import torch
    from hpfg_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("loss_bits: no GPU; nothing computed")
    lib, dev = L.load(), torch.device("cuda:0")
    return {name: _case(lib, L, dev, ncls, shape, form, seed) for name, ncls, shape, form, seed in cases()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="the JSON file to write (keep it out of the tracked tree)")
    a = ap.parse_args()
    r = results()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(r[k], sort_keys=True)}" for k in sorted(r)) + "\n}\n")      # one line per case
    print(f"loss_bits: {len(r)} cases -> {a.out}")
