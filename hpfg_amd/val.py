"""Evaluation of the hot path's models on the device (reference val.py:154-193, 268-287, 376-387).

``test_single_volume`` keeps the reference's signature and arithmetic -- every slice is resized to ``patch_size`` with
``scipy.ndimage.zoom(order=0)``, run through ``net`` in eval mode, arg-maxed, resized back, and scored per foreground class with
medpy's binary Dice ``2 n(A&B) / (n(A) + n(B))`` -- but without the per-slice host round trips: the nearest-neighbour resize
becomes ONE device gather through an index map that scipy itself produces for the (shape, patch) pair (so the mapping is scipy's
by construction), all slices go through the HIP engine in fixed-size batches, arg-max and the class-confusion counts are HIP
kernels, and only C*C integers per volume cross to the host.
HD95 (medpy ``hd95``) is reported as 0.0 unless asked for: ``with_hd95=True`` runs the scipy restatement below on the host (distance
transforms of the whole volume, per class and direction), ``with_hd95="device"`` runs ``hd95_device``: surface extraction and an exact
integer nearest-surface search in HIP (csrc/surface.hip), one sort, and two integers per class back to the host.

``test_synapse`` / ``test_single_volume_synapse`` (val.py:196-265) are the same machinery behind the other resize of the reference: every
Synapse slice goes to ``patch_size`` with ``zoom(order=3)``, a cubic B-spline.  ``resize_cubic`` does that for a whole volume on the device
(hpfg_resize_cubic, csrc/resize.hip) from per-axis tap tables built here on the host in fp64; the resize back stays order 0.

``test_lidc`` / ``test_isic`` (val.py:86-151) score 2-D image test sets: batches ``[B,Cin,H,W]`` at network size, no resize, class 1 only, every
batch one ``[B,H,W]`` array for the metrics.  Dice and Jaccard come from the confusion counts; HD95 and medpy's average surface distance (ASD)
by the same ``with_hd95`` routes -- on the device one surface pass serves both (``surface_metrics_device``): hpfg_surface_sums adds the
distances of a segment exactly in integers, so the mean does not depend on the order the surface points were found in.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .train import argmax_labels

EVAL_BATCH = 8      # slices per engine launch (one engine shape for every volume; the last batch is zero padded)


@lru_cache(maxsize=64)
def _zoom_index(src_hw: Tuple[int, int], dst_hw: Tuple[int, int]) -> np.ndarray:
    """Flat source index of every destination pixel under scipy.ndimage.zoom(order=0) with the reference's factors
    (val.py:274,280: zoom(slice, (dst/src, dst/src), order=0))."""
    from scipy.ndimage import zoom
    h, w = src_hw
    idx = np.arange(1, h * w + 1, dtype=np.float64).reshape(h, w)
    out = zoom(idx, (dst_hw[0] / h, dst_hw[1] / w), order=0)
    assert out.shape == tuple(dst_hw), (out.shape, dst_hw)
    return np.rint(out).astype(np.int64).reshape(-1) - 1      # -1: scipy wrote its constant 0 (coordinate a rounding error past the edge)


def _resize_nearest(t: torch.Tensor, dst_hw: Sequence[int]) -> torch.Tensor:
    """[S,h,w] -> [S,H,W] with scipy's order-0 mapping, one gather on the device."""
    s, h, w = t.shape
    if (h, w) == tuple(dst_hw):
        return t
    idx = torch.from_numpy(_zoom_index((h, w), (int(dst_hw[0]), int(dst_hw[1])))).to(t.device)
    out = t.reshape(s, h * w).index_select(1, idx.clamp(min=0))
    out = torch.where(idx.unsqueeze(0) >= 0, out, torch.zeros((), dtype=t.dtype, device=t.device))
    return out.reshape(s, int(dst_hw[0]), int(dst_hw[1]))


_CUBIC_REACH = 16      # samples on either side of the four B-spline taps that a tap table keeps: |sqrt(3) - 2|^16 < 1e-9


def _cubic_prefilter_matrix(n: int) -> np.ndarray:
    """The cubic spline prefilter of scipy.ndimage (spline_filter1d, order 3, mode 'mirror') on a line of n samples as an n x n matrix,
    fp64: gain (1 - z)(1 - 1/z) with the pole z = sqrt(3) - 2, the closed-form causal start under whole-sample mirror boundaries, the
    causal recursion, the anti-causal start and the anti-causal recursion -- applied to the columns of the identity."""
    z = np.sqrt(3.0) - 2.0
    c = np.eye(n) * ((1.0 - z) * (1.0 - 1.0 / z))
    zp = z ** np.arange(2 * n - 1, dtype=np.float64)
    i = np.arange(1, n - 1)
    c[0] = (c[0] + zp[n - 1] * c[n - 1] + ((zp[i] + zp[2 * n - 2 - i])[:, None] * c[i]).sum(0)) / (1.0 - zp[2 * n - 2])
    for j in range(1, n):
        c[j] += z * c[j - 1]
    c[n - 1] = z / (z * z - 1.0) * (z * c[n - 2] + c[n - 1])
    for j in range(n - 2, -1, -1):
        c[j] = z * (c[j + 1] - c[j])
    return c


def _cubic_axis_matrix(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One axis of scipy.ndimage.zoom(a, n_out / n_in, order=3) with scipy's defaults as a matrix [n_out, n_in] (fp64), the floor of every
    output coordinate, and scipy's own verdict on which outputs it computes at all: its last coordinate o * (n_in - 1) / (n_out - 1) can land a
    rounding error beyond n_in - 1, and it then writes the constant 0 (at 512 -> 224, the Synapse case).  Like ``_zoom_index`` the verdict
    is taken from scipy, not re-derived."""
    from scipy.ndimage import zoom
    x = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1))
    f = np.floor(x)
    t = x - f
    w = np.stack([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], 1)
    period = 2 * (n_in - 1)
    idx = np.abs(f.astype(np.int64)[:, None] - 1 + np.arange(4)[None]) % period          # mirrored tap indices
    idx = np.where(idx > n_in - 1, period - idx, idx)
    valid = zoom(np.ones(n_in), n_out / n_in, order=3) > 0.5
    assert valid.shape == (n_out,), (valid.shape, n_in, n_out)
    m = (w[:, :, None] * _cubic_prefilter_matrix(n_in)[idx]).sum(1) * valid[:, None]
    return m, f.astype(np.int64), valid


@lru_cache(maxsize=64)
def _cubic_axis_table(n_in: int, n_out: int) -> np.ndarray:
    """The tap table of hpfg_resize_cubic for one axis (include/hpfg_hip.h): int32 words, float32 w[n_out][RESIZE_TAPS] then first[n_out].
    Row o of the axis matrix is kept on the RESIZE_TAPS columns from first[o] = floor(x_o) - 1 - 16, moved inside the line at its ends (the
    mirror images are already folded into the columns that exist), i.e. whole for n_in <= RESIZE_TAPS; what is cut off is below 1e-9."""
    m, f, valid = _cubic_axis_matrix(n_in, n_out)
    first = np.clip(f - 1 - _CUBIC_REACH, 0, max(n_in - L.RESIZE_TAPS, 0))
    cols = first[:, None] + np.arange(L.RESIZE_TAPS)[None]
    w = np.where(cols < n_in, np.take_along_axis(m, np.minimum(cols, n_in - 1), 1), 0.0)
    assert float((np.abs(m).sum(1) - np.abs(w).sum(1)).max()) < 1e-9, (n_in, n_out)
    return np.concatenate([w.astype(np.float32).reshape(-1).view(np.int32), np.where(valid, first, -1).astype(np.int32)])


_cubic_dev = {}      # (n_in, n_out, device) -> tap table on the device; (device,) -> scratch buffer (grown on demand, reused by every call)


def _cubic_table_dev(n_in: int, n_out: int, device) -> torch.Tensor:
    key = (n_in, n_out, str(device))
    if key not in _cubic_dev:
        _cubic_dev[key] = torch.from_numpy(_cubic_axis_table(n_in, n_out)).to(device)
    return _cubic_dev[key]


def resize_cubic(t: torch.Tensor, dst_hw: Sequence[int]) -> torch.Tensor:
    """[S,h,w] float32 on the device -> [S,H,W]: scipy.ndimage.zoom(slice, (H/h, W/w), order=3) of every slice (the reference's Synapse
    evaluation resize, val.py:243) by hpfg_resize_cubic on the current stream.  A (h, w) == dst_hw input is returned as is."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        raise ValueError("resize_cubic takes a float32 [S,h,w] tensor on the device (no CPU fallback)")
    s, h, w = t.shape
    H, W = int(dst_hw[0]), int(dst_hw[1])
    if (h, w) == (H, W):
        return t
    lib = L.load()
    need = lib.hpfg_resize_cubic_scratch_bytes(s, h, w, H, W)
    if need < 0:
        raise ValueError(f"resize_cubic: [{s},{h},{w}] -> [{H},{W}]: every axis needs 2 .. 8192 samples and S 1 .. 65535")
    ty, tx = _cubic_table_dev(h, H, t.device), _cubic_table_dev(w, W, t.device)
    scratch = _cubic_dev.get((str(t.device),))
    if scratch is None or scratch.numel() < need:
        scratch = _cubic_dev[(str(t.device),)] = torch.empty(need, dtype=torch.uint8, device=t.device)
    src = t.contiguous()
    out = torch.empty((s, H, W), dtype=torch.float32, device=t.device)
    L.check(lib.hpfg_resize_cubic(L.ptr(src), s, h, w, L.ptr(out), H, W, L.ptr(ty), L.ptr(tx), L.ptr(scratch), scratch.numel(),
                                  torch.cuda.current_stream(t.device).cuda_stream), "resize_cubic")
    return out


def predict_volume(image: torch.Tensor, net, patch_size: Sequence[int] = (256, 256), order: int = 0) -> torch.Tensor:
    """image [S,h,w] (float, any device) -> predicted labels uint8 [S,h,w] on the model's device.  order: the spline order of the resize
    to ``patch_size`` -- 0 (ACDC, val.py:274) or 3 (Synapse, val.py:243); the resize back is order 0 in both."""
    if order not in (0, 3):
        raise ValueError(f"predict_volume: spline order {order} (0 or 3)")
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("hpfg_amd.val runs on the HIP library only (no CPU fallback)")
    vol = image.to(dev, torch.float32)
    s, h, w = vol.shape
    x = resize_cubic(vol, patch_size) if order == 3 else _resize_nearest(vol, patch_size)
    was_training = net.training
    net.eval()
    fwd = net.val if hasattr(net, "val") else net
    preds: List[torch.Tensor] = []
    with torch.no_grad():
        for i in range(0, s, EVAL_BATCH):
            chunk = x[i:i + EVAL_BATCH]
            n = chunk.shape[0]
            if n < EVAL_BATCH:
                chunk = torch.cat([chunk, chunk.new_zeros(EVAL_BATCH - n, *chunk.shape[1:])], 0)
            logits = fwd(chunk.unsqueeze(1).contiguous())
            preds.append(argmax_labels(logits)[:n])       # argmax(softmax(z)) == argmax(z)
    net.train(was_training)
    return _resize_nearest(torch.cat(preds, 0), (h, w)).contiguous()


def confusion_counts(pred: torch.Tensor, gt: torch.Tensor, classes: int) -> np.ndarray:
    """counts[g, p] over all voxels (uint8 label tensors on the device) -> int64 [classes, classes] on the host."""
    assert pred.shape == gt.shape and pred.is_cuda and gt.is_cuda
    p8, g8 = pred.to(torch.uint8).contiguous(), gt.to(torch.uint8).contiguous()
    out = torch.zeros(classes * classes, dtype=torch.int64, device=pred.device)
    L.check(L.load().hpfg_confusion_counts(L.ptr(p8), L.ptr(g8), p8.numel(), classes, L.ptr(out),
                                           torch.cuda.current_stream(pred.device).cuda_stream), "confusion_counts")
    return out.cpu().numpy().reshape(classes, classes)


def dice_from_counts(cm: np.ndarray, cls: int) -> float:
    """The reference's per-class rule (val.py:376-387): 0 if the class is never predicted, else medpy dc."""
    n_pred, n_gt, inter = int(cm[:, cls].sum()), int(cm[cls, :].sum()), int(cm[cls, cls])
    if n_pred == 0:
        return 0.0
    return 2.0 * inter / float(n_pred + n_gt)


def jaccard_from_counts(cm: np.ndarray, cls: int) -> float:
    """medpy jc, intersection over union, from the confusion counts; 0 if the class is never predicted (val.py:109-122)."""
    n_pred, n_gt, inter = int(cm[:, cls].sum()), int(cm[cls, :].sum()), int(cm[cls, cls])
    if n_pred == 0:
        return 0.0
    return inter / float(n_pred + n_gt - inter)


def hd95_host(pred: np.ndarray, gt: np.ndarray) -> float:
    """medpy.metric.binary.hd95 restated with scipy (voxel spacing 1, connectivity 1): 95th percentile of the symmetric surface
    distances.  Host only; raises like medpy when one of the objects is empty."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

    def surf_dist(a, b):
        a, b = np.atleast_1d(a.astype(bool)), np.atleast_1d(b.astype(bool))
        if not a.any():
            raise RuntimeError("The first supplied array does not contain any binary object.")
        if not b.any():
            raise RuntimeError("The second supplied array does not contain any binary object.")
        fp = generate_binary_structure(a.ndim, 1)
        ab = a ^ binary_erosion(a, structure=fp, iterations=1)
        bb = b ^ binary_erosion(b, structure=fp, iterations=1)
        dt = distance_transform_edt(~bb)
        return dt[ab]

    return float(np.percentile(np.hstack((surf_dist(pred, gt), surf_dist(gt, pred))), 95))


def hd95_order_stats(n: int) -> Tuple[int, int, float]:
    """(k, k1, t): np.percentile(v, 95) of n values with numpy's default linear interpolation is lerp(sorted v[k], sorted v[k1], t) --
    numpy's own virtual index n q + (alpha + q (1 - alpha - beta)) - 1 with q = 95 / 100, alpha = beta = 1, its floor and its fraction."""
    q = 95 / 100
    vi = n * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0
    if vi >= n - 1:
        return n - 1, n - 1, 0.0
    if vi < 0.0:
        return 0, 0, 0.0
    k = int(np.floor(vi))
    return k, k + 1, float(vi - k)


def hd95_finish(lo2: int, hi2: int, t: float) -> float:
    """The 95th percentile from its two order statistics, given as the integer squared distances the device found: fp64 square roots, then
    numpy's interpolation rule (a + (b - a) t, and b - (b - a)(1 - t) for t >= 0.5).  Pure host arithmetic."""
    a, b = float(np.sqrt(np.float64(lo2))), float(np.sqrt(np.float64(hi2)))
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


_HD95_EMPTY_GT = "The second supplied array does not contain any binary object."      # medpy's text (hd95_host raises the same)


def asd_host(pred: np.ndarray, gt: np.ndarray) -> float:
    """medpy.metric.binary.asd(result=pred, reference=gt) restated with scipy (voxel spacing 1, connectivity 1): the mean distance from the
    surface voxels of ``pred`` to the surface of ``gt`` -- one direction only.  Host only; raises like medpy when one of the objects is empty."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    a, b = np.atleast_1d(np.asarray(pred).astype(bool)), np.atleast_1d(np.asarray(gt).astype(bool))
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError(_HD95_EMPTY_GT)
    fp = generate_binary_structure(a.ndim, 1)
    ab = a ^ binary_erosion(a, structure=fp, iterations=1)
    bb = b ^ binary_erosion(b, structure=fp, iterations=1)
    return float(distance_transform_edt(~bb)[ab].mean())


def asd_limbs(d2) -> Tuple[np.ndarray, np.ndarray]:
    """The two integers hpfg_surface_sums adds per point (include/hpfg_hip.h), for integer squared distances ``d2`` below 2^28: with
    x = sqrt(d2) in fp64, hi = rint(x * 2^19) and lo = (x - hi * 2^-19) * 2^52, so that x == hi * 2^-19 + lo * 2^-52 exactly.  Host
    restatement of the device arithmetic (int64 arrays)."""
    x = np.sqrt(np.asarray(d2, dtype=np.float64))
    hi = np.rint(x * 2.0 ** 19)
    lo = (x - hi * 2.0 ** -19) * 2.0 ** 52
    return hi.astype(np.int64), lo.astype(np.int64)


def asd_finish(hi: int, lo: int, n: int) -> float:
    """The mean of n distances from their exact sum hi * 2^-19 + lo * 2^-52 (the two integer words of hpfg_surface_sums): rational arithmetic,
    rounded once to fp64.  Pure host arithmetic."""
    from fractions import Fraction
    return float(Fraction((int(hi) << 33) + int(lo), int(n) << 52))


def _surface_pass(who: str, pred: torch.Tensor, gt: torch.Tensor, classes: int, ndim, with_asd: bool):
    """The body of ``hd95_device`` and ``surface_metrics_device``: (hd95, asd), float64 [classes - 1] each (asd is None unless asked for)."""
    if not (pred.is_cuda and gt.is_cuda and pred.dtype == torch.uint8 and gt.dtype == torch.uint8 and pred.shape == gt.shape):
        raise ValueError(f"{who} takes two uint8 label tensors of one shape on the device (no CPU fallback)")
    ndim = pred.dim() if ndim is None else int(ndim)
    if pred.dim() not in (2, 3) or ndim not in (2, 3) or (pred.dim() == 2 and ndim != 2):
        raise ValueError(f"{who}: a {pred.dim()}-D tensor with ndim={ndim} ([S,h,w] with ndim 3, [h,w] or [1,h,w] with ndim 2)")
    s, h, w = (1,) + tuple(pred.shape) if pred.dim() == 2 else tuple(pred.shape)
    lib = L.load()
    p8, g8 = pred.contiguous(), gt.contiguous()
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    counts_dev = torch.empty(L.SURFACE_SEGS, dtype=torch.int32, device=pred.device)
    L.check(lib.hpfg_surface_counts(L.ptr(p8), L.ptr(g8), s, h, w, classes, ndim, L.ptr(counts_dev), stream), "surface_counts")
    keep = counts_dev.cpu().numpy().astype(np.uint32)
    out = np.zeros(classes - 1, dtype=np.float64)
    asd = np.zeros(classes - 1, dtype=np.float64) if with_asd else None
    for c in range(1, classes):
        n_pred, n_gt = int(keep[2 * c - 2]), int(keep[2 * c - 1])          # a mask is empty exactly when its surface is
        if n_pred == 0:
            keep[2 * c - 2:2 * c] = 0
        elif n_gt == 0:
            raise RuntimeError(_HD95_EMPTY_GT)
    total = int(keep.sum(dtype=np.int64))
    if total == 0:
        return out, asd
    need = lib.hpfg_surface_workspace_bytes(classes, total)
    if need < 0:
        raise ValueError(f"{who}: {total} surface points (below 2^31)")
    ws = torch.empty(need, dtype=torch.uint8, device=pred.device)
    L.check(lib.hpfg_surface_distances(L.ptr(p8), L.ptr(g8), s, h, w, classes, ndim, keep.ctypes.data_as(C.c_void_p), L.ptr(ws), need, stream),
            "surface_distances")
    if with_asd:          # from the unsorted keys, which stay in the workspace: the sort below makes a copy
        sums = torch.empty(2 * L.SURFACE_SEGS, dtype=torch.int64, device=pred.device)
        L.check(lib.hpfg_surface_sums(L.ptr(ws), need, classes, keep.ctypes.data_as(C.c_void_p), L.ptr(sums), stream), "surface_sums")
    keys = torch.sort(ws[256:256 + 4 * total].view(torch.int32)).values          # by (class, d^2): every class' two segments are adjacent
    live, where, frac = [], [], []
    base = 0
    for c in range(1, classes):
        n = int(keep[2 * c - 2]) + int(keep[2 * c - 1])
        if n:
            k, k1, t = hd95_order_stats(n)
            live.append(c)
            where += [base + k, base + k1]
            frac.append(t)
        base += n
    got = (keys.index_select(0, torch.tensor(where, dtype=torch.int64).to(pred.device)).cpu().numpy().astype(np.int64) & 0x0FFFFFFF).reshape(-1, 2)
    for c, (lo2, hi2), t in zip(live, got, frac):
        out[c - 1] = hd95_finish(int(lo2), int(hi2), t)
    if with_asd:
        words = sums.cpu().numpy().reshape(L.SURFACE_SEGS, 2)
        for c in live:          # segment (c - 1) * 2: pred -> gt (medpy asd(result, reference))
            asd[c - 1] = asd_finish(int(words[2 * c - 2, 0]) & (2 ** 64 - 1), int(words[2 * c - 2, 1]), int(keep[2 * c - 2]))
    return out, asd


def hd95_device(pred: torch.Tensor, gt: torch.Tensor, classes: int, ndim: int = None) -> np.ndarray:
    """HD95 of every foreground class (float64 [classes - 1]) of two uint8 label tensors on the device, [S,h,w] (ndim 3) or [h,w] (ndim 2; a
    [1,h,w] tensor with ndim=2 is that slice): medpy hd95(pred == c, gt == c) with unit spacing, by hpfg_surface_counts / hpfg_surface_distances
    (include/hpfg_hip.h) on the current stream.  The reference's rule per class (val.py:376-387): 0.0 if the class is never predicted; predicted
    but absent from ``gt`` raises medpy's RuntimeError, decided from the surface counts before anything is searched.  Two transfers to the host:
    the counts, and two order statistics per class.  No CPU fallback."""
    return _surface_pass("hd95_device", pred, gt, classes, ndim, False)[0]


def surface_metrics_device(pred: torch.Tensor, gt: torch.Tensor, classes: int, ndim: int = None) -> Tuple[np.ndarray, np.ndarray]:
    """(hd95, asd) of every foreground class, float64 [classes - 1] each: ``hd95_device`` (the same pass, the same bits) and medpy
    asd(pred == c, gt == c) -- the mean distance from the surface of the prediction to the surface of ``gt`` -- from the same surface
    distances, summed exactly by hpfg_surface_sums and divided on the host (``asd_finish``).  The rule per class and the RuntimeError are
    those of ``hd95_device``: a class that is never predicted gives 0.0 for both.  One more transfer to the host: the 64 sum words."""
    return _surface_pass("surface_metrics_device", pred, gt, classes, ndim, True)


def _hd95_route(with_hd95):
    """False: none (0.0), True: ``hd95_host``, "device": ``hd95_device``."""
    if isinstance(with_hd95, (bool, np.bool_)):
        return bool(with_hd95)
    if isinstance(with_hd95, str) and with_hd95 == "device":
        return with_hd95
    raise ValueError(f"with_hd95={with_hd95!r}: False (0.0), True (host) or \"device\"")


def _volume_metrics(pred, lab, classes, with_hd95, ndim):
    """[(dice, hd95)] for classes 1..classes-1 of a predicted and a true label tensor on the device (val.py:376-387 per class)."""
    route = _hd95_route(with_hd95)
    lab8 = lab.to(torch.uint8)
    cm = confusion_counts(pred, lab8, classes)
    hd = np.zeros(classes - 1)
    if route == "device":
        hd = hd95_device(pred, lab8, classes, ndim)
    elif route:
        pred_h, lab_h = pred.cpu().numpy(), lab.cpu().numpy()
        hd = [hd95_host(pred_h == c, lab_h == c) if cm[:, c].sum() > 0 else 0.0 for c in range(1, classes)]
    return [(dice_from_counts(cm, c), float(hd[c - 1])) for c in range(1, classes)]


def test_single_volume(image, label, net, classes, patch_size=(256, 256), with_hd95=False, _pred_out: list = None):
    """Reference signature (val.py:268).  image, label: [1,S,h,w].  Returns [(dice, hd95)] for classes 1..classes-1; hd95 is 0.0 with
    ``with_hd95=False``, ``hd95_host`` with True and ``hd95_device`` with "device".
    _pred_out: optional list that receives the predicted label volume (uint8 [S,h,w], device) -- test_acdc's TensorBoard image hook."""
    _hd95_route(with_hd95)
    dev = next(net.parameters()).device
    img = image.squeeze(0)
    lab = label.squeeze(0).to(dev)
    pred = predict_volume(img, net, patch_size)
    if _pred_out is not None:
        _pred_out.append(pred)
    return _volume_metrics(pred, lab, classes, with_hd95, 3)


test_single_volume.__test__ = False      # reference name, not a pytest case


def test_single_volume_synapse(image, label, net, classes, patch_size=(256, 256), test_save_path=None, case=None, z_spacing=1, _pred_out: list = None,
                               with_hd95=False):
    """Reference signature (val.py:235).  image, label: [1,S,h,w], or [1,h,w] for the reference's 2-D branch (one slice, forwarded at its
    own size).  Every slice whose size differs from ``patch_size`` is resized with the cubic spline (``resize_cubic`` = zoom(order=3),
    val.py:243), forwarded, arg-maxed and resized back with order 0 (val.py:251).  Returns [(dice, hd95)] for classes 1..classes-1 with
    hd95 chosen by ``with_hd95`` as in ``test_single_volume`` (the 2-D branch measures in the plane: ndim 2); ``test_save_path`` / ``case`` /
    ``z_spacing`` are unused in the reference as well (medpy is called without voxelspacing)."""
    _hd95_route(with_hd95)
    dev = next(net.parameters()).device
    img, lab = image.squeeze(0), label.squeeze(0).to(dev)
    if img.dim() == 2:
        pred = predict_volume(img.unsqueeze(0), net, tuple(img.shape))[0]
    else:
        pred = predict_volume(img, net, patch_size, order=3)
    if _pred_out is not None:
        _pred_out.append(pred if pred.dim() == 3 else pred.unsqueeze(0))
    return _volume_metrics(pred, lab, classes, with_hd95, pred.dim())


test_single_volume_synapse.__test__ = False


def _test_volumes(single_volume, test_loader, args, cur_itrs, name):
    """The body ``test_acdc`` and ``test_synapse`` share (val.py:154-193, 196-232): the mean over the volumes of ``test_loader`` (bs=1 volumes
    ``(image [1,S,h,w], label [1,S,h,w])``) of ``single_volume(image, label, keep)``, and the image hooks of the first volume."""
    metric_list = 0.0
    n = 0
    writer = getattr(args, "writer", None)
    to_img = getattr(getattr(test_loader, "dataset", None), "label_to_img", None)
    for image, label in test_loader:
        hook = n == 0 and writer is not None and hasattr(writer, "add_image") and to_img is not None
        keep = [] if hook else None
        metric_list = metric_list + np.array(single_volume(image, label, keep))
        if hook:
            first = image[0, 0].to(keep[0].device, torch.float32)
            shown = _resize_nearest(first.unsqueeze(0), args.test_crop_size)          # [1,H,W], order 0 in both reference loops (val.py:178,215)
            writer.add_image("{}/Image".format(name), shown.cpu(), cur_itrs)
            writer.add_image("{}/label_pred".format(name), to_img(keep[0][0].cpu().numpy()), cur_itrs, dataformats="HWC")
            writer.add_image("{}/label_true".format(name), to_img(label[0, 0].cpu().numpy()), cur_itrs, dataformats="HWC")
        n += 1
    metric_list = metric_list / max(n, 1)
    logger = getattr(args, "logger", None)
    if logger is not None:
        logger.info("class dice:{}".format(metric_list[:, 0]))
    return float(np.mean(metric_list, axis=0)[0]), float(np.mean(metric_list, axis=0)[1])


def test_acdc(model, test_loader, args, cur_itrs=0, name="test", with_hd95=False):
    """Reference signature (val.py:154): mean foreground Dice and mean HD95 over the volumes of ``test_loader`` (bs=1 volumes
    ``(image [1,S,h,w], label [1,S,h,w])``).  With ``args.writer`` (anything with TensorBoard's ``add_image``) the first volume's first slice
    is logged the way main.py:309-325 does: ``<name>/Image`` (the slice resized to ``test_crop_size``, [1,H,W]), ``<name>/label_pred`` and
    ``<name>/label_true`` (the dataset's ``label_to_img`` palette images, HWC) -- the prediction is slice 0 of the volume prediction above
    (resize -> eval forward -> arg-max -> resize back: the arithmetic of the reference's separate forward of that slice)."""
    return _test_volumes(lambda image, label, keep: test_single_volume(image, label, model, classes=args.num_classes, patch_size=args.test_crop_size,
                                                                       with_hd95=with_hd95, _pred_out=keep), test_loader, args, cur_itrs, name)


test_acdc.__test__ = False


def test_synapse(model, test_loader, args, cur_itrs=0, name="test", with_hd95=False):
    """Reference signature (val.py:196): ``test_acdc`` with ``test_single_volume_synapse`` per volume -- the slices reach the network through
    the cubic-spline resize.  The image hooks are those of ``test_acdc`` (the shown slice is resized with order 0 there too, val.py:215); the
    logged prediction is slice 0 of the scored volume prediction."""
    return _test_volumes(lambda image, label, keep: test_single_volume_synapse(image, label, model, classes=args.num_classes,
                                                                               patch_size=args.test_crop_size, _pred_out=keep, with_hd95=with_hd95),
                         test_loader, args, cur_itrs, name)


test_synapse.__test__ = False


def predict_images(images: torch.Tensor, net) -> torch.Tensor:
    """images [B,Cin,H,W] (float, any device) -> predicted labels uint8 [B,H,W] on the model's device: the eval-mode forward and arg-max of
    val.py:94,135 at the images' own size, in engine batches of ``EVAL_BATCH`` (the last one zero padded), as ``predict_volume`` runs its slices."""
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("hpfg_amd.val runs on the HIP library only (no CPU fallback)")
    if images.dim() != 4:
        raise ValueError(f"predict_images: a {images.dim()}-D tensor ([B,Cin,H,W])")
    x = images.to(dev, torch.float32)
    b = x.shape[0]
    was_training = net.training
    net.eval()
    fwd = net.val if hasattr(net, "val") else net
    preds: List[torch.Tensor] = []
    with torch.no_grad():
        for i in range(0, b, EVAL_BATCH):
            chunk = x[i:i + EVAL_BATCH]
            n = chunk.shape[0]
            if n < EVAL_BATCH:
                chunk = torch.cat([chunk, chunk.new_zeros(EVAL_BATCH - n, *chunk.shape[1:])], 0)
            preds.append(argmax_labels(fwd(chunk.contiguous()))[:n])       # argmax(softmax(z)) == argmax(z)
    net.train(was_training)
    return torch.cat(preds, 0).contiguous()


def _batch_metrics(pred: torch.Tensor, lab: torch.Tensor, with_hd95) -> Tuple[float, float, float, float]:
    """(dice, hd95, jac, asd) of class 1 of one image batch scored as a whole, the reference's ``cal`` (val.py:109-122) on (pred == 1) against
    (label == 1) as one [B,H,W] array: nothing predicted -> zeros; Dice and Jaccard from the device confusion counts; the two surface metrics
    by the ``with_hd95`` route (0.0 / host / device), where a prediction against labels without the class raises medpy's RuntimeError."""
    route = _hd95_route(with_hd95)
    p1, g1 = (pred == 1).to(torch.uint8), (lab == 1).to(torch.uint8)
    cm = confusion_counts(p1, g1, 2)
    if cm[:, 1].sum() == 0:
        return 0.0, 0.0, 0.0, 0.0
    hd, asd = 0.0, 0.0
    if route == "device":
        hd, asd = (float(v[0]) for v in surface_metrics_device(p1, g1, 2, 3))
    elif route:
        ph, gh = p1.cpu().numpy() == 1, g1.cpu().numpy() == 1
        hd, asd = hd95_host(ph, gh), asd_host(ph, gh)
    return dice_from_counts(cm, 1), hd, jaccard_from_counts(cm, 1), asd


def _side_by_side(img: np.ndarray) -> np.ndarray:
    """[B,H,W,3] palette images of a batch -> one [H,B*W,3] image (a ``label_to_img`` that already returns one image passes through)."""
    return np.concatenate(list(img), axis=1) if img.ndim == 4 else img


def _test_images(model, test_loader, args, cur_itrs, name, with_hd95) -> np.ndarray:
    """The body ``test_lidc`` and ``test_isic`` share (val.py:86-106, 125-151): [dice, hd95, jac, asd] of class 1, every batch of
    ``test_loader`` (``(image [B,Cin,H,W], label [B,H,W])``) scored as a whole and weighted by its size, over ``len(test_loader.dataset)``."""
    _hd95_route(with_hd95)
    dev = next(model.parameters()).device
    total = np.zeros(4, dtype=np.float64)
    writer = getattr(args, "writer", None)
    to_img = getattr(getattr(test_loader, "dataset", None), "label_to_img", None)
    for i, (img, label_true) in enumerate(test_loader):
        pred = predict_images(img, model)
        lab = label_true.to(dev)
        total += np.array(_batch_metrics(pred, lab, with_hd95), dtype=np.float64) * img.shape[0]
        if i == 0 and writer is not None and hasattr(writer, "add_image") and to_img is not None:
            writer.add_image("{}/label_pred".format(name), _side_by_side(to_img(pred.cpu().numpy())), cur_itrs, dataformats="HWC")
            writer.add_image("{}/label_true".format(name), _side_by_side(to_img(label_true.cpu().numpy())), cur_itrs, dataformats="HWC")
    return total / len(test_loader.dataset)


def test_lidc(model, test_loader, args, cur_itrs=0, name="test", with_hd95=False):
    """Reference signature (val.py:86) plus ``with_hd95``: (dice, hd95) of class 1 over a loader of image batches, each batch one [B,H,W]
    array for the metrics (surfaces connect across the batch axis; a batch of one is a one-slice volume), whatever ``num_classes`` is.
    With ``args.writer`` the first batch's ``<name>/label_pred`` and ``<name>/label_true`` palette images are logged; the reference's
    ``make_grid`` picture of the input images (``<name>/Image``) is not."""
    m = _test_images(model, test_loader, args, cur_itrs, name, with_hd95)
    return float(m[0]), float(m[1])


test_lidc.__test__ = False


def test_isic(model, test_loader, args, cur_itrs=0, name="test", with_hd95=False):
    """Reference signature (val.py:125) plus ``with_hd95``: ``test_lidc`` with medpy's Jaccard index and average surface distance,
    (dice, hd95, jac, asd); ``with_hd95`` chooses the route of both surface metrics."""
    m = _test_images(model, test_loader, args, cur_itrs, name, with_hd95)
    return float(m[0]), float(m[1]), float(m[2]), float(m[3])


test_isic.__test__ = False
