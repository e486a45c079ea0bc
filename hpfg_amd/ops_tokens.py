"""Autograd bindings of the token-layout HIP kernels (csrc/tokens.hip) used by the SegFormer branch: LayerNorm, the attention core
softmax(q k^T) v, depthwise-3x3 + GELU, and the shifted-window attention, GELU and patch merging of the Swin blocks (csrc/attn_window.hip; csrc/attn_window_packed.hip for windows of at most 16 tokens), and the window mask, mask-token substitution and masked loss of the Swin-MAE pretraining (csrc/mae.hip).  Device tensors only; the library raises if it is missing (no fallback)."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib as L


def _st(t):
    return torch.cuda.current_stream(t.device).cuda_stream


MATH = {"mode": None}


def gemm_math() -> str:
    """Arithmetic of the token GEMMs and the attention core: HPFG_MATH (default bf16x3), like the U-Net convolutions."""
    import os
    return MATH["mode"] or os.environ.get("HPFG_MATH", "bf16x3")


def _need_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"hpfg_amd.{what} runs on the HIP library only (no CPU fallback)")


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta):
        _need_gpu(x, "layer_norm")
        lib = L.load()
        xc = x.contiguous().float()
        C_ = xc.shape[-1]
        rows = xc.numel() // C_
        y = torch.empty_like(xc)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        L.check(lib.hpfg_ln_fwd(L.ptr(xc), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd), rows, C_, _st(x)), "ln_fwd")
        ctx.save_for_backward(xc, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        C_ = x.shape[-1]
        rows = x.numel() // C_
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        dgb = torch.empty(2, C_, dtype=torch.float32, device=x.device)          # [dgamma ; dbeta]: one reduction launch fills both
        dg, db = dgb[0], dgb[1]
        part = torch.empty(lib.hpfg_ln_bwd_blocks(rows) * 2 * C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_ln_bwd(L.ptr(x), L.ptr(dyc), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(part), rows, C_,
                                _st(x)), "ln_bwd")
        return dx, dg, db


LN_PX_MAX_C, LN_PX_FACTORS = 1536, (1, 2, 4)          # what hpfg_ln_px_fwd / _bwd are built for


class _LayerNormPx(torch.autograd.Function):
    """hpfg_ln_px_fwd / _bwd: LayerNorm with eps as an argument whose rows are written through the pixel shuffle of a patch expanding."""

    @staticmethod
    def forward(ctx, x, gamma, beta, P, eps):
        lib = L.load()
        xc = x.contiguous().float()
        C_ = gamma.numel()
        if P == 1:          # the identity map needs a row count only: any shape [.., C]
            B, H, W = 1, 1, xc.numel() // C_
            y = torch.empty_like(xc)
        else:
            H, W = xc.shape[-3], xc.shape[-2]
            B = xc.numel() // (H * W * P * P * C_)
            y = torch.empty(*xc.shape[:-3], H * P, W * P, C_, dtype=torch.float32, device=x.device)
        mean = torch.empty(B * H * W * P * P, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        L.check(lib.hpfg_ln_px_fwd(L.ptr(xc), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean), L.ptr(rstd), B, H, W, P, C_, eps, _st(x)), "ln_px_fwd")
        ctx.save_for_backward(xc, gamma, mean, rstd)
        ctx.geo = (B, H, W, P, C_)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        B, H, W, P, C_ = ctx.geo
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        dgb = torch.empty(2, C_, dtype=torch.float32, device=x.device)          # [dgamma ; dbeta]: one reduction launch fills both
        part = torch.empty(lib.hpfg_ln_px_bwd_blocks(mean.numel()) * 2 * C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_ln_px_bwd(L.ptr(x), L.ptr(dyc), L.ptr(gamma), L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dgb[0]), L.ptr(dgb[1]), L.ptr(part),
                                   B, H, W, P, C_, _st(x)), "ln_px_bwd")
        return dx, dgb[0], dgb[1], None, None


def _ln_px_args(who, x, gamma, beta, C_, eps):
    if C_ % 4 or not 4 <= C_ <= LN_PX_MAX_C:
        raise ValueError(f"{who}: C = {C_} is not built; the LayerNorm kernels take C % 4 == 0, 4 <= C <= {LN_PX_MAX_C}")
    if gamma.numel() != C_ or beta.numel() != C_:
        raise ValueError(f"{who}: gamma / beta must have C = {C_} elements, got {gamma.numel()} / {beta.numel()}")
    if not eps > 0.0:
        raise ValueError(f"{who}: eps = {eps} must be positive")
    _need_gpu(x, who)


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """nn.LayerNorm(C, eps) over the last dimension.  eps 1e-5 with C <= 1024 is hpfg_ln_fwd as before; any other eps and 1024 < C <= 1536 go
    through hpfg_ln_px_fwd with the identity row map (the same bits where both apply)."""
    if eps == 1e-5 and x.shape[-1] <= 1024:
        return _LayerNorm.apply(x, gamma, beta)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"layer_norm: x {tuple(x.shape)} must be a non-empty [.., C]")
    _ln_px_args("layer_norm", x, gamma, beta, x.shape[-1], eps)
    return _LayerNormPx.apply(x, gamma, beta, 1, float(eps))


def expand_layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, factor: int, eps: float = 1e-5) -> torch.Tensor:
    """rearrange(x, 'B H W (P1 P2 C) -> B (H P1) (W P2) C') followed by nn.LayerNorm(C, eps), in one pass over x (PatchExpanding /
    FinalPatchExpanding of the Swin-UNet after their Linear): x [B,H,W,P*P*C] -> [B,H*P,W*P,C], P = factor in LN_PX_FACTORS."""
    if factor not in LN_PX_FACTORS:
        raise ValueError(f"expand_layer_norm: factor {factor} is not built; the kernels take {LN_PX_FACTORS}")
    if x.dim() != 4 or x.shape[-1] % (factor * factor):
        raise ValueError(f"expand_layer_norm: x {tuple(x.shape)} must be [B, H, W, {factor * factor} C]")
    _ln_px_args("expand_layer_norm", x, gamma, beta, x.shape[-1] // (factor * factor), eps)
    return _LayerNormPx.apply(x, gamma, beta, int(factor), float(eps))


def _drop_args(who, p, seed_dev, mask, n):
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{who}: p = {p} must be in [0, 1)")
    if n >= 1 << 32:
        raise ValueError(f"{who}: {n} mask elements; the dropout hash indexes them with 32 bits")
    if seed_dev is not None and (seed_dev.dtype != torch.int32 or seed_dev.numel() != 1 or not seed_dev.is_cuda):
        raise ValueError(f"{who}: seed_dev must be one int32 word on the device")
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n or not mask.is_cuda or not mask.is_contiguous()):
        raise ValueError(f"{who}: mask must be a contiguous uint8 device tensor of {n} elements, got {mask.dtype} {tuple(mask.shape)}")


class _TokenDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, seed_dev, mask):
        xc = x.contiguous().float()
        y = torch.empty_like(xc)
        L.check(L.load().hpfg_token_dropout(L.ptr(xc), L.ptr(y), xc.numel(), p, seed, L.ptr(seed_dev), L.ptr(mask), _st(x)), "token_dropout")
        ctx.args = (p, seed, seed_dev, mask)          # seed_dev is the forward's own copy of the seed word: a later forward does not change it
        return y

    @staticmethod
    def backward(ctx, dy):
        p, seed, seed_dev, mask = ctx.args
        dyc = dy.contiguous()
        dx = torch.empty_like(dyc)
        L.check(L.load().hpfg_token_dropout(L.ptr(dyc), L.ptr(dx), dyc.numel(), p, seed, L.ptr(seed_dev), L.ptr(mask), _st(dy)), "token_dropout (backward)")
        return dx, None, None, None, None


def token_dropout(x: torch.Tensor, p: float, seed: int = 0, seed_dev=None, mask=None) -> torch.Tensor:
    """nn.Dropout(p) in train mode over a flat fp32 tensor: y = x * keep / (1 - p).  keep is the hash rule of hpfg_dropout_mask(n, p, seed,
    seed_dev) (``dropout_mask`` below) or an explicit uint8 mask of x's element count; the count must be a multiple of 4."""
    if x.numel() == 0 or x.numel() % 4:
        raise ValueError(f"token_dropout: {x.numel()} elements; the kernel moves 4 floats per lane, so the count must be a positive multiple of 4")
    _drop_args("token_dropout", p, seed_dev, mask, x.numel())
    _need_gpu(x, "token_dropout")
    return _TokenDropout.apply(x, float(p), int(seed) & 0xFFFFFFFF, seed_dev, mask)


def dropout_mask(n: int, p: float, seed: int, seed_dev=None, device="cuda") -> torch.Tensor:
    """The keep mask (uint8 [n]) of the hash rule: element i is kept iff hpfg_keep(i, seed + *seed_dev, threshold(p))."""
    _drop_args("dropout_mask", p, seed_dev, None, n)
    out = torch.empty(n, dtype=torch.uint8, device=device)
    L.check(L.load().hpfg_dropout_mask(L.ptr(out), n, float(p), int(seed) & 0xFFFFFFFF, L.ptr(seed_dev), _st(out)), "dropout_mask")
    return out


def seed_word_add(word: torch.Tensor, v: int = 1) -> None:
    """*word = (*word + v) & 0x7fffffff on the stream (hpfg_word_add): the advance of a network's dropout seed word; captured in a hipGraph it
    makes every replay draw new masks."""
    if word.dtype != torch.int32 or word.numel() != 1 or not word.is_cuda:
        raise ValueError("seed_word_add: the seed word must be one int32 on the device")
    L.check(L.load().hpfg_word_add(L.ptr(word), int(v), _st(word)), "word_add")


HEAD_DIMS, MAX_KEYS = (32, 64), 64          # what csrc/attn.hip and the exact-fp32 kernels of csrc/tokens.hip are built for


class _Attention(torch.autograd.Function):
    """softmax(scale q k^T) v on the matrix cores (csrc/attn.hip): split-bf16 MFMA products in the default math mode; HPFG_MATH=f32 keeps
    the exact-fp32 one-thread-per-query kernels of csrc/tokens.hip (dK / dV then through the exact GEMM)."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        _need_gpu(q, "attention")
        lib = L.load()
        qc, kvc = q.contiguous().float(), kv.contiguous().float()
        B, N, C_ = qc.shape
        M = kvc.shape[1]
        out = torch.empty_like(qc)
        ctx.math = gemm_math()
        d = C_ // heads
        if ctx.math == "bf16x3":
            L.check(lib.hpfg_attn_mfma_fwd_hd(L.ptr(qc), L.ptr(kvc), L.ptr(out), B, N, M, heads, d, scale, _st(q)), "attn_mfma_fwd")
        else:
            L.check(lib.hpfg_attn_fwd_hd(L.ptr(qc), L.ptr(kvc), L.ptr(out), B, N, M, heads, d, scale, _st(q)), "attn_fwd")
        ctx.save_for_backward(qc, kvc)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        q, kv = ctx.saved_tensors
        B, N, C_ = q.shape
        M, h = kv.shape[1], ctx.heads
        d = C_ // h
        do = dout.contiguous()
        dq = torch.empty_like(q)
        if ctx.math == "bf16x3":
            dkv = torch.empty_like(kv)
            scratch = torch.empty(lib.hpfg_attn_mfma_scratch_floats(B, N, h, d), dtype=torch.float32, device=q.device)
            L.check(lib.hpfg_attn_mfma_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scratch), B, N, M, h, d, ctx.scale, _st(q)),
                    "attn_mfma_bwd")
            return dq, dkv, None, None
        P = torch.empty(B, h, N, M, dtype=torch.float32, device=q.device)
        dS = torch.empty_like(P)
        L.check(lib.hpfg_attn_bwd_hd(L.ptr(q), L.ptr(kv), L.ptr(do), L.ptr(dq), L.ptr(P), L.ptr(dS), B, N, M, h, d, ctx.scale, _st(q)), "attn_bwd")
        # dV = P^T dO, dK = scale * dS^T Q per (image, head): exact-fp32 MFMA GEMMs (hpfg_gemm_f32) writing straight into the [B,M,2,h,d] layout
        dkv = torch.empty(B, M, 2, h, d, dtype=torch.float32, device=q.device)
        st = _st(q)
        for b in range(B):
            for hh in range(h):
                pbh, sbh = P[b, hh], dS[b, hh]                      # [N, M] each: A(m, k) = X[k, m] -> sam = 1, sak = M
                L.check(lib.hpfg_gemm_f32(L.ptr(pbh), 1, M, do.data_ptr() + 4 * (b * N * C_ + hh * d), C_, 1, L.ptr(dkv[b, 0, 1, hh]), 2 * C_,
                                          M, d, N, None, 0, 0, st), "attn dV")
                L.check(lib.hpfg_gemm_f32(L.ptr(sbh), 1, M, q.data_ptr() + 4 * (b * N * C_ + hh * d), C_, 1, L.ptr(dkv[b, 0, 0, hh]), 2 * C_,
                                          M, d, N, None, 0, 0, st), "attn dK")
        dkv[:, :, 0].mul_(ctx.scale)
        dkv = dkv.view(B, M, 2 * C_)
        return dq, dkv, None, None


def attention(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """softmax(scale * q k^T) v per head.  q [B,N,C], kv [B,M,2C] laid out [.., 2, heads, C/heads] (the kv Linear's output); the head
    dim C/heads is 32 (MiT-B0) or 64 (MiT-B1 and wider), at most 64 keys."""
    C_ = q.shape[-1]
    if C_ % heads or C_ // heads not in HEAD_DIMS:
        raise ValueError(f"attention: head dim {C_}/{heads} is not built; the HIP attention kernels exist for head dims {HEAD_DIMS}")
    if kv.shape[-1] != 2 * C_ or kv.shape[1] > MAX_KEYS:
        raise ValueError(f"attention: kv {tuple(kv.shape)} must be [B, M <= {MAX_KEYS}, {2 * C_}] for q {tuple(q.shape)}")
    return _Attention.apply(q, kv, heads, scale)


MAX_KEYS_LONG = 256          # what csrc/attn_keys.hip walks in blocks of 64 (hpfg_attn_keys_max()): the keys of a MiT stage at 512 x 512
_MATH_CODE = {"f32": 0, "bf16x3": 1}          # HPFG_MATH_F32 / HPFG_MATH_BF16X3 of include/hpfg_hip.h


class _AttentionKeys(torch.autograd.Function):
    """softmax(scale q k^T) v over up to MAX_KEYS_LONG keys (csrc/attn_keys.hip): the forward keeps out and the row log-sum-exp, the
    backward rebuilds P = exp(S - lse) key block by key block.  Both math modes go through the same two entry points."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        _need_gpu(q, "attention_keys")
        lib = L.load()
        qc, kvc = q.contiguous().float(), kv.contiguous().float()
        B, N, C_ = qc.shape
        M, d = kvc.shape[1], C_ // heads
        out = torch.empty_like(qc)
        lse = torch.empty(B, heads, N, dtype=torch.float32, device=q.device)
        ctx.math = _MATH_CODE[gemm_math()]
        L.check(lib.hpfg_attn_keys_fwd(L.ptr(qc), L.ptr(kvc), L.ptr(out), L.ptr(lse), B, N, M, heads, d, scale, ctx.math, _st(q)), "attn_keys_fwd")
        ctx.save_for_backward(qc, kvc, out, lse)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        q, kv, out, lse = ctx.saved_tensors
        B, N, C_ = q.shape
        M, h = kv.shape[1], ctx.heads
        d = C_ // h
        do = dout.contiguous()
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        n_scr = lib.hpfg_attn_keys_scratch_floats(B, N, M, h, d, ctx.math)
        if n_scr < 0:
            L.check(-1, "attn_keys_scratch_floats")
        scratch = torch.empty(n_scr, dtype=torch.float32, device=q.device)
        L.check(lib.hpfg_attn_keys_bwd(L.ptr(q), L.ptr(kv), L.ptr(out), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dkv), L.ptr(scratch), B, N, M, h, d,
                                       ctx.scale, ctx.math, _st(q)), "attn_keys_bwd")
        return dq, dkv, None, None


def attention_keys(q: torch.Tensor, kv: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """``attention`` for 1 .. MAX_KEYS_LONG keys (SegFormer above 256 x 256: a MiT stage has H/32 * W/32 keys).  Same layouts; for at
    most MAX_KEYS keys the forward gives the bits of ``attention`` in the default math mode."""
    C_ = q.shape[-1]
    if C_ % heads or C_ // heads not in HEAD_DIMS:
        raise ValueError(f"attention_keys: head dim {C_}/{heads} is not built; the HIP attention kernels exist for head dims {HEAD_DIMS}")
    if kv.shape[-1] != 2 * C_ or not 1 <= kv.shape[1] <= MAX_KEYS_LONG:
        raise ValueError(f"attention_keys: kv {tuple(kv.shape)} must be [B, 1 <= M <= {MAX_KEYS_LONG}, {2 * C_}] for q {tuple(q.shape)}: "
                         f"the attention kernels take at most {MAX_KEYS_LONG} keys")
    return _AttentionKeys.apply(q, kv, heads, scale)


def attention_for(n_keys: int):
    """The attention op the SegFormer branch uses for ``n_keys`` keys -- a function of the key count alone: ``attention`` up to MAX_KEYS
    (every result at or below 256 x 256 keeps its bits), ``attention_keys`` above."""
    return attention if n_keys <= MAX_KEYS else attention_keys


MAX_WINDOW_KEYS = MAX_KEYS          # window^2 tokens of one window are the keys of csrc/attn_window.hip: one 64-key LDS image


class _WindowAttention(torch.autograd.Function):
    """Shifted-window attention (csrc/attn_window.hip): roll, window partition / reverse, the relative-position bias and the shifted-window
    mask all inside the kernels; gradients to qkv and to the bias table (deterministic partial sums).  Both math modes go through the same
    two entry points."""

    @staticmethod
    def forward(ctx, qkv, bias_table, heads, window, shift, scale):
        lib = L.load()
        qc, tc = qkv.contiguous().float(), bias_table.contiguous().float()
        B, H, W, C3 = qc.shape
        d = C3 // 3 // heads
        out = torch.empty(B, H, W, C3 // 3, dtype=torch.float32, device=qkv.device)
        ctx.math = _MATH_CODE[gemm_math()]
        L.check(lib.hpfg_attn_window_fwd(L.ptr(qc), L.ptr(tc), L.ptr(out), B, H, W, heads, d, window, shift, scale, ctx.math, _st(qkv)), "attn_window_fwd")
        ctx.save_for_backward(qc, tc)
        ctx.geo = (heads, d, window, shift, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        qkv, table = ctx.saved_tensors
        heads, d, window, shift, scale = ctx.geo
        B, H, W, _ = qkv.shape
        do = dout.contiguous()
        dqkv, dtable = torch.empty_like(qkv), torch.empty_like(table)
        n_scr = lib.hpfg_attn_window_scratch_floats(B, H, W, heads, d, window, ctx.math)
        if n_scr < 0:
            L.check(-1, "attn_window_scratch_floats")
        scratch = torch.empty(n_scr, dtype=torch.float32, device=qkv.device)
        L.check(lib.hpfg_attn_window_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtable), L.ptr(scratch), B, H, W, heads, d, window, shift,
                                         scale, ctx.math, _st(qkv)), "attn_window_bwd")
        return dqkv, dtable, None, None, None, None


def _window_args(who, qkv, bias_table, heads, window, shift):
    if qkv.dim() != 4 or qkv.shape[-1] % 3:
        raise ValueError(f"{who}: qkv {tuple(qkv.shape)} must be [B, H, W, 3 C]")
    B, H, W, C3 = qkv.shape
    C_ = C3 // 3
    if window < 1 or window * window > MAX_WINDOW_KEYS:
        raise ValueError(f"{who}: a {window} x {window} window has {window * window} keys; the window kernels take at most "
                         f"{MAX_WINDOW_KEYS} keys (window <= 8)")
    if H != W:
        raise ValueError(f"{who}: the map must be square (H == W), got {H} x {W}")
    if H % window or W % window:
        raise ValueError(f"{who}: map sides {H} x {W} must be divisible by the window {window}")
    if heads < 1 or C_ % heads or C_ // heads not in HEAD_DIMS:
        raise ValueError(f"{who}: head dim {C_}/{heads} is not built; the HIP attention kernels exist for head dims {HEAD_DIMS}")
    if shift not in (0, window // 2):
        raise ValueError(f"{who}: shift {shift} must be 0 or window // 2 = {window // 2}")
    if tuple(bias_table.shape) != ((2 * window - 1) ** 2, heads):
        raise ValueError(f"{who}: bias_table {tuple(bias_table.shape)} must be [(2 window - 1)^2 = {(2 * window - 1) ** 2}, heads = {heads}]")
    _need_gpu(qkv, who)


def window_attention(qkv: torch.Tensor, bias_table: torch.Tensor, heads: int, window: int, shift: int, scale: float) -> torch.Tensor:
    """softmax(scale q k^T + relative-position bias + shifted-window mask) v inside window x window windows of the token map rolled by
    -shift (WindowAttention.forward of a Swin block between its qkv and proj Linear).  qkv [B,H,W,3C] NHWC as the qkv Linear writes it
    (channel = t C + head d + p), bias_table [(2 window - 1)^2, heads]; returns [B,H,W,C] with every token's row where the token is.
    window^2 <= MAX_WINDOW_KEYS, H == W divisible by window, head dim C / heads in HEAD_DIMS, shift 0 or window // 2."""
    _window_args("window_attention", qkv, bias_table, heads, window, shift)
    return _WindowAttention.apply(qkv, bias_table, int(heads), int(window), int(shift), float(scale))


class _WindowAttentionDrop(torch.autograd.Function):
    """_WindowAttention with dropout of the probabilities inside the kernels (hpfg_attn_window_drop_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, qkv, bias_table, heads, window, shift, scale, p, seed, seed_dev, mask):
        lib = L.load()
        qc, tc = qkv.contiguous().float(), bias_table.contiguous().float()
        B, H, W, C3 = qc.shape
        d = C3 // 3 // heads
        out = torch.empty(B, H, W, C3 // 3, dtype=torch.float32, device=qkv.device)
        ctx.math = _MATH_CODE[gemm_math()]
        L.check(lib.hpfg_attn_window_drop_fwd(L.ptr(qc), L.ptr(tc), L.ptr(out), B, H, W, heads, d, window, shift, scale, ctx.math, p, seed, L.ptr(seed_dev),
                                              L.ptr(mask), _st(qkv)), "attn_window_drop_fwd")
        ctx.save_for_backward(qc, tc)
        ctx.geo = (heads, d, window, shift, scale)
        ctx.drop = (p, seed, seed_dev, mask)          # seed_dev is the forward's own copy of the seed word
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        qkv, table = ctx.saved_tensors
        heads, d, window, shift, scale = ctx.geo
        p, seed, seed_dev, mask = ctx.drop
        B, H, W, _ = qkv.shape
        do = dout.contiguous()
        dqkv, dtable = torch.empty_like(qkv), torch.empty_like(table)
        n_scr = lib.hpfg_attn_window_scratch_floats(B, H, W, heads, d, window, ctx.math)
        if n_scr < 0:
            L.check(-1, "attn_window_scratch_floats")
        scratch = torch.empty(n_scr, dtype=torch.float32, device=qkv.device)
        L.check(lib.hpfg_attn_window_drop_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtable), L.ptr(scratch), B, H, W, heads, d, window,
                                              shift, scale, ctx.math, p, seed, L.ptr(seed_dev), L.ptr(mask), _st(qkv)), "attn_window_drop_bwd")
        return dqkv, dtable, None, None, None, None, None, None, None, None


def window_attention_mask_elems(B: int, H: int, W: int, heads: int, window: int) -> int:
    """Elements of the dropout mask of ``window_attention_dropout``: the reference's attn tensor [B nW, heads, window^2, window^2]."""
    return B * (H // window) * (W // window) * heads * window ** 4


def window_attention_dropout(qkv: torch.Tensor, bias_table: torch.Tensor, heads: int, window: int, shift: int, scale: float, p: float, seed: int = 0,
                             seed_dev=None, mask=None) -> torch.Tensor:
    """``window_attention`` with nn.Dropout(p) on the probabilities between the softmax and attn @ v (WindowAttention.attn_drop), inside the
    kernels.  The keep decision of element e of the reference's attn tensor [B nW, heads, L, L] (rolled, window-partitioned order) is byte e
    of the explicit uint8 ``mask`` or the hash rule hpfg_keep(e, seed + *seed_dev, threshold(p)) (``window_attention_drop_mask`` writes it
    out).  p = 0 without a mask gives the bits of ``window_attention``."""
    if qkv.dim() != 4:
        raise ValueError(f"window_attention_dropout: qkv {tuple(qkv.shape)} must be [B, H, W, 3 C]")
    B, H, W, _ = qkv.shape
    if window >= 1 and H % window == 0 and W % window == 0:
        _drop_args("window_attention_dropout", p, seed_dev, mask, window_attention_mask_elems(B, H, W, heads, window))
    elif not 0.0 <= p < 1.0:
        raise ValueError(f"window_attention_dropout: p = {p} must be in [0, 1)")
    if p == 0.0 and mask is None:
        return window_attention(qkv, bias_table, heads, window, shift, scale)
    _window_args("window_attention_dropout", qkv, bias_table, heads, window, shift)
    return _WindowAttentionDrop.apply(qkv, bias_table, int(heads), int(window), int(shift), float(scale), float(p), int(seed) & 0xFFFFFFFF, seed_dev, mask)


MAX_PACKED_WINDOW = 4          # csrc/attn_window_packed.hip: windows of at most 16 tokens, 64 // window^2 of them per tile


class _WindowAttentionPacked(torch.autograd.Function):
    """_WindowAttentionDrop on the packed small-window kernels (hpfg_attn_window_packed_fwd / _bwd); p = 0 without a mask is their
    no-dropout form."""

    @staticmethod
    def forward(ctx, qkv, bias_table, heads, window, shift, scale, p, seed, seed_dev, mask):
        lib = L.load()
        qc, tc = qkv.contiguous().float(), bias_table.contiguous().float()
        B, H, W, C3 = qc.shape
        d = C3 // 3 // heads
        out = torch.empty(B, H, W, C3 // 3, dtype=torch.float32, device=qkv.device)
        ctx.math = _MATH_CODE[gemm_math()]
        L.check(lib.hpfg_attn_window_packed_fwd(L.ptr(qc), L.ptr(tc), L.ptr(out), B, H, W, heads, d, window, shift, scale, ctx.math, p, seed,
                                                L.ptr(seed_dev), L.ptr(mask), _st(qkv)), "attn_window_packed_fwd")
        ctx.save_for_backward(qc, tc)
        ctx.geo = (heads, d, window, shift, scale)
        ctx.drop = (p, seed, seed_dev, mask)          # seed_dev is the forward's own copy of the seed word
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        qkv, table = ctx.saved_tensors
        heads, d, window, shift, scale = ctx.geo
        p, seed, seed_dev, mask = ctx.drop
        B, H, W, _ = qkv.shape
        do = dout.contiguous()
        dqkv, dtable = torch.empty_like(qkv), torch.empty_like(table)
        n_scr = lib.hpfg_attn_window_packed_scratch_floats(B, H, W, heads, d, window, ctx.math)
        if n_scr < 0:
            L.check(-1, "attn_window_packed_scratch_floats")
        scratch = torch.empty(n_scr, dtype=torch.float32, device=qkv.device)
        L.check(lib.hpfg_attn_window_packed_bwd(L.ptr(qkv), L.ptr(table), L.ptr(do), L.ptr(dqkv), L.ptr(dtable), L.ptr(scratch), B, H, W, heads, d, window,
                                                shift, scale, ctx.math, p, seed, L.ptr(seed_dev), L.ptr(mask), _st(qkv)), "attn_window_packed_bwd")
        return dqkv, dtable, None, None, None, None, None, None, None, None


def window_attention_packed(qkv: torch.Tensor, bias_table: torch.Tensor, heads: int, window: int, shift: int, scale: float, p: float = 0.0, seed: int = 0,
                            seed_dev=None, mask=None) -> torch.Tensor:
    """``window_attention`` / ``window_attention_dropout`` for windows of at most MAX_PACKED_WINDOW = 4 tokens a side on the packed kernels
    (csrc/attn_window_packed.hip): 64 // window^2 windows share one 64-row tile instead of one padded tile per window.  Same arguments, same
    result up to the rounding of a differently ordered softmax sum (equal bits in HPFG_MATH_F32), same dropout elements, so
    ``window_attention_drop_mask`` and a mask recorded from the reference serve both.  p = 0 without a mask is the no-dropout form."""
    if not 2 <= window <= MAX_PACKED_WINDOW:
        raise ValueError(f"window_attention_packed: window {window} is outside 2 .. {MAX_PACKED_WINDOW}: the packed kernels take windows of at most "
                         f"{MAX_PACKED_WINDOW} x {MAX_PACKED_WINDOW} = {MAX_PACKED_WINDOW ** 2} tokens (larger windows: window_attention)")
    _window_args("window_attention_packed", qkv, bias_table, heads, window, shift)
    B, H, W, _ = qkv.shape
    _drop_args("window_attention_packed", p, seed_dev, mask, window_attention_mask_elems(B, H, W, heads, window))
    return _WindowAttentionPacked.apply(qkv, bias_table, int(heads), int(window), int(shift), float(scale), float(p), int(seed) & 0xFFFFFFFF, seed_dev, mask)


def window_attention_drop_mask(B: int, H: int, W: int, heads: int, window: int, p: float, seed: int, seed_dev=None, device="cuda") -> torch.Tensor:
    """The hash keep mask of ``window_attention_dropout`` in the explicit layout (uint8 [B nW, heads, L, L]), as hpfg_attn_window_drop_mask writes it."""
    n = window_attention_mask_elems(B, H, W, heads, window)
    _drop_args("window_attention_drop_mask", p, seed_dev, None, n)
    L_ = window * window
    out = torch.empty(B * (H // window) * (W // window), heads, L_, L_, dtype=torch.uint8, device=device)
    L.check(L.load().hpfg_attn_window_drop_mask(L.ptr(out), B, H, W, heads, window, float(p), int(seed) & 0xFFFFFFFF, L.ptr(seed_dev), _st(out)),
            "attn_window_drop_mask")
    return out


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous().float()
        y = torch.empty_like(xc)
        L.check(L.load().hpfg_gelu_fwd(L.ptr(xc), L.ptr(y), xc.numel(), _st(x)), "gelu_fwd")
        ctx.save_for_backward(xc)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        L.check(L.load().hpfg_gelu_bwd(L.ptr(x), L.ptr(dyc), L.ptr(dx), x.numel(), _st(x)), "gelu_bwd")
        return dx


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Exact (erf) GELU, nn.GELU(); the element count must be a multiple of 4 (the kernel moves 4 floats per lane)."""
    if x.numel() == 0 or x.numel() % 4:
        raise ValueError(f"gelu: {x.numel()} elements; the kernel moves 4 floats per lane, so the count must be a positive multiple of 4")
    _need_gpu(x, "gelu")
    return _Gelu.apply(x)


class _PatchMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous().float()
        B, H, W, C_ = xc.shape
        y = torch.empty(B, H // 2, W // 2, 4 * C_, dtype=torch.float32, device=x.device)
        L.check(L.load().hpfg_patch_merge_fwd(L.ptr(xc), L.ptr(y), B, H, W, C_, _st(x)), "patch_merge_fwd")
        ctx.geo = (B, H, W, C_)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C_ = ctx.geo
        dyc = dy.contiguous()
        dx = torch.empty(B, H, W, C_, dtype=torch.float32, device=dy.device)
        L.check(L.load().hpfg_patch_merge_bwd(L.ptr(dyc), L.ptr(dx), B, H, W, C_, _st(dy)), "patch_merge_bwd")
        return dx


def patch_merge(x: torch.Tensor) -> torch.Tensor:
    """The 2 x 2 neighbours of NHWC x [B,H,W,C] gathered into [B,H/2,W/2,4C] in the order (0,0), (1,0), (0,1), (1,1) of Swin's
    PatchMerging; H and W even, C % 4 == 0."""
    if x.dim() != 4 or x.shape[1] % 2 or x.shape[2] % 2 or x.shape[3] % 4:
        raise ValueError(f"patch_merge: x {tuple(x.shape)} must be [B, even H, even W, C % 4 == 0]")
    _need_gpu(x, "patch_merge")
    return _PatchMerge.apply(x)


class _DWGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, "dwconv_gelu")
        lib = L.load()
        xc = x.contiguous().float()
        B, H, W, C_ = xc.shape
        w9 = weight.reshape(C_, 9).t().contiguous()
        y = torch.empty_like(xc)
        L.check(lib.hpfg_dwgelu_fwd(L.ptr(xc), L.ptr(w9), L.ptr(bias), L.ptr(y), B, H, W, C_, _st(x)), "dwgelu_fwd")
        ctx.save_for_backward(xc, w9, bias)
        ctx.wshape = weight.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        x, w9, bias = ctx.saved_tensors
        B, H, W, C_ = x.shape
        dyc = dy.contiguous()
        du, dx = torch.empty_like(x), torch.empty_like(x)
        dwb = torch.empty(10, C_, dtype=torch.float32, device=x.device)         # [dw9 (9 rows) ; dbias]: one reduction launch fills both
        dw9, db = dwb[:9], dwb[9]
        part = torch.empty(lib.hpfg_dwgelu_bwd_blocks(B, H, W) * 10 * C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_dwgelu_bwd(L.ptr(x), L.ptr(w9), L.ptr(bias), L.ptr(dyc), L.ptr(du), L.ptr(dx), L.ptr(dw9), L.ptr(db), L.ptr(part), B, H, W, C_,
                                    _st(x)), "dwgelu_bwd")
        return dx, dw9.t().reshape(ctx.wshape), db


def dwconv_gelu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """gelu(depthwise_conv3x3(x) + bias) on x [B,H,W,C] (NHWC); weight [C,1,3,3] as nn.Conv2d(C, C, 3, 1, 1, groups=C) holds it."""
    return _DWGelu.apply(x, weight, bias)


class _DWConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, k, residual, res_is_x):
        lib = L.load()
        xc = x.contiguous()
        B, H, W, C_ = xc.shape
        wk = weight.reshape(C_, k * k).t().contiguous()
        res = xc if res_is_x else (None if residual is None else residual.contiguous())
        y = torch.empty_like(xc)
        L.check(lib.hpfg_dwconv_fwd(L.ptr(xc), L.ptr(wk), L.ptr(bias), L.ptr(res), L.ptr(y), B, H, W, C_, k, _st(x)), "dwconv_fwd")
        ctx.save_for_backward(xc, wk)
        ctx.k, ctx.wshape = k, weight.shape
        ctx.res, ctx.res_is_x = residual is not None, res_is_x
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        x, wk = ctx.saved_tensors
        B, H, W, C_ = x.shape
        k = ctx.k
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        dwb = torch.empty(k * k + 1, C_, dtype=torch.float32, device=x.device)
        part = torch.empty(lib.hpfg_dwconv_bwd_blocks(B, H, W, k) * (k * k + 1) * C_, dtype=torch.float32, device=x.device)
        # x + dw(x): the residual's gradient is dy itself, added to dx inside the kernel
        L.check(lib.hpfg_dwconv_bwd(L.ptr(x), L.ptr(wk), L.ptr(dyc), L.ptr(dx), 1 if ctx.res_is_x else 0, L.ptr(dwb), L.ptr(dwb[k * k]), L.ptr(part),
                                    B, H, W, C_, k, _st(x)), "dwconv_bwd")
        return dx, dwb[:k * k].t().reshape(ctx.wshape), dwb[k * k], None, dyc if ctx.res else None, None


def dwconv(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, k: int, residual=None) -> torch.Tensor:
    """residual + depthwise_conv_kxk(x) + bias on x [B,H,W,C] (NHWC), k = 3 or 5, padding k // 2; weight [C,1,k,k] as
    nn.Conv2d(C, C, k, padding=k // 2, groups=C) holds it.  ``residual`` is None, x itself (x + dwconv(x): one gradient for both uses) or
    another [B,H,W,C] tensor."""
    _need_gpu(x, "dwconv")
    if k not in (3, 5):
        raise ValueError(f"dwconv: k must be 3 or 5 (got {k})")
    if x.dim() != 4 or x.dtype != torch.float32 or x.shape[3] % 4 != 0 or x.numel() == 0:
        raise ValueError(f"dwconv: x must be a non-empty float32 [B,H,W,C] with C % 4 == 0 (got {tuple(x.shape)}, {x.dtype})")
    C_ = x.shape[3]
    if tuple(weight.shape) != (C_, 1, k, k) or tuple(bias.shape) != (C_,):
        raise ValueError(f"dwconv: weight must be [{C_},1,{k},{k}] and bias [{C_}] (got {tuple(weight.shape)}, {tuple(bias.shape)})")
    if residual is not None and (residual.shape != x.shape or residual.dtype != torch.float32):
        raise ValueError(f"dwconv: residual must be a float32 tensor of x's shape {tuple(x.shape)} (got {tuple(residual.shape)}, {residual.dtype})")
    return _DWConv.apply(x, weight, bias, k, None if residual is x else residual, residual is x)


class _BNTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        lib = L.load()
        C_ = x.shape[-1]
        xc = x.contiguous()
        R = xc.numel() // C_
        part = torch.empty(lib.hpfg_tok_stat_blocks(R) * 2 * C_, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_bn_tok_stats(L.ptr(xc), R, C_, L.ptr(part), L.ptr(sums), _st(x)), "bn_tok_stats")
        mean = sums[0] / R
        var = sums[1] / R          # centred squares: no E[x^2] - mean^2 to cancel
        rstd = torch.rsqrt(var + eps)
        y = torch.empty_like(xc)
        L.check(lib.hpfg_bn_tok_apply(L.ptr(xc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), L.ptr(y), R, C_, _st(x)), "bn_tok_apply")
        ctx.save_for_backward(xc, gamma, mean, rstd)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        lib = L.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        C_ = x.shape[-1]
        R = x.numel() // C_
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        part = torch.empty(lib.hpfg_tok_stat_blocks(R) * 2 * C_, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_bn_tok_bwd(L.ptr(x), L.ptr(dyc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(dx), L.ptr(part), L.ptr(sums), R, C_, _st(x)),
                "bn_tok_bwd")
        return dx, sums[1], sums[0], None


def batch_norm_tokens(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """Train-mode BatchNorm over all tokens of x [..., C] (every leading axis is a batch axis), no activation.  Returns (y, batch mean, biased
    batch variance); the caller updates the running statistics."""
    _need_gpu(x, "batch_norm_tokens")
    if x.dim() < 2 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError(f"batch_norm_tokens: x must be a non-empty float32 [..., C] (got {tuple(x.shape)}, {x.dtype})")
    C_ = x.shape[-1]
    if C_ % 4 != 0 or C_ > 1024:
        raise ValueError(f"batch_norm_tokens: C must be a multiple of 4, at most 1024 (got {C_})")
    if tuple(gamma.shape) != (C_,) or tuple(beta.shape) != (C_,):
        raise ValueError(f"batch_norm_tokens: gamma and beta must be [{C_}] (got {tuple(gamma.shape)}, {tuple(beta.shape)})")
    if not eps > 0.0:
        raise ValueError(f"batch_norm_tokens: eps must be positive (got {eps})")
    return _BNTokens.apply(x, gamma, beta, eps)


class _BNTokensEval(torch.autograd.Function):
    """y = (x - running_mean) * rstd * gamma + beta with fixed statistics.  Backward: dbeta = sum dy and dgamma = sum dy xhat are the sums of
    hpfg_bn_tok_bwd (its dx, the train-mode formula, is discarded); dx = dy * rstd * gamma is the apply kernel on dy with mean 0, beta 0."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, rstd):
        C_ = x.shape[-1]
        xc = x.contiguous()
        y = torch.empty_like(xc)
        L.check(L.load().hpfg_bn_tok_apply(L.ptr(xc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), L.ptr(y), xc.numel() // C_, C_, _st(x)),
                "bn_tok_apply")
        ctx.save_for_backward(xc, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        x, gamma, mean, rstd = ctx.saved_tensors
        C_ = x.shape[-1]
        R = x.numel() // C_
        dyc = dy.contiguous()
        dx, scratch = torch.empty_like(x), torch.empty_like(x)
        part = torch.empty(lib.hpfg_tok_stat_blocks(R) * 2 * C_, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_bn_tok_bwd(L.ptr(x), L.ptr(dyc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(scratch), L.ptr(part), L.ptr(sums), R, C_, _st(x)),
                "bn_tok_bwd")
        zero = torch.zeros_like(mean)
        L.check(lib.hpfg_bn_tok_apply(L.ptr(dyc), L.ptr(zero), L.ptr(rstd), L.ptr(gamma), L.ptr(zero), L.ptr(dx), R, C_, _st(x)), "bn_tok_apply")
        return dx, sums[1], sums[0], None, None


def batch_norm_tokens_eval(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor,
                           eps: float = 1e-5) -> torch.Tensor:
    """Eval-mode BatchNorm over tokens x [..., C]: the affine map of the running statistics, differentiable in x, gamma and beta (the
    running statistics are constants)."""
    _need_gpu(x, "batch_norm_tokens_eval")
    C_ = x.shape[-1]
    if x.dtype != torch.float32 or x.numel() == 0 or C_ % 4 != 0 or C_ > 1024:
        raise ValueError(f"batch_norm_tokens_eval: x must be a non-empty float32 [..., C], C a multiple of 4 up to 1024 (got {tuple(x.shape)}, {x.dtype})")
    if any(tuple(t.shape) != (C_,) for t in (gamma, beta, running_mean, running_var)):
        raise ValueError(f"batch_norm_tokens_eval: gamma, beta and the running statistics must be [{C_}]")
    return _BNTokensEval.apply(x, gamma, beta, running_mean.detach(), torch.rsqrt(running_var.detach() + eps))


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W):
        _need_gpu(x, "resize_bilinear")
        xc = x.contiguous().float()
        B, h, w, C_ = xc.shape
        y = torch.empty(B, H, W, C_, dtype=torch.float32, device=x.device)
        L.check(L.load().hpfg_resize_bilinear_fwd(L.ptr(xc), L.ptr(y), B, h, w, H, W, C_, _st(x)), "resize_fwd")
        ctx.shape = (B, h, w, H, W, C_)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, h, w, H, W, C_ = ctx.shape
        dyc = dy.contiguous()
        dx = torch.empty(B, h, w, C_, dtype=torch.float32, device=dy.device)
        L.check(L.load().hpfg_resize_bilinear_bwd(L.ptr(dyc), L.ptr(dx), B, h, w, H, W, C_, _st(dy)), "resize_bwd")
        return dx, None, None


class _ResizeSum(torch.autograd.Function):
    """base [B,H,W,C] + sum_k resize(x_k [B,h_k,w_k,C]) in one pass (hpfg_resize_sum_fwd); backward: the gradient itself for base, the
    resize backward of it for every x_k."""

    @staticmethod
    def forward(ctx, base, *xs):
        _need_gpu(base, "resize_sum")
        bc = base.contiguous().float()
        B, H, W, C_ = bc.shape
        xc = [x.contiguous().float() for x in xs]
        assert 1 <= len(xc) <= 3 and all(x.shape[0] == B and x.shape[3] == C_ for x in xc)
        y = torch.empty_like(bc)
        ptrs = (C.c_void_p * len(xc))(*[x.data_ptr() for x in xc])
        hs, ws = (C.c_int * len(xc))(*[x.shape[1] for x in xc]), (C.c_int * len(xc))(*[x.shape[2] for x in xc])
        L.check(L.load().hpfg_resize_sum_fwd(L.ptr(bc), ptrs, hs, ws, len(xc), L.ptr(y), B, H, W, C_, _st(base)), "resize_sum_fwd")
        ctx.geo = (B, H, W, C_, [(x.shape[1], x.shape[2]) for x in xc])
        return y

    @staticmethod
    def backward(ctx, dy):
        B, H, W, C_, lows = ctx.geo
        dyc = dy.contiguous()
        outs = [dyc if ctx.needs_input_grad[0] else None]
        for k, (h, w) in enumerate(lows):
            if not ctx.needs_input_grad[1 + k]:
                outs.append(None)
                continue
            dx = torch.empty(B, h, w, C_, dtype=torch.float32, device=dy.device)
            L.check(L.load().hpfg_resize_bilinear_bwd(L.ptr(dyc), L.ptr(dx), B, h, w, H, W, C_, _st(dy)), "resize_bwd")
            outs.append(dx)
        return tuple(outs)


def resize_sum(base: torch.Tensor, *xs: torch.Tensor) -> torch.Tensor:
    """base + sum_k F.interpolate(x_k, size=base's, mode="bilinear", align_corners=False), NHWC, C % 4 == 0, up to 3 addends."""
    return _ResizeSum.apply(base, *xs)


def resize_bilinear(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """F.interpolate(..., size=(H, W), mode="bilinear", align_corners=False) on NHWC x [B,h,w,C] (C % 4 == 0), upsampling."""
    return _Resize.apply(x, H, W)


class _BNReLUDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mask, keep, eps):
        _need_gpu(x, "bn_relu_dropout")
        lib = L.load()
        B, N, C_ = x.shape
        xc = x.contiguous().float()
        R = B * N
        part = torch.empty(lib.hpfg_tok_stat_blocks(R) * 2 * C_, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_tok_col_stats(L.ptr(xc), R, C_, L.ptr(part), L.ptr(sums), _st(x)), "tok_col_stats")
        mean = sums[0] / R
        var = sums[1] / R          # centred squares (hpfg_tok_col_stats): no E[x^2] - mean^2 to cancel
        rstd = torch.rsqrt(var + eps)
        y = torch.empty_like(xc)
        m = None if mask is None else mask.reshape(B, C_).float().contiguous()
        L.check(lib.hpfg_bnrelu_apply(L.ptr(xc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), L.ptr(m), 1.0 / keep, N, L.ptr(y), R, C_, _st(x)),
                "bnrelu_apply")
        ctx.save_for_backward(xc, gamma, beta, mean, rstd, m if m is not None else xc.new_empty(0))
        ctx.keep, ctx.N = keep, N
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dm, _dv):
        lib = L.load()
        x, gamma, beta, mean, rstd, m = ctx.saved_tensors
        B, N, C_ = x.shape
        R = B * N
        dyc = dy.contiguous()
        dx = torch.empty_like(x)
        part = torch.empty(lib.hpfg_tok_stat_blocks(R) * 2 * C_, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, C_, dtype=torch.float32, device=x.device)
        L.check(lib.hpfg_bnrelu_bwd(L.ptr(x), L.ptr(dyc), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(beta), L.ptr(m if m.numel() else None),
                                    1.0 / ctx.keep, N, L.ptr(dx), L.ptr(part), L.ptr(sums), R, C_, _st(x)), "bnrelu_bwd")
        return dx, sums[1].clone(), sums[0].clone(), None, None, None


def bn_relu_dropout(x, gamma, beta, mask=None, keep: float = 0.9, eps: float = 1e-5):
    """Train-mode BatchNorm over all tokens of x [B,N,C] + ReLU + per-(image, channel) dropout mask [B,C] (0/1, scaled by 1/keep).
    Returns (y, batch mean, biased batch variance); the caller updates the running statistics."""
    return _BNReLUDrop.apply(x, gamma, beta, mask, keep, eps)


TALL_ROWS = 8192          # from this many tokens on, the weight gradient of a Linear runs on the row-split HIP kernel


def _gemm(a, sam, sak, b, sbk, sbn, m, n, k, bias=None, math="bf16x3"):
    """out[m,n] = sum_k a(m,k) b(k,n) + bias[n] on the HIP library: split-bf16 MFMA when the operands allow it (unit stride along one
    index, 4-element alignment) and `math` asks for it, exact-fp32 MFMA otherwise (include/hpfg_hip.h: hpfg_gemm_bf16x3 / hpfg_gemm_f32)."""
    lib = L.load()
    out = torch.empty(m, n, dtype=torch.float32, device=a.device)
    if math == "bf16x3" and lib.hpfg_gemm_bf16x3_ok(L.ptr(a), sam, sak, L.ptr(b), sbk, sbn, m, n, k):
        splits = lib.hpfg_gemm_bf16x3_splits(m, n, k)      # few output tiles + long K (the 1568-token layers): split the contraction
        if splits > 1:
            scratch = torch.empty(splits * m * n, dtype=torch.float32, device=a.device)
            L.check(lib.hpfg_gemm_bf16x3_splitk(L.ptr(a), sam, sak, L.ptr(b), sbk, sbn, L.ptr(out), n, m, n, k, L.ptr(bias), 0, 0, L.ptr(scratch), _st(a)),
                    "gemm_bf16x3_splitk")
        else:
            L.check(lib.hpfg_gemm_bf16x3(L.ptr(a), sam, sak, L.ptr(b), sbk, sbn, L.ptr(out), n, m, n, k, L.ptr(bias), 0, 0, _st(a)), "gemm_bf16x3")
    else:
        L.check(lib.hpfg_gemm_f32(L.ptr(a), sam, sak, L.ptr(b), sbk, sbn, L.ptr(out), n, m, n, k, L.ptr(bias), 0, 0, _st(a)), "gemm_f32")
    return out


class _Linear(torch.autograd.Function):
    """y = x W^T + b over tokens x [.., K] -- nn.Linear, the kernel == stride spatial-reduction conv, the patch embeddings after im2col and
    the head's 1x1 convs of reference model/segformer.py -- entirely on the HIP library: forward and dX on hpfg_gemm_bf16x3 (or the exact
    fp32 GEMM), dW on the row-split deterministic kernel when there are many tokens (tall-skinny dY^T X) and on the GEMM otherwise, db as
    a column sum."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_gpu(x, "linear")
        N, K = weight.shape
        xc = x.reshape(-1, K).contiguous().float()
        w = weight.contiguous()
        math = gemm_math()
        y = _gemm(xc, K, 1, w, 1, K, xc.shape[0], N, K, bias, math)
        ctx.save_for_backward(xc, w)
        ctx.has_bias, ctx.math, ctx.xshape = bias is not None, math, x.shape
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        xc, w = ctx.saved_tensors
        N, K = w.shape
        R = xc.shape[0]
        dyc = dy.reshape(-1, N).contiguous()
        dx = _gemm(dyc, N, 1, w, K, 1, R, K, N, None, ctx.math).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        db = None
        if ctx.math == "bf16x3":          # dY^T X on MFMA; the bias gradient (column sums of dY) comes out of the same pass
            wb = torch.empty(N * K + (N if ctx.has_bias else 0), dtype=torch.float32, device=w.device)
            part = torch.empty(lib.hpfg_gemm_tn_splits(R, N, K) * wb.numel(), dtype=torch.float32, device=w.device)
            L.check(lib.hpfg_gemm_tn_bf16x3(L.ptr(dyc), L.ptr(xc), L.ptr(wb), L.ptr(part), R, N, K, 1 if ctx.has_bias else 0, _st(w)), "gemm_tn_bf16x3")
            dw = wb[:N * K].view(N, K)
            if ctx.has_bias:
                db = wb[N * K:]
            return dx, dw, db
        if R >= TALL_ROWS and N % 4 == 0 and K % 4 == 0:
            dw = torch.empty_like(w)
            part = torch.empty(lib.hpfg_linear_wgrad_splits(R, N, K) * N * K, dtype=torch.float32, device=w.device)
            L.check(lib.hpfg_linear_wgrad(L.ptr(dyc), L.ptr(xc), L.ptr(dw), L.ptr(part), R, N, K, _st(w)), "linear_wgrad")
        else:
            dw = _gemm(dyc, 1, N, xc, K, 1, N, K, R, None, ctx.math)                   # dY^T X, exact fp32
        if ctx.has_bias:
            db = torch.empty(N, dtype=torch.float32, device=w.device)
            scratch = torch.empty(lib.hpfg_col_sum_splits(R) * N, dtype=torch.float32, device=w.device)
            L.check(lib.hpfg_col_sum2(L.ptr(dyc), R, N, N, L.ptr(db), L.ptr(scratch), _st(w)), "col_sum2")
        return dx, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """F.linear on the HIP library (no rocBLAS call): see _Linear."""
    return _Linear.apply(x, weight, bias)


class _Im2col(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s):
        _need_gpu(x, "im2col")
        xc = x.contiguous().float()
        B, H, W, C_ = xc.shape
        p = k // 2
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        cols = torch.empty(B, Ho * Wo, k * k * C_, dtype=torch.float32, device=x.device)
        L.check(L.load().hpfg_im2col_nhwc(L.ptr(xc), L.ptr(cols), B, H, W, C_, k, s, _st(x)), "im2col")
        ctx.geo = (B, H, W, C_, k, s)
        return cols

    @staticmethod
    def backward(ctx, dcols):
        B, H, W, C_, k, s = ctx.geo
        dc = dcols.contiguous()
        dx = torch.empty(B, H, W, C_, dtype=torch.float32, device=dc.device)
        L.check(L.load().hpfg_col2im_nhwc(L.ptr(dc), L.ptr(dx), B, H, W, C_, k, s, _st(dc)), "col2im")
        return dx, None, None


def im2col(x: torch.Tensor, k: int, s: int) -> torch.Tensor:
    """Patches of a conv with kernel k, stride s, padding k // 2 over NHWC x [B,H,W,C] -> [B, Ho*Wo, k*k*C], patch order (u, v, c)."""
    return _Im2col.apply(x, k, s)


class _ResidualScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, scale):
        _need_gpu(x, "residual_scale")
        xc, yc = x.contiguous().float(), y.contiguous().float()
        B = xc.shape[0]
        per = xc.numel() // B
        out = torch.empty_like(xc)
        sc = None if scale is None else scale.reshape(B).float().contiguous()
        L.check(L.load().hpfg_residual_scale(L.ptr(xc), L.ptr(yc), L.ptr(sc), L.ptr(out), B, per, _st(x)), "residual_scale")
        ctx.sc, ctx.geo = sc, (B, per)
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.sc is None:
            return dout, dout, None
        B, per = ctx.geo
        d = dout.contiguous()
        dy = torch.empty_like(d)
        L.check(L.load().hpfg_scale_rows(L.ptr(d), L.ptr(ctx.sc), L.ptr(dy), B, per, _st(d)), "scale_rows")
        return dout, dy, None


def residual_scale(x: torch.Tensor, y: torch.Tensor, scale=None) -> torch.Tensor:
    """x + y * scale[b] per sample b (scale None = 1): a residual branch with stochastic depth in one kernel."""
    return _ResidualScale.apply(x, y, scale)


# ---- Swin-MAE pretraining (csrc/mae.hip) ------------------------------------------------------------------------------------------------------
MAE_MAX_GROUPS, MAE_MAX_C, MAE_PATCH, MAE_MAX_CIN = 1024, 1536, 4, 4          # what hpfg_mae_window_mask / _mask_tokens_* / _loss are built for


def mae_keep_count(d: int, mask_ratio: float) -> int:
    """Groups the window masking keeps out of d * d: the reference's own expression in Python floats, truncation included
    (model/swin_mae.py:673; 0.6 at d = 14 gives 78)."""
    return int(d ** 2 * (1 - mask_ratio))


def _mask_args(who, mask, n):
    if mask.dtype != torch.uint8 or mask.numel() != n:
        raise ValueError(f"{who}: mask must be uint8 with {n} elements (one per token), got {mask.dtype} {tuple(mask.shape)}")


def mae_window_mask(noise: torch.Tensor, side: int, r: int, n_keep: int) -> torch.Tensor:
    """window_masking(remove=False, mask_len_sparse=False) of the reference's SwinMAE from its noise: noise [B, d * d] (d = side / r) ->
    uint8 mask [B, side * side] in token order y * side + x, 1 = removed; the n_keep groups of r x r tokens with the smallest (noise, index)
    are kept.  No host round trip (the reference's np.setdiff1d loop), so the call can be captured."""
    if side < 1 or r < 1 or side % r:
        raise ValueError(f"mae_window_mask: the token side {side} must be a positive multiple of the group side r = {r}")
    d = side // r
    if d * d > MAE_MAX_GROUPS:
        raise ValueError(f"mae_window_mask: {d} x {d} groups; the kernel ranks at most {MAE_MAX_GROUPS} per image")
    if noise.dim() != 2 or noise.shape[1] != d * d or noise.shape[0] < 1:
        raise ValueError(f"mae_window_mask: noise {tuple(noise.shape)} must be [B, d * d = {d * d}]")
    if not 0 <= n_keep <= d * d:
        raise ValueError(f"mae_window_mask: n_keep = {n_keep} must be in 0 .. {d * d}")
    _need_gpu(noise, "mae_window_mask")
    nc = noise.contiguous().float()
    mask = torch.empty(nc.shape[0], side * side, dtype=torch.uint8, device=noise.device)
    L.check(L.load().hpfg_mae_window_mask(L.ptr(nc), L.ptr(mask), nc.shape[0], int(side), int(r), int(n_keep), _st(noise)), "mae_window_mask")
    return mask


class _MaeMaskTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, token):
        xc, tc = x.contiguous().float(), token.contiguous().float().reshape(-1)
        C_ = xc.shape[-1]
        rows = xc.numel() // C_
        y = torch.empty_like(xc)
        L.check(L.load().hpfg_mae_mask_tokens_fwd(L.ptr(xc), L.ptr(mask), L.ptr(tc), L.ptr(y), rows, C_, _st(x)), "mae_mask_tokens_fwd")
        ctx.mask, ctx.geo = mask, (rows, C_, token.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        rows, C_, tshape = ctx.geo
        dyc = dy.contiguous()
        dx = torch.empty_like(dyc)
        dtok = torch.empty(C_, dtype=torch.float32, device=dy.device)
        part = torch.empty(lib.hpfg_mae_mask_tokens_bwd_blocks(rows) * C_, dtype=torch.float32, device=dy.device)
        L.check(lib.hpfg_mae_mask_tokens_bwd(L.ptr(dyc), L.ptr(ctx.mask), L.ptr(dx), L.ptr(dtok), L.ptr(part), rows, C_, _st(dy)), "mae_mask_tokens_bwd")
        return dx, None, dtok.view(tshape)


def mae_mask_tokens(x: torch.Tensor, mask: torch.Tensor, token: torch.Tensor) -> torch.Tensor:
    """x [.., C] with every token whose mask byte is non-zero replaced by ``token`` (C values; the reference's per-image
    ``x_masked[i, index_mask[i], :] = self.mask_token``, model/swin_mae.py:706-709).  Gradients: dx = dy on kept tokens, 0 on masked ones;
    dtoken = the sum of dy over the masked tokens (fixed order).  C % 4 == 0, 4 <= C <= MAE_MAX_C; mask uint8, one byte per token."""
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"mae_mask_tokens: x {tuple(x.shape)} must be a non-empty [.., tokens, C]")
    C_ = x.shape[-1]
    if C_ % 4 or not 4 <= C_ <= MAE_MAX_C:
        raise ValueError(f"mae_mask_tokens: C = {C_} is not built; the kernels take C % 4 == 0, 4 <= C <= {MAE_MAX_C}")
    if token.numel() != C_:
        raise ValueError(f"mae_mask_tokens: the mask token must have C = {C_} elements, got {tuple(token.shape)}")
    _mask_args("mae_mask_tokens", mask, x.numel() // C_)
    _need_gpu(x, "mae_mask_tokens")
    if not mask.is_cuda:
        raise ValueError("mae_mask_tokens: mask must be on the device")
    return _MaeMaskTokens.apply(x, mask.contiguous(), token)


class _MaeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, img, mask, scale, norm_pix):
        lib = L.load()
        pc, ic = pred.contiguous().float(), img.contiguous().float()
        B, Cin, H, W = ic.shape
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pc)
        part = torch.empty(lib.hpfg_mae_loss_blocks(B, H, W, MAE_PATCH), dtype=torch.float32, device=pred.device)
        L.check(lib.hpfg_mae_loss(L.ptr(pc), L.ptr(ic), L.ptr(mask), scale, 1 if norm_pix else 0, L.ptr(loss), L.ptr(dpred), L.ptr(part), B, Cin, H, W,
                                  MAE_PATCH, _st(pred)), "mae_loss")
        ctx.dpred = dpred          # the gradient for an upstream gradient of 1, written by the forward launch
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dpred = ctx.dpred
        out = torch.empty_like(dpred)
        L.check(L.load().hpfg_scale_rows(L.ptr(dpred), L.ptr(dloss.contiguous().float().reshape(1)), L.ptr(out), 1, dpred.numel(), _st(dpred)),
                "mae_loss (backward)")
        return out, None, None, None, None


def mae_loss(pred: torch.Tensor, img: torch.Tensor, mask: torch.Tensor, scale: float, norm_pix: bool = False) -> torch.Tensor:
    """scale * sum over masked tokens of sum_j (pred - patchify(img))^2 as a 0-dim device tensor (no host synchronisation), its gradient to
    ``pred`` saved from the same launch.  pred [B, L, 16 Cin] as ``decoder_pred`` writes it (channel order (p, q, c)), img [B, Cin, H, W] read
    in place through the patchify addressing, mask uint8 [B, L] (non-zero = removed).  scale = 1 / (B Cin H W mask_ratio) is the driver's
    ``mean((pred_img - img)^2 mask_img) / mask_ratio`` (2022_12_CVPR_Swin-MAE.py:112), scale = 1 / (16 Cin n_masked) the model's
    ``forward_loss`` (model/swin_mae.py:775-791), whose per-patch target normalisation ``norm_pix`` switches on.  Patch 4, 1 <= Cin <= 4."""
    if img.dim() != 4 or not 1 <= img.shape[1] <= MAE_MAX_CIN or img.shape[2] % MAE_PATCH or img.shape[3] % MAE_PATCH or img.numel() == 0:
        raise ValueError(f"mae_loss: img {tuple(img.shape)} must be [B, 1 <= Cin <= {MAE_MAX_CIN}, H, W] with sides divisible by the patch {MAE_PATCH}")
    B, Cin, H, W = img.shape
    Ltok, D = (H // MAE_PATCH) * (W // MAE_PATCH), MAE_PATCH * MAE_PATCH * Cin
    if tuple(pred.shape) != (B, Ltok, D):
        raise ValueError(f"mae_loss: pred {tuple(pred.shape)} must be [B, L, patch^2 Cin] = [{B}, {Ltok}, {D}] for img {tuple(img.shape)}")
    _mask_args("mae_loss", mask, B * Ltok)
    _need_gpu(pred, "mae_loss")
    if not (mask.is_cuda and img.is_cuda):
        raise ValueError("mae_loss: img and mask must be on the device")
    return _MaeLoss.apply(pred, img, mask.contiguous(), float(scale), bool(norm_pix))
