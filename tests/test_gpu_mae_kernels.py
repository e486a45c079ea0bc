"""GPU: the three Swin-MAE kernels of csrc/mae.hip, each against a float64 / integer law written here.

* window mask: exact equality with torch.argsort-based masking on the CPU (the reference's law, model/swin_mae.py:649-710, written per group),
  on noise without equal values inside an image (asserted: the tie rule only matters otherwise), plus one case with deliberate ties that pins
  the (noise, index) order against a Python sort;
* mask tokens: forward and dx bit-equal to the select law, dmask_token against float64 within the fp32 summation bound
  n_masked * 2^-24 * sum |dy[masked, c]| per channel, two launches bit-equal;
* loss: against float64.  norm_pix off: |loss - ref| <= (n + 4) 2^-24 sum |terms| (n summed terms: n - 1 additions, three roundings per term,
  the scale's rounding and the final product), dpred within 2^-22 |value| element-wise and exactly 0 on kept tokens.  norm_pix on: the same law
  is evaluated with torch float32 ops on the same inputs and its worst error against float64 is measured -- element-wise for dpred, per
  token for the loss (the sum of the tokens' |error|, scaled: the worst the composition's token errors can add up to) -- and the kernel is
  allowed 8 x that (it may order the normalisation differently), the loss in addition to the summation bound above, which does not depend on
  the normalisation.  The measured values are printed (DESIGN.md records them).
"""
import functools

import pytest
import torch

from hpfg_amd.ops_tokens import mae_loss, mae_mask_tokens, mae_window_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U24 = 2.0 ** -24


# ---- window mask ---------------------------------------------------------------------------------------------------------------------------
def _mask_from_keep(keep_groups, S, r):
    """uint8 [S * S] from the kept group indices of one image: token (y, x) belongs to group (y // r) * d + x // r."""
    d = S // r
    kept = torch.zeros(d * d, dtype=torch.bool)
    kept[keep_groups] = True
    ys, xs = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    return (~kept[(ys // r) * d + xs // r]).reshape(-1).to(torch.uint8)


@pytest.mark.parametrize("S,r,n_keep", [(4, 4, 0), (4, 4, 1), (8, 4, 2), (56, 4, 98), (56, 4, 49), (56, 4, 78), (128, 4, 512)])
def test_window_mask_equals_argsort_masking(S, r, n_keep):
    B, d = 3, S // r
    noise = torch.rand(B, d * d, generator=torch.Generator().manual_seed(100 + S + n_keep))
    assert all(row.unique().numel() == row.numel() for row in noise), "the noise must have no two equal values inside an image"
    keep = torch.argsort(noise, dim=1)[:, :n_keep]
    want = torch.stack([_mask_from_keep(keep[b], S, r) for b in range(B)])
    got = mae_window_mask(noise.to(DEV), S, r, n_keep)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, S * S)
    assert torch.equal(got.cpu(), want)
    assert got.sum(1).tolist() == [S * S - n_keep * r * r] * B


@pytest.mark.parametrize("S,r,n_keep", [(8, 2, 5), (16, 4, 9), (24, 3, 40)])
def test_window_mask_breaks_ties_by_index(S, r, n_keep):
    """Noise drawn from four values only: most comparisons are ties; the kept groups are the first n_keep of a Python sort by (noise, index)."""
    B, d = 3, S // r
    noise = torch.randint(0, 4, (B, d * d), generator=torch.Generator().manual_seed(7 + S)).float() / 4
    want = []
    for b in range(B):
        order = sorted(range(d * d), key=lambda g: (float(noise[b, g]), g))
        want.append(_mask_from_keep(torch.tensor(order[:n_keep], dtype=torch.long), S, r))
    got = mae_window_mask(noise.to(DEV), S, r, n_keep)
    assert torch.equal(got.cpu(), torch.stack(want))


# ---- mask tokens ---------------------------------------------------------------------------------------------------------------------------
def _token_mask(kind, B, L, seed):
    if kind == "none":
        return torch.zeros(B, L, dtype=torch.uint8)
    if kind == "all":
        return torch.ones(B, L, dtype=torch.uint8)
    m = torch.zeros(B * L, dtype=torch.uint8)
    m[torch.randperm(B * L, generator=torch.Generator().manual_seed(seed))[:B * L // 2]] = 1
    return m.reshape(B, L)


@functools.lru_cache(maxsize=None)
def _token_data(C_, L_):
    B = 2 if L_ == 16 else 1
    g = torch.Generator().manual_seed(C_ + L_)
    return torch.randn(B, L_, C_, generator=g), torch.randn(1, 1, C_, generator=g), torch.randn(B, L_, C_, generator=g)


@pytest.mark.parametrize("kind", ["none", "all", "half"])
@pytest.mark.parametrize("L_", [16, 3136])
@pytest.mark.parametrize("C_", [32, 96, 1536])
def test_mask_tokens_forward_and_backward(C_, L_, kind):
    x, token, dy = _token_data(C_, L_)
    mask = _token_mask(kind, x.shape[0], L_, 5)
    sel = mask.bool().unsqueeze(-1)
    outs = []
    for _ in range(2):
        xd, td = x.to(DEV).requires_grad_(True), token.to(DEV).requires_grad_(True)
        y = mae_mask_tokens(xd, mask.to(DEV), td)
        y.backward(dy.to(DEV))
        outs.append((y.detach().cpu(), xd.grad.cpu(), td.grad.cpu()))
    y, dx, dtok = outs[0]
    assert torch.equal(y, torch.where(sel, token.expand_as(x), x))
    assert torch.equal(dx, torch.where(sel, torch.zeros_like(dy), dy))
    masked = dy.double() * sel
    want, bound = masked.sum((0, 1)), int(mask.sum()) * U24 * masked.abs().sum((0, 1))
    err = (dtok.reshape(-1).double() - want).abs()
    print(f"mask_tokens C {C_} L {L_} {kind}: worst dmask_token error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert tuple(dtok.shape) == (1, 1, C_) and bool((err <= bound).all())
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "two launches must give identical bits"


# ---- loss ------------------------------------------------------------------------------------------------------------------------------------
def _patchify(img, p=4):
    B, Cin, H, W = img.shape
    return img.reshape(B, Cin, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, (H // p) * (W // p), p * p * Cin)


def _normalise(t):
    return (t - t.mean(dim=-1, keepdim=True)) / (t.var(dim=-1, keepdim=True) + 1.e-6) ** .5


@functools.lru_cache(maxsize=None)
def _loss_data(Cin, side):
    """Inputs and, per norm_pix flag, the float64 target and the torch-float32 target of the same law -- computed once, shared, never changed."""
    B = 3 if side == 16 else 1
    g = torch.Generator().manual_seed(10 * Cin + side)
    img = torch.randn(B, Cin, side, side, generator=g)
    pred = torch.randn(B, (side // 4) ** 2, 16 * Cin, generator=g)
    t64, t32 = _patchify(img.double()), _patchify(img)
    return img, pred, {False: (t64, t32), True: (_normalise(t64), _normalise(t32))}


@pytest.mark.parametrize("norm_pix", [False, True])
@pytest.mark.parametrize("kind", ["none", "all", "half"])
@pytest.mark.parametrize("side", [16, 224])
@pytest.mark.parametrize("Cin", [1, 3])
def test_loss_and_gradient_against_float64(Cin, side, kind, norm_pix):
    img, pred, targets = _loss_data(Cin, side)
    t64, t32 = targets[norm_pix]
    B, L_, D = pred.shape
    mask = _token_mask(kind, B, L_, 9)
    n_masked = int(mask.sum())
    # the two laws of the reference: the driver's scale with norm_pix off, forward_loss's with it on
    scale = 1.0 / (D * max(n_masked, 1)) if norm_pix else 1.0 / (img.numel() * 0.5)
    m = mask.double().unsqueeze(-1)
    terms = scale * (pred.double() - t64) ** 2 * m
    want_loss, want_d = float(terms.sum()), 2.0 * scale * (pred.double() - t64) * m
    outs = []
    for _ in range(2):
        pd = pred.to(DEV).requires_grad_(True)
        loss = mae_loss(pd, img.to(DEV), mask.to(DEV), scale, norm_pix)
        assert loss.dim() == 0 and loss.is_cuda
        loss.backward()
        outs.append((loss.detach().cpu(), pd.grad.cpu()))
    loss, dpred = outs[0]
    assert torch.isfinite(loss) and torch.isfinite(dpred).all()
    assert torch.equal(dpred * (1 - mask).unsqueeze(-1), torch.zeros_like(dpred)), "kept tokens get a gradient of exactly 0"
    n = n_masked * D
    sum_bound = (n + 4) * U24 * float(terms.abs().sum()) if n else 0.0
    err_loss, err_d = abs(float(loss) - want_loss), (dpred.double() - want_d).abs()
    if not norm_pix:
        print(f"loss Cin {Cin} {side}x{side} {kind}: |loss error| {err_loss:.3e} (<= {sum_bound:.3e}), worst dpred error / |value| "
              f"{float((err_d / want_d.abs().clamp_min(1e-300)).max()) / 2.0 ** -22:.3f} x 2^-22")
        assert err_loss <= sum_bound
        assert bool((err_d <= 2.0 ** -22 * want_d.abs()).all())
    else:
        s32 = torch.tensor(scale, dtype=torch.float32)
        tok32 = (s32 * (pred - t32) ** 2 * mask.float().unsqueeze(-1)).sum(-1)          # the composition's token losses, fp32 throughout
        comp_loss = float((tok32.double() - terms.sum(-1)).abs().sum())
        comp_d = float(((2.0 * s32 * (pred - t32) * mask.float().unsqueeze(-1)).double() - want_d).abs().max())
        print(f"loss norm_pix Cin {Cin} {side}x{side} {kind}: torch-fp32 composition error: loss {comp_loss:.3e}, dpred {comp_d:.3e}; kernel: loss "
              f"{err_loss:.3e} (<= {8 * comp_loss + sum_bound:.3e}), dpred {float(err_d.max()):.3e} (<= {8 * comp_d:.3e})")
        assert err_loss <= 8 * comp_loss + sum_bound
        assert float(err_d.max()) <= 8 * comp_d
    if kind == "none":
        assert float(loss) == 0.0 and not dpred.any()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two launches must give identical bits"
