"""Error metrics for the kernel-vs-oracle tests.

``row_err`` is the one the kernel tests gate on: the worst row's max abs error relative to
that row's max magnitude.  Tiled kernels fail tile by tile, and a wrong 16x16 or 32-row tile
moves a tensor-wide Frobenius ratio by well under 1 % on realistic shapes, so the norm ratio
(``rel_frob``) is only used for reductions over rows (weight / bias gradients)."""

from __future__ import annotations

import torch


def rel_frob(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.float(), b.float()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def row_err(got: torch.Tensor, want: torch.Tensor, floor: float = 0.0) -> float:
    """``floor`` > 0 scales rows by at least ``floor`` x the median row magnitude: for outputs
    with rows whose exact value cancels to ~0 (causal dQ of the first query: P = 1 and
    dP - rowsum(dO*O) = 0), where any rounding residue is an infinite relative error."""
    g = got.float().reshape(-1, got.shape[-1])
    w = want.float().reshape(-1, want.shape[-1])
    scale = w.abs().amax(1)
    if floor > 0:
        scale = scale.clamp_min(floor * scale.median().item())
    return ((g - w).abs().amax(1) / scale.clamp_min(1e-6)).max().item()


def int4_grid(N: int, K: int, seed: int = 0, emin: int = -9, emax: int = -3):
    """A weight that group-128 int4 (``quantizers.quantize_int4_g128``) holds exactly: ``q * 2^e``
    with ``q`` in [-7, 7], an exponent ``e`` drawn per (row, group of 128) from ``[emin, emax]`` and
    one ``|q| = 7`` in every group, so the quantizer's scale is exactly ``2^e``.  Returns
    ``(w fp32 [N, K], e int64 [N, K/128])``; ``w`` is exact in bf16 too."""
    g = torch.Generator().manual_seed(seed)
    G = K // 128
    q = torch.randint(-7, 8, (N, G, 128), generator=g)
    pos = torch.randint(0, 128, (N, G, 1), generator=g)
    sign = torch.randint(0, 2, (N, G, 1), generator=g) * 2 - 1
    q.scatter_(2, pos, 7 * sign)
    e = torch.randint(emin, emax + 1, (N, G), generator=g)
    return (q.float() * torch.exp2(e.float()).unsqueeze(2)).reshape(N, K), e


def snap_int4_grid(w: torch.Tensor) -> torch.Tensor:
    """``w [N, K]`` (K % 128 == 0) moved onto the grid of :func:`int4_grid`: per (row, group) the
    power-of-two step ``2^e`` with ``7 * 2^e >= max|w|``, values rounded to ``q * 2^e`` with ``q`` in
    [-7, 7], the group's largest element set to ``+-7 * 2^e``.  Same dtype and device as ``w``."""
    N, K = w.shape
    wg = w.detach().float().reshape(N, K // 128, 128)
    amax = wg.abs().amax(2, keepdim=True).clamp_min(2.0 ** -20)
    step = torch.exp2(torch.ceil(torch.log2(amax / 7.0)))
    q = torch.clamp(torch.round(wg / step), -7, 7)
    pos = wg.abs().argmax(2, keepdim=True)
    top = torch.where(wg.gather(2, pos) < 0, -7.0, 7.0)
    q.scatter_(2, pos, top)
    return (q * step).reshape(N, K).to(w.dtype)
