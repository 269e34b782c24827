"""Grouped-expert MLP kernels (csrc/moe_grouped.hip) vs the fp32 oracle ``ref.moe_grouped_mlp``, and the
router above 64 rows vs the 64-row op (GPU only)."""

import functools

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.testing.numerics import row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(8, 2, 1280, 1152), (4, 2, 256, 256)]
# 64-row tiles below 128 E copies, 128-row tiles from there on: (4, 2, ..) at 300 rows takes the latter
CASES = ([(*s, M, kind) for s in SHAPES for M in (1, 65, 129, 300) for kind in ("random", "skew")]
         + [(64, 8, 1280, 128, 40, "random")])  # many nearly empty experts


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _experts(E, h, F):
    return ([_bf(2 * F, h, scale=0.05, seed=200 + e) for e in range(E)],
            [_bf(h, F, scale=0.05, seed=300 + e) for e in range(E)])


def _routing(E, k, M, kind):
    g = torch.Generator().manual_seed(17 * M + E)
    if kind == "random":
        topi = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(M)])
    else:  # every token picks expert 0 first (M copies in one expert); "skew-1": the last expert stays unused
        last = E - 1 if kind == "skew" else E - 2
        topi = torch.tensor([[0, 1 + t % last] for t in range(M)])
    topw = torch.rand(M, k, generator=g).add_(0.1).sort(-1, descending=True).values
    return topi.to(torch.int32).to(DEV), (topw / topw.sum(-1, keepdim=True)).float().to(DEV)


@pytest.mark.parametrize("E,k,h,F,M,kind", CASES)
def test_moe_grouped_mlp_vs_oracle(native_lib, E, k, h, F, M, kind):
    ups, downs = _experts(E, h, F)
    up_t, down_t = ops.MoEExpertTable(ups), ops.MoEExpertTable(downs)
    x = _bf(M, h, seed=400 + M)
    topi, topw = _routing(E, k, M, kind)
    assert ops.moe_grouped_ok(x, E, k, h, F)
    y = ops.moe_grouped_mlp(x, up_t, down_t, topi, topw)
    assert y.shape == (M, h) and y.dtype == torch.bfloat16 and torch.isfinite(y.float()).all()
    err = row_err(y, ref.moe_grouped_mlp(x, ups, downs, topi, topw))
    print(f"moe_grouped_mlp E={E} k={k} h={h} F={F} M={M} {kind}: row_err {err:.2e}")
    assert err < 2e-2
    assert torch.equal(native_lib.moe_grouped_mlp(x, up_t.ptrs, down_t.ptrs, topi, topw, F), y)  # and again: same bits


def test_moe_grouped_unrouted_experts_contribute_nothing(native_lib):
    E, k, h, F = SHAPES[0]
    ups, downs = _experts(E, h, F)
    x = _bf(65, h, seed=465)
    topi, topw = _routing(E, k, 65, "skew-1")
    assert E - 1 not in topi.flatten().tolist()
    nan = lambda ws: ws[:-1] + [torch.full_like(ws[-1], float("nan"))]
    y = ops.moe_grouped_mlp(x, ops.MoEExpertTable(ups), ops.MoEExpertTable(downs), topi, topw)
    y2 = ops.moe_grouped_mlp(x, ops.MoEExpertTable(nan(ups)), ops.MoEExpertTable(nan(downs)), topi, topw)
    assert torch.isfinite(y2.float()).all() and torch.equal(y2, y)


def test_moe_route_above_64_rows_is_the_64_row_op(native_lib):
    E, k, h = 8, 2, 1280
    x = _bf(130, h, seed=7)
    x = (x.float() / x.float().pow(2).mean(-1, keepdim=True).sqrt()).to(torch.bfloat16)
    w = _bf(E, h, scale=0.02, seed=8)
    topi, topw = ops.moe_route(x, w, k)
    assert topi.shape == (130, k) and topi.dtype == torch.int32 and topw.dtype == torch.float32
    for a, b in ((0, 64), (64, 128), (128, 130)):
        wi, ww = native_lib.moe_route(x[a:b].contiguous(), w, k)
        assert torch.equal(topi[a:b], wi) and torch.equal(topw[a:b], ww)


@pytest.mark.parametrize("M,h", [(1, 192), (8193, 256)])
def test_moe_grouped_out_of_limit_arguments(native_lib, M, h):
    E, k, F = 4, 2, 256
    x = _bf(M, h, seed=1)
    assert not ops.moe_grouped_ok(x, E, k, h, F)
    up_t = ops.MoEExpertTable([_bf(2 * F, h, scale=0.05, seed=3)] * E)
    down_t = ops.MoEExpertTable([_bf(h, F, scale=0.05, seed=4)] * E)
    topi = torch.arange(k, dtype=torch.int32, device=DEV).repeat(M, 1)
    topw = torch.full((M, k), 1.0 / k, device=DEV)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_grouped_mlp(x, up_t.ptrs, down_t.ptrs, topi, topw, F)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_route_rows(x, _bf(E, h, scale=0.02, seed=2), k)
