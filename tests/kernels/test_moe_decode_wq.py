"""Routed-expert decode kernels over fp8 / int4 experts (csrc/moe_decode_wq.hip) vs the fp32 oracle
``ref.moe_decode_mlp`` on the dequantised experts: the quantisation error is not in the comparison."""

import functools
import types

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.testing.numerics import int4_grid, row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
KINDS = ["fp8", "int4"]
SHAPES = [(8, 2, 1280, 1152),  # two K chunks each: the last one 256 deep (gate/up), 128 deep (down)
          (4, 2, 256, 256)]    # a single chunk (tiny-moe)
MS = [1, 5, 16, 17, 40]        # one tile, a tile boundary, a paired pass with a partial second tile


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _experts(E, h, F, kind):
    ups = [_bf(2 * F, h, scale=0.05, seed=200 + e) for e in range(E)]
    downs = [_bf(h, F, scale=0.05, seed=300 + e) for e in range(E)]
    up, down = ops.MoEQuantExperts(ups, kind), ops.MoEQuantExperts(downs, kind)
    return up, down, up.dequantized(), down.dequantized()


def _routing(E, k, M, route):
    g = torch.Generator().manual_seed(17 * M + E)
    if route == "random":
        topi = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(M)])
    else:  # skew: every token picks expert 0 first (M copies: at 40, one paired pass + a partial tile)
        topi = torch.tensor([[0, 1 + t % (E - 1)] for t in range(M)])
    topw = torch.rand(M, k, generator=g).add_(0.1).sort(-1, descending=True).values
    return topi.to(torch.int32).to(DEV), (topw / topw.sum(-1, keepdim=True)).float().to(DEV)


def _inputs(E, k, h, M, route):
    nw = (1.0 + 0.1 * torch.randn(h, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))).to(torch.bfloat16)
    return (_bf(M, h, seed=400 + M), _bf(M, h, seed=500 + M), nw) + _routing(E, k, M, route)


def _run(lib, up, down, x, res, nw, topi, topw):
    act = lib.moe_decode_up_swiglu_wq(x, up.qweight, up.scale, topi)
    xn, res_out = lib.moe_decode_down_add_rmsnorm_wq(act, down.qweight, down.scale, topi, topw, res, nw, EPS)
    return act, xn, res_out


def _check(got, want, what):
    errs = [row_err(g, w) for g, w in zip(got, want)]
    print(f"{what}: act {errs[0]:.2e} xn {errs[1]:.2e} res {errs[2]:.2e}")
    assert all(torch.isfinite(g.float()).all() for g in got)
    assert errs[0] < 2e-2 and errs[1] < 2e-2 and errs[2] < 1.5e-2


@pytest.mark.parametrize("route", ["random", "skew"])
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("E,k,h,F", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_moe_decode_wq_vs_oracle(native_lib, kind, E, k, h, F, M, route):
    up, down, ups, downs = _experts(E, h, F, kind)
    x, res, nw, topi, topw = _inputs(E, k, h, M, route)
    want = (ref.moe_decode_up_swiglu(x, ups, topi),) + ref.moe_decode_mlp(x, ups, downs, topi, topw, res, nw, EPS)
    got = _run(native_lib, up, down, x, res, nw, topi, topw)
    assert [tuple(t.shape) for t in got] == [(M * k, F), (M, h), (M, h)]
    _check(got, want, f"moe_decode_wq {kind} E={E} k={k} h={h} F={F} M={M} {route}")
    # the op wrappers take the same path
    act2 = ops.moe_decode_up_swiglu(x, up, topi)
    got2 = (act2,) + tuple(ops.moe_decode_down_add_rmsnorm(act2, down, topi, topw, res, nw, EPS))
    assert all(torch.equal(a, b) for a, b in zip(got2, got))


def test_moe_decode_int4_lossless_grid(native_lib):
    """Experts that int4 holds exactly: the int4 kernel and the bf16 routed kernel stream the same values."""
    E, k, h, F = SHAPES[0]
    ups = [int4_grid(2 * F, h, seed=e)[0].to(DEV).to(torch.bfloat16) for e in range(E)]
    downs = [int4_grid(h, F, seed=50 + e)[0].to(DEV).to(torch.bfloat16) for e in range(E)]
    up, down = ops.MoEQuantExperts(ups, "int4"), ops.MoEQuantExperts(downs, "int4")
    assert all(torch.equal(d, w.float()) for d, w in zip(up.dequantized(), ups))
    x, res, nw, topi, topw = _inputs(E, k, h, 17, "random")
    up_t, down_t = ops.MoEExpertTable(ups), ops.MoEExpertTable(downs)
    act = native_lib.moe_decode_up_swiglu(x, up_t.ptrs, topi, E, F)
    want = (act,) + tuple(native_lib.moe_decode_down_add_rmsnorm(act, down_t.ptrs, topi, topw, res, nw, EPS, E))
    _check(_run(native_lib, up, down, x, res, nw, topi, topw), want, "int4 grid vs bf16 routed kernel")


@pytest.mark.parametrize("kind", KINDS)
def test_moe_decode_wq_unrouted_experts_contribute_nothing(native_lib, kind):
    """6 of 8 experts unrouted: their scales NaN (fp8: payload 0x7F = NaN too) change no output bit."""
    E, k, h, F = SHAPES[0]
    up, down = _experts(E, h, F, kind)[:2]
    x, res, nw, topi, topw = _inputs(E, k, h, 1, "random")
    dead = [e for e in range(E) if e not in set(topi.flatten().tolist())]
    assert len(dead) == E - 2
    bad = []
    for q in (up, down):
        p = types.SimpleNamespace(qweight=q.qweight.clone(), scale=q.scale.clone())
        p.scale[dead] = float("nan")
        if kind == "fp8":
            p.qweight.view(torch.uint8)[dead] = 0x7F
        bad.append(p)
    clean, poisoned = _run(native_lib, up, down, x, res, nw, topi, topw), _run(native_lib, *bad, x, res, nw, topi, topw)
    assert all(torch.isfinite(t.float()).all() for t in poisoned)
    assert all(torch.equal(a, b) for a, b in zip(clean, poisoned))


@pytest.mark.parametrize("kind", KINDS)
def test_moe_decode_wq_deterministic(native_lib, kind):
    E, k, h, F = SHAPES[0]
    up, down = _experts(E, h, F, kind)[:2]
    args = _inputs(E, k, h, 40, "skew")
    a, b = _run(native_lib, up, down, *args), _run(native_lib, up, down, *args)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,h", [(65, 256), (1, 192)])
def test_moe_decode_wq_out_of_limit_arguments(native_lib, kind, M, h):
    """More than 64 tokens and a hidden size that is no multiple of 128 raise before any launch."""
    E, k, F = 4, 2, 128
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=DEV)  # noqa: E731
    if kind == "fp8":
        up, su = z(E, 2 * F, h).view(torch.float8_e4m3fn), torch.ones(E, 2 * F, device=DEV)
        down, sd = z(E, h, F).view(torch.float8_e4m3fn), torch.ones(E, h, device=DEV)
    else:
        up, su = z(E, 2 * F, h // 2), torch.ones(E, 2 * F, max(h // 128, 1), device=DEV)
        down, sd = z(E, h, F // 2), torch.ones(E, h, F // 128, device=DEV)
    x = _bf(M, h, seed=1)
    topi = torch.arange(k, dtype=torch.int32, device=DEV).repeat(M, 1)
    topw = torch.full((M, k), 1.0 / k, device=DEV)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_decode_up_swiglu_wq(x, up, su, topi)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_decode_down_add_rmsnorm_wq(_bf(M * k, F, seed=5), down, sd, topi, topw, x, _bf(h, seed=6), EPS)
