"""Routed-expert decode kernels (csrc/moe_decode.hip) vs the fp32 oracles ``ref.moe_route`` and
``ref.moe_decode_mlp`` (GPU only)."""

import functools

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.testing.numerics import row_err as _row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ----------------------------------------------------------------------------- router
ROUTE_SHAPES = [(4, 2, 256), (8, 2, 1280), (8, 1, 1280), (64, 8, 1280)]
ROUTE_M = [1, 16, 40]
# Seeds chosen on the CPU so that the ORACLE alone leaves out at most 10 % of a case's rows (rows whose
# k-th and (k+1)-th bf16 logits are within 2 ulps: there a one-ulp difference of the fp32 summation
# order may legitimately flip a pick).  Share of such rows over 4,096 random rows, measured on the
# CPU: 1.0 % at (4, 2, 256), 1.8 % at (8, 2, 1280), 2.0 % at (8, 1, 1280), 18 % at (64, 8, 1280): the
# first seed that meets the cap is taken (rows left out: 1 of 16 at (8, 2, 1280) and (64, 8, 1280),
# 4 of 40 at (64, 8, 1280), none elsewhere).
ROUTE_SEEDS = {
    (4, 2, 256, 1): 0, (4, 2, 256, 16): 0, (4, 2, 256, 40): 0,
    (8, 2, 1280, 1): 0, (8, 2, 1280, 16): 0, (8, 2, 1280, 40): 0,
    (8, 1, 1280, 1): 0, (8, 1, 1280, 16): 0, (8, 1, 1280, 40): 0,
    (64, 8, 1280, 1): 2, (64, 8, 1280, 16): 3, (64, 8, 1280, 40): 2,
}


def _route_inputs(E, h, M, seed):
    """CPU bf16 ``x [M, h]`` with rows of unit RMS and ``w_router ~ N(0, 0.02 sqrt(256 / h))``."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, h, generator=g)
    x = x / x.pow(2).mean(-1, keepdim=True).sqrt()
    w = torch.randn(E, h, generator=g) * (0.02 * (256.0 / h) ** 0.5)
    return x.to(torch.bfloat16), w.to(torch.bfloat16)


def _compared_rows(x, w, k):
    """(mask of the rows whose routing is compared, the oracle's bf16 logits): the k-th and (k+1)-th
    largest logits differ by more than 2 bf16 ulps (ulp of the larger magnitude of the two)."""
    logits = (x.float() @ w.float().t()).to(torch.bfloat16).float()
    s = logits.sort(-1, descending=True).values
    a, b = s[:, k - 1], s[:, k]
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -120)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return (a - b) > 2 * ulp, logits


def _check_every_row(topi, topw, E, k):
    assert topi.dtype == torch.int32 and topw.dtype == torch.float32
    assert ((topi >= 0) & (topi < E)).all()
    srt = topi.sort(-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all()  # distinct
    assert (topw.sum(-1) - 1.0).abs().max().item() < 1e-5
    assert (topw[:, 1:] <= topw[:, :-1]).all()  # non-increasing


@pytest.mark.parametrize("M", ROUTE_M)
@pytest.mark.parametrize("E,k,h", ROUTE_SHAPES)
def test_moe_route_vs_oracle(native_lib, E, k, h, M):
    x, w = _route_inputs(E, h, M, ROUTE_SEEDS[(E, k, h, M)])
    cmp_rows, logits = _compared_rows(x, w, k)
    assert logits.abs().max().item() < 4
    left_out = int((~cmp_rows).sum().item())
    print(f"moe_route E={E} k={k} h={h} M={M}: {left_out} of {M} rows left out")
    assert 10 * left_out <= M  # at most 10 % (in integers: 4 of 40 is exactly the cap)
    want_i, want_w = ref.moe_route(x, w, k)  # the oracle, on the CPU (the seeds were chosen there)
    topi, topw = native_lib.moe_route(x.to(DEV), w.to(DEV), k)
    topi, topw = topi.cpu(), topw.cpu()
    assert topi.shape == (M, k) and topw.shape == (M, k)
    _check_every_row(topi, topw, E, k)
    gi, wi = topi[cmp_rows].long(), want_i[cmp_rows].long()
    assert torch.equal(gi.sort(-1).values, wi.sort(-1).values)  # the expert set
    dense_g = torch.zeros(gi.shape[0], E).scatter_(1, gi, topw[cmp_rows])
    dense_w = torch.zeros(gi.shape[0], E).scatter_(1, wi, want_w[cmp_rows])
    err = (dense_g - dense_w).abs().max().item() if gi.numel() else 0.0
    print(f"  weights by expert: max abs err {err:.2e}")
    assert err < 1e-2


@pytest.mark.parametrize("E,k,h", ROUTE_SHAPES)
def test_moe_route_exact_ties(native_lib, E, k, h):
    _, w = _route_inputs(E, h, 1, 7)
    # x = 0: every logit 0, every probability 1 / E -> experts 0 .. k-1 with weights 1 / k
    topi, topw = native_lib.moe_route(torch.zeros(3, h, dtype=torch.bfloat16, device=DEV), w.to(DEV), k)
    assert topi.tolist() == [list(range(k))] * 3
    assert torch.equal(topw.cpu(), torch.full((3, k), 1.0 / k))
    # two identical router rows: the lower index is preferred
    lo, hi = 1, E - 1
    w2 = w.clone()
    w2[hi] = w2[lo]
    x, _ = _route_inputs(E, h, 40, 8)
    topi, topw = native_lib.moe_route(x.to(DEV), w2.to(DEV), k)
    _check_every_row(topi.cpu(), topw.cpu(), E, k)
    seen = 0
    for row in topi.tolist():
        seen += int(lo in row)
        if hi in row:
            assert lo in row and row.index(lo) < row.index(hi)
    assert seen >= 3  # (the oracle picks expert `lo` in 4 or more of the 40 rows at every shape)


# ----------------------------------------------------------------------------- routed MLP
MLP_SHAPES = [(8, 2, 1280, 1152),  # two K chunks each: the last one 256 deep (gate/up), 128 deep (down)
              (4, 2, 256, 256)]    # a single chunk (tiny-moe)
MLP_M = [1, 5, 16, 17, 40]
EPS = 1e-5


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _experts(E, h, F):
    ups = [_bf(2 * F, h, scale=0.05, seed=200 + e) for e in range(E)]
    downs = [_bf(h, F, scale=0.05, seed=300 + e) for e in range(E)]
    return ups, downs, ops.MoEExpertTable(ups), ops.MoEExpertTable(downs)


def _routing(E, k, M, kind):
    g = torch.Generator().manual_seed(17 * M + E)
    if kind == "random":
        topi = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(M)])
    else:  # every token picks expert 0 first (one expert with M copies), a round-robin second pick
        assert k == 2
        topi = torch.tensor([[0, 1 + t % (E - 1)] for t in range(M)])
    topw = torch.rand(M, k, generator=g).add_(0.1).sort(-1, descending=True).values
    topw = topw / topw.sum(-1, keepdim=True)
    return topi.to(torch.int32).to(DEV), topw.float().to(DEV)


@functools.lru_cache(maxsize=None)
def _case(E, k, h, F, M, kind):
    """Inputs, the kernels' outputs and the fp32 oracle's, computed once per case."""
    ups, downs, up_t, down_t = _experts(E, h, F)
    x = _bf(M, h, seed=400 + M)
    res = _bf(M, h, seed=500 + M)
    nw = (1.0 + 0.1 * torch.randn(h, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))).to(torch.bfloat16)
    topi, topw = _routing(E, k, M, kind)
    want_act = ref.moe_decode_up_swiglu(x, ups, topi)
    want_xn, want_res = ref.moe_decode_mlp(x, ups, downs, topi, topw, res, nw, EPS)
    return dict(x=x, res=res, nw=nw, topi=topi, topw=topw, want_act=want_act, want_xn=want_xn, want_res=want_res)


def _run(native_lib, c, up_t, down_t):
    F = up_t.shape[0] // 2
    act = native_lib.moe_decode_up_swiglu(c["x"], up_t.ptrs, c["topi"], up_t.E, F)
    xn, res_out = native_lib.moe_decode_down_add_rmsnorm(act, down_t.ptrs, c["topi"], c["topw"], c["res"], c["nw"], EPS,
                                                         down_t.E)
    return act, xn, res_out


@pytest.mark.parametrize("kind", ["random", "skew"])
@pytest.mark.parametrize("M", MLP_M)
@pytest.mark.parametrize("E,k,h,F", MLP_SHAPES)
def test_moe_decode_mlp_vs_oracle(native_lib, E, k, h, F, M, kind):
    _, _, up_t, down_t = _experts(E, h, F)
    c = _case(E, k, h, F, M, kind)
    assert ops.moe_decode_ok(c["x"], E, k, h, F)
    act, xn, res_out = _run(native_lib, c, up_t, down_t)
    assert act.shape == (M * k, F) and xn.shape == (M, h) and res_out.shape == (M, h)
    assert torch.isfinite(act.float()).all() and torch.isfinite(xn.float()).all()
    e_act, e_res, e_xn = _row_err(act, c["want_act"]), _row_err(res_out, c["want_res"]), _row_err(xn, c["want_xn"])
    print(f"moe_decode_mlp E={E} k={k} h={h} F={F} M={M} {kind}: act {e_act:.2e} res {e_res:.2e} xn {e_xn:.2e}")
    assert e_act < 2e-2
    assert e_res < 1.5e-2
    assert e_xn < 2e-2
    # the op wrappers take the same path
    act2 = ops.moe_decode_up_swiglu(c["x"], up_t, c["topi"])
    xn2, res2 = ops.moe_decode_down_add_rmsnorm(act2, down_t, c["topi"], c["topw"], c["res"], c["nw"], EPS)
    assert torch.equal(act2, act) and torch.equal(xn2, xn) and torch.equal(res2, res_out)


@pytest.mark.parametrize("E,k,h,F", MLP_SHAPES)
def test_moe_decode_skipped_experts_contribute_nothing(native_lib, E, k, h, F):
    """One token leaves E - 2 experts unrouted: with their weights NaN both outputs stay finite and
    equal, bit for bit, the run with finite weights."""
    ups, downs, up_t, down_t = _experts(E, h, F)
    c = _case(E, k, h, F, 1, "random")
    routed = set(c["topi"].flatten().tolist())
    assert len(routed) == 2
    ups2 = [u if e in routed else torch.full_like(u, float("nan")) for e, u in enumerate(ups)]
    downs2 = [d if e in routed else torch.full_like(d, float("nan")) for e, d in enumerate(downs)]
    act, xn, res_out = _run(native_lib, c, up_t, down_t)
    act2, xn2, res2 = _run(native_lib, c, ops.MoEExpertTable(ups2), ops.MoEExpertTable(downs2))
    assert torch.isfinite(xn2.float()).all() and torch.isfinite(res2.float()).all()
    assert torch.equal(act2, act) and torch.equal(xn2, xn) and torch.equal(res2, res_out)


@pytest.mark.parametrize("M,kind", [(17, "random"), (40, "skew")])
def test_moe_decode_deterministic(native_lib, M, kind):
    E, k, h, F = MLP_SHAPES[0]
    _, _, up_t, down_t = _experts(E, h, F)
    c = _case(E, k, h, F, M, kind)
    a, b = _run(native_lib, c, up_t, down_t), _run(native_lib, c, up_t, down_t)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    x, w = _route_inputs(E, h, M, 3)
    r1, r2 = native_lib.moe_route(x.to(DEV), w.to(DEV), k), native_lib.moe_route(x.to(DEV), w.to(DEV), k)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


@pytest.mark.parametrize("M,h,k", [(65, 256, 2), (1, 192, 2), (1, 256, 9)])
def test_moe_decode_out_of_limit_arguments(native_lib, M, h, k):
    """More than 64 tokens, a hidden size that is no multiple of 128 and more than 8 picks each raise
    (before any launch), and the predicate is false for them."""
    E, F = 16, 128
    x = _bf(M, h, seed=1)
    assert not ops.moe_decode_ok(x, E, k, h, F)
    w = _bf(E, h, scale=0.02, seed=2)
    up_t = ops.MoEExpertTable([_bf(2 * F, h, scale=0.05, seed=3)] * E)
    down_t = ops.MoEExpertTable([_bf(h, F, scale=0.05, seed=4)] * E)
    topi = torch.arange(k, dtype=torch.int32, device=DEV).repeat(M, 1)
    topw = torch.full((M, k), 1.0 / k, device=DEV)
    act = _bf(M * k, F, seed=5)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_route(x, w, k)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_decode_up_swiglu(x, up_t.ptrs, topi, E, F)
    with pytest.raises(RuntimeError, match="llmctl"):
        native_lib.moe_decode_down_add_rmsnorm(act, down_t.ptrs, topi, topw, x, _bf(h, seed=6), EPS, E)
