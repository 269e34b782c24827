"""The routed-expert decode ops on the CPU (fp32 oracles): the op-level chain is the model's
MoE MLP, and the expert pointer-table holder validates what the kernels assume."""

import pytest
import torch

from llmctl import ops
from llmctl.models import get_model_config
from llmctl.models.moe import MoEMLP


def _moe():
    cfg = get_model_config("tiny-moe")
    torch.manual_seed(0)
    return cfg, MoEMLP(cfg, cfg.layers, device="cpu", dtype=torch.float32)


def test_op_chain_matches_moe_module():
    """route -> up + SwiGLU -> down + combine + residual + RMSNorm == MoEMLP.forward + add_rmsnorm
    in fp32: ties the oracles to the model's definition."""
    cfg, moe = _moe()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, cfg.hidden, generator=g)
    res = torch.randn(7, cfg.hidden, generator=g)
    nw = 1.0 + 0.1 * torch.randn(cfg.hidden, generator=g)
    eps = cfg.layer_norm_eps
    with torch.no_grad():
        want_xn, want_res = ops.add_rmsnorm(moe(x), res, nw, eps)
        up, down = ops.MoEExpertTable(moe.experts_up), ops.MoEExpertTable(moe.experts_down)
        topi, topw = ops.moe_route(x, moe.w_router, moe.k)
        assert topi.shape == (7, moe.k) and topi.dtype == torch.int32 and topw.dtype == torch.float32
        act = ops.moe_decode_up_swiglu(x, up, topi)
        assert act.shape == (7 * moe.k, cfg.moe_ffn)
        xn, res_out = ops.moe_decode_down_add_rmsnorm(act, down, topi, topw, res, nw, eps)
        # and the one-call oracle of the whole routed MLP
        xn2, res2 = ops.ref.moe_decode_mlp(x, list(moe.experts_up), list(moe.experts_down), topi, topw, res, nw, eps)
    torch.testing.assert_close(res_out, want_res)
    torch.testing.assert_close(xn, want_xn)
    torch.testing.assert_close(res2, want_res)
    torch.testing.assert_close(xn2, want_xn)


def test_route_oracle_ties_prefer_lowest_index():
    w = torch.randn(4, 256, generator=torch.Generator().manual_seed(2))
    w[2] = w[0]  # experts 0 and 2 always tie
    x = torch.randn(9, 256, generator=torch.Generator().manual_seed(3))
    topi, topw = ops.moe_route(x, w, 3)
    for row in topi.tolist():
        assert len(set(row)) == 3
        if 0 in row and 2 in row:
            assert row.index(0) + 1 == row.index(2)
        else:
            assert 2 not in row or 0 in row
    torch.testing.assert_close(topw.sum(-1), torch.ones(9))
    ti, tw = ops.moe_route(torch.zeros(2, 256), w, 2)
    assert ti.tolist() == [[0, 1], [0, 1]] and torch.equal(tw, torch.full((2, 2), 0.5))


def test_expert_table_checks():
    cfg, moe = _moe()
    t = ops.MoEExpertTable(moe.experts_down)
    assert t.E == cfg.num_experts and t.shape == (cfg.hidden, cfg.moe_ffn) and not t.stale()
    assert t.ptrs.dtype == torch.int64 and t.ptrs.tolist() == [p.data_ptr() for p in moe.experts_down]
    good = [p.detach() for p in moe.experts_down]
    with pytest.raises(ValueError, match="contiguous"):
        ops.MoEExpertTable(good[:1] + [good[1].t().contiguous().t()] + good[2:])
    with pytest.raises(ValueError, match="expert 2"):
        ops.MoEExpertTable(good[:2] + [good[2][:, :128].contiguous()] + good[3:])
    with pytest.raises(ValueError, match="expert 1"):
        ops.MoEExpertTable([good[0], good[1].double()])
