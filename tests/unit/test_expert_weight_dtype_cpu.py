"""``expert_weight_dtype`` off the GPU: ignored by the engine, carried by the CLI, oracle fallback of the ops."""

import inspect

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.serve.engine import InferenceEngine


@pytest.mark.parametrize("model", ["tiny", "tiny-moe"])
def test_engine_accepts_and_ignores(model):
    with InferenceEngine(model, device="cpu", num_kv_blocks=16, expert_weight_dtype="int4") as eng:
        assert eng.expert_weight_dtype == "auto" and eng._moe_q is None
    with pytest.raises(ValueError, match="expert_weight_dtype"):
        InferenceEngine(model, device="cpu", num_kv_blocks=16, expert_weight_dtype="int3")


def test_cli_and_server_carry_the_flag():
    from llmctl.benchmarks.serving import run_serving_benchmark
    from llmctl.cli.commands import bench, serve
    from llmctl.serve.server import InferenceServer

    for fn in (serve.start, bench.e2e, run_serving_benchmark, InferenceServer.__init__, InferenceEngine.__init__):
        assert "expert_weight_dtype" in inspect.signature(fn).parameters, fn
    srv = InferenceServer("tiny-moe", device="cpu", expert_weight_dtype="fp8")
    assert srv.engine_kwargs["expert_weight_dtype"] == "fp8"


@pytest.mark.parametrize("kind", ["fp8", "int4"])
def test_quant_experts_and_cpu_fallback(kind):
    E, k, h, F, M = 4, 2, 256, 128, 5
    g = torch.Generator().manual_seed(0)
    ups = [torch.randn(2 * F, h, generator=g) * 0.05 for _ in range(E)]
    downs = [torch.randn(h, F, generator=g) * 0.05 for _ in range(E)]
    up, down = ops.MoEQuantExperts(ups, kind), ops.MoEQuantExperts(downs, kind)
    assert (up.E, up.shape, down.shape, up.kind) == (E, (2 * F, h), (h, F), kind)
    want = ((torch.float8_e4m3fn, (E, 2 * F, h), (E, 2 * F)) if kind == "fp8" else (torch.uint8, (E, 2 * F, h // 2), (E, 2 * F, h // 128)))
    assert (up.qweight.dtype, tuple(up.qweight.shape), tuple(up.scale.shape)) == want and up.scale.dtype == torch.float32
    dq = up.dequantized()
    assert len(dq) == E and dq[0].shape == (2 * F, h) and dq[0].dtype == torch.float32
    assert (dq[0] - ups[0]).abs().max() < (0.02 if kind == "fp8" else 0.05)
    with pytest.raises(ValueError):
        ops.MoEQuantExperts(ups, "int8")
    x, res, nw = torch.randn(M, h, generator=g), torch.randn(M, h, generator=g), torch.ones(h)
    topi = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(M)]).int()
    topw = torch.full((M, k), 0.5)
    act = ops.moe_decode_up_swiglu(x, up, topi)
    xn, s = ops.moe_decode_down_add_rmsnorm(act, down, topi, topw, res, nw, 1e-5)
    assert torch.equal(act, ref.moe_decode_up_swiglu(x, dq, topi))
    want_xn, want_s = ref.moe_decode_mlp(x, dq, down.dequantized(), topi, topw, res, nw, 1e-5)
    assert torch.equal(xn, want_xn) and torch.equal(s, want_s)
