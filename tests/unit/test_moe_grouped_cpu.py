"""``ops.moe_route`` + ``ops.moe_grouped_mlp`` off the GPU (the fp32 oracle) against the model's
``MoEMLP.forward``, and the ``moe_max_rows`` option of the engine, the server and the CLI."""

import inspect

import pytest
import torch

from llmctl import ops
from llmctl.serve.engine import InferenceEngine


def _engine(**kw):
    return InferenceEngine("tiny-moe", device="cpu", max_batch_size=4, num_kv_blocks=16, block_size=16, max_model_len=64,
                           use_graphs=False, **kw)


def test_grouped_mlp_cpu_equals_the_module():
    moe = _engine().model.layers[0].moe
    x = torch.randn(70, moe.w_router.shape[1], generator=torch.Generator().manual_seed(3))
    topi, topw = ops.moe_route(x, moe.w_router, moe.k)
    y = ops.moe_grouped_mlp(x, ops.MoEExpertTable(moe.experts_up), ops.MoEExpertTable(moe.experts_down), topi, topw)
    with torch.no_grad():
        torch.testing.assert_close(y, moe(x), rtol=1e-4, atol=1e-5)


def test_moe_max_rows_validation():
    for rows in (63, 8193, 0):
        with pytest.raises(ValueError, match="moe_max_rows"):
            _engine(moe_max_rows=rows)
    e = _engine(moe_max_rows=256)  # accepted; no routed-expert kernels on the CPU: ignored
    assert e.moe_max_rows == 64 and not e._moe_grouped(128) and e.stats["moe_grouped_steps"] == 0


def test_moe_max_rows_is_threaded_through():
    from llmctl.benchmarks.serving import run_serving_benchmark
    from llmctl.cli.commands import bench, serve
    from llmctl.serve.server import InferenceServer

    for fn in (InferenceEngine.__init__, InferenceServer.__init__, serve.start, bench.e2e, run_serving_benchmark):
        assert "moe_max_rows" in inspect.signature(fn).parameters, fn
