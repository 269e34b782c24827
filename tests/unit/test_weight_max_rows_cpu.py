"""``InferenceEngine(weight_max_rows=...)``: validation and ``_dw`` routing on a CPU engine, and the
M-generic fallback of ``ops.decode_linear_int4`` above 16 rows."""

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.plugins.quantizers import quantize_int4_g128
from llmctl.serve.engine import InferenceEngine


def _engine(**kw):
    return InferenceEngine("tiny", device="cpu", max_batch_size=4, num_kv_blocks=16, block_size=16, max_model_len=64,
                           use_graphs=False, **kw)


def test_weight_max_rows_validation():
    for rows in (16, 32, 64):
        e = _engine(weight_max_rows=rows)  # weight_dtype auto: accepted, ignored
        assert e.weight_max_rows == rows and e.weight_dtype == "auto"
    with pytest.raises(ValueError, match="16, 32 or 64"):
        _engine(weight_dtype="int4", weight_max_rows=48)
    assert InferenceEngine.W8_MAX_ROWS == 16 and _engine().weight_max_rows == 16


@pytest.mark.parametrize("rows", [16, 64])
def test_dw_routing(rows):
    e = _engine(weight_max_rows=rows)
    layer = e.model.layers[0]
    # a CPU engine makes no copies: stand-ins, which _dw only hands out
    q = (torch.zeros(layer.wqkv.shape[0], layer.wqkv.shape[1] // 2, dtype=torch.uint8), torch.ones(1))
    e._wq = [{"wqkv": q} for _ in e.model.layers]
    for n in (16, 17, 64, 65):
        w, s = e._dw(0, layer, "wqkv", n)
        assert (w is q[0] and s is q[1]) if n <= rows else (w is layer.wqkv and s is None), (rows, n)


def test_decode_linear_int4_cpu_mid_rows():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 256, generator=g)
    qd = quantize_int4_g128(torch.randn(64, 256, generator=g) * 0.05)
    y = ops.decode_linear_int4(x, qd["qweight"], qd["scale"])
    torch.testing.assert_close(y, x @ ref.dequant_int4_g128(qd["qweight"], qd["scale"]).t(), rtol=1e-5, atol=1e-5)
