"""Group-128 int4 decode weights (W4A16) without a GPU: the ``int4-g128`` quantizer and its
packed format, the fp32 oracle, the CPU paths of the decode ops (which use the dequantised weight)
and the engine option."""

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.plugins.quantizers import QUANTIZERS, dequantize, quantize_int4_g128
from llmctl.testing.numerics import int4_grid, snap_int4_grid


def _x(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def test_int4_g128_round_trip():
    w = _x(96, 384, seed=1) * 0.05
    qd = quantize_int4_g128(w)
    assert qd["qweight"].dtype == torch.uint8 and qd["qweight"].shape == (96, 192) and qd["qweight"].is_contiguous()
    assert qd["scale"].dtype == torch.float32 and qd["scale"].shape == (96, 3) and qd["scale"].is_contiguous()
    torch.testing.assert_close(qd["scale"], w.reshape(96, 3, 128).abs().amax(2) / 7.0)
    wd = dequantize("int4-g128", qd, (96, 384))
    assert wd.dtype == torch.float32 and wd.shape == w.shape
    half = qd["scale"].repeat_interleave(128, dim=1) / 2
    assert ((wd - w).abs() <= half * (1 + 1e-6) + 1e-12).all()
    assert torch.equal(wd, ref.dequant_int4_g128(qd["qweight"], qd["scale"]))


def test_int4_g128_nibble_order():
    """Byte j of a row: k = 2j in the low nibble, k = 2j + 1 in the high one, u = q + 8."""
    w = torch.zeros(2, 256)
    w[1, 131] = -0.7  # odd k, second group
    qd = quantize_int4_g128(w)
    want = torch.full((2, 128), 0x88, dtype=torch.uint8)
    want[1, 65] = 0x08 | (1 << 4)  # q = -7 -> u = 1 in the high nibble of byte 65
    assert torch.equal(qd["qweight"], want)
    assert qd["scale"][1, 1].item() == pytest.approx(0.1, rel=1e-6) and qd["scale"][1, 0].item() == pytest.approx(1e-12)
    wd = ref.dequant_int4_g128(qd["qweight"], qd["scale"])
    torch.testing.assert_close(wd, w)


def test_int4_g128_needs_k_multiple_of_128():
    with pytest.raises(ValueError):
        quantize_int4_g128(torch.zeros(64, 192))
    with pytest.raises(ValueError):
        ref.dequant_int4_g128(torch.zeros(64, 96, dtype=torch.uint8), torch.ones(64, 2))


def test_int4_g128_lossless_grid():
    w, e = int4_grid(80, 512, seed=3)
    assert len(e.unique()) > 1 and (w.reshape(80, 4, 128).abs().amax(2) == 7 * torch.exp2(e.float())).all()
    qd = quantize_int4_g128(w)
    assert torch.equal(qd["scale"], torch.exp2(e.float()))
    assert torch.equal(ref.dequant_int4_g128(qd["qweight"], qd["scale"]), w)
    assert torch.equal(w.to(torch.bfloat16).float(), w)
    # snapping an arbitrary weight lands on the same kind of grid
    s = snap_int4_grid(_x(64, 256, seed=4) * 0.05)
    qs = quantize_int4_g128(s)
    assert torch.equal(ref.dequant_int4_g128(qs["qweight"], qs["scale"]), s)
    assert torch.equal(qs["scale"], torch.exp2(torch.log2(qs["scale"]).round()))


def test_int4_decode_ops_cpu_fallbacks():
    """The CPU paths of the int4 projection and of the three fused ops use the dequantised weight."""
    x = _x(3, 256, seed=21)
    qd = quantize_int4_g128(_x(128, 256, seed=22) * 0.1)
    w4, sc = qd["qweight"], qd["scale"]
    wd = ref.dequant_int4_g128(w4, sc)
    assert not ops.decode_fused_ok(x, w4)
    b = _x(128, seed=25)
    torch.testing.assert_close(ops.decode_linear_int4(x, w4, sc), ops.decode_linear(x, wd))
    torch.testing.assert_close(ops.decode_linear_int4(x, w4, sc, b), ops.decode_linear(x, wd, b))
    torch.testing.assert_close(ops.decode_linear_int4(x, w4, sc, b), ref.decode_linear_int4(x, w4, sc, b))
    torch.testing.assert_close(ops.decode_up_swiglu(x, w4, None, w_scale=sc), ops.decode_up_swiglu(x, wd))
    res, nw = _x(3, 128, seed=23), 1 + 0.1 * _x(128, seed=24)
    y, r = ops.decode_linear_add_rmsnorm(x, w4, None, res, nw, 1e-5, w_scale=sc)
    y2, r2 = ops.decode_linear_add_rmsnorm(x, wd, None, res, nw, 1e-5)
    torch.testing.assert_close(r, r2)
    torch.testing.assert_close(y, y2)
    # QKV + RoPE + cache write
    nq, nkv, D, bs, nb = 4, 2, 16, 4, 8
    cos, sin = ref.rope_tables(64, D)
    pos = torch.tensor([5, 2, 9], dtype=torch.int32)
    slots = torch.tensor([1 * bs + 1, -1, 3 * bs + 2])
    kc, vc = torch.zeros(nb, bs, nkv, D), torch.zeros(nb, bs, nkv, D)
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    q = ops.decode_qkv_rope_cache(x, w4, None, cos, sin, nq, nkv, pos, kc, vc, slots, w_scale=sc)
    q2 = ops.decode_qkv_rope_cache(x, wd, None, cos, sin, nq, nkv, pos, kc2, vc2, slots)
    torch.testing.assert_close(q, q2)
    torch.testing.assert_close(kc, kc2)
    torch.testing.assert_close(vc, vc2)
    assert kc.abs().sum() > 0


def test_int4_g128_registered():
    from llmctl.plugins import quantizers

    assert QUANTIZERS["int4-g128"] is quantize_int4_g128

    class Reg:
        def __init__(self):
            self.d = {}

        def add(self, group, name, fn):
            self.d[(group, name)] = fn

    reg = Reg()
    quantizers.register(reg)
    assert reg.d[("quantizers", "int4-g128")] is quantize_int4_g128
    assert reg.d[("quantizers", "int4")] is quantizers.quantize_int4  # the per-row format is unchanged


def test_engine_int4_option_cpu():
    """On a CPU device the option is accepted and nothing is quantised: same tokens as ``auto``."""
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    prompts = [[3, 17, 42, 9, 5], [7, 7, 100, 250]]
    p = SamplingParams(max_tokens=5, temperature=0.0, ignore_eos=True)
    outs = {}
    for wd in ("auto", "int4"):
        e = InferenceEngine("tiny", device="cpu", num_kv_blocks=32, max_model_len=128, weight_dtype=wd)
        assert e.weight_dtype == "auto" and e._w4 is None and e._w8 is None
        outs[wd] = [s.output_ids for s in e.generate(prompts, p)]
        e.close()
    assert outs["int4"] == outs["auto"]
    with pytest.raises(ValueError):
        InferenceEngine("tiny", device="cpu", num_kv_blocks=32, max_model_len=128, weight_dtype="int3")
