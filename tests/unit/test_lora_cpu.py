"""LoRA adapters off the GPU: the ops-layer oracle and fallback, the PEFT import (fusing q/k/v and
gate/up), rank padding and refusal, the safetensors round trip, the HTTP field and the TP refusal."""

import json
import types

import pytest
import torch

from llmctl import ops
from llmctl.models import build_model, get_model_config
from llmctl.serve.lora import LoRAAdapter, fuse_hf, merge_into, projection_shapes, random_adapter
from llmctl.serve.scheduler import SamplingParams


@pytest.fixture(scope="module")
def cfg():
    return get_model_config("tiny")


def _hf_adapter(cfg, r, seed=0, layers=(0, 1)):
    """Separate q/k/v/o and gate/up/down adapters of rank ``r`` in PEFT key style."""
    g = torch.Generator().manual_seed(seed)
    sh = projection_shapes(cfg)
    D = cfg.head_dim or cfg.hidden // cfg.heads
    kv = cfg.kv_heads or cfg.heads
    rows = {"self_attn.q_proj": (cfg.heads * D, cfg.hidden), "self_attn.k_proj": (kv * D, cfg.hidden),
            "self_attn.v_proj": (kv * D, cfg.hidden), "self_attn.o_proj": sh["wo"],
            "mlp.gate_proj": (cfg.ffn, cfg.hidden), "mlp.up_proj": (cfg.ffn, cfg.hidden), "mlp.down_proj": sh["w_down"]}
    out = {}
    for li in layers:
        for mod, (n, k) in rows.items():
            p = f"base_model.model.model.layers.{li}.{mod}"
            out[f"{p}.lora_A.weight"] = torch.randn(r, k, generator=g) * 0.05
            out[f"{p}.lora_B.weight"] = torch.randn(n, r, generator=g) * 0.05
    return out


def test_ref_lora_delta_and_fallback():
    """The oracle's definition, exact zeros on rows without an adapter, and the unfused ops adding
    the delta (CPU: every decode op takes the fallback)."""
    g = torch.Generator().manual_seed(0)
    M, N, K, R, S = 6, 64, 128, 16, 3
    x = torch.randn(M, K, generator=g)
    A, B = torch.randn(S, R, K, generator=g) * 0.1, torch.randn(S, N, R, generator=g) * 0.1
    sc = torch.tensor([2.0, 0.5, 1.0])
    idx = torch.tensor([2, -1, 0, 2, 1, -1], dtype=torch.int32)
    d = ops.lora_delta(x, idx, A, B, sc)
    assert d.dtype == torch.float32 and d.shape == (M, N)
    for m, s in enumerate(idx.tolist()):
        want = torch.zeros(N) if s < 0 else sc[s] * ((x[m] @ A[s].t()) @ B[s].t())
        assert torch.allclose(d[m], want, atol=1e-5)
    assert (d[idx < 0] == 0).all()
    assert ops.ref.lora_delta(x.double(), idx, A.double(), B.double(), sc.double()).dtype == torch.float64
    w = torch.randn(N, K, generator=g) * 0.1
    rows = ops.LoRARows(idx, A, B, sc)
    assert torch.allclose(ops.decode_linear(x, w, None, lora=rows), x @ w.t() + d, atol=1e-5)
    none = rows.rows(torch.full((M,), -1, dtype=torch.int32))
    assert torch.equal(ops.decode_linear(x, w, None, lora=none), ops.decode_linear(x, w))
    w2 = torch.randn(2 * N, K, generator=g) * 0.1
    B2 = torch.randn(S, 2 * N, R, generator=g) * 0.1
    gu = x @ w2.t() + ops.lora_delta(x, idx, A, B2, sc)
    act = ops.decode_up_swiglu(x, w2, lora=ops.LoRARows(idx, A, B2, sc))
    assert torch.allclose(act, torch.nn.functional.silu(gu[:, :N]) * gu[:, N:], atol=1e-5)


def test_peft_import_fuses_qkv_and_gate_up(cfg, tmp_path):
    """Separate q/k/v and gate/up adapters, fused and merged, equal the per-matrix merges."""
    from safetensors.torch import save_file

    r = 4
    raw = _hf_adapter(cfg, r, seed=1)
    (tmp_path / "adapter_config.json").write_text(json.dumps(
        {"r": r, "lora_alpha": 8, "target_modules": ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]}))
    save_file(raw, str(tmp_path / "adapter_model.safetensors"))
    ad = LoRAAdapter.load(str(tmp_path), cfg)
    assert ad.rank == r and ad.scale == 2.0
    assert ad.tensors[(0, "wqkv")][0].shape[0] == 3 * r and ad.tensors[(0, "w_up")][0].shape[0] == 2 * r
    assert ad.tensors[(0, "wo")][0].shape[0] == r and ad.max_rank == 3 * r
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=0)
    before = {(li, n): getattr(model.layers[li], n).detach().clone() for li in (0, 1) for n in ("wqkv", "wo", "w_up", "w_down")}
    untouched = model.layers[2].wqkv.detach().clone() if cfg.layers > 2 else None
    merge_into(model, ad)

    def ba(li, mod):
        p = f"base_model.model.model.layers.{li}.{mod}"
        return 2.0 * (raw[f"{p}.lora_B.weight"] @ raw[f"{p}.lora_A.weight"])

    for li in (0, 1):
        want = {"wqkv": torch.cat([ba(li, "self_attn.q_proj"), ba(li, "self_attn.k_proj"), ba(li, "self_attn.v_proj")]),
                "wo": ba(li, "self_attn.o_proj"),
                "w_up": torch.cat([ba(li, "mlp.gate_proj"), ba(li, "mlp.up_proj")]), "w_down": ba(li, "mlp.down_proj")}
        for n, d in want.items():
            assert torch.allclose(getattr(model.layers[li], n), before[(li, n)] + d, atol=1e-6), (li, n)
    if untouched is not None:
        assert torch.equal(model.layers[2].wqkv, untouched)  # a missing layer means a zero delta


def test_rank_padding_refusal_and_round_trip(cfg, tmp_path):
    ad = random_adapter(cfg, rank=8, seed=5, std=0.02, alpha=16.0, layers=[0], projections=("wqkv", "w_down"))
    assert ad.scale == 2.0 and set(ad.tensors) == {(0, "wqkv"), (0, "w_down")}
    N, K = projection_shapes(cfg)["wqkv"]
    A, B = ad.padded(0, "wqkv", 16, N, K)
    assert A.shape == (16, K) and B.shape == (N, 16)
    assert torch.equal(B @ A, ad.tensors[(0, "wqkv")][1] @ ad.tensors[(0, "wqkv")][0])  # zero padding changes nothing
    assert (A[8:] == 0).all() and (B[:, 8:] == 0).all()
    assert ad.padded(0, "wo", 16, cfg.hidden, cfg.hidden) is None
    ad.save(str(tmp_path / "ad"))
    back = LoRAAdapter.load(str(tmp_path / "ad"), cfg)
    assert back.rank == 8 and back.alpha == 16.0 and set(back.tensors) == set(ad.tensors)
    for k in ad.tensors:
        assert torch.equal(back.tensors[k][0], ad.tensors[k][0]) and torch.equal(back.tensors[k][1], ad.tensors[k][1])
    # a fused rank that does not fit is refused, naming the rank needed; the engine's slots stay clean
    from llmctl.serve.engine import InferenceEngine

    mods = {}
    for key, t in _hf_adapter(cfg, 8, seed=2, layers=(0,)).items():
        li, mod, ab = 0, key.split(".")[-3], key.split(".")[-2][-1]
        mods.setdefault((li, mod), {})[ab] = t
    fused = LoRAAdapter(8, 16.0, fuse_hf(mods, cfg))
    assert fused.max_rank == 24
    with InferenceEngine("tiny", device="cpu", max_batch_size=2, num_kv_blocks=32, block_size=8, max_model_len=64,
                         max_loras=1, max_lora_rank=16) as e:
        with pytest.raises(ValueError, match="needs rank 24"):
            e.load_lora("big", fused)
        assert e.loras == [] and all((t == 0).all() for d in e._lora for ts in d.values() for t in ts)
        assert e.load_lora("small", str(tmp_path / "ad")) == 0  # from a directory
        with pytest.raises(ValueError, match="already loaded"):
            e.load_lora("small", ad)
    with pytest.raises(ValueError, match="max_lora_rank must be one of"):
        InferenceEngine("tiny", device="cpu", max_batch_size=2, num_kv_blocks=32, block_size=8, max_model_len=64,
                        max_loras=1, max_lora_rank=8)


def test_moe_refused_by_name(cfg):
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(is_moe=True), tp=1)
    from llmctl.serve.engine import InferenceEngine

    eng._lora_refusal = lambda: InferenceEngine._lora_refusal(eng)
    with pytest.raises(ValueError, match="LoRA adapters not supported with MoE models"):
        InferenceEngine.load_lora(eng, "a", random_adapter(cfg, rank=8))


def test_tp_refuses_lora_requests():
    """TP > 1: the stacked adapters are not sharded; the request is refused by name."""
    from llmctl.serve.tp import TPInferenceEngine

    eng = types.SimpleNamespace(tp_size=2)
    with pytest.raises(ValueError, match="lora not supported with tensor parallelism > 1"):
        TPInferenceEngine.add_request(eng, [1, 2], SamplingParams(lora="a"))


# ----------------------------------------------------------------------------- server
@pytest.fixture(scope="module")
def client(cfg):
    from fastapi.testclient import TestClient

    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.server import InferenceServer

    eng = InferenceEngine("tiny", device="cpu", max_batch_size=4, num_kv_blocks=64, block_size=8, max_model_len=128,
                          max_loras=2)
    eng.load_lora("ft-a", random_adapter(cfg, rank=8, seed=1, std=0.05, alpha=16.0))
    srv = InferenceServer("tiny", engine=eng, max_concurrent=16)
    with TestClient(srv.app) as c:
        yield c


@pytest.mark.parametrize("stream", [False, True])
def test_http_unknown_lora_is_400(client, stream):
    r = client.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 2, "stream": stream, "lora": "nope"})
    assert r.status_code == 400 and "unknown LoRA adapter 'nope'" in r.json()["detail"]


def test_http_lora_field_and_model_alias(client):
    base = {"prompt": [1, 2, 3, 4, 5, 6], "max_tokens": 12, "temperature": 0.0, "ignore_eos": True}
    plain = client.post("/v1/completions", json=base).json()["text"]
    by_field = client.post("/v1/completions", json=dict(base, lora="ft-a"))
    assert by_field.status_code == 200
    by_model = client.post("/v1/completions", json=dict(base, model="ft-a")).json()["text"]
    other = client.post("/v1/completions", json=dict(base, model="some-other-name")).json()["text"]
    assert by_field.json()["text"] == by_model != plain  # the adapter changes what is generated
    assert other == plain  # any other model value is served by the base


def test_http_models_lists_adapters(client):
    data = client.get("/v1/models").json()["data"]
    assert "parent" not in data[0]
    assert [d for d in data if d["id"] == "ft-a"] == [dict(data[1], id="ft-a", parent=data[0]["id"])]
