"""The ``sample_ext`` oracle (``ops.ref``), the sampler-state reset and the server's handling of
the extended sampling fields, on the CPU."""

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref


def _params(N, V, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(N, V, generator=g) * 3).round()
    temp = torch.rand(N, generator=g) + 0.3
    temp[::2] = 0.0
    topk = torch.randint(0, 20, (N,), generator=g, dtype=torch.int32)
    topp = torch.rand(N, generator=g) * 0.6 + 0.4
    u = torch.rand(N, generator=g)
    return logits, temp, topk, topp, u


def _neutral(N):
    return (torch.ones(N), torch.zeros(N), torch.zeros(N), torch.zeros(N, dtype=torch.int32))


def test_neutral_parameters_reproduce_sample():
    N, V, S = 6, 97, 8
    logits, temp, topk, topp, u = _params(N, V)
    counts = torch.randint(0, 4, (S, V), dtype=torch.int32)
    mask = torch.randint(0, 2, (S, V), dtype=torch.uint8)
    exp = ref.sample(logits, temp, topk, topp, u)
    rep, freq, pres, nlp = _neutral(N)
    for slot in (torch.full((N,), -1, dtype=torch.int32), torch.arange(N, dtype=torch.int32)):
        c = counts.clone()
        toks, lp, top_ids, top_lp = ops.sample_ext(logits, temp, topk, topp, u, slot, rep, freq, pres, nlp, c, mask)
        assert torch.equal(toks, exp)
        assert (top_ids == -1).all() and (top_lp == -float("inf")).all()
        full = torch.log_softmax(logits.double(), dim=-1).gather(1, toks.view(N, 1)).view(N)
        assert torch.allclose(lp.double(), full, atol=1e-6)


def test_penalty_order():
    """Repetition, then frequency, then presence: a logit of 4 (then 1) seen twice in the output
    with rep = 2, freq = 1, pres = 0.5 gives 4/2 - 2 - 0.5 = -0.5 (then 1/2 - 2 - 0.5 = -2);
    subtracting first would give (4 - 2 - 0.5) / 2 = 0.75 (then (1 - 2 - 0.5) * 2 = -3)."""
    logits = torch.tensor([[4.0, 1.0, -1.0, 0.25]])
    counts = torch.tensor([[2, 2, 0, 0]], dtype=torch.int32)
    mask = torch.tensor([[0, 0, 1, 0]], dtype=torch.uint8)
    x = ref.penalize(logits, torch.tensor([0], dtype=torch.int32), torch.tensor([2.0]), torch.tensor([1.0]),
                     torch.tensor([0.5]), counts, mask)
    # token 2: in the prompt only -> repetition (negative logits are multiplied), no freq / pres
    assert x.tolist() == [[-0.5, -2.0, -2.0, 0.25]]


def test_counts_updated_only_for_stateful_rows():
    N, V, S = 5, 40, 6
    logits, temp, topk, topp, u = _params(N, V, seed=1)
    slot = torch.tensor([4, -1, 0, -1, 2], dtype=torch.int32)
    counts = torch.randint(0, 3, (S, V), dtype=torch.int32)
    before = counts.clone()
    rep, freq, pres, nlp = torch.full((N,), 2.0), torch.full((N,), 0.5), torch.full((N,), 0.25), \
        torch.tensor([8, 3, 0, 1, 5], dtype=torch.int32)
    toks, lp, top_ids, top_lp = ops.sample_ext(logits, temp, topk, topp, u, slot, rep, freq, pres, nlp, counts,
                                               torch.zeros(S, V, dtype=torch.uint8))
    exp = before.clone()
    for i, s in enumerate(slot.tolist()):
        if s >= 0:
            exp[s, int(toks[i])] += 1
    assert torch.equal(counts, exp)
    x = ref.penalize(logits, slot, rep, freq, pres, before, torch.zeros(S, V, dtype=torch.uint8))
    assert torch.equal(x[1], logits[1]) and torch.equal(x[3], logits[3])  # stateless rows: untouched
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for i, k in enumerate(nlp.tolist()):
        assert top_ids[i, :k].tolist() == order[i, :k].tolist() and (top_ids[i, k:] == -1).all()
        assert (top_lp[i, :k - 1] >= top_lp[i, 1:k]).all() if k > 1 else True


def test_state_reset_equals_replay():
    V, S = 50, 3
    prompt, output = [3, 7, 7, 49], [7, 1, 1, 1, 0]
    counts = torch.randint(0, 5, (S, V), dtype=torch.int32)
    mask = torch.randint(0, 2, (S, V), dtype=torch.uint8)
    keep_c, keep_m = counts.clone(), mask.clone()
    ops.sampler_state_reset(counts, mask, 1, prompt, output)
    # replay from empty: mark the prompt, then let sample_ext (greedy on one-hot logits) generate ``output``
    rc, rm = torch.zeros(1, V, dtype=torch.int32), torch.zeros(1, V, dtype=torch.uint8)
    rm[0, prompt] = 1
    rep, freq, pres, nlp = _neutral(1)
    for t in output:
        logits = torch.zeros(1, V)
        logits[0, t] = 5.0
        toks = ops.sample_ext(logits, torch.zeros(1), torch.zeros(1, dtype=torch.int32), torch.ones(1),
                              torch.zeros(1), torch.zeros(1, dtype=torch.int32), rep, freq, pres, nlp, rc, rm)[0]
        assert int(toks[0]) == t
    assert torch.equal(counts[1], rc[0]) and torch.equal(mask[1], rm[0])
    for s in (0, 2):  # the other slots are not touched
        assert torch.equal(counts[s], keep_c[s]) and torch.equal(mask[s], keep_m[s])


def test_sampling_params_defaults_are_plain():
    from llmctl.serve.scheduler import SamplingParams

    assert not SamplingParams().extended
    assert SamplingParams(logprobs=0).extended and not SamplingParams(logprobs=0).penalized
    for kw in ({"repetition_penalty": 1.1}, {"presence_penalty": 0.5}, {"frequency_penalty": -0.5}):
        assert SamplingParams(**kw).extended and SamplingParams(**kw).penalized


# ----------------------------------------------------------------------------- server
@pytest.fixture(scope="module")
def client():
    from fastapi.testclient import TestClient

    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.server import InferenceServer

    eng = InferenceEngine("tiny", device="cpu", max_batch_size=4, num_kv_blocks=64, block_size=8, max_model_len=128)
    srv = InferenceServer("tiny", engine=eng, max_concurrent=16)
    with TestClient(srv.app) as c:
        yield c


@pytest.mark.parametrize("field,value", [("presence_penalty", 2.5), ("presence_penalty", -2.01),
                                         ("frequency_penalty", 3.0), ("frequency_penalty", -5.0),
                                         ("repetition_penalty", 0.0), ("repetition_penalty", -1.0),
                                         ("repetition_penalty", 10.5), ("logprobs", 9), ("logprobs", -1)])
@pytest.mark.parametrize("stream", [False, True])
def test_http_out_of_range_is_400(client, field, value, stream):
    r = client.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 2, "stream": stream, field: value})
    assert r.status_code == 400 and field in r.json()["detail"]


def test_http_logprobs_only_when_asked(client):
    base = {"prompt": [1, 2, 3], "max_tokens": 6, "temperature": 0.0}
    plain = client.post("/v1/completions", json=base).json()
    assert "logprobs" not in plain["choices"][0]
    assert set(plain["choices"][0]) == {"index", "text", "finish_reason"}
    r = client.post("/v1/completions", json=dict(base, logprobs=3, presence_penalty=2.0, frequency_penalty=-2.0,
                                                 repetition_penalty=10.0))
    assert r.status_code == 200
    lp = r.json()["choices"][0]["logprobs"]
    assert set(lp) == {"tokens", "token_ids", "token_logprobs", "top_logprobs"}
    assert [len(lp[k]) for k in ("tokens", "token_ids", "token_logprobs", "top_logprobs")] == [6] * 4
    assert all(v <= 0 for v in lp["token_logprobs"]) and all(1 <= len(t) <= 3 for t in lp["top_logprobs"])
    zero = client.post("/v1/completions", json=dict(base, logprobs=0)).json()["choices"][0]
    assert zero["logprobs"]["token_ids"] and all(t == {} for t in zero["logprobs"]["top_logprobs"])
    assert zero["text"] == plain["text"]  # logprobs alone do not change the tokens


def test_http_streaming_logprob(client):
    import json

    def chunks(**kw):
        with client.stream("POST", "/v1/completions", json=dict({"prompt": "abc", "max_tokens": 4, "stream": True,
                                                                  "temperature": 0.0}, **kw)) as r:
            lines = [l for l in r.iter_lines() if l.startswith("data: ") and l != "data: [DONE]"]
        return [json.loads(l[6:])["choices"][0] for l in lines]

    toks = [c for c in chunks(logprobs=1) if c["finish_reason"] is None]
    assert len(toks) == 4 and all(isinstance(c["logprob"], float) and c["logprob"] <= 0 for c in toks)
    assert all("logprob" not in c for c in chunks())
