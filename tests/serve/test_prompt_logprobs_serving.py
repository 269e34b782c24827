"""Prompt scoring end to end on the CPU engine (scenarios: ``llmctl/testing/prompt_logprobs.py``) and
through ``/v1/completions``: ``echo`` + ``logprobs`` (the OpenAI shape), ``prompt_logprobs`` (the vLLM
shape), ``max_tokens = 0`` and the refusals."""

import math

import pytest

from llmctl.testing import prompt_logprobs as scenarios

DEV = "cpu"


@pytest.mark.parametrize("scenario", ["check_concurrent", "check_chunked", "check_mixed", "check_score_only",
                                      "check_prefix_cache", "check_preemption", "check_interactions",
                                      "check_tp_refusal"])
def test_scenario(scenario):
    getattr(scenarios, scenario)(DEV)


# ----------------------------------------------------------------------------- server
@pytest.fixture(scope="module")
def served():
    from fastapi.testclient import TestClient

    from llmctl.serve.server import InferenceServer

    eng = scenarios.engine(DEV)
    srv = InferenceServer("tiny", engine=eng, max_concurrent=16)
    with TestClient(srv.app) as c:
        yield c, eng
    eng.close()


PROMPT = scenarios.PROMPTS[2]


def test_http_echo_logprobs_openai_shape(served):
    client, eng = served
    want = scenarios.oracle()[2]
    r = client.post("/v1/completions", json={"prompt": PROMPT, "echo": True, "logprobs": 1, "max_tokens": 0})
    assert r.status_code == 200, r.text
    body = r.json()
    ch = body["choices"][0]
    assert ch["finish_reason"] == "length" and body["usage"]["completion_tokens"] == 0
    assert ch["text"] == eng.tokenizer.decode(PROMPT) == body["text"]
    lp = ch["logprobs"]
    assert set(lp) == {"tokens", "token_ids", "token_logprobs", "top_logprobs", "text_offset"}
    assert [len(lp[k]) for k in ("tokens", "token_ids", "token_logprobs", "top_logprobs", "text_offset")] == [len(PROMPT)] * 5
    assert lp["token_ids"] == PROMPT and lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    for i in range(1, len(PROMPT)):
        assert abs(lp["token_logprobs"][i] - want[i - 1, PROMPT[i]].item()) <= scenarios.bound(DEV)
        assert len(lp["top_logprobs"][i]) == 1
    assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])
    assert "prompt_logprobs" not in ch
    # with a completion: the prompt's entries, then the generated tokens'
    r = client.post("/v1/completions", json={"prompt": PROMPT, "echo": True, "logprobs": 2, "max_tokens": 3,
                                             "temperature": 0.0, "ignore_eos": True})
    ch2 = r.json()["choices"][0]
    n = len(PROMPT) + 3
    assert [len(ch2["logprobs"][k]) for k in ("tokens", "token_ids", "token_logprobs", "top_logprobs", "text_offset")] == [n] * 5
    assert ch2["logprobs"]["token_ids"][:len(PROMPT)] == PROMPT and ch2["text"].startswith(ch["text"])
    assert all(isinstance(v, float) and v <= 0 for v in ch2["logprobs"]["token_logprobs"][1:])
    assert all(1 <= len(t) <= 2 for t in ch2["logprobs"]["top_logprobs"][1:])  # (keyed by token text)


def test_http_prompt_logprobs_vllm_shape(served):
    client, eng = served
    want = scenarios.oracle()[2]
    r = client.post("/v1/completions", json={"prompt": PROMPT, "prompt_logprobs": 3, "max_tokens": 2, "temperature": 0.0,
                                             "ignore_eos": True})
    assert r.status_code == 200, r.text
    ch = r.json()["choices"][0]
    assert "logprobs" not in ch and r.json()["usage"]["completion_tokens"] == 2
    pl = ch["prompt_logprobs"]
    assert len(pl) == len(PROMPT) and pl[0] is None
    for i in range(1, len(PROMPT)):
        ent = pl[i]
        own = ent[str(PROMPT[i])]
        assert set(own) == {"logprob", "rank", "decoded_token"} and own["rank"] >= 1
        assert abs(own["logprob"] - want[i - 1, PROMPT[i]].item()) <= scenarios.bound(DEV)
        assert own["decoded_token"] == eng.tokenizer.decode([PROMPT[i]])
        assert len(ent) == (3 if own["rank"] <= 3 else 4)
        ranks = sorted(v["rank"] for k, v in ent.items() if k != str(PROMPT[i]) or own["rank"] <= 3)
        assert ranks == [1, 2, 3]
        for k, v in ent.items():
            assert abs(v["logprob"] - want[i - 1, int(k)].item()) <= scenarios.bound(DEV)
    # echo without logprobs only prepends the prompt text: no scoring happens
    before = len(eng.prefix_cache)
    r = client.post("/v1/completions", json={"prompt": PROMPT, "echo": True, "max_tokens": 2, "temperature": 0.0,
                                             "ignore_eos": True})
    ch3 = r.json()["choices"][0]
    assert set(ch3) == {"index", "text", "finish_reason"} and ch3["text"] == eng.tokenizer.decode(PROMPT) + ch["text"]
    assert len(eng.prefix_cache) >= before


def test_http_max_tokens_zero_only_when_scoring(served):
    client, _ = served
    r = client.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 0, "temperature": 0.0})
    assert r.status_code == 200 and r.json()["usage"]["completion_tokens"] == 1  # today's max(1, ...) stays
    r = client.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 0, "prompt_logprobs": 0})
    assert r.status_code == 200 and r.json()["usage"]["completion_tokens"] == 0
    pl = r.json()["choices"][0]["prompt_logprobs"]
    assert pl[0] is None and [list(e) for e in pl[1:]] == [["2"], ["3"]] and all(math.isfinite(e[k]["logprob"]) for e in pl[1:] for k in e)


@pytest.mark.parametrize("body,name", [({"prompt_logprobs": 9}, "prompt_logprobs"), ({"prompt_logprobs": -1}, "prompt_logprobs"),
                                       ({"echo": True, "logprobs": 9}, "logprobs"), ({"echo": True, "logprobs": -1}, "logprobs"),
                                       ({"echo": True, "stream": True}, "echo"),
                                       ({"echo": True, "logprobs": 1, "stream": True}, "echo"),
                                       ({"prompt_logprobs": 1, "stream": True}, "prompt_logprobs")])
def test_http_refusals_are_400(served, body, name):
    client, _ = served
    r = client.post("/v1/completions", json=dict({"prompt": [1, 2, 3], "max_tokens": 2}, **body))
    assert r.status_code == 400 and name in r.json()["detail"], r.text


def test_http_tensor_parallel_is_400(served):
    client, eng = served
    eng.tp = 2  # the check itself: an engine that reports two ranks
    try:
        for body in ({"prompt_logprobs": 1}, {"echo": True, "logprobs": 1}):
            r = client.post("/v1/completions", json=dict({"prompt": [1, 2, 3], "max_tokens": 2}, **body))
            assert r.status_code == 400 and "prompt_logprobs" in r.json()["detail"] and "tensor parallelism" in r.json()["detail"]
        r = client.post("/v1/completions", json={"prompt": [1, 2, 3], "max_tokens": 2, "echo": True})
        assert r.status_code == 200  # echo alone scores nothing
    finally:
        eng.tp = 1
