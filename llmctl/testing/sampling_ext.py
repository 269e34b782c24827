"""Serving scenarios of the extended sampler (penalties, logprobs: ``ops.sample_ext``) on the tiny
model, shared by the CPU suite (the fp32 oracle behind ``ops``) and the GPU suite (the HIP kernel,
captured decode graphs, the asynchronous pipeline).  Every function asserts its scenario on
``device``."""

from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams, Sequence

ENGINE = dict(max_batch_size=4, num_kv_blocks=128, block_size=16, max_model_len=512)
PROMPTS = [[1, 2, 3, 4, 5], [9] * 37, [7, 7], [3] * 70]

# graphs + the asynchronous pipeline, graphs with a host read per step, no graphs
MODES = (dict(use_graphs=True, perf_knobs={"async_decode": True}),
         dict(use_graphs=True, perf_knobs={"async_decode": False}),
         dict(use_graphs=False, perf_knobs={"async_decode": True}))


def lp_tolerance(device: str) -> float:
    """4 x the max abs error of torch's fp32 ``log_softmax`` on ``device`` against fp64, on
    ``randn * 3`` logits of 64 x 32000: the margin the kernel's logprobs get against the oracle."""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(64, 32000, generator=g) * 3).to(device)
    err = (torch.log_softmax(x, dim=-1).double() - torch.log_softmax(x.double(), dim=-1)).abs().max().item()
    assert err > 0
    return 4 * err


def _engine(device: str, seed: int = 3, **kw) -> InferenceEngine:
    return InferenceEngine("tiny", device=device, seed=seed, **dict(ENGINE, **kw))


def _run(e: InferenceEngine, params: List[SamplingParams], prompts=PROMPTS) -> List[Sequence]:
    seqs = [e.add_request(p, sp) for p, sp in zip(prompts, params)]
    while any(s.status != "finished" for s in seqs):
        e.step()
    return seqs


def check_distinct_tokens(device: str) -> None:
    """A huge presence (frequency) penalty under greedy decoding never repeats a token."""
    for field in ("presence_penalty", "frequency_penalty"):
        with _engine(device) as e:
            p = SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True, **{field: 1e4})
            for s in _run(e, [p, p], PROMPTS[:2]):
                assert len(s.output_ids) == 24 and len(set(s.output_ids)) == 24, (field, s.output_ids)
            plain = _run(e, [SamplingParams(max_tokens=24, temperature=0.0, ignore_eos=True)], PROMPTS[:1])[0]
            assert len(set(plain.output_ids)) < 24  # the tiny model does repeat itself when left alone


def _mixed_params(temperature: float, extended: bool = True) -> List[SamplingParams]:
    base = dict(max_tokens=16, temperature=temperature, top_k=50, top_p=0.9, ignore_eos=True)
    if not extended:
        return [SamplingParams(**base) for _ in range(4)]
    return [SamplingParams(presence_penalty=0.5, frequency_penalty=0.25, logprobs=5, **base), SamplingParams(**base),
            SamplingParams(repetition_penalty=2.0, logprobs=2, **base), SamplingParams(**base)]


def check_mode_equivalence(device: str, temperature: float, tol: float) -> None:
    """Four concurrent requests -- two extended with different parameters, two plain -- give the
    same tokens, top ids and (within ``tol``) logprobs in every engine mode, and the plain
    requests the tokens of a run without extended requests.  (That run is the two plain requests
    alone under greedy decoding; with a temperature it is the same four requests all plain,
    because the engine draws one uniform per batch row and step: a plain request keeps its
    uniforms only in a batch of the same composition.)"""
    runs = []
    for mode in MODES:
        with _engine(device, **mode) as e:
            seqs = _run(e, _mixed_params(temperature))
            if e.use_graphs:
                assert e._graphs_ext and e.stats["graph_replays"] > 0
                if mode["perf_knobs"]["async_decode"]:
                    assert e.stats.get("async_continued", 0) > 5
            else:
                assert not e._graphs_ext and not e._graphs
            runs.append(seqs)
    first = runs[0]
    for s, sp in zip(first, _mixed_params(temperature)):
        n = len(s.output_ids)
        assert n == 16
        if sp.logprobs is None:
            assert s.output_logprobs == [] and s.output_top_logprobs == []
        else:
            assert len(s.output_logprobs) == len(s.output_top_logprobs) == n
            assert all(len(t) == sp.logprobs for t in s.output_top_logprobs)
    for other in runs[1:]:
        for a, b in zip(first, other):
            assert a.output_ids == b.output_ids
            assert [[i for i, _ in t] for t in a.output_top_logprobs] == [[i for i, _ in t] for t in b.output_top_logprobs]
            for x, y in zip(a.output_logprobs, b.output_logprobs):
                assert abs(x - y) <= tol, (x, y, tol)
            for ta, tb in zip(a.output_top_logprobs, b.output_top_logprobs):
                assert all(abs(x - y) <= tol for (_, x), (_, y) in zip(ta, tb))
    with _engine(device, **MODES[0]) as e:
        if temperature <= 0:
            plain = _run(e, _mixed_params(temperature, extended=False)[:2], [PROMPTS[1], PROMPTS[3]])
        else:
            allp = _run(e, _mixed_params(temperature, extended=False))
            plain = [allp[1], allp[3]]
        assert not e._graphs_ext and e._sampler_state is None
    assert [s.output_ids for s in plain] == [first[1].output_ids, first[3].output_ids]
    # the extended requests did change what is generated
    with _engine(device, **MODES[0]) as e:
        allp = _run(e, _mixed_params(temperature, extended=False))
    assert allp[0].output_ids != first[0].output_ids or allp[2].output_ids != first[2].output_ids


def check_preemption(device: str) -> None:
    """An extended sequence preempted mid-generation gives up its state slot, gets one back --
    initialised from its prompt and the tokens generated so far -- when it resumes, and finishes
    with the ids of an undisturbed run."""
    base = [(7 * i) % 200 + 1 for i in range(40)]
    p = SamplingParams(max_tokens=20, temperature=0.0, ignore_eos=True, presence_penalty=1.0, repetition_penalty=1.5,
                       logprobs=2)
    # synchronous decode: the scheduler state is read between steps
    with _engine(device, perf_knobs={"async_decode": False}) as e:
        seq = e.add_request(base, p)
        for _ in range(9):
            e.step()
        assert len(seq.output_ids) == 9 and seq.sampler_slot >= 0
        e.scheduler._preempt(seq)
        assert seq.sampler_slot == -1 and len(e._sampler_free) == e.max_batch_size
        while seq.status != "finished":
            e.step()
        assert seq.preemptions == 1 and len(seq.output_logprobs) == len(seq.output_ids) == 20
    with _engine(device, perf_knobs={"async_decode": False}) as e:
        ref = _run(e, [p], [base])[0]
    assert seq.output_ids == ref.output_ids
    assert [[i for i, _ in t] for t in seq.output_top_logprobs] == [[i for i, _ in t] for t in ref.output_top_logprobs]


def check_structure(device: str) -> None:
    """Plain batches never touch the extended machinery; slots all return; close() drops both
    graph dicts and the state."""
    e = _engine(device)
    _run(e, _mixed_params(0.0, extended=False))
    assert e._graphs_ext == {} and e._sampler_state is None
    graphs = dict(e._graphs)
    _run(e, _mixed_params(0.0))
    assert e._sampler_state is not None and sorted(e._sampler_free) == list(range(e.max_batch_size))
    assert dict(e._graphs) == graphs  # the plain graphs are the ones captured before
    if e.use_graphs:
        assert e._graphs_ext and graphs
    e.close()
    assert e._graphs == {} and e._graphs_ext == {} and e._sampler_state is None


def check_logprob_fields(device: str, tol: float) -> None:
    """Greedy, neutral penalties, logprobs = 5: the chosen token heads its top list with the same
    logprob, and the lists are descending."""
    with _engine(device) as e:
        p = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, logprobs=5)
        seqs = _run(e, [p, p], PROMPTS[:2])
        assert e._sampler_state is not None and len(e._sampler_free) == e.max_batch_size  # no slot needed
        plain = _run(e, [SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)] * 2, PROMPTS[:2])
    for s, q in zip(seqs, plain):
        assert s.output_ids == q.output_ids  # logprobs alone change no token
        for tok, lp, top in zip(s.output_ids, s.output_logprobs, s.output_top_logprobs):
            assert len(top) == 5 and top[0][0] == tok and top[0][1] == lp and lp <= 0 and math.isfinite(lp)
            assert all(a[1] >= b[1] for a, b in zip(top, top[1:]))
