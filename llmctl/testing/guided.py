"""Guided decoding (``ops.sample_guided``, ``llmctl/serve/guided.py``): the kernel tests' inputs and
the serving scenarios on the tiny model, shared by the CPU suite (the fp32 oracle behind ``ops``) and
the GPU suite (the HIP kernel, captured decode graphs, the asynchronous pipeline).  Every ``check_*``
function asserts its scenario on ``device``."""

from __future__ import annotations

import json
import math
import re
from typing import Dict, List, Optional

import torch

from llmctl.serve import guided
from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams, Sequence
from llmctl.testing.sampling_ext import ENGINE, MODES, PROMPTS, lp_tolerance  # noqa: F401  (re-exported)

# ----------------------------------------------------------------------------- kernel-test inputs
# table slots of the random arena: (states, classes) per slot -- the degenerate guide, two small
# ones, and the LDS edge C = 8192 with several states and with one
GUIDE_SHAPES = ((1, 1), (7, 2), (7, 300), (7, 8192), (1, 8192))
GUIDE_WORDS = 7 * 8192


def random_arena(V: int, gen: torch.Generator, shapes=GUIDE_SHAPES, words: int = GUIDE_WORDS):
    """Random well-formed guides built directly as tables (no regex): ``(cls [G, V], next [G, W],
    meta [G, 2])`` on the CPU.  About half of a state's classes are dead; every state allows at
    least one token that exists."""
    G = len(shapes)
    cls = torch.zeros(G, V, dtype=torch.int32)
    nxt = torch.full((G, words), -1, dtype=torch.int32)
    meta = torch.tensor(shapes, dtype=torch.int32)
    for g, (S, C) in enumerate(shapes):
        cls[g] = torch.randint(0, C, (V,), generator=gen, dtype=torch.int32)
        t = torch.randint(0, S, (S, C), generator=gen, dtype=torch.int32)
        t[torch.rand(S, C, generator=gen) < 0.5] = -1
        live = cls[g][torch.randint(0, V, (S,), generator=gen)].long()  # the class of some token, per state
        t[torch.arange(S), live] = torch.randint(0, S, (S,), generator=gen, dtype=torch.int32)
        nxt[g, :S * C] = t.reshape(-1)
    return cls, nxt, meta


def kernel_inputs(N: int, V: int, dtype=torch.bfloat16, seed: int = 0) -> Dict[str, torch.Tensor]:
    """The inputs of one ``sample_guided`` case, made on the CPU (the same on every machine): the
    sampling parameters and the sampler state of ``tests/kernels/test_sampling_ext.py`` (dyadic
    penalties, a third of the rows stateless, an eighth greedy) plus a random guide arena, a mix of
    guided and unguided rows (about a quarter unguided), rows sharing a guide at different states,
    and one distinct ``gslot`` per guided row out of N + 2."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * N + V)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    logits = (torch.randn(N, V, generator=gen) * 3).to(torch.bfloat16).to(dtype)
    temp = rnd(N) + 0.3
    temp[:(N + 7) // 8] = 0.0
    topk = torch.randint(0, 100, (N,), generator=gen, dtype=torch.int32)
    topp = rnd(N) * 0.6 + 0.4
    topp[::3] = 1.0
    S = N + 3
    slot = torch.randperm(S, generator=gen)[:N].to(torch.int32)
    slot[2::3] = -1
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (N,), generator=gen)]
    rep, freq, pres = pick([1.0, 2.0, 0.5]), pick([0.0, 0.25, 0.5, 1.0]), pick([0.0, 0.25, 0.5, 1.0])
    nlp = torch.tensor([0, 1, 5, 8], dtype=torch.int32).repeat((N + 3) // 4)[:N].contiguous()
    counts = (torch.randint(0, 9, (S, V), generator=gen) * (rnd(S, V) < 0.3)).to(torch.int32)
    mask = (rnd(S, V) < 0.2).to(torch.uint8)
    cls, nxt, meta = random_arena(V, gen)
    G = cls.shape[0]
    guide = torch.randint(0, G, (N,), generator=gen, dtype=torch.int32)
    guide[rnd(N) < 0.25] = -1
    if N >= 3:  # always: one unguided row, and two rows on one guide
        guide[1] = -1
        guide[2] = guide[0] = 2
    gslot = torch.randperm(N + 2, generator=gen)[:N].to(torch.int32)
    gslot[guide < 0] = -1
    state = torch.zeros(N + 2, dtype=torch.int32)
    for i in range(N):
        if guide[i] >= 0:
            state[gslot[i]] = int(torch.randint(0, int(meta[guide[i], 0]), (1,), generator=gen))
    return dict(logits=logits, temp=temp, topk=topk, topp=topp, u=rnd(N), slot=slot, rep=rep, freq=freq, pres=pres,
                nlp=nlp, counts=counts, mask=mask, guide=guide, gslot=gslot, cls=cls, next=nxt, meta=meta, state=state)


ARGS = ("logits", "temp", "topk", "topp", "u", "slot", "rep", "freq", "pres", "nlp", "counts", "mask", "guide",
        "gslot", "cls", "next", "meta", "state")


def call(fn, c: Dict[str, torch.Tensor], **kw):
    """``fn`` (``ops.sample_guided`` / ``ref.sample_guided`` / the native op) on a case; ``counts``
    and ``state`` of ``c`` are updated in place."""
    return fn(*(c[k] for k in ARGS), **kw)


def to_device(c: Dict[str, torch.Tensor], device) -> Dict[str, torch.Tensor]:
    return {k: v.to(device) for k, v in c.items()}


def single_guide(allowed: torch.Tensor, rows: int) -> Dict[str, torch.Tensor]:
    """One one-state guide that allows exactly the tokens of ``allowed`` (bool [V]), used by
    ``rows`` rows with a state word each: the ``guide`` .. ``state`` entries of a case."""
    V = allowed.numel()
    return dict(guide=torch.zeros(rows, dtype=torch.int32), gslot=torch.arange(rows, dtype=torch.int32),
                cls=allowed.to(torch.int32).view(1, V).contiguous(),
                next=torch.tensor([[-1, 0]], dtype=torch.int32), meta=torch.tensor([[1, 2]], dtype=torch.int32),
                state=torch.zeros(rows, dtype=torch.int32))


def neutral_case(logits: torch.Tensor, temp, topk: int, topp: float, u: torch.Tensor, allowed: torch.Tensor, nlp: int = 0):
    """A case without penalties: every row of ``logits`` under the one-state guide of ``allowed``."""
    N, V = logits.shape
    full = lambda v, dt: torch.full((N,), v, dtype=dt)
    temp = torch.as_tensor(temp, dtype=torch.float32).expand(N).contiguous()
    return dict(logits=logits, temp=temp, topk=full(topk, torch.int32), topp=full(topp, torch.float32), u=u,
                slot=full(-1, torch.int32), rep=full(1.0, torch.float32), freq=full(0.0, torch.float32),
                pres=full(0.0, torch.float32), nlp=full(nlp, torch.int32), counts=torch.zeros(1, V, dtype=torch.int32),
                mask=torch.zeros(1, V, dtype=torch.uint8), **single_guide(allowed, N))


# ----------------------------------------------------------------------------- serving scenarios
DATE = r"\d{4}-\d{2}-\d{2}"
CHOICES = ["yes", "no", "maybe"]
SCHEMA = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"}}}
# guides that cannot complete within 16 tokens (every request then ends by length at the same step)
LONG = (dict(guided_regex=r"[a-f]{30}\d+"), dict(guided_choice=["x" * 30, "xy" * 15, "z" * 40]),
        dict(guided_json={"type": "array", "items": {"type": "integer"}, "minItems": 20}))


def _engine(device: str, seed: int = 3, **kw) -> InferenceEngine:
    return InferenceEngine("tiny", device=device, seed=seed, **dict(ENGINE, **kw))


def _run(e: InferenceEngine, params: List[SamplingParams], prompts=PROMPTS) -> List[Sequence]:
    seqs = [e.add_request(p, sp) for p, sp in zip(prompts, params)]
    while any(s.status != "finished" for s in seqs):
        e.step()
    return seqs


def _conformance_params(temperature: float, guides: bool = True, lengths: Optional[List[int]] = None):
    """Regex, 3-way choice, 2-property schema and one unguided request (16 tokens).  Without
    ``guides``: the same batch composition, request ``i`` generating exactly ``lengths[i]`` tokens."""
    base = dict(temperature=temperature)
    if not guides:
        return [SamplingParams(max_tokens=n, ignore_eos=True, **base) for n in lengths]
    return [SamplingParams(max_tokens=64, guided_regex=DATE, **base),
            SamplingParams(max_tokens=64, guided_choice=CHOICES, **base),
            SamplingParams(max_tokens=64, guided_json=SCHEMA, **base),
            SamplingParams(max_tokens=16, ignore_eos=True, **base)]


def _pattern(sp: SamplingParams) -> str:
    return guided.constraint_regex(*guided.params_guide(sp))


def _check_outputs(e: InferenceEngine, seqs: List[Sequence]) -> None:
    """Every guided request that stopped is a full match ending with EOS (and, for a schema, parses
    to its types); one that ran out of tokens is a viable prefix."""
    eos = e.tokenizer.eos_token_id
    for s in seqs:
        if not s.params.guided:
            continue
        assert s.finish_reason in ("stop", "length"), s.finish_reason
        if s.finish_reason == "length":
            s.guide.walk(s.output_ids)  # raises on a token that was not allowed
            continue
        assert s.output_ids[-1] == eos and eos not in s.output_ids[:-1]
        assert s.guide.walk(s.output_ids) == s.guide.done
        text = bytes(s.output_ids[:-1]).decode("utf-8")
        assert re.fullmatch(_pattern(s.params), text), (text, _pattern(s.params))
        if s.params.guided_json is not None:
            v = json.loads(text)
            assert list(v) == ["ok", "n"] and isinstance(v["ok"], bool) and type(v["n"]) is int, v
        if s.params.guided_choice is not None:
            assert text in s.params.guided_choice


def check_conformance(device: str, temperature: float) -> None:
    with _engine(device) as e:
        seqs = _run(e, _conformance_params(temperature))
        _check_outputs(e, seqs)
        assert any(s.finish_reason == "stop" for s in seqs[:3])
        # the random-init model left alone matches nothing: the guides did the work
        plain = bytes(t for t in seqs[3].output_ids if t < 256).decode("utf-8", errors="replace")
        assert len(seqs[3].output_ids) == 16
        assert not any(re.fullmatch(_pattern(sp), plain[:n]) for sp in _conformance_params(temperature)[:3]
                       for n in range(len(plain) + 1))


def check_mode_equivalence(device: str, temperature: float) -> None:
    """Graphs + async, graphs, and eager give identical tokens, and the unguided request the tokens
    it gets in a batch of the same composition without guides.  Greedy: the conformance requests,
    which end with EOS at different steps.  With a temperature: guides that cannot complete within
    ``max_tokens``, so that all four requests end at the same step -- the engine draws one uniform
    per batch row and step, and the asynchronous pipeline's speculative row for a sequence that
    has just ended would shift the stream of the modes against each other."""
    if temperature <= 0:
        params = _conformance_params(temperature)
    else:
        base = dict(max_tokens=16, temperature=temperature, top_k=50, top_p=0.9)
        params = [SamplingParams(**base, **g) for g in LONG] + [SamplingParams(ignore_eos=True, **base)]
    runs = []
    for mode in MODES:
        with _engine(device, **mode) as e:
            seqs = _run(e, params)
            _check_outputs(e, seqs)
            if mode["perf_knobs"]["async_decode"]:
                assert e.stats.get("async_continued", 0) > 5, e.stats
            if e.use_graphs:
                assert e._graphs_guided and e.stats["graph_replays"] > 0
            else:
                assert not e._graphs_guided and not e._graphs
            runs.append([list(s.output_ids) for s in seqs])
    assert runs[0] == runs[1] == runs[2], runs
    if temperature > 0:
        assert all(len(o) == 16 for o in runs[0])
    with _engine(device, **MODES[0]) as e:
        sp = [SamplingParams(max_tokens=len(o), ignore_eos=True, temperature=temperature,
                             top_k=params[3].top_k, top_p=params[3].top_p) for o in runs[0]]
        plain = _run(e, sp)
        assert e._guide_arena is None and not e._graphs_guided
    assert plain[3].output_ids == runs[0][3]
    assert any(plain[i].output_ids != runs[0][i] for i in range(3))  # the guides did change the output


STAMP = r"\d{4}-\d{2}-\d{2}T\d{2}:\d{2}:\d{2}"  # 19 tokens: the 4th KV block is needed mid-pattern


def check_preemption(device: str) -> None:
    """Seven KV blocks for two guided sequences of a 40-token prompt: each holds three, and when
    both need a fourth -- nine tokens into the pattern -- one is preempted.  It gives up its state
    word and table reference, is pinned again when it resumes (state = the walk over what it has
    generated), and finishes with the ids of an undisturbed run."""
    base = [[(7 * i) % 200 + 1 for i in range(40)], [(11 * i) % 190 + 3 for i in range(40)]]
    p = SamplingParams(max_tokens=32, temperature=0.0, guided_regex=STAMP)
    with _engine(device, num_kv_blocks=7) as e:
        pins: Dict[int, int] = {}
        pin = e._pin_guide

        def counted(seq):
            pins[seq.seq_id] = pins.get(seq.seq_id, 0) + 1
            assert seq.guide_slot < 0 and seq.guide_table < 0
            pin(seq)

        e._pin_guide = counted
        seqs = _run(e, [p, p], base)
        _check_outputs(e, seqs)
        assert sum(s.preemptions for s in seqs) >= 1
        for s in seqs:
            assert s.finish_reason == "stop" and pins[s.seq_id] == 1 + s.preemptions
        assert sorted(e._sampler_free) == list(range(e.max_batch_size)) and not e._guide_tables
    with _engine(device) as e:
        ref = _run(e, [p, p], base)
        assert all(s.preemptions == 0 for s in ref)
    assert [s.output_ids for s in seqs] == [s.output_ids for s in ref]


def check_structure(device: str) -> None:
    """A run without guides allocates no arena and captures no guided graph; equal guides share a
    table slot; all slots return; close() drops the graphs and the arena."""
    e = _engine(device)
    _run(e, [SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True)] * 4)
    assert e._guide_arena is None and e._graphs_guided == {} and e._sampler_state is None
    graphs = dict(e._graphs)
    p = [SamplingParams(max_tokens=32, temperature=0.0, guided_regex=STAMP),
         SamplingParams(max_tokens=32, temperature=0.0, guided_regex=STAMP),
         SamplingParams(max_tokens=32, temperature=0.0, guided_choice=CHOICES)]
    seqs = [e.add_request(pr, sp) for pr, sp in zip(PROMPTS, p)]
    assert seqs[0].guide is seqs[1].guide and seqs[0].guide is not seqs[2].guide  # the compile cache
    while any(s.guide_slot < 0 for s in seqs):
        e.step()
    assert seqs[0].guide_table == seqs[1].guide_table >= 0 and seqs[2].guide_table not in (-1, seqs[0].guide_table)
    assert e._guide_tables[seqs[0].guide.key] == [seqs[0].guide_table, 2]
    assert len({s.guide_slot for s in seqs}) == 3
    while any(s.status != "finished" for s in seqs):
        e.step()
    _check_outputs(e, seqs)
    G = e.max_batch_size
    assert e._guide_arena is not None and e._sampler_state is None  # no penalized request: no counts
    assert sorted(e._sampler_free) == list(range(G)) and sorted(e._guide_table_free) == list(range(G))
    assert e._guide_tables == {} and all(s.guide_slot == s.guide_table == -1 for s in seqs)
    assert dict(e._graphs) == graphs  # the plain graphs are the ones captured before
    if e.use_graphs:
        assert e._graphs_guided and graphs and not e._graphs_ext
    e.close()
    assert e._graphs == {} and e._graphs_guided == {} and e._guide_arena is None


def check_composition(device: str, tol: float) -> None:
    """A guided request with logprobs = 3 and a presence penalty beside an unguided one: the top
    lists hold only allowed tokens, their probabilities sum to at most 1 (to exactly 1 when no more
    than three tokens are allowed), and the token's logprob is its entry in the list."""
    with _engine(device) as e:
        sp = SamplingParams(max_tokens=48, temperature=0.8, guided_json=SCHEMA, logprobs=3, presence_penalty=0.5)
        seqs = _run(e, [sp, SamplingParams(max_tokens=24, temperature=0.8, ignore_eos=True)], PROMPTS[:2])
        _check_outputs(e, seqs)
        assert e._sampler_state is not None and sorted(e._sampler_free) == list(range(e.max_batch_size))
    s = seqs[0]
    g, st = s.guide, s.guide.start
    assert len(s.output_logprobs) == len(s.output_top_logprobs) == len(s.output_ids)
    for tok, lp, top in zip(s.output_ids, s.output_logprobs, s.output_top_logprobs):
        allowed = g.allowed(st)
        n = int(allowed.sum())
        assert len(top) == min(3, n) and all(allowed[t] for t, _ in top), (st, top)
        # every logprob is within tol of the exact one, so every exp() within a factor e^tol
        mass = sum(math.exp(v) for _, v in top)
        assert mass <= 1 + 2 * tol and (n > 3 or abs(mass - 1) <= 2 * tol), (mass, n)
        assert allowed[tok] and lp <= tol and math.isfinite(lp)
        for t, v in top:
            if t == tok:
                assert v == lp
        assert all(a[1] >= b[1] for a, b in zip(top, top[1:]))
        st = g.step(st, tok)


def check_lora_composition(device: str) -> None:
    """A guided request on a LoRA adapter beside a guided request on the base model: both conform,
    and on the graph path the step replays the LoRA family's guided graph."""
    from llmctl.serve.lora import random_adapter

    with _engine(device, max_loras=1, max_lora_rank=16) as e:
        e.load_lora("tuned", random_adapter(e.cfg, rank=16, seed=5, std=0.05))
        p = [SamplingParams(max_tokens=32, temperature=0.0, guided_regex=STAMP, lora="tuned"),
             SamplingParams(max_tokens=32, temperature=0.0, guided_regex=STAMP)]
        seqs = _run(e, p, PROMPTS[:2])
        _check_outputs(e, seqs)
        assert all(s.finish_reason == "stop" for s in seqs)
        if e.use_graphs:
            assert any(kind == 2 for _, kind in e._graphs_lora) and not e._graphs_guided
        assert sorted(e._sampler_free) == list(range(e.max_batch_size)) and not e._guide_tables
