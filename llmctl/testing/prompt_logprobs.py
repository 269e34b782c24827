"""Serving scenarios of prompt scoring (``SamplingParams.prompt_logprobs``: ``ops.prompt_logprobs``
in the prefill pass) on the tiny model, shared by the CPU suite (the fp64 oracle behind ``ops``) and
the GPU suite (``csrc/prompt_logprobs.hip`` behind the prefill and mixed steps).  Every function
asserts its scenario on ``device``.

The oracle uses none of the scoring code: a CPU fp32 engine on the shared model
(``llmctl.testing.lora``) is given a prompt's first token and teacher-forced through the rest with an
instance-level ``sample`` override that records every position's logits; fp64 ``log_softmax`` of those
is what the scores are compared with."""

from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional

import torch

from llmctl.serve.lora import merge_into
from llmctl.serve.scheduler import SamplingParams, Sequence
from llmctl.testing import lora as tl

ENGINE = tl.ENGINE


def _prompt(n: int, k: int) -> List[int]:
    return [(k * i * i + 3 * i + k) % 250 + 1 for i in range(n)]


PROMPTS = [_prompt(2, 1), _prompt(5, 2), _prompt(37, 3), _prompt(70, 4)]  # the lengths of testing.lora.PROMPTS
TOPS = [None, 0, 1, 8]  # prompt_logprobs of each request of the batch
GEN = 4

_CACHE: Dict = {}


def engine(device: str, **kw):
    return tl.engine(device, loras=kw.pop("loras", ()), **kw)


def forced_logprobs(eng, prompts: List[List[int]], lora: Optional[str] = None) -> List[torch.Tensor]:
    """Per prompt the fp64 log-softmax ``[len - 1, V]`` of the logits at positions 0 .. len - 2, from
    ``eng`` started on the prompt's first token and teacher-forced through the rest (parent code
    only: the decode path and an instance-level ``sample`` override, as ``testing.lora.run_forced``)."""
    todo = [i for i, p in enumerate(prompts) if len(p) > 1]
    seqs = {i: eng.add_request(prompts[i][:1], SamplingParams(max_tokens=len(prompts[i]) - 1, temperature=0.0,
                                                               ignore_eos=True, lora=lora)) for i in todo}
    idx = {s.seq_id: i for i, s in seqs.items()}
    rec: Dict[int, List[torch.Tensor]] = {i: [] for i in todo}

    def sample(logits, batch):
        out = []
        for row, s in zip(logits.float().cpu(), batch):
            i = idx[s.seq_id]
            rec[i].append(row)
            out.append(prompts[i][1 + len(s.output_ids)])
        return out

    eng.sample = sample
    try:
        while any(s.status != "finished" for s in seqs.values()):
            eng.step()
    finally:
        del eng.sample
    V = eng.cfg.vocab_size
    return [torch.log_softmax(torch.stack(rec[i]).double(), dim=-1) if i in rec else torch.zeros(0, V, dtype=torch.float64)
            for i in range(len(prompts))]


def oracle(prompts=PROMPTS, key: str = "oracle") -> List[torch.Tensor]:
    """The CPU fp32 engine's teacher-forced log-softmax of ``prompts``, once per process."""
    if key not in _CACHE:
        with engine("cpu") as e:
            _CACHE[key] = forced_logprobs(e, prompts)
    return _CACHE[key]


def _target_err(lps: List[torch.Tensor], want: List[torch.Tensor], prompts) -> float:
    err = 0.0
    for a, b, p in zip(lps, want, prompts):
        t = torch.tensor(p[1:]).view(-1, 1)
        if len(p) > 1:
            err = max(err, (a.gather(1, t) - b.gather(1, t)).abs().max().item())
    return err


def bound(device: str) -> float:
    """What a prompt logprob may differ from the oracle's by.  CPU: ``testing.lora.CPU_TOL`` (the same
    fp32 oracle under two summation orders).  GPU: measured here, once per process: 2 x the error of
    the GPU engine teacher-forced through its decode path, against the CPU oracle, on the prompt
    tokens' logprobs (prefill and decode kernels are two bf16 routes to the same fp32 truth)."""
    if device == "cpu":
        return tl.CPU_TOL
    if ("bound", device) not in _CACHE:
        want = oracle()
        with engine(device) as e:
            got = forced_logprobs(e, PROMPTS)
        err = _target_err(got, want, PROMPTS)
        print(f"prompt logprobs: err_base ({device} engine teacher-forced vs CPU fp32 oracle, prompt tokens) {err:.3e}, "
              f"bound {2 * err:.3e}")
        assert 0 < err < 3e-2, err
        _CACHE[("bound", device)] = 2 * err
    return _CACHE[("bound", device)]


def _params(top: Optional[int], max_tokens: int = GEN, **kw) -> SamplingParams:
    return SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, prompt_logprobs=top, **kw)


def _run(e, prompts, params: List[SamplingParams], **kw) -> List[Sequence]:
    seqs = [e.add_request(p, sp, **kw) for p, sp in zip(prompts, params)]
    while any(s.status != "finished" for s in seqs):
        e.step()
    return seqs


def check_seq(seq: Sequence, want: torch.Tensor, tol: float, top: Optional[int], what: str = "") -> float:
    """One sequence's lists against the oracle's log-softmax ``want [len - 1, V]``: lengths, entry 0,
    the logprobs and every listed alternative within ``tol``, lists descending and of length ``top``,
    rank consistent with the list.  Returns the largest logprob error."""
    P = len(seq.prompt_ids)
    if top is None:
        assert seq.prompt_logprobs == [] and seq.prompt_ranks == [] and seq.prompt_top_logprobs == [], what
        return 0.0
    assert len(seq.prompt_logprobs) == len(seq.prompt_ranks) == len(seq.prompt_top_logprobs) == P, (
        what, P, len(seq.prompt_logprobs))
    assert seq.prompt_logprobs[0] is None and seq.prompt_ranks[0] is None and seq.prompt_top_logprobs[0] is None, what
    err = 0.0
    for i in range(1, P):
        tok, lp, rank, lst = seq.prompt_ids[i], seq.prompt_logprobs[i], seq.prompt_ranks[i], seq.prompt_top_logprobs[i]
        assert math.isfinite(lp) and lp <= 0, (what, i, lp)
        err = max(err, abs(lp - want[i - 1, tok].item()))
        assert len(lst) == min(top, want.shape[1]), (what, i, lst)
        assert all(a[1] >= b[1] for a, b in zip(lst, lst[1:])), (what, i, lst)
        assert len({t for t, _ in lst}) == len(lst), (what, i, lst)
        for t, v in lst:
            err = max(err, abs(v - want[i - 1, t].item()))
        assert rank >= 1
        listed = [t for t, _ in lst]
        assert (rank <= len(lst)) == (tok in listed), (what, i, rank, listed)
        if tok in listed:
            assert listed[rank - 1] == tok and lst[rank - 1][1] == lp, (what, i)
    assert err <= tol, (what, err, tol)
    return err


def _close(a: Sequence, b: Sequence, tol: float) -> None:
    """Two runs of one request agree (``tol`` 0: exactly)."""
    assert len(a.prompt_logprobs) == len(b.prompt_logprobs)
    assert a.prompt_logprobs[:1] == b.prompt_logprobs[:1]
    for x, y in zip(a.prompt_logprobs[1:], b.prompt_logprobs[1:]):
        assert abs(x - y) <= tol, (x, y, tol)
    if tol == 0:
        assert a.prompt_ranks == b.prompt_ranks and a.prompt_top_logprobs == b.prompt_top_logprobs


def baseline(device: str) -> List[Sequence]:
    """Scenario 1's scored batch (one prefill step for all four prompts), once per process and device."""
    if ("base", device) not in _CACHE:
        with engine(device) as e:
            _CACHE[("base", device)] = _run(e, PROMPTS, [_params(t) for t in TOPS])
    return _CACHE[("base", device)]


# ------------------------------------------------------------------------------------- scenarios
def check_concurrent(device: str) -> None:
    """1. Four concurrent requests with prompt_logprobs None, 0, 1 and 8."""
    want, tol = oracle(), bound(device)
    seqs = baseline(device)
    for s, w, t in zip(seqs, want, TOPS):
        err = check_seq(s, w, tol, t, f"len {len(s.prompt_ids)} top {t}")
        print(f"concurrent on {device}: prompt of {len(s.prompt_ids)}, top {t}: err {err:.3e} (bound {tol:.3e})")
        assert len(s.output_ids) == GEN and s.finish_reason == "length"
    seen = []

    def on_token(seq, tok):  # complete before the first generated token is appended
        if len(seq.output_ids) == 1:
            seen.append(len(seq.prompt_logprobs))

    with engine(device) as e:
        plain = _run(e, PROMPTS, [_params(None) for _ in TOPS])
        assert e._score_scratch is None
        again = _run(e, PROMPTS, [_params(t) for t in TOPS], on_token=on_token)
        assert e._score_scratch is not None and tuple(e._score_scratch.shape) == (e.SCORE_TILE, e.cfg.vocab_size)
    assert [s.output_ids for s in plain] == [s.output_ids for s in seqs] == [s.output_ids for s in again]
    assert seen == [len(p) if t is not None else 0 for p, t in zip(PROMPTS, TOPS)], seen
    assert e._score_scratch is None  # close() releases the scratch


def check_chunked(device: str) -> None:
    """2. max_batch_tokens = 16: chunk boundaries inside prompts and on a block edge."""
    want, tol = oracle(), bound(device)
    with engine(device, max_batch_tokens=16) as e:
        seqs = _run(e, PROMPTS, [_params(t) for t in TOPS])
        assert e.stats["steps"] > 8
    for s, b, w, t in zip(seqs, baseline(device), want, TOPS):
        check_seq(s, w, tol, t, f"chunked len {len(s.prompt_ids)}")
        assert len(s.output_ids) == GEN
        if device == "cpu":  # (bf16: chunked and whole prefill are two attention kernels)
            assert s.output_ids == b.output_ids
        if t is not None:
            _close(s, b, tol)


def check_mixed(device: str) -> None:
    """3. A scoring request admitted while others decode: its chunks ride in mixed steps."""
    want, tol = oracle(), bound(device)
    with engine(device, max_batch_tokens=24, perf_knobs={"async_decode": False}) as e:
        others = [e.add_request(p, _params(None, max_tokens=12)) for p in PROMPTS[:2]]
        for _ in range(3):
            e.step()
        assert all(len(s.output_ids) >= 2 for s in others)
        late = [e.add_request(PROMPTS[3], _params(8)), e.add_request(PROMPTS[2], _params(1))]
        while any(s.status != "finished" for s in others + late):
            e.step()
        assert e.stats.get("mixed_steps", 0) >= 3
    check_seq(late[0], want[3], tol, 8, "mixed 70")
    check_seq(late[1], want[2], tol, 1, "mixed 37")
    _close(late[0], baseline(device)[3], tol)


def check_score_only(device: str) -> None:
    """4. max_tokens = 0: scored, nothing generated, finished with "length"; ``score()``."""
    want, tol = oracle(), bound(device)
    with engine(device) as e:
        seqs = e.score(PROMPTS + [[5]], top=2)
        for s, w in zip(seqs[:4], want):
            assert s.output_ids == [] and s.finish_reason == "length" and s.status == "finished"
            check_seq(s, w, tol, 2, "score-only")
        one = seqs[4]
        assert one.output_ids == [] and one.finish_reason == "length"
        assert one.prompt_logprobs == [None] and one.prompt_ranks == [None] and one.prompt_top_logprobs == [None]
        assert e.kv.num_free_blocks + (len(e.prefix_cache) if e.prefix_cache is not None else 0) == ENGINE["num_kv_blocks"]
        for bad in (dict(max_tokens=0), dict(prompt_logprobs=9), dict(prompt_logprobs=-1)):
            try:
                SamplingParams(**bad)
                raise AssertionError(f"no refusal: {bad}")
            except ValueError as ex:
                assert "prompt_logprobs" in str(ex), ex


def check_prefix_cache(device: str) -> None:
    """5. A scoring request computes every position (no entries missing for cached blocks), publishes
    its blocks, and a plain request on the same prompt then hits them."""
    want, tol = oracle(), bound(device)
    with engine(device) as e:
        first, = e.score([PROMPTS[3]], top=3)
        assert len(e.prefix_cache) >= len(PROMPTS[3]) // ENGINE["block_size"]
        second, = e.score([PROMPTS[3]], top=3)
        assert first.cached_tokens == 0 and second.cached_tokens == 0
        assert e.stats.get("prefix_hit_tokens", 0) == 0 and e.prefix_cache.stats["hit_tokens"] == 0
        check_seq(first, want[3], tol, 3, "first")
        check_seq(second, want[3], tol, 3, "second")
        _close(first, second, 0.0 if device == "cpu" else tol)
        plain, = _run(e, [PROMPTS[3]], [_params(None)])
        assert plain.cached_tokens == 64 and e.stats["prefix_hit_tokens"] == 64
        # a scoring request that also generates: same tokens as the plain one (which used the cache)
        both, = _run(e, [PROMPTS[3]], [_params(0)])
        assert both.cached_tokens == 0 and len(both.prompt_logprobs) == len(PROMPTS[3])
        if device == "cpu":  # (bf16: the cached and the fresh prefill are two attention kernels)
            assert both.output_ids == plain.output_ids


def check_preemption(device: str) -> None:
    """6. Preempted mid-prefill (with and without the prefix cache) and, under a KV budget that forces
    it, mid-decode: the lists are complete, nothing is scored twice, the values are the oracle's."""
    want, tol = oracle(), bound(device)
    for prefix_caching in (True, False):
        with engine(device, max_batch_tokens=16, prefix_caching=prefix_caching) as e:
            seq = e.add_request(PROMPTS[3], _params(8))
            for _ in range(3):
                e.step()
            assert seq.num_computed == 48 and len(seq.prompt_logprobs) == 49
            kept = list(seq.prompt_logprobs)
            e.scheduler._preempt(seq)
            while seq.status != "finished":
                e.step()
            assert seq.preemptions == 1 and seq.prompt_logprobs[:49] == kept
            assert seq.cached_tokens == (48 if prefix_caching else 0)
        check_seq(seq, want[3], tol, 8, f"preempted mid-prefill, prefix cache {prefix_caching}")
        assert len(seq.output_ids) == GEN
        if device == "cpu":
            assert seq.output_ids == baseline(device)[3].output_ids
    # 8 blocks of 16: both 37-token requests are admitted (3 blocks each) and grow to 5 blocks each
    with engine(device, num_kv_blocks=8, perf_knobs={"async_decode": False}) as e:
        seqs = _run(e, [PROMPTS[2], PROMPTS[2][:36] + [77]], [_params(8, max_tokens=40), _params(8, max_tokens=40)])
        assert sum(s.preemptions for s in seqs) >= 1
    check_seq(seqs[0], want[2], tol, 8, "KV budget, first")
    assert len(seqs[1].prompt_logprobs) == 37 and all(len(s.output_ids) == 40 for s in seqs)
    for a, b in zip(seqs[1].prompt_logprobs[1:36], seqs[0].prompt_logprobs[1:36]):
        assert abs(a - b) <= tol


def check_interactions(device: str) -> None:
    """7. Penalties and a guide never touch prompt logprobs; an adapter's rows are scored under it."""
    want, tol = oracle(), bound(device)
    exact = 0.0 if device == "cpu" else tol
    with engine(device, loras=("a",)) as e:
        plain, = _run(e, [PROMPTS[2]], [_params(8)])
        pen, = _run(e, [PROMPTS[2]], [_params(8, repetition_penalty=1.8, presence_penalty=1.0, frequency_penalty=0.5,
                                              logprobs=2)])
        guided, = _run(e, [PROMPTS[2]], [SamplingParams(max_tokens=GEN, temperature=0.0, prompt_logprobs=8,
                                                        guided_regex=r"\d{8}")])
        lora, = _run(e, [PROMPTS[2]], [_params(8, lora="a")])
    check_seq(plain, want[2], tol, 8, "plain")
    for other in (pen, guided):
        _close(other, plain, exact)
    assert len(pen.output_logprobs) == GEN
    if "lora_a" not in _CACHE:
        merged = merge_into(copy.deepcopy(tl._model()[0]), tl.adapter("a"))
        with tl.engine("cpu", model=merged, loras=()) as e:
            _CACHE["lora_a"] = forced_logprobs(e, [PROMPTS[2]])[0]
    ltol = tl.bound(device)
    err = max(abs(lp - _CACHE["lora_a"][i, tok].item())
              for i, (tok, lp) in enumerate(zip(lora.prompt_ids[1:], lora.prompt_logprobs[1:])))
    move = max(abs(a - b) for a, b in zip(lora.prompt_logprobs[1:], plain.prompt_logprobs[1:]))
    print(f"adapter a on {device}: prompt logprobs vs merged oracle {err:.3e} (bound {ltol:.3e}), vs base {move:.3e}")
    assert err <= ltol, (err, ltol)
    assert move > 2 * ltol, move  # the adapter was applied


def check_folded(device: str) -> None:
    """(GPU) The folded prefill (RMSNorms folded into the projections: a model whose shapes fit it
    and a 256-token prompt) hands the scoring rows its residual stream: same oracle, same bound."""
    import dataclasses

    from llmctl.models import build_model, get_model_config
    from llmctl.serve.engine import InferenceEngine

    cfg = dataclasses.replace(get_model_config("tiny"), ffn=768)
    model = build_model(cfg, device="cpu", dtype=torch.float32, seed=5)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.bfloat16().float())

    class FoldableEngine(InferenceEngine):
        def _load(self, model_path, dtype, seed):
            return copy.deepcopy(model).to(device=self.device, dtype=dtype), cfg, None

    prompt = [_prompt(256, 5)]
    with FoldableEngine("tiny", device="cpu", seed=3, **ENGINE) as e:
        want = forced_logprobs(e, prompt)[0]
    # the bound by the rule of :func:`bound`, measured on this model and this prompt
    with FoldableEngine("tiny", device=device, seed=3, **ENGINE) as e:
        err_base = _target_err(forced_logprobs(e, prompt), [want], prompt)
    print(f"folded model: err_base ({device} engine teacher-forced vs CPU fp32 oracle, prompt tokens) {err_base:.3e}")
    assert 0 < err_base < 3e-2, err_base
    tol = 2 * err_base
    for fold in (True, False):
        with FoldableEngine("tiny", device=device, seed=3, perf_knobs={"prefill_norm_fold": fold}, **ENGINE) as e:
            assert (e._nf is not None) == fold and e._norm_fold_ok(256) == fold
            seq, = e.score(prompt, top=8)
        err = check_seq(seq, want, tol, 8, f"fold {fold}")
        print(f"folded prefill {fold} on {device}: 256-token prompt err {err:.3e} (bound {tol:.3e})")


def check_tp_refusal(device: str) -> None:
    """8. Tensor parallelism > 1 refuses the field by name (the check itself: a TP = 1 engine that
    reports two ranks)."""
    with engine(device) as e:
        e.tp = 2
        try:
            e.add_request([1, 2, 3], _params(1))
            raise AssertionError("no refusal at TP = 2")
        except ValueError as ex:
            assert "prompt_logprobs" in str(ex) and "tensor parallelism" in str(ex), ex
        assert not e.scheduler.has_work()
        e.tp = 1
