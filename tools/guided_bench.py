#!/usr/bin/env python3
"""Guided decoding (``ops.sample_guided``, ``llmctl/serve/guided.py``):

1. the op alone at N = 1 and 16 rows x V = 32000 bf16 logits (T = 0.8, top-k 50, top-p 0.9,
   every row penalized, 5 top logprobs): ``sample_guided`` with every row guided (a date regex
   over a synthetic 32k-token vocabulary, one shared table, a state word per row) and with no row
   guided, against ``sample_ext`` on the same inputs.  Device events around ``--iters`` back-to-back
   launches, ``--reps`` times per variant, alternated; the median is reported.  Guided minus
   extended is the feature's cost;
2. a GPT-7B decode step of 16 sequences x ``--ctx`` tokens of context on the captured plain,
   extended and guided graphs (captured by serving the batch through the engine, then replayed back
   to back, timed like the op);
3. guide compilation on the host (no GPU needed: ``--compile-only``): a date regex, a 3-property
   schema and a 50-way choice against the byte tokenizer and the synthetic 32k vocabulary; cold
   (the tokenizer's bytes are known, the guide is not cached) and from the cache.

    python tools/guided_bench.py [--iters 200] [--reps 5] [--ctx 2048] [--model gpt-7b] [--compile-only] [--skip-step]
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl.serve import guided
from llmctl.serve.tokenizer import ByteTokenizer

DEV = "cuda"
V = 32000
DATE = r"\d{4}-\d{2}-\d{2}"
SCHEMA = {"type": "object", "properties": {"name": {"type": "string", "maxLength": 32}, "age": {"type": "integer"},
                                           "tags": {"type": "array", "items": {"enum": ["a", "b", "c"]}, "maxItems": 4}}}
CHOICES = [f"option-{i:02d}-{'xyz'[i % 3] * (i % 5 + 1)}" for i in range(50)]
LONG = r"[a-z0-9 ]{64,}"  # cannot complete within the timed steps


class SyntheticTokenizer:
    """32k tokens: the 256 bytes, then common two-character pieces, then random 3..8-character
    pieces of lowercase letters / digits / punctuation (a third with a leading space); EOS last."""
    eos_token_id = V - 1

    def __init__(self):
        rng = random.Random(0)
        seen = {bytes([i]) for i in range(256)}
        toks = [bytes([i]) for i in range(256)]
        alpha = "abcdefghijklmnopqrstuvwxyz0123456789 -:,.\"{}[]_"
        for a in alpha:
            for b in alpha:
                toks.append((a + b).encode())
                seen.add(toks[-1])
        while len(toks) < V - 1:
            w = "".join(rng.choice(alpha[:36] if rng.random() < 0.9 else alpha) for _ in range(rng.randint(3, 8)))
            t = ((" " if rng.random() < 0.33 else "") + w).encode()
            if t not in seen:
                seen.add(t)
                toks.append(t)
        self._toks = toks + [None]

    def token_bytes(self):
        return self._toks


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, reps):
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(r, scale=1e3):
    return f"{r[0] * scale:7.1f} ({r[1] * scale:.1f}-{r[2] * scale:.1f})"


@torch.inference_mode()
def bench_op(iters, reps):
    from llmctl import ops

    g = guided.compile_guide("regex", DATE, SyntheticTokenizer(), V)
    S, C = g.next.shape
    print(f"# 1. the op, V = {V}, bf16 logits, T = 0.8 / top-k 50 / top-p 0.9, penalties + 5 logprobs; guide: {DATE} "
          f"({S} states x {C} classes); us per launch, median (min-max) of {reps} x {iters} launches, alternated")
    print("# rows | sample_ext        | sample_guided, no row guided | sample_guided, all rows guided | guided - ext")
    for N in (1, 16):
        torch.manual_seed(0)
        logits = (torch.randn(N, V, device=DEV) * 3).to(torch.bfloat16)
        f = lambda v, dt=torch.float32: torch.full((N,), v, dtype=dt, device=DEV)
        base = (logits, f(0.8), f(50, torch.int32), f(0.9), torch.rand(N, device=DEV))
        counts = (torch.randint(0, 9, (N, V), device=DEV) * (torch.rand(N, V, device=DEV) < 0.02)).to(torch.int32)
        ext = (torch.arange(N, dtype=torch.int32, device=DEV), f(1.25), f(0.25), f(0.5), f(5, torch.int32), counts,
               (torch.rand(N, V, device=DEV) < 0.05).to(torch.uint8))
        cls = torch.from_numpy(g.cls).to(DEV).view(1, V).contiguous()
        nxt = torch.from_numpy(g.next.reshape(1, -1)).to(DEV).contiguous()
        meta = torch.tensor([[S, C]], dtype=torch.int32, device=DEV)
        state = torch.full((N,), g.start, dtype=torch.int32, device=DEV)
        on = (f(0, torch.int32), torch.arange(N, dtype=torch.int32, device=DEV), cls, nxt, meta, state)
        off = (f(-1, torch.int32), f(-1, torch.int32), cls, nxt, meta, state)

        def all_guided():  # from the start state every launch: the same mask, the same work
            state.fill_(g.start)
            return ops.sample_guided(*base, *ext, *on, check_slots=False)

        r = alternate({"ext": lambda: ops.sample_ext(*base, *ext, check_slots=False),
                       "none": lambda: ops.sample_guided(*base, *ext, *off, check_slots=False),
                       "all": all_guided,
                       "fill": lambda: state.fill_(g.start)}, iters, reps)
        cost = r["all"][0] - r["fill"][0] - r["ext"][0]
        print(f"{N:6d} | {fmt(r['ext'])} | {fmt(r['none'])} | {fmt(r['all'])} (incl. a {r['fill'][0] * 1e3:.1f} us state reset) "
              f"| {cost * 1e3:+6.1f} us")


def bench_step(model, ctx, iters, reps):
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    B = 16
    max_len = ctx + 64
    eng = InferenceEngine(model, device=DEV, max_batch_size=B, max_batch_tokens=8192, max_model_len=max_len,
                          num_kv_blocks=B * ((max_len + 15) // 16) + 64, block_size=16, prefix_caching=False,
                          scheduler="prefill_first")  # all prompts first: the batch then decodes, and ends, together
    prompts = [[(7 * i + 13 * r) % V for i in range(ctx)] for r in range(B)]
    kw = dict(max_tokens=6, temperature=0.0)
    eng.generate(prompts, SamplingParams(ignore_eos=True, **kw))
    eng.generate(prompts, SamplingParams(presence_penalty=0.5, frequency_penalty=0.25, repetition_penalty=1.25,
                                         logprobs=5, ignore_eos=True, **kw))
    eng.generate(prompts, SamplingParams(guided_regex=LONG, **kw))
    torch.cuda.synchronize()
    (gp, bp), (ge, be), (gg, bg) = eng._graphs[B], eng._graphs_ext[B], eng._graphs_guided[B]
    assert min(int(b["ctx_lens"].min()) for b in (bp, be, bg)) >= ctx
    assert int((be["slot"] >= 0).sum()) == B and int((bg["guide"] >= 0).sum()) == B
    r = alternate({"plain": gp.replay, "ext": ge.replay, "guided": gg.replay}, iters, reps)
    p = r["plain"]
    print(f"# 2. {eng.cfg.name} decode step, {B} sequences x {ctx} tokens of context, captured graph replays: ms per "
          f"step, median (min-max) of {reps} x {iters} replays, alternated")
    for name, key in (("plain graph (sample)", "plain"), ("extended graph (sample_ext)", "ext"),
                      ("guided graph (sample_guided)", "guided")):
        x = r[key]
        print(f"{name:30s}: {x[0]:7.3f} ms ({x[1]:.3f}-{x[2]:.3f})  {(x[0] - p[0]) * 1e3:+.0f} us vs plain")
    eng.close()


def bench_compile():
    print("# 3. guide compilation on the host: ms, cold (not cached; the vocabulary's bytes known) and from the cache")
    print("# vocabulary      | constraint         | states x classes | cold ms | cached ms")
    for vname, tok, vs in (("byte (512 logits)", ByteTokenizer(), 512), ("synthetic 32k", SyntheticTokenizer(), V)):
        guided.compile_guide("regex", "warm", tok, vs)  # token bytes + their identity, once per tokenizer
        guided._CACHE.clear()  # section 1 compiled the date regex already
        for cname, kind, spec in (("date regex", "regex", DATE), ("3-property schema", "json", SCHEMA),
                                  ("50-way choice", "choice", CHOICES)):
            t0 = time.perf_counter()
            g = guided.compile_guide(kind, spec, tok, vs)
            t1 = time.perf_counter()
            guided.compile_guide(kind, spec, tok, vs)
            t2 = time.perf_counter()
            S, C = g.next.shape
            print(f"{vname:17s} | {cname:18s} | {S:5d} x {C:5d}    | {(t1 - t0) * 1e3:7.1f} | {(t2 - t1) * 1e3:7.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--model", default="gpt-7b")
    ap.add_argument("--skip-step", action="store_true", help="no decode-step timings")
    ap.add_argument("--compile-only", action="store_true", help="only the host-side compile timings (no GPU)")
    a = ap.parse_args()
    if not a.compile_only:
        assert torch.cuda.is_available(), "guided_bench needs a GPU (or --compile-only)"
        print(f"# guided sampler bench, {torch.cuda.get_device_name(0)}")
        bench_op(a.iters, a.reps)
        print("#")
        if not a.skip_step:
            bench_step(a.model, a.ctx, a.iters, a.reps)
            print("#")
    bench_compile()


if __name__ == "__main__":
    main()
