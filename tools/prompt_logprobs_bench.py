#!/usr/bin/env python3
"""Prompt scoring (``ops.prompt_logprobs``, ``SamplingParams.prompt_logprobs``):

1. the op alone at R = 2048 rows x V = 32000 bf16 logits, nlp = 0, 1 and 8, against the torch
   composite on the same tensor (``log_softmax`` in fp32, gather, ``topk``, the rank by comparison).
   Device events around ``--iters`` back-to-back launches, ``--reps`` times per variant, alternated;
   the median is reported, and R * V * 2 bytes over it.  "same tensor": every launch reads the one
   131 MB tensor again (it fits the Infinity Cache, as a tile does right after its GEMM); "rotating":
   the launches cycle over four such tensors (524 MB: the rows come from HBM);
2. what a scoring request pays: a single ``--ctx``-token prompt on ``--model``, TTFT with
   ``prompt_logprobs = 1`` against without, alternated on one engine (no prefix cache); and the two
   pieces of a 1024-row tile on their own: the vocabulary projection and the kernel;
3. ``--plain``: the paths that do not score -- the same single-prompt TTFT and the 16 x ``--ctx``
   decode step on the captured plain graph.  Run it on this tree and, with ``--tree``, on a checkout
   (with its own build) of the commit to compare against, in alternated processes;
4. ``--score-once``: one warmed scoring request and nothing else (for a kernel trace of its own).

    python tools/prompt_logprobs_bench.py [--iters 50] [--reps 5] [--ctx 2048] [--model gpt-7b]
                                          [--plain | --score-once] [--tree PATH] [--skip-engine]
"""
import argparse
import os
import statistics
import sys
import time

_args = argparse.ArgumentParser()
_args.add_argument("--iters", type=int, default=50)
_args.add_argument("--reps", type=int, default=5)
_args.add_argument("--ctx", type=int, default=2048)
_args.add_argument("--model", default="gpt-7b")
_args.add_argument("--plain", action="store_true", help="only section 3 (runs on a tree without the feature too)")
_args.add_argument("--score-once", action="store_true", help="only one warmed scoring request")
_args.add_argument("--skip-engine", action="store_true", help="section 1 only")
_args.add_argument("--tree", default=None, help="import llmctl from this checkout instead of the script's")
ARGS = _args.parse_args()
sys.path.insert(0, ARGS.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DEV = "cuda"
R, V = 2048, 32000


def timed(fn, iters, warmup=3):
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
    return f"{r[0] * scale:8.1f} ({r[1] * scale:.1f}-{r[2] * scale:.1f})"


def composite(logits, target, k):
    """What the kernel replaces, in torch: fp32 log_softmax, the target's logprob, top-k, the rank."""
    lsm = torch.log_softmax(logits.float(), dim=-1)
    t = target.view(-1, 1)
    lp = lsm.gather(1, t)
    idx = torch.arange(logits.shape[1], device=logits.device).view(1, -1)
    rank = ((lsm > lp) | ((lsm == lp) & (idx < t))).sum(1) + 1
    top = lsm.topk(k, dim=1) if k > 0 else None
    return lp, rank, top


@torch.inference_mode()
def bench_op(iters, reps):
    from llmctl import ops

    torch.manual_seed(0)
    bufs = [(torch.randn(R, V, device=DEV) * 3).to(torch.bfloat16) for _ in range(4)]
    target = torch.randint(0, V, (R,), device=DEV)
    nbytes = R * V * 2
    print(f"# 1. the op, R = {R}, V = {V}, bf16 logits; us per launch, median (min-max) of {reps} x {iters} launches, "
          f"alternated; TB/s = {nbytes / 1e6:.0f} MB / median")
    print("# nlp | prompt_logprob_kernel, same tensor | TB/s | kernel, rotating over 4 tensors | TB/s | torch composite, same tensor | composite / kernel")
    for k in (0, 1, 8):
        nlp = torch.full((R,), k, dtype=torch.int32, device=DEV)
        turn = [0]

        def rotating():
            turn[0] = (turn[0] + 1) % 4
            return ops.prompt_logprobs(bufs[turn[0]], target, nlp)

        r = alternate({"kernel": lambda: ops.prompt_logprobs(bufs[0], target, nlp), "rot": rotating,
                       "torch": lambda: composite(bufs[0], target, k)}, iters, reps)
        print(f"{k:5d} | {fmt(r['kernel'])} | {nbytes / r['kernel'][0] / 1e9:5.2f} | {fmt(r['rot'])} | "
              f"{nbytes / r['rot'][0] / 1e9:5.2f} | {fmt(r['torch'])} | {r['torch'][0] / r['kernel'][0]:5.1f} x")


def _engine(model, ctx, batch):
    from llmctl.serve.engine import InferenceEngine

    max_len = ctx + 64
    return InferenceEngine(model, device=DEV, max_batch_size=batch, max_batch_tokens=8192, max_model_len=max_len,
                           num_kv_blocks=batch * ((max_len + 15) // 16) + 64, block_size=16, prefix_caching=False,
                           scheduler="prefill_first")


def _ttft(eng, prompt, params):
    s = eng.add_request(prompt, params)
    s.arrival_time = time.time()
    while s.status != "finished":
        eng.step()
    return s.first_token_time - s.arrival_time


def _ttfts(eng, ctx, variants, reps):
    Vm = eng.cfg.vocab_size
    out = {k: [] for k in variants}
    for r in range(reps + 1):
        for k, p in variants.items():
            t = _ttft(eng, [(7 * i + 13 * r) % Vm for i in range(ctx)], p)
            if r:  # the first round warms the paths
                out[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def bench_request(model, ctx, iters, reps):
    from llmctl import ops
    from llmctl.serve.scheduler import SamplingParams

    eng = _engine(model, ctx, 1)
    kw = dict(max_tokens=1, temperature=0.0, ignore_eos=True)
    r = _ttfts(eng, ctx, {"plain": SamplingParams(**kw), "scored": SamplingParams(prompt_logprobs=1, **kw)}, reps)
    print(f"# 2. {eng.cfg.name}, one {ctx}-token prompt, TTFT ms, median (min-max) of {reps}, alternated on one engine")
    print(f"without prompt_logprobs: {fmt(r['plain'], 1e3)} ms")
    print(f"prompt_logprobs = 1    : {fmt(r['scored'], 1e3)} ms   {(r['scored'][0] - r['plain'][0]) * 1e3:+.2f} ms")
    with torch.inference_mode():
        w = eng.model.head_weight()
        T = eng.SCORE_TILE
        xn = torch.randn(T, w.shape[1], device=DEV).to(w.dtype)
        out = torch.empty(T, w.shape[0], dtype=w.dtype, device=DEV)
        target = torch.randint(0, w.shape[0], (T,), device=DEV)
        nlp = torch.ones(T, dtype=torch.int32, device=DEV)
        p = alternate({"proj": lambda: torch.mm(xn, w.t(), out=out),
                       "kernel": lambda: ops.prompt_logprobs(out, target, nlp)}, iters, reps)
    print(f"one {T}-row tile, us: vocabulary projection [{T} x {w.shape[1]}] x [{w.shape[1]} x {w.shape[0]}] "
          f"{fmt(p['proj'])}; prompt_logprob_kernel right after it {fmt(p['kernel'])}")
    eng.close()


def bench_plain(model, ctx, iters, reps):
    from llmctl.serve.scheduler import SamplingParams

    eng = _engine(model, ctx, 16)
    kw = dict(temperature=0.0, ignore_eos=True)
    r = _ttfts(eng, ctx, {"plain": SamplingParams(max_tokens=1, **kw)}, reps)
    print(f"# 3. {eng.cfg.name}, paths that do not score ({os.path.abspath(sys.path[0])})")
    print(f"single {ctx}-token prompt TTFT: {fmt(r['plain'], 1e3)} ms, median (min-max) of {reps}")
    Vm = eng.cfg.vocab_size
    eng.generate([[(7 * i + 13 * q) % Vm for i in range(ctx)] for q in range(16)], SamplingParams(max_tokens=6, **kw))
    torch.cuda.synchronize()
    g, b = eng._graphs[16]
    assert int(b["ctx_lens"].min()) >= ctx
    s = alternate({"plain": g.replay}, iters, reps)["plain"]
    print(f"decode step, 16 x {ctx}, plain graph: {s[0]:.3f} ms ({s[1]:.3f}-{s[2]:.3f}), median (min-max) of "
          f"{reps} x {iters} replays")
    eng.close()


def score_once(model, ctx):
    from llmctl.serve.scheduler import SamplingParams

    eng = _engine(model, ctx, 1)
    p = SamplingParams(max_tokens=1, temperature=0.0, ignore_eos=True, prompt_logprobs=1)
    eng.generate([[1] * 64], p)
    t = _ttft(eng, [(7 * i) % eng.cfg.vocab_size for i in range(ctx)], p)
    print(f"one scored {ctx}-token prompt on {eng.cfg.name}: TTFT {t * 1e3:.2f} ms")
    eng.close()


def main():
    a = ARGS
    assert torch.cuda.is_available(), "prompt_logprobs_bench needs a GPU"
    print(f"# prompt logprobs bench, {torch.cuda.get_device_name(0)}")
    if a.plain:
        return bench_plain(a.model, a.ctx, a.iters, a.reps)
    if a.score_once:
        return score_once(a.model, a.ctx)
    bench_op(a.iters, a.reps)
    if not a.skip_engine:
        print("#")
        bench_request(a.model, a.ctx, a.iters, a.reps)


if __name__ == "__main__":
    main()
