#!/usr/bin/env python3
"""The extended sampler (``ops.sample_ext``: penalties, logprobs, device-resident state) against
the plain one (``ops.sample``), in one process on the GPU:

1. the op alone at N = 1, 16, 64 rows x V = 32000 bf16 logits, greedy and sampled (T = 0.8,
   top-k 50, top-p 0.9); ``sample_ext`` with every row penalized (its own state slot) and 5 top
   logprobs.  Device events around ``--iters`` back-to-back launches, ``--reps`` times per
   variant, alternated; the median is reported;
2. a GPT-7B decode step of 16 sequences x ``--ctx`` tokens of context: the captured decode graph
   of a plain batch against the extended graph of the same batch with every request penalized
   and asking for 5 logprobs.  Both graphs are captured by serving the batch through the engine,
   then replayed back to back (same positions each time: the step's work does not depend on
   them), timed like the op;
3. the logprob error: torch's fp32 ``log_softmax`` and the kernel against the fp64 oracle on the
   N = 64, V = 32000 inputs of the kernel test.

    python tools/sampling_bench.py [--iters 200] [--reps 5] [--ctx 2048] [--model gpt-7b]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl import ops
from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams

DEV = "cuda"
V = 32000


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


def op_inputs(N, temperature):
    torch.manual_seed(0)
    logits = (torch.randn(N, V, device=DEV) * 3).to(torch.bfloat16)
    temp = torch.full((N,), temperature, device=DEV)
    topk = torch.full((N,), 50, dtype=torch.int32, device=DEV)
    topp = torch.full((N,), 0.9, device=DEV)
    u = torch.rand(N, device=DEV)
    slot = torch.arange(N, dtype=torch.int32, device=DEV)
    rep, freq, pres = (torch.full((N,), v, device=DEV) for v in (1.25, 0.25, 0.5))
    nlp = torch.full((N,), 5, dtype=torch.int32, device=DEV)
    counts = (torch.randint(0, 9, (N, V), device=DEV) * (torch.rand(N, V, device=DEV) < 0.02)).to(torch.int32)
    mask = (torch.rand(N, V, device=DEV) < 0.05).to(torch.uint8)
    return (logits, temp, topk, topp, u), (slot, rep, freq, pres, nlp, counts, mask)


@torch.inference_mode()
def bench_op(iters, reps):
    print(f"# 1. the op, V = {V}, bf16 logits: us per launch, median (min-max) of {reps} x {iters} launches, alternated")
    print("# rows | draw    | sample            | sample_ext (penalties + 5 logprobs) | extra")
    for N in (1, 16, 64):
        for name, T in (("greedy", 0.0), ("sampled", 0.8)):
            base, ext = op_inputs(N, T)
            r = alternate({"sample": lambda: ops.sample(*base),
                           "ext": lambda: ops.sample_ext(*base, *ext, check_slots=False)}, iters, reps)
            s, e = r["sample"], r["ext"]
            print(f"{N:6d} | {name:7s} | {s[0] * 1e3:6.1f} ({s[1] * 1e3:.1f}-{s[2] * 1e3:.1f}) | "
                  f"{e[0] * 1e3:6.1f} ({e[1] * 1e3:.1f}-{e[2] * 1e3:.1f}) | {(e[0] - s[0]) * 1e3:+6.1f} us")


def bench_step(model, ctx, iters, reps):
    B = 16
    max_len = ctx + 64
    eng = InferenceEngine(model, device=DEV, max_batch_size=B, max_batch_tokens=8192, max_model_len=max_len,
                          num_kv_blocks=B * ((max_len + 15) // 16) + 64, block_size=16, prefix_caching=False,
                          scheduler="prefill_first")  # all prompts first: the batch then decodes, and ends, together
    prompts = [[(7 * i + 13 * r) % V for i in range(ctx)] for r in range(B)]
    kw = dict(max_tokens=6, temperature=0.0, ignore_eos=True)
    eng.generate(prompts, SamplingParams(**kw))
    eng.generate(prompts, SamplingParams(presence_penalty=0.5, frequency_penalty=0.25, repetition_penalty=1.25,
                                         logprobs=5, **kw))
    torch.cuda.synchronize()
    (gp, bp), (ge, be) = eng._graphs[B], eng._graphs_ext[B]
    assert int(bp["ctx_lens"].min()) >= ctx and int(be["ctx_lens"].min()) >= ctx and int((be["slot"] >= 0).sum()) == B
    r = alternate({"plain": gp.replay, "ext": ge.replay}, iters, reps)
    p, e = r["plain"], r["ext"]
    print(f"# 2. {eng.cfg.name} decode step, {B} sequences x {ctx} tokens of context, captured graph replays: ms per "
          f"step, median (min-max) of {reps} x {iters} replays, alternated")
    print(f"plain graph (sample)        : {p[0]:7.3f} ms ({p[1]:.3f}-{p[2]:.3f})")
    print(f"extended graph (sample_ext) : {e[0]:7.3f} ms ({e[1]:.3f}-{e[2]:.3f})  {(e[0] - p[0]) * 1e3:+.0f} us, "
          f"{(e[0] / p[0] - 1) * 100:+.2f} %")
    eng.close()


@torch.inference_mode()
def logprob_error():
    # the inputs of tests/kernels/test_sampling_ext.py::_inputs(64, 32000) without the state
    torch.manual_seed(0)
    N = 64
    logits = (torch.randn(N, V, device=DEV) * 3).to(torch.bfloat16)
    temp = torch.zeros(N, device=DEV)
    topk = torch.zeros(N, dtype=torch.int32, device=DEV)
    one = torch.ones(N, device=DEV)
    slot = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    nlp = torch.full((N,), 8, dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, V, dtype=torch.int32, device=DEV)
    toks, lp, top_ids, top_lp = ops.sample_ext(logits, temp, topk, one, one * 0.5, slot, one, one * 0, one * 0, nlp,
                                               counts, torch.zeros(1, V, dtype=torch.uint8, device=DEV))
    x = logits.float()
    lp64 = torch.log_softmax(x.double(), dim=-1)
    t_err = (torch.log_softmax(x, dim=-1).double() - lp64).abs().max().item()
    k_err = max((lp.double() - lp64.gather(1, toks.view(N, 1)).view(N)).abs().max().item(),
                (top_lp.double() - lp64.gather(1, top_ids.long())).abs().max().item())
    print(f"# 3. logprob max abs error against the fp64 oracle, {N} x {V} (randn * 3, bf16)")
    print(f"torch fp32 log_softmax (all {N * V} entries)      : {t_err:.3e}")
    print(f"sample_ext (chosen + top-8 entries, {N * 9} values) : {k_err:.3e}   (tests allow 4 x torch's = {4 * t_err:.3e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--model", default="gpt-7b")
    ap.add_argument("--skip-step", action="store_true", help="only the op timings and the logprob error")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sampling_bench needs a GPU"
    print(f"# extended sampler bench, {torch.cuda.get_device_name(0)}")
    bench_op(a.iters, a.reps)
    print("#")
    if not a.skip_step:
        bench_step(a.model, a.ctx, a.iters, a.reps)
        print("#")
    logprob_error()


if __name__ == "__main__":
    main()
