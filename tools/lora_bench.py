#!/usr/bin/env python3
"""Multi-LoRA decode cost on the MI355X at GPT-7B dimensions.

1. ``ops.lora_delta`` (``csrc/lora_decode.hip``: shrink + expand, two launches) at the four GPT-7B
   projection shapes for M = 1, 4, 16 rows and padded rank R = 16, 64, with all rows on one adapter
   and with every row on its own adapter (16 resident slots).  Device events around ``--op-iters``
   back-to-back calls after a warm-up: the adapters stay cache-resident between calls, so this is the
   launch-bound floor of the op, not its cost behind a 13 GB weight stream.
2. The 16 x 2k GPT-7B decode step (random weights, every sequence holds a 2k-token context prefilled
   through the engine), ``decode_exec`` of one plan replayed back to back, on
     plain      the plain graph (what a batch without adapter rows replays),
     lora-none  the LoRA graph with every row at -1,
     lora-one   the LoRA graph with all rows on one adapter,
     lora-all   the LoRA graph with every row on its own adapter,
   alternated ``--reps`` times; median (min-max) ms per step.

``--plain-only`` times the plain graph alone and touches no adapter API, so the same file runs on a
checkout that predates adapters (the parent-commit comparison of the plain path).

    python tools/lora_bench.py [--steps 100] [--warmup 5] [--reps 5] [--ctx 2048] [--plain-only] [--skip-ops]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams

MODEL = "gpt-7b"
BATCH = 16
SLOTS = 16
SHAPES = (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate/up", 22016, 4096), ("down", 4096, 11008))


def time_calls(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def bench_ops(iters):
    from llmctl import ops

    print(f"# ops.lora_delta, us per call (shrink + expand), {iters} back-to-back calls, {SLOTS} resident slots")
    print("# projection      N      K   R |  M=1 one | M=4 one  M=4 distinct | M=16 one  M=16 distinct")
    for name, N, K in SHAPES:
        for R in (16, 64):
            A = (torch.randn(SLOTS, R, K, device="cuda") * 0.02).bfloat16()
            B = (torch.randn(SLOTS, N, R, device="cuda") * 0.02).bfloat16()
            sc = torch.full((SLOTS,), 2.0, device="cuda")
            t = {}
            for M in (1, 4, 16):
                x = torch.randn(M, K, device="cuda").bfloat16()
                for kind, idx in (("one", [3] * M), ("distinct", list(range(M)))):
                    ii = torch.tensor(idx, dtype=torch.int32, device="cuda")
                    t[(M, kind)] = time_calls(lambda: ops.lora_delta(x, ii, A, B, sc), iters)
            print(f"{name:>10} {N:6d} {K:6d} {R:3d} | {t[(1, 'one')]:8.2f} | {t[(4, 'one')]:7.2f}  {t[(4, 'distinct')]:12.2f} | "
                  f"{t[(16, 'one')]:8.2f}  {t[(16, 'distinct')]:13.2f}")
            del A, B
    torch.cuda.empty_cache()


def prefill(eng, ctx):
    """BATCH sequences with a ``ctx``-token context each, scheduled for one decode step."""
    p = SamplingParams(max_tokens=32, temperature=0.0, ignore_eos=True)
    seqs = [eng.add_request([(7 * i + 13 * r) % 32000 for i in range(ctx)], p) for r in range(BATCH)]
    while any(s.first_token_time is None for s in seqs):
        eng.step()
    if eng._pending is not None:
        eng._finalize(eng._pending)
        eng._pending = None
    out = eng.scheduler.schedule()
    assert len(out.decode) == len(seqs) and not out.prefill
    return list(out.decode)


def time_steps(eng, plan, steps, warmup):
    for _ in range(warmup):
        eng.decode_exec(plan)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.decode_exec(plan)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--op-iters", type=int, default=300)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    a = ap.parse_args()
    print(f"# multi-LoRA decode: {MODEL} dimensions, bf16, {torch.cuda.get_device_name(0)}")
    if not a.plain_only and not a.skip_ops:
        bench_ops(a.op_iters)
    max_len = a.ctx + 64
    kw = dict(device="cuda", max_batch_size=BATCH, max_model_len=max_len,
              num_kv_blocks=BATCH * ((max_len + 15) // 16) + 64, block_size=16, prefix_caching=False)
    if not a.plain_only:
        kw.update(max_loras=SLOTS, max_lora_rank=a.rank)
    eng = InferenceEngine(MODEL, **kw)
    assert eng.use_graphs and eng._fused_decode()
    if not a.plain_only:
        from llmctl.serve.lora import random_adapter

        for i in range(SLOTS):
            eng.load_lora(f"lora{i}", random_adapter(eng.cfg, rank=a.rank, seed=i, std=0.01))
    seqs = prefill(eng, a.ctx)
    plain = eng.decode_plan(seqs)
    plans = {"plain": plain}
    if not a.plain_only:
        plans["lora-none"] = dict(plain, lora=[-1] * BATCH)
        plans["lora-one"] = dict(plain, lora=[3] * BATCH)
        plans["lora-all"] = dict(plain, lora=list(range(BATCH)))
    t = {m: [] for m in plans}
    for _ in range(a.reps):
        for m, plan in plans.items():
            t[m].append(time_steps(eng, plan, a.steps, a.warmup))
    print(f"# {BATCH} x {a.ctx} decode step, {eng.cfg.layers} layers, adapter rank {a.rank} on wqkv / wo / w_up / w_down of every "
          f"layer; ms per step: median (min-max) of {a.reps} x {a.steps} replays after {a.warmup} warm-up, modes alternated")
    for m in plans:
        extra = "" if m == "plain" else f"  (+{statistics.median(t[m]) - statistics.median(t['plain']):.3f} ms vs plain)"
        print(f"{m:>10}: {statistics.median(t[m]):7.3f} ms/step ({min(t[m]):.3f}-{max(t[m]):.3f}){extra}")
    if not a.plain_only:
        assert set(eng._graphs_lora) == {(BATCH, False)} and set(eng._graphs) == {BATCH}
    eng.close()


if __name__ == "__main__":
    main()
