"""Grouped-expert MoE MLP (csrc/moe_grouped.hip) against the eager ``MoEMLP`` module, on the GPU.

1. One layer's MLP at Mixtral-8x7B dimensions (h 4096, F 14336, E 8, k 2, random weights): the
   eager module (argsort, host sync, rows padded to 256, one pair of library GEMMs per expert) and
   ``ops.moe_route`` + ``ops.moe_grouped_mlp``, alternated in one process, at 128 / 256 / 1024 / 4096
   rows; device-event times, and the outputs' row error against each other.
2. A 128-row decode step of a 2-layer Mixtral-8x7B slice (128 sequences, short contexts): the
   engine with ``moe_max_rows=128`` (captured graph, grouped kernels) against the default engine
   (eager step through the module).

    python tools/moe_grouped_bench.py [--rows 128 256 1024 4096] [--iters 20] [--no-step]

Run the command twice to see the spread.  Needs a GPU: there is no CPU fallback.
"""

import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl import ops
from llmctl.models import build_model, get_model_config
from llmctl.models.moe import MoEMLP
from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams
from llmctl.testing.numerics import row_err

_MODEL = {}


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


@torch.inference_mode()
def layer_bench(rows, iters):
    cfg = get_model_config("mixtral-8x7b")
    torch.manual_seed(0)
    moe = MoEMLP(cfg, cfg.layers, device="cuda", dtype=torch.bfloat16)
    up, down = ops.MoEExpertTable(moe.experts_up), ops.MoEExpertTable(moe.experts_down)
    h, F, E, k = cfg.hidden, cfg.moe_ffn, cfg.num_experts, cfg.experts_per_token
    print(f"# layer MLP, h {h} F {F} E {E} k {k}, bf16, {iters} iterations per timing, ms per call")
    print("# rows | eager module | grouped | grouped / eager | TFLOP/s grouped | row_err grouped vs eager")

    def grouped(x):
        topi, topw = ops.moe_route(x, moe.w_router, k)
        return ops.moe_grouped_mlp(x, up, down, topi, topw)

    for M in rows:
        x = torch.randn(M, h, device="cuda", dtype=torch.bfloat16)
        assert ops.moe_grouped_ok(x, E, k, h, F)
        te, tg = [], []
        for _ in range(2):  # alternate the two paths
            te.append(timed(lambda: moe(x), iters))
            tg.append(timed(lambda: grouped(x), iters))
        e, g = min(te), min(tg)
        flops = 2.0 * M * k * 3 * h * F
        print(f"{M:6d} | {e:8.3f} ({max(te):.3f}) | {g:8.3f} ({max(tg):.3f}) | {g / e:5.2f} | {flops / g / 1e9:7.1f} | "
              f"{row_err(grouped(x), moe(x)):.2e}", flush=True)


class SliceEngine(InferenceEngine):
    """An engine over the first 2 layers of mixtral-8x7b (random weights, shared by the engines)."""

    def _load(self, model_path, dtype, seed):
        if not _MODEL:
            cfg = dataclasses.replace(get_model_config("mixtral-8x7b"), layers=2)
            _MODEL["m"] = (build_model(cfg, device=self.device, dtype=dtype, seed=seed), cfg)
        return (*_MODEL["m"], None)


def step_bench(n, ctx, iters):
    print(f"# decode step, 2-layer mixtral-8x7b slice, {n} sequences x {ctx} context tokens, ms per step")
    res = {}
    for rows in (64, n, 64, n):  # alternate the two engines
        with SliceEngine("mixtral-8x7b", device="cuda", max_batch_size=n, max_model_len=ctx + 64,
                         num_kv_blocks=n * ((ctx + 79) // 16) + 64, block_size=16, prefix_caching=False,
                         moe_max_rows=rows) as eng:
            p = SamplingParams(max_tokens=32, temperature=0.0, ignore_eos=True)
            seqs = [eng.add_request([(7 * i + 13 * r) % 32000 for i in range(ctx)], p) for r in range(n)]
            while any(s.first_token_time is None for s in seqs):
                eng.step()
            if eng._pending is not None:
                eng._finalize(eng._pending)
                eng._pending = None
            out = eng.scheduler.schedule()
            assert len(out.decode) == n and not out.prefill
            plan = eng.decode_plan(list(out.decode))
            t = timed(lambda: eng.decode_exec(plan), iters)
            res.setdefault(rows, []).append(t)
            print(f"moe_max_rows={rows:4d} graph={eng._graph_ok(n)} grouped_steps={eng.stats['moe_grouped_steps']}: "
                  f"{t:.3f}", flush=True)
    print(f"# {n}-row step: eager {min(res[64]):.3f} ms, grouped in graph {min(res[n]):.3f} ms, "
          f"ratio {min(res[n]) / min(res[64]):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[128, 256, 1024, 4096])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-rows", type=int, default=128)
    ap.add_argument("--ctx", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_grouped_bench: needs a GPU")
    print(f"# {torch.cuda.get_device_name(0)}")
    layer_bench(a.rows, a.iters)
    torch.cuda.empty_cache()
    if not a.no_step:
        step_bench(a.step_rows, a.ctx, a.iters)


if __name__ == "__main__":
    main()
