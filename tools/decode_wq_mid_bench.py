#!/usr/bin/env python3
"""fp8 / int4 decode weights at 17-64 token rows (csrc/decode_gemm_mid.hip) against what such steps
ran before: the kept bf16 weights through ``ops.decode_linear`` plus the separate RoPE / cache-write,
SwiGLU and add + RMSNorm passes.  Old and new alternate in one process; device events; medians.

Per projection of GPT-7B (QKV, o, gate/up, down, LM head) at 32 and 64 rows: the op the decode layer
calls (``ops.decode_qkv_rope_cache`` / ``decode_linear_add_rmsnorm`` / ``decode_up_swiglu`` /
``decode_linear_*``) with the bf16 weight (old) or the quantised copy (new), cycling through > 512 MB
of weight copies so that no cache serves repeats; bytes/s counts the weight (+ scale) bytes read.

Per decode step: GPT-7B (random weights), every sequence at a ``--ctx`` context, batches 16 / 32 / 64,
one engine per weight dtype whose ``weight_max_rows`` alternates between 16 (the bf16 stream above 16
rows: the old step) and 64, each with its own captured graphs.  At 16 rows both settings run the
same kernels: the parity row.

    python tools/decode_wq_mid_bench.py [--steps 100] [--warmup 3] [--reps 5] [--ctx 2048] [--skip-steps]
    python tools/decode_wq_mid_bench.py --check [--device cpu]   # no timing: old vs new results, tiny shapes
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.testing.numerics import row_err

KINDS = ("fp8", "int4")
ROWS = (32, 64)
BATCHES = (16, 32, 64)


def shapes(hidden, ffn, vocab, heads, kv_heads, head_dim):
    return {"qkv": ((heads + 2 * kv_heads) * head_dim, hidden), "o": (hidden, heads * head_dim),
            "up": (2 * ffn, hidden), "down": (hidden, ffn), "lm_head": (vocab, hidden)}


def random_weights(kind, N, K, dev, n):
    """``n`` random (weight, scales) pairs in the format of ``kind`` (timing does not read values)."""
    out = []
    for _ in range(n):
        if kind == "bf16":
            out.append((torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02, None))
        elif kind == "fp8":
            out.append((torch.randn(N, K, device=dev).to(torch.float8_e4m3fn), torch.rand(N, device=dev) * 1e-2 + 1e-3))
        else:
            out.append((torch.randint(0, 256, (N, K // 2), device=dev, dtype=torch.uint8),
                        torch.rand(N, K // 128, device=dev) * 1e-2 + 1e-3))
    return out


def weight_bytes(kind, N, K):
    return {"bf16": 2 * N * K, "fp8": N * K + 4 * N, "int4": N * K // 2 + 4 * N * (K // 128)}[kind]


class Projection:
    """One decode projection as the fused layer calls it, on a (weight, scales) pair of any kind."""

    def __init__(self, name, M, N, K, dev, heads=32, kv_heads=32, head_dim=128):
        self.name, self.M = name, M
        dt = torch.bfloat16 if dev != "cpu" else torch.float32
        self.x = torch.randn(M, K, device=dev).to(dt)
        if name == "qkv":
            self.nq, self.nkv = heads, kv_heads
            self.rope = ref.rope_tables(256, head_dim, base=10000.0, device=dev)
            self.pos = torch.arange(M, dtype=torch.int32, device=dev)
            self.slots = torch.arange(M, device=dev)
            self.kc = torch.zeros(-(-M // 16), 16, kv_heads, head_dim, device=dev, dtype=dt)
            self.vc = torch.zeros_like(self.kc)
        elif name in ("o", "down"):
            self.res = torch.randn(M, N, device=dev).to(dt)
            self.nw = torch.ones(N, device=dev, dtype=dt)

    def __call__(self, w, s):
        x = self.x
        if self.name == "qkv":
            return ops.decode_qkv_rope_cache(x, w, None, self.rope[0], self.rope[1], self.nq, self.nkv, self.pos,
                                             self.kc, self.vc, self.slots, w_scale=s)
        if self.name in ("o", "down"):
            return ops.decode_linear_add_rmsnorm(x, w, None, self.res, self.nw, 1e-5, w_scale=s)[0]
        if self.name == "up":
            return ops.decode_up_swiglu(x, w, None, w_scale=s)
        if s is None:
            return ops.decode_linear(x, w)
        return ops.decode_linear_int4(x, w, s) if w.dtype == torch.uint8 else ops.decode_linear_fp8(x, w, s)


def check(dev):
    """Old (dequantised weight, unfused passes) against new results on the same quantised weights."""
    from llmctl.ops.functional import _dequant
    from llmctl.plugins.quantizers import quantize_fp8, quantize_int4_g128

    dt = torch.bfloat16 if dev != "cpu" else torch.float32
    for name, (N, K) in shapes(256, 384, 512, 4, 4, 64).items():
        for kind in KINDS:
            p = Projection(name, 40, N, K, dev, 4, 4, 64)
            qd = (quantize_fp8 if kind == "fp8" else quantize_int4_g128)(torch.randn(N, K, device=dev).to(dt) * 0.05)
            q, s = qd["qweight"].contiguous(), qd["scale"].float().contiguous()
            new, old = p(q, s), p(_dequant(q, s, dt), None)
            err = row_err(new.reshape(40, -1), old.reshape(40, -1))
            print(f"check {name:8s} {kind}: 40x{N}x{K} new vs old row_err {err:.3e}")
            assert err < 3e-2, err


def time_fn(fn, iters, warmup):
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


def bench_projections(a, cfg):
    print("# per projection: us median (min-max) of the op the decode layer calls; TB/s of the weight stream")
    print("# proj rows | bf16 (old) | fp8 (new) | int4 (new)")
    for name, (N, K) in shapes(cfg.hidden, cfg.ffn, cfg.vocab_size, cfg.heads, cfg.kv_heads, cfg.head_dim).items():
        pools = {k: random_weights(k, N, K, "cuda", max(2, -(-512 * 2 ** 20 // weight_bytes(k, N, K))))
                 for k in ("bf16",) + KINDS}
        for M in ROWS:
            p = Projection(name, M, N, K, "cuda", cfg.heads, cfg.kv_heads, cfg.head_dim)
            t = {k: [] for k in pools}
            count = iter(range(1 << 30))
            for _ in range(a.reps):
                for k, pool in pools.items():
                    t[k].append(time_fn(lambda: p(*pool[next(count) % len(pool)]), a.steps, a.warmup) * 1e3)
            cells = []
            for k in pools:
                med = statistics.median(t[k])
                cells.append(f"{med:7.1f} us ({min(t[k]):.1f}-{max(t[k]):.1f}) {weight_bytes(k, N, K) / med / 1e6:5.2f} TB/s")
            old = statistics.median(t["bf16"])
            verdict = ", ".join(f"{k} {old / statistics.median(t[k]):.2f}x" for k in KINDS)
            print(f"{name:8s} {M:2d} | " + " | ".join(cells) + f" | speed-up over bf16: {verdict}", flush=True)
        del pools
        torch.cuda.empty_cache()


def bench_steps(a):
    from llmctl.models import build_model, get_model_config
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    shared = {}

    class Engine(InferenceEngine):
        def _load(self, model_path, dtype, seed):
            if "m" not in shared:
                cfg = get_model_config("gpt-7b")
                shared["m"] = (build_model(cfg, device=self.device, dtype=dtype, seed=seed), cfg)
            return (*shared["m"], None)

    print(f"# per decode step, GPT-7B, context {a.ctx}: ms median (min-max) of {a.reps} x {a.steps} steps, settings alternated")
    print("# dtype batch | weight_max_rows=16 (old above 16 rows) | weight_max_rows=64 | speed-up")
    B, max_len = max(BATCHES), a.ctx + 64
    for kind in KINDS:
        eng = Engine("gpt-7b", device="cuda", max_batch_size=B, max_model_len=max_len, block_size=16,
                     num_kv_blocks=B * ((max_len + 15) // 16) + 64, prefix_caching=False, weight_dtype=kind)
        sp = SamplingParams(max_tokens=32, temperature=0.0, ignore_eos=True)
        seqs = [eng.add_request([(7 * i + 13 * r) % 32000 for i in range(a.ctx)], sp) for r in range(B)]
        while any(s.first_token_time is None for s in seqs):
            eng.step()
        if eng._pending is not None:
            eng._finalize(eng._pending)
            eng._pending = None
        out = eng.scheduler.schedule()
        assert len(out.decode) == B and not out.prefill
        graphs = {16: {}, 64: {}}  # each setting replays its own captured graphs
        for n in BATCHES:
            plan = eng.decode_plan(list(out.decode)[:n])
            t = {r: [] for r in graphs}
            for _ in range(a.reps):
                for r in graphs:
                    eng.weight_max_rows, eng._graphs = r, graphs[r]
                    t[r].append(time_fn(lambda: eng.decode_exec(plan), a.steps, a.warmup))
            med = {r: statistics.median(v) for r, v in t.items()}
            ratio = med[16] / med[64]
            spread = max((max(v) - min(v)) / med[r] for r, v in t.items())
            note = "same kernels: parity" if n <= 16 else ("faster" if ratio - 1 > spread else "NOT faster beyond the spread")
            print(f"{kind:5s} {n:2d} | {med[16]:7.3f} ms ({min(t[16]):.3f}-{max(t[16]):.3f}) | {med[64]:7.3f} ms "
                  f"({min(t[64]):.3f}-{max(t[64]):.3f}) | {ratio:.3f}x, spread {100 * spread:.1f} %: {note}", flush=True)
        for g in graphs.values():
            eng._graphs = g
            eng.release_graphs()
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--skip-steps", action="store_true", help="projections only")
    ap.add_argument("--check", action="store_true", help="compare old and new results at tiny shapes, no timing")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    if a.check:
        return check(a.device)
    assert torch.cuda.is_available(), "timing needs the GPU"
    from llmctl.models import get_model_config

    print(f"# {torch.cuda.get_device_name(0)}; {a.reps} reps x {a.steps} iterations after {a.warmup} warm-up, old / new alternated")
    bench_projections(a, get_model_config("gpt-7b"))
    if not a.skip_steps:
        bench_steps(a)


if __name__ == "__main__":
    main()
