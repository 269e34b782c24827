#!/usr/bin/env python3
"""MoE decode A/B on a Mixtral-8x7B-dimension slice: the routed-expert kernels in the captured
decode graph (knob ``moe_decode_fused`` on) against the eager ``MoEMLP`` path (knob off: what MoE
serving ran before the kernels existed), alternated in one process.

Dimensions: hidden 4096, 8 experts x ffn 14336, top-2, GQA 32/8, random weights.  A 2-layer and a
4-layer slice are measured so that per-layer time is a slope (embedding, LM head and the per-step
host work cancel).  Every sequence holds a 2k-token context (prefilled through the engine); a decode
step of batch 1, 4 and 16 is then timed with device events around ``--steps`` back-to-back
``decode_exec`` calls after ``--warmup`` untimed ones, ``--reps`` times per mode, alternating modes;
the median is reported.  Also printed: kernels launched per layer (profiler count of one uncaptured
step, as a slope) and the expert bytes a step must move (from the routing of one untimed step: the
distinct experts picked per layer x 3 h F x 2 B) next to the bytes of all experts.

    python tools/moe_decode_bench.py [--steps 200] [--warmup 3] [--reps 5] [--ctx 2048]
"""
import argparse
import dataclasses
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from llmctl import ops
from llmctl.models import build_model, get_model_config
from llmctl.serve import engine as engine_mod
from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams

BATCHES = (1, 4, 16)
_MODELS = {}


class SliceEngine(InferenceEngine):
    """An engine over the first ``SLICE_LAYERS`` layers of mixtral-8x7b (random weights); engines of
    one slice share the model."""
    SLICE_LAYERS = 2

    def _load(self, model_path, dtype, seed):
        L = self.SLICE_LAYERS
        if L not in _MODELS:
            cfg = dataclasses.replace(get_model_config("mixtral-8x7b"), layers=L)
            _MODELS[L] = (build_model(cfg, device=self.device, dtype=dtype, seed=seed), cfg)
        model, cfg = _MODELS[L]
        return model, cfg, None


def make_engine(L, ctx, fused):
    cls = type(f"SliceEngine{L}", (SliceEngine,), {"SLICE_LAYERS": L})
    max_len = ctx + 64
    return cls("mixtral-8x7b", device="cuda", max_batch_size=max(BATCHES), max_model_len=max_len,
               num_kv_blocks=max(BATCHES) * ((max_len + 15) // 16) + 64, block_size=16, prefix_caching=False,
               perf_knobs={"moe_decode_fused": int(fused)})


def prefill(eng, ctx):
    """max(BATCHES) sequences with a ``ctx``-token context each, scheduled for one decode step."""
    p = SamplingParams(max_tokens=32, temperature=0.0, ignore_eos=True)
    seqs = [eng.add_request([(7 * i + 13 * r) % 32000 for i in range(ctx)], p) for r in range(max(BATCHES))]
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


def body_args(eng, plan):
    d = eng.device
    return (torch.tensor(plan["ids"], device=d), torch.tensor(plan["positions"], dtype=torch.int32, device=d),
            torch.tensor(plan["slots"], device=d), torch.from_numpy(plan["bt"]).to(d),
            torch.tensor(plan["ctx"], dtype=torch.int32, device=d))


@torch.inference_mode()
def count_kernels(eng, plan):
    """Kernels launched by one uncaptured decode step (None when the profiler is unavailable)."""
    from llmctl.config.knobs import use as use_knobs

    use_knobs(eng.knobs)
    args = body_args(eng, plan)
    eng._decode_body(*args)
    torch.cuda.synchronize()
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eng._decode_body(*args)
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
    except Exception as e:  # pragma: no cover - depends on the box
        print(f"# kernel count unavailable: {e}")
        return None


@torch.inference_mode()
def routed_experts(eng, plan):
    """Distinct experts picked per layer in one (untimed, uncaptured) step of the fused engine."""
    from llmctl.config.knobs import use as use_knobs

    use_knobs(eng.knobs)
    picked = []
    orig = ops.moe_route

    def spy(x, w, k):
        topi, topw = orig(x, w, k)
        picked.append(topi)
        return topi, topw

    engine_mod.ops.moe_route = spy
    try:
        eng._decode_body(*body_args(eng, plan))
        torch.cuda.synchronize()
    finally:
        engine_mod.ops.moe_route = orig
    return [int(t.unique().numel()) for t in picked]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ctx", type=int, default=2048)
    a = ap.parse_args()
    cfg = get_model_config("mixtral-8x7b")
    h, F, E, k = cfg.hidden, cfg.moe_ffn, cfg.num_experts, cfg.experts_per_token
    expert_bytes = 3 * h * F * 2
    print(f"# MoE decode A/B: mixtral-8x7b dimensions (hidden {h}, {E} experts x ffn {F}, top-{k}, GQA "
          f"{cfg.heads}/{cfg.kv_heads}), bf16, context {a.ctx}, {torch.cuda.get_device_name(0)}")
    print(f"# eager = knob moe_decode_fused off (MoEMLP module per layer, no graph); fused = knob on (routed-expert "
          f"kernels, captured graph with in-graph sampling)")
    print(f"# ms per decode step: median (min-max) of {a.reps} x {a.steps} steps after {a.warmup} warm-up steps, modes alternated")
    ms, kern, routed = {}, {}, {}
    for L in (2, 4):
        engs = {"eager": make_engine(L, a.ctx, False), "fused": make_engine(L, a.ctx, True)}
        assert engs["fused"].use_graphs and not engs["eager"].use_graphs
        seqs = {m: prefill(e, a.ctx) for m, e in engs.items()}
        for B in BATCHES:
            plans = {m: engs[m].decode_plan(seqs[m][:B]) for m in engs}
            t = {m: [] for m in engs}
            for _ in range(a.reps):
                for m in ("eager", "fused"):
                    t[m].append(time_steps(engs[m], plans[m], a.steps, a.warmup))
            for m in engs:
                ms[(L, B, m)] = statistics.median(t[m])
                kern[(L, B, m)] = count_kernels(engs[m], plans[m])
            routed[(L, B)] = routed_experts(engs["fused"], plans["fused"])
            print(f"layers {L} batch {B:2d}: eager {ms[(L, B, 'eager')]:7.3f} ms/step ({min(t['eager']):.3f}-"
                  f"{max(t['eager']):.3f})  fused {ms[(L, B, 'fused')]:7.3f} ms/step ({min(t['fused']):.3f}-"
                  f"{max(t['fused']):.3f})  (kernels per uncaptured step: eager {kern[(L, B, 'eager')]}, fused "
                  f"{kern[(L, B, 'fused')]}; distinct experts per layer {routed[(L, B)]})")
        for e in engs.values():
            e.close()
        del engs, seqs
        _MODELS.clear()
        torch.cuda.empty_cache()
    print("#")
    print("# per layer (slope between the 4- and the 2-layer slice)")
    print("# batch | eager ms/layer | fused ms/layer | speed-up | kernels/layer eager | fused | expert MB a step must "
          "move per layer (all experts)")
    for B in BATCHES:
        pe = (ms[(4, B, "eager")] - ms[(2, B, "eager")]) / 2
        pf = (ms[(4, B, "fused")] - ms[(2, B, "fused")]) / 2
        ke, kf = (None if kern[(4, B, m)] is None or kern[(2, B, m)] is None else (kern[(4, B, m)] - kern[(2, B, m)]) / 2
                  for m in ("eager", "fused"))
        need = statistics.mean(routed[(4, B)]) * expert_bytes / 1e6
        print(f"{B:7d} | {pe:14.3f} | {pf:14.3f} | {pe / pf:7.2f}x | {ke!s:>19} | {kf!s:>5} | {need:8.0f} ({E * expert_bytes / 1e6:.0f})")
    for B in BATCHES:
        for L in (2, 4):
            r = ms[(L, B, "eager")] / ms[(L, B, "fused")]
            print(f"# whole step, {L} layers, batch {B}: fused is {r:.2f}x the eager path's speed"
                  + ("" if r > 1 else "  (NOT faster)"))


if __name__ == "__main__":
    main()
