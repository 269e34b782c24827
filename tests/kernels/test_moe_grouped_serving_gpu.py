"""Serving ``tiny-moe`` with ``moe_max_rows`` above 64: prefill chunks and decode steps of more than 64
rows on the grouped-expert kernels (csrc/moe_grouped.hip), the latter inside the captured graph."""

import pytest

pytestmark = pytest.mark.gpu


def _generate(prompts, max_tokens, **kw):
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    with InferenceEngine("tiny-moe", device="cuda", block_size=16, max_model_len=512, **kw) as e:
        seqs = e.generate(prompts, SamplingParams(max_tokens=max_tokens, temperature=0.0))
        return [s.output_ids for s in seqs], dict(e.stats)


def test_moe_grouped_prefill_matches_default_engine(native_lib):
    # test_moe_serving_gpu.py's prompts, the 37-token one grown to 200.  (A 200-token prompt of mixed
    # tokens, (5 i) % 97 + 1, is no usable reference: the default engine's own greedy continuation of
    # it changes at the fifth token with the prefill chunking alone, 234 vs 212 at 256-token steps.)
    prompts = [[3] * 70, [9] * 200, [1, 2, 3, 4, 5], [7, 7]]
    # the scheduler packs all four prompts into one prefill step of 277 rows, so the limit is 512
    kw = dict(max_batch_size=4, num_kv_blocks=128)
    toks, stats = _generate(prompts, 12, moe_max_rows=512, **kw)
    assert stats["moe_grouped_steps"] > 0
    toks_d, stats_d = _generate(prompts, 12, **kw)
    assert stats_d["moe_grouped_steps"] == 0
    agree = sum(int(a == b) for s, t in zip(toks, toks_d) for a, b in zip(s, t))
    total = sum(len(s) for s in toks)
    print(f"grouped vs eager MoE prefill: {agree} of {total} tokens agree")
    assert agree / total > 0.9


def test_moe_grouped_decode_in_graph_matches_uncaptured(native_lib):
    prompts = [[1 + i % 90, 2 + i % 7, 3] for i in range(80)]
    kw = dict(max_batch_size=96, num_kv_blocks=256, moe_max_rows=128)
    toks, stats = _generate(prompts, 4, **kw)
    assert stats["graph_replays"] > 0 and stats["moe_grouped_steps"] > 0
    toks_e, stats_e = _generate(prompts, 4, use_graphs=False, **kw)
    assert stats_e["graph_replays"] == 0
    assert toks == toks_e
