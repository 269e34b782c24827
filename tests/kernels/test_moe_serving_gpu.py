"""Serving a mixture-of-experts model on the GPU: the routed-expert decode kernels inside the
captured decode graph, against the same kernels uncaptured and the eager ``MoEMLP`` path."""

import pytest

pytestmark = pytest.mark.gpu

PROMPTS = [[1, 2, 3, 4, 5], [9] * 37, [7, 7], [3] * 70]


def _generate(native_lib, use_graphs=True, **knobs):
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    with InferenceEngine("tiny-moe", device="cuda", max_batch_size=4, num_kv_blocks=128, block_size=16,
                         max_model_len=512, use_graphs=use_graphs, perf_knobs=knobs or None) as e:
        seqs = e.generate(PROMPTS, SamplingParams(max_tokens=12, temperature=0.0))
        return [s.output_ids for s in seqs], dict(e.stats), e.use_graphs


@pytest.fixture(scope="module")
def fused_graph(native_lib):
    return _generate(native_lib)


def test_moe_graph_decode_matches_uncaptured(native_lib, fused_graph):
    """Graphs on, knob on: the MoE engine captures and replays, and its tokens are those of the same
    kernels launched uncaptured."""
    toks, stats, graphs = fused_graph
    assert graphs and stats["graph_replays"] > 0
    toks_e, stats_e, graphs_e = _generate(native_lib, use_graphs=False)
    assert not graphs_e and stats_e["graph_replays"] == 0
    assert toks == toks_e


def test_moe_fused_decode_matches_eager_module(native_lib, fused_graph):
    """Against the eager MoEMLP path (knob off): the first generated token of every sequence (pure
    prefill, the same code in both) is equal and more than 0.9 of all tokens agree (bf16 path
    differences)."""
    toks, _, _ = fused_graph
    toks_off, stats_off, graphs_off = _generate(native_lib, moe_decode_fused=0)
    assert not graphs_off and stats_off["graph_replays"] == 0
    assert [t[0] for t in toks] == [t[0] for t in toks_off]
    agree = sum(int(a == b) for s, t in zip(toks, toks_off) for a, b in zip(s, t))
    total = sum(len(s) for s in toks)
    print(f"fused vs eager MoE decode: {agree} of {total} tokens agree")
    assert agree / total > 0.9


def test_moe_async_pipeline_same_tokens(native_lib, fused_graph):
    """The asynchronous decode pipeline (step N + 1 launched before step N's tokens are read) and
    in-graph sampling apply to the MoE engine: same tokens with async_decode on and off."""
    toks, stats, _ = fused_graph
    assert stats.get("async_continued", 0) > 0
    toks_sync, stats_sync, _ = _generate(native_lib, async_decode=0)
    assert stats_sync.get("async_continued", 0) == 0 and stats_sync["graph_replays"] > 0
    assert toks == toks_sync
