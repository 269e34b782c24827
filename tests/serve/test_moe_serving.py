"""Serving a mixture-of-experts model on the CPU (the eager MoE path): greedy decode must follow
the model's full forward."""

import torch

from llmctl.serve.engine import InferenceEngine
from llmctl.serve.scheduler import SamplingParams


def test_moe_greedy_decode_matches_full_forward():
    e = InferenceEngine("tiny-moe", device="cpu", max_batch_size=4, num_kv_blocks=64, block_size=8,
                        max_model_len=256, max_batch_tokens=512)
    prompts = [[1, 2, 3, 4, 5], [9] * 37, [7, 7], [3] * 70]
    seqs = e.generate(prompts, SamplingParams(max_tokens=12, temperature=0.0))
    assert not e.use_graphs
    for s in seqs:
        assert len(s.output_ids) == 12 and s.finish_reason == "length"
        logits = e.model(torch.tensor([s.all_ids[:-1]]))
        ref_next = logits.view(-1, logits.shape[-1]).argmax(-1)[len(s.prompt_ids) - 1:].tolist()
        assert ref_next == s.output_ids
