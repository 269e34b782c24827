"""Prompt scoring end to end on the GPU: ``csrc/prompt_logprobs.hip`` behind the prefill and mixed
steps, against the CPU fp32 teacher-forced oracle (scenarios: ``llmctl/testing/prompt_logprobs.py``)."""

import pytest

from llmctl.testing import prompt_logprobs as scenarios

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_bound_is_measured():
    """2 x the existing GPU engine's teacher-forced error on the prompt tokens' logprobs; printed
    (and recorded in profiles/prompt_logprobs.txt)."""
    assert 0 < scenarios.bound(DEV) < 6e-2


@pytest.mark.parametrize("scenario", ["check_concurrent", "check_chunked", "check_mixed", "check_score_only",
                                      "check_prefix_cache", "check_preemption", "check_interactions",
                                      "check_folded", "check_tp_refusal"])
def test_scenario(scenario):
    getattr(scenarios, scenario)(DEV)
