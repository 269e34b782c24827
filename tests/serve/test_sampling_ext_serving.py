"""Penalties and logprobs through the serving engine on the CPU (the ``sample_ext`` oracle behind
``ops``); ``tests/kernels/test_sampling_ext_serving_gpu.py`` runs the same scenarios on the GPU."""

import types

import pytest

from llmctl.serve.scheduler import SamplingParams
from llmctl.testing import sampling_ext as scen


@pytest.fixture(scope="module")
def tol():
    return scen.lp_tolerance("cpu")


def test_huge_penalty_gives_distinct_tokens():
    scen.check_distinct_tokens("cpu")


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_modes_agree(tol, temperature):
    scen.check_mode_equivalence("cpu", temperature, tol)


def test_preempted_sequence_resumes_with_its_state():
    scen.check_preemption("cpu")


def test_plain_batches_leave_no_trace_and_slots_return():
    scen.check_structure("cpu")


def test_logprob_fields(tol):
    scen.check_logprob_fields("cpu", tol)


def test_tp_refuses_extended_requests():
    """TP > 1: the sampler state lives on one rank only; the request is refused by name."""
    from llmctl.serve.tp import TPInferenceEngine

    eng = types.SimpleNamespace(tp_size=2)
    with pytest.raises(ValueError, match="frequency_penalty, logprobs.*tensor parallelism"):
        TPInferenceEngine.add_request(eng, [1, 2], SamplingParams(frequency_penalty=0.5, logprobs=1))
