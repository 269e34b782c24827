"""Guided decoding through the serving engine on the GPU: the ``sample_guided`` kernel inside the
guided decode graph, the asynchronous pipeline and the eager path (scenarios:
``llmctl.testing.guided``; the CPU twin is ``tests/serve/test_guided_serving.py``)."""

import pytest

from llmctl.testing import guided as scen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tol():
    # 4 x torch's fp32 log_softmax error against fp64 on 64 x 32000 logits, as for the extended sampler
    return scen.lp_tolerance("cuda")


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_guided_outputs_conform(native_lib, temperature):
    scen.check_conformance("cuda", temperature)


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_modes_agree(native_lib, temperature):
    scen.check_mode_equivalence("cuda", temperature)


def test_preempted_sequence_resumes_mid_pattern(native_lib):
    scen.check_preemption("cuda")


def test_plain_runs_leave_no_trace_and_slots_return(native_lib):
    scen.check_structure("cuda")


def test_guide_composes_with_penalties_and_logprobs(native_lib, tol):
    scen.check_composition("cuda", tol)


def test_guide_composes_with_a_lora_adapter(native_lib):
    scen.check_lora_composition("cuda")
