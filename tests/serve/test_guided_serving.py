"""Guided decoding through the serving engine on the CPU (the ``sample_guided`` oracle behind
``ops``); ``tests/kernels/test_guided_serving_gpu.py`` runs the same scenarios on the GPU."""

import pytest

from llmctl.testing import guided as scen


@pytest.fixture(scope="module")
def tol():
    return scen.lp_tolerance("cpu")


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_guided_outputs_conform(temperature):
    scen.check_conformance("cpu", temperature)


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_modes_agree(temperature):
    scen.check_mode_equivalence("cpu", temperature)


def test_preempted_sequence_resumes_mid_pattern():
    scen.check_preemption("cpu")


def test_plain_runs_leave_no_trace_and_slots_return():
    scen.check_structure("cpu")


def test_guide_composes_with_penalties_and_logprobs(tol):
    scen.check_composition("cpu", tol)


def test_guide_composes_with_a_lora_adapter():
    scen.check_lora_composition("cpu")
