"""Penalties and logprobs through the serving engine on the GPU: the ``sample_ext`` kernel inside
the extended decode graph, the asynchronous pipeline and the eager path (scenarios:
``llmctl.testing.sampling_ext``; the CPU twin is ``tests/serve/test_sampling_ext_serving.py``)."""

import pytest

from llmctl.testing import sampling_ext as scen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tol():
    # 4 x torch's fp32 log_softmax error against fp64 on 64 x 32000 logits (1-2e-6 on MI355X:
    # profiles/sampling_ext.txt); every mode runs the same kernel, so the logprobs usually agree exactly
    return scen.lp_tolerance("cuda")


def test_huge_penalty_gives_distinct_tokens(native_lib):
    scen.check_distinct_tokens("cuda")


@pytest.mark.parametrize("temperature", [0.0, 0.9])
def test_modes_agree(native_lib, tol, temperature):
    scen.check_mode_equivalence("cuda", temperature, tol)


def test_preempted_sequence_resumes_with_its_state(native_lib):
    scen.check_preemption("cuda")


def test_plain_batches_leave_no_trace_and_slots_return(native_lib):
    scen.check_structure("cuda")


def test_logprob_fields(native_lib, tol):
    scen.check_logprob_fields("cuda", tol)
