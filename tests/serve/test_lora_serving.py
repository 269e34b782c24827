"""Per-request LoRA adapters in the serving engine on the CPU (the fp32 oracle behind ``ops``): the
scenarios of ``llmctl.testing.lora``; the GPU suite runs the same functions on the HIP kernels."""

import pytest

from llmctl.testing import lora as L

SCENARIOS = [L.check_merged_oracle, L.check_modes, L.check_base_rows_untouched, L.check_prefix_cache,
             L.check_slot_reuse, L.check_preemption, L.check_structure, L.check_extended_sampler]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
def test_lora_serving_cpu(scenario):
    scenario("cpu")
