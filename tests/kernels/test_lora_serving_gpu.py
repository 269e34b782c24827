"""Per-request LoRA adapters in the serving engine on the GPU: the scenarios of
``llmctl.testing.lora`` on ``csrc/lora_decode.hip`` behind the fused decode projections, the
captured LoRA graph family and the asynchronous pipeline, against the merged-weights CPU oracle."""

import pytest

from llmctl.testing import lora as L

pytestmark = pytest.mark.gpu

SCENARIOS = [L.check_merged_oracle, L.check_modes, L.check_base_rows_untouched, L.check_prefix_cache,
             L.check_slot_reuse, L.check_preemption, L.check_structure, L.check_extended_sampler, L.check_int4_base]


@pytest.mark.parametrize("scenario", SCENARIOS, ids=lambda f: f.__name__)
def test_lora_serving_gpu(native_lib, scenario):
    scenario("cuda")
