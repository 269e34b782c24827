"""``InferenceEngine(expert_weight_dtype=...)`` on tiny-moe: fp8 / int4 experts in the captured decode graphs."""

import pytest
import torch

from llmctl.testing.decode_wq import grid_engine, run_forced
from llmctl.testing.numerics import row_err

pytestmark = pytest.mark.gpu

PROMPTS = [[(11 * i + r) % 400 + 1 for i in range(5 + r)] for r in range(6)]


def _engine(**kw):
    return grid_engine(model="tiny-moe", max_batch_size=8, num_kv_blocks=128, **kw)


@pytest.mark.parametrize("kind", ["int4", "fp8"])
def test_engine_expert_weight_dtype(native_lib, kind):
    """Experts on the lossless int4 grid: the int4 engine follows the bf16 engine's logits on the same
    token stream; either kind replays captured graphs and decodes the tokens of its uncaptured run."""
    eng = _engine(expert_weight_dtype=kind)
    assert eng.expert_weight_dtype == kind and eng.weight_dtype == "auto" and eng._moe_fused(6)
    toks, lg = run_forced(eng, PROMPTS, 6)
    assert eng.stats["graph_replays"] > 0 and torch.isfinite(lg).all()
    eng.close()
    eager = _engine(expert_weight_dtype=kind, use_graphs=False)
    toks_eager, _ = run_forced(eager, PROMPTS, 6)
    assert eager.stats["graph_replays"] == 0 and toks_eager == toks
    eager.close()
    assert eager._moe_q is None  # close() releases the copies
    if kind == "int4":
        ref_eng = _engine()
        assert ref_eng.expert_weight_dtype == "auto" and ref_eng._moe_q is None
        toks_ref, lg_ref = run_forced(ref_eng, PROMPTS, 6)
        ref_eng.close()
        eng = _engine(expert_weight_dtype=kind)
        _, lg = run_forced(eng, PROMPTS, 6, forced=toks_ref)
        eng.close()
        err = row_err(lg[:, 1:].reshape(-1, lg.shape[-1]), lg_ref[:, 1:].reshape(-1, lg_ref.shape[-1]))
        print(f"int4-expert engine decode logits row_err {err:.3e}")
        assert err < 3e-2, err
