"""Engine helpers for the quantised-decode-weight tests: the tiny model on the lossless int4 grid
(int4 and bf16 decode then stream the same weight values) and a teacher-forced run that records
every step's logits."""

from __future__ import annotations

import torch

from llmctl.testing.numerics import snap_int4_grid

_GRID_MODEL: dict = {}


def grid_engine(device: str = "cuda", model: str = "tiny", **kw):
    """``InferenceEngine`` on the tiny model (or another template, e.g. ``tiny-moe``) with every
    projection the quantised path can take (the LM head and an MoE layer's experts too) snapped by
    :func:`snap_int4_grid`.  The model is built once per device."""
    from llmctl.models import build_model, get_model_config
    from llmctl.serve.engine import InferenceEngine

    class GridEngine(InferenceEngine):
        def _load(self, model_path, dtype, seed):
            key = (str(self.device), dtype) if model_path == "tiny" else (str(self.device), dtype, model_path)
            if key not in _GRID_MODEL:
                cfg = get_model_config(model_path)
                model = build_model(cfg, device=self.device, dtype=dtype, seed=seed)
                with torch.no_grad():
                    ws = [getattr(layer, n, None) for layer in model.layers for n in self._W8_NAMES] + [model.head_weight()]
                    for layer in model.layers:
                        if layer.moe is not None:
                            ws += list(layer.moe.experts_up) + list(layer.moe.experts_down)
                    for w in ws:
                        if w is not None and w.dim() == 2 and w.shape[0] % 64 == 0 and w.shape[1] % 128 == 0:
                            w.copy_(snap_int4_grid(w))
                _GRID_MODEL[key] = (model, cfg)
            model, cfg = _GRID_MODEL[key]
            return model, cfg, None

    kw = {"block_size": 16, "max_model_len": 256, "seed": 0, **kw}
    return GridEngine(model, device=device, **kw)


def run_forced(eng, prompts, max_tokens, forced=None):
    """Greedy (or teacher-forced on ``forced[i]``) generation; returns (tokens per sequence, logits
    [sequence, step, vocab] fp32 on the CPU)."""
    from llmctl.serve.scheduler import SamplingParams

    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True)) for p in prompts]
    idx = {s.seq_id: i for i, s in enumerate(seqs)}
    rec: dict = {}
    greedy = eng.sample

    def sample(logits, batch):
        toks = greedy(logits, batch)
        out = []
        for row, s, t in zip(logits.float().cpu(), batch, toks):
            i = idx[s.seq_id]
            rec.setdefault(i, []).append(row)
            out.append(forced[i][len(s.output_ids)] if forced is not None else t)
        return out

    eng.sample = sample
    while any(s.status != "finished" for s in seqs):
        eng.step()
    return [s.output_ids for s in seqs], torch.stack([torch.stack(rec[i]) for i in range(len(seqs))])
