"""LoRA adapters for the serving engine: many fine-tunes of one base model served by one engine.

An adapter adds ``scale * B A`` (``scale = alpha / rank``) to any of the engine's four fused
projections of any layer -- ``wqkv`` (q, k, v rows), ``wo``, ``w_up`` (gate, up rows), ``w_down`` --
and a missing (layer, projection) means a zero delta.  The engine keeps the loaded adapters resident
in stacked per-projection tensors (``InferenceEngine.load_lora``) and every request picks one by name
(``SamplingParams.lora``); the decode hot path is ``ops.lora_delta`` (``csrc/lora_decode.hip``).

On disk an adapter is a directory with ``adapter_config.json`` (``r``, ``lora_alpha``,
``target_modules``) and ``adapter_model.safetensors``, in either key style:

* native: ``layers.{i}.{wqkv|wo|w_up|w_down}.lora_A`` / ``.lora_B``;
* PEFT / HF-Llama: ``...layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight`` and
  ``...layers.{i}.mlp.{gate,up,down}_proj.lora_{A,B}.weight``.  Separate q / k / v (gate / up)
  adapters become one adapter of the fused projection: their A matrices stacked along the rank
  axis, their B matrices block-placed on the output rows of their part (the exporter's row order:
  q, k, v; gate, up), so the fused rank is the sum of the parts' ranks.
"""

from __future__ import annotations

import json
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch

PROJECTIONS = ("wqkv", "wo", "w_up", "w_down")
LORA_RANKS = (16, 32, 64)  # the kernels' padded ranks (``InferenceEngine(max_lora_rank=...)``)


def projection_shapes(cfg) -> Dict[str, Tuple[int, int]]:
    """``(out features, in features)`` of the four fused projections of a dense decoder layer."""
    D = cfg.head_dim or cfg.hidden // cfg.heads
    kv = cfg.kv_heads or cfg.heads
    gated = cfg.activation == "silu"
    return {"wqkv": ((cfg.heads + 2 * kv) * D, cfg.hidden), "wo": (cfg.hidden, cfg.heads * D),
            "w_up": ((2 if gated else 1) * cfg.ffn, cfg.hidden), "w_down": (cfg.hidden, cfg.ffn)}


def _parts(cfg) -> Dict[str, Tuple[str, int, int]]:
    """HF module name -> (fused projection, first output row, rows)."""
    D = cfg.head_dim or cfg.hidden // cfg.heads
    kv = cfg.kv_heads or cfg.heads
    q, k = cfg.heads * D, kv * D
    return {"q_proj": ("wqkv", 0, q), "k_proj": ("wqkv", q, k), "v_proj": ("wqkv", q + k, k),
            "o_proj": ("wo", 0, cfg.hidden), "gate_proj": ("w_up", 0, cfg.ffn), "up_proj": ("w_up", cfg.ffn, cfg.ffn),
            "down_proj": ("w_down", 0, cfg.hidden)}


@dataclass
class LoRAAdapter:
    """``tensors[(layer, projection)] = (A [r, K], B [N, r])`` fp32; ``scale = alpha / rank``.  ``rank``
    is the nominal rank the scale is defined with; a fused (PEFT-imported) projection may hold a
    larger one (the sum of its parts)."""
    rank: int
    alpha: float
    tensors: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=dict)

    @property
    def scale(self) -> float:
        return float(self.alpha) / float(self.rank)

    @property
    def max_rank(self) -> int:
        """The largest rank any (layer, projection) holds: what ``max_lora_rank`` must cover."""
        return max([a.shape[0] for a, _ in self.tensors.values()], default=0)

    def padded(self, li: int, name: str, R: int, N: int, K: int):
        """``(A [R, K], B [N, R])`` zero-padded to rank ``R``, or None when the adapter leaves this
        projection alone.  Raises naming the rank needed when it does not fit."""
        t = self.tensors.get((li, name))
        if t is None:
            return None
        A, B = t
        r = A.shape[0]
        if tuple(A.shape) != (r, K) or tuple(B.shape) != (N, r):
            raise ValueError(f"LoRA adapter: layer {li} {name} has A {tuple(A.shape)}, B {tuple(B.shape)}; "
                             f"the model needs A [r, {K}], B [{N}, r]")
        if r > R:
            raise ValueError(f"LoRA adapter: layer {li} {name} needs rank {r} (after fusing), above the "
                             f"engine's max_lora_rank {R}")
        Ap = torch.zeros(R, K, dtype=A.dtype)
        Bp = torch.zeros(N, R, dtype=B.dtype)
        Ap[:r], Bp[:, :r] = A, B
        return Ap, Bp

    # ------------------------------------------------------------------ disk
    def save(self, path: str) -> None:
        """Write the native on-disk form."""
        from safetensors.torch import save_file

        p = Path(path)
        p.mkdir(parents=True, exist_ok=True)
        names = sorted({n for _, n in self.tensors})
        (p / "adapter_config.json").write_text(json.dumps({"r": self.rank, "lora_alpha": self.alpha,
                                                           "target_modules": names}))
        out = {}
        for (li, n), (A, B) in self.tensors.items():
            out[f"layers.{li}.{n}.lora_A"] = A.contiguous()
            out[f"layers.{li}.{n}.lora_B"] = B.contiguous()
        save_file(out, str(p / "adapter_model.safetensors"))

    @classmethod
    def load(cls, path: str, cfg) -> "LoRAAdapter":
        """Read an adapter directory in the native or the PEFT / HF-Llama key style."""
        from safetensors.torch import load_file

        p = Path(path)
        conf = json.loads((p / "adapter_config.json").read_text())
        rank, alpha = int(conf["r"]), float(conf["lora_alpha"])
        raw = load_file(str(p / "adapter_model.safetensors"))
        native: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
        hf: Dict[Tuple[int, str], Dict[str, torch.Tensor]] = {}
        pat_native = re.compile(r"(?:^|\.)layers\.(\d+)\.(wqkv|wo|w_up|w_down)\.lora_([AB])$")
        pat_hf = re.compile(r"(?:^|\.)layers\.(\d+)\.(?:self_attn|mlp)\.([a-z]+_proj)\.lora_([AB])(?:\.[a-z]+)?\.weight$")
        for key, t in raw.items():
            m = pat_native.search(key)
            if m:
                native.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = t.float()
                continue
            m = pat_hf.search(key)
            if m:
                hf.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = t.float()
                continue
            raise ValueError(f"LoRA adapter {path}: unrecognised tensor name {key!r}")
        ad = cls(rank, alpha)
        for k, ab in native.items():
            if set(ab) != {"A", "B"}:
                raise ValueError(f"LoRA adapter {path}: layer {k[0]} {k[1]} lacks lora_A or lora_B")
            ad.tensors[k] = (ab["A"], ab["B"])
        if hf:
            for k, t in fuse_hf(hf, cfg, path).items():
                if k in ad.tensors:
                    raise ValueError(f"LoRA adapter {path}: layer {k[0]} {k[1]} given in both key styles")
                ad.tensors[k] = t
        return ad


def fuse_hf(mods: Dict[Tuple[int, str], Dict[str, torch.Tensor]], cfg, where: str = "adapter"):
    """Per-HF-module ``{"A": [r, K], "B": [rows, r]}`` -> fused ``(A, B)`` per (layer, projection):
    the parts' A stacked along the rank axis, each B placed on its part's output rows and its own
    rank columns (zeros elsewhere), so ``B A`` is the row-wise concatenation of the parts' ``B A``."""
    parts, shapes = _parts(cfg), projection_shapes(cfg)
    order = list(parts)  # q, k, v / gate, up: the exporter's row order
    grouped: Dict[Tuple[int, str], List[Tuple[int, torch.Tensor, torch.Tensor]]] = {}
    for (li, mod), ab in sorted(mods.items(), key=lambda kv: (kv[0][0], order.index(kv[0][1]) if kv[0][1] in order else -1)):
        if mod not in parts:
            raise ValueError(f"LoRA {where}: module {mod!r} is not served (embedding / LM-head adapters are out of scope)")
        if set(ab) != {"A", "B"}:
            raise ValueError(f"LoRA {where}: layer {li} {mod} lacks lora_A or lora_B")
        name, row0, rows = parts[mod]
        N, K = shapes[name]
        A, B = ab["A"].float(), ab["B"].float()
        if A.shape[1] != K or B.shape[0] != rows or B.shape[1] != A.shape[0]:
            raise ValueError(f"LoRA {where}: layer {li} {mod} has A {tuple(A.shape)}, B {tuple(B.shape)}; "
                             f"the model needs A [r, {K}], B [{rows}, r]")
        grouped.setdefault((li, name), []).append((row0, A, B))
    out = {}
    for (li, name), items in grouped.items():
        N, K = shapes[name]
        r = sum(A.shape[0] for _, A, _ in items)
        Af, Bf = torch.zeros(r, K), torch.zeros(N, r)
        c = 0
        for row0, A, B in items:
            Af[c:c + A.shape[0]] = A
            Bf[row0:row0 + B.shape[0], c:c + A.shape[0]] = B
            c += A.shape[0]
        out[(li, name)] = (Af, Bf)
    return out


def random_adapter(cfg, rank: int = 8, seed: int = 0, std: float = 0.02, alpha: Optional[float] = None,
                   layers=None, projections=PROJECTIONS) -> LoRAAdapter:
    """An adapter with normal(0, std) A and B on every listed (layer, projection): tests, benchmarks.
    (A trained adapter starts from B = 0; a random B makes the delta visible.)"""
    g = torch.Generator().manual_seed(seed)
    shapes = projection_shapes(cfg)
    ad = LoRAAdapter(rank, float(alpha if alpha is not None else 2 * rank))
    for li in (range(cfg.layers) if layers is None else layers):
        for name in projections:
            N, K = shapes[name]
            ad.tensors[(li, name)] = (torch.randn(rank, K, generator=g) * std, torch.randn(N, rank, generator=g) * std)
    return ad


@torch.no_grad()
def merge_into(model, adapter: LoRAAdapter):
    """``W += scale * B A`` in fp32 on the model's fused projection weights (rounded back to the
    weight's dtype): the end-to-end oracle of adapter serving, and the way to export a merged model."""
    for (li, name), (A, B) in adapter.tensors.items():
        w = getattr(model.layers[li], name)
        d = adapter.scale * (B.float() @ A.float())
        w.copy_((w.float() + d.to(w.device)).to(w.dtype))
    return model
