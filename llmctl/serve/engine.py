"""Inference engine: batched prefill + paged-KV decode on llmctl's HIP kernels, with
hipGraph-captured decode steps.

Reference ``InferenceEngine`` (``server.py:127-251``) re-ran a full-prefix HF forward for
every generated token with ``use_cache=True`` but discarded the cache, right-padded
batches and read the logits of the padded last position (wrong tokens for shorter
prompts), and sampled with a host sync per request per token.  Here:

* prefill (round 2): CHUNKED and prefix-aware.  The scheduler hands out chunks (sequence,
  first position, count) under a per-step token budget; the chunks of all sequences are packed
  back to back (no padding), RoPE'd and written into the paged cache in one fused pass, and
  attend through ``paged_prefill_attention`` (csrc/paged_prefill.hip): every query reads its
  keys from the block table, so a cached prefix (earlier chunk, prefix-cache hit, resumed
  sequence) and the chunk itself are one key range.  Logits are taken only at the last token
  of chunks that complete a sequence's known tokens -- and, for requests that score their prompt
  (``SamplingParams.prompt_logprobs``), at the prompt rows still to score, in tiles that go
  through ``ops.prompt_logprobs`` (the next token's logprob, rank and top list per row);
* decode: one token per running sequence; per layer ``rope_qkv`` (explicit positions) ->
  ``kv_cache_write`` -> ``paged_attention_decode`` (block tables, GQA) -> o-proj -> MLP;
  the whole decode step (embedding .. lm_head) is captured once per batch-size bucket in
  a HIP graph and replayed with static input buffers (no per-layer launch overhead);
* sampling: one batched kernel (temperature / top-k / top-p / greedy) with uniforms drawn
  once per step; the only host sync per step is reading the sampled ids.  Requests with
  repetition / presence / frequency penalties or logprobs sample through ``ops.sample_ext``,
  which keeps the per-sequence token counts on the device and returns the logprobs with the ids.
  Guided requests (regex / choice / JSON schema, ``llmctl/serve/guided.py``) sample through
  ``ops.sample_guided``: the compiled token automaton sits in a preallocated device arena and the
  sampler masks the logits by, and advances, the row's automaton state inside the step.
"""

from __future__ import annotations

import logging
import math
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from llmctl import ops
from llmctl.config.knobs import use as use_knobs
from llmctl.io.artifact import load_model
from llmctl.models import DecoderLM
from llmctl.utils.env import graph_capture_gc_guard

from .block_manager import PagedKVCache, make_kv_manager
from .prefix_cache import PrefixCache
from .scheduler import ContinuousBatchScheduler, PrefillChunk, SamplingParams, Sequence
from .tokenizer import load_tokenizer

log = logging.getLogger("llmctl.serve")


class InferenceEngine:
    def __init__(self, model_path: str = "tiny", device: str = "auto", dtype=torch.bfloat16, max_batch_size: int = 8,
                 max_batch_tokens: int = 8192, max_model_len: Optional[int] = None, kv_cache_fraction: float = 0.85,
                 block_size: int = 16, num_kv_blocks: Optional[int] = None, scheduler: str = "dynamic",
                 use_graphs: bool = True, seed: int = 0, pc=None, prefix_caching: bool = True,
                 tuning_cache: Optional[str] = None, perf_knobs: Optional[Dict] = None,
                 kv_cache_dtype: str = "auto", weight_dtype: str = "auto", max_loras: int = 0,
                 max_lora_rank: int = 16, guide_table_words: int = 1 << 18):
        from llmctl.config import knobs as perf

        self.knobs = perf.configure(perf_knobs)  # defaults + perf_knobs + LLMCTL_KNOBS
        if device == "auto":
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device.type == "cpu" and dtype == torch.bfloat16:
            dtype = torch.float32  # the CPU oracle path
        if self.device.type == "cuda":  # pre-tuned prefill projection GEMMs (llmctl.exec.gemm_tuning)
            from llmctl.exec.gemm_tuning import enable_tuned_gemms

            enable_tuned_gemms()
        from llmctl.plugins import tuning_cache as _tc

        tc = _tc.resolve(tuning_cache)
        self.tuned = _tc.apply_serving(tc) if tc is not None else {}
        self.knobs = perf.knobs()  # perf_knobs + tuning cache + LLMCTL_KNOBS: this engine's routing
        self.dtype = dtype
        self.model_path = model_path
        self.model: DecoderLM
        self.pc = pc
        self.tp = pc.tp_size if pc is not None else 1
        self.model, self.cfg, self.ckpt = self._load(model_path, dtype, seed)
        self.model.eval()
        self.tokenizer = load_tokenizer(str(self.ckpt) if self.ckpt else None)
        cfg = self.cfg
        self.max_model_len = max_model_len or cfg.max_position_embeddings
        self.block_size = block_size
        self.max_blocks_per_seq = (self.max_model_len + block_size - 1) // block_size
        # decode projection weights: the model's ("auto"), or a quantised copy that the fused decode
        # path streams instead (the decode GEMMs are HBM-bound): "fp8" = OCP e4m3fn with fp32 row
        # scales (W8A16, half the bytes), "int4" = group-128 int4 with fp32 group scales (W4A16, 4.25
        # bits per weight).  Prefill keeps the bf16 weights.  Made before the KV cache is sized.
        self._wq: Optional[List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]] = None
        self._wq_head: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._wq_kind: Optional[str] = None
        if weight_dtype in ("fp8", "fp8_e4m3", "float8_e4m3fn"):
            self._wq_kind = "fp8"
        elif weight_dtype in ("int4", "int4-g128", "w4a16"):
            self._wq_kind = "int4"
        elif weight_dtype not in ("auto", "model", "bf16", "bfloat16"):
            raise ValueError(f"weight_dtype must be auto / bf16 / fp8 / int4, got {weight_dtype!r}")
        if self._wq_kind is not None and self.device.type == "cuda":
            self._wq = self._quantize_decode_weights(self._wq_kind)
        self.weight_dtype = self._wq_kind if self._wq is not None else "auto"
        # prefill with the RMSNorms folded into the QKV / gate-up projections (knob
        # prefill_norm_fold): copies of those weights with the norm weight multiplied into their K
        # columns ((H + 2 kv) D + 2 F) H bf16 per layer, made before the KV cache is sized
        self._nf: Optional[List[Tuple[torch.Tensor, torch.Tensor]]] = (
            self._fold_norm_weights() if self.knobs.prefill_norm_fold else None)
        # LoRA adapters (llmctl/serve/lora.py): ``max_loras`` resident slots of rank ``max_lora_rank``
        # per (layer, projection), made before the KV cache is sized; 0 = none, nothing changes
        self.max_loras, self.max_lora_rank = int(max_loras), int(max_lora_rank)
        self._lora: Optional[List[Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]]] = None
        self._lora_slots: Dict[str, int] = {}  # adapter name -> slot
        self._lora_salt: Dict[str, bytes] = {}  # adapter name -> prefix-cache salt of this load
        self._lora_scale: Dict[int, float] = {}  # slot -> scale (host copy, for the eager prefill)
        if self.max_loras > 0:
            self._lora = self._alloc_lora()
        # KV cache element: the model dtype ("auto"), or OCP fp8 e4m3fn ("fp8": half the bytes per
        # token, so twice the blocks and half the decode attention's HBM stream; saturating at +-448)
        if kv_cache_dtype in ("auto", "model", "bf16", "bfloat16"):
            self.kv_dtype = dtype
        elif kv_cache_dtype in ("fp8", "fp8_e4m3", "float8_e4m3fn"):
            self.kv_dtype = torch.float8_e4m3fn
        else:
            raise ValueError(f"kv_cache_dtype must be auto / bf16 / fp8, got {kv_cache_dtype!r}")
        if num_kv_blocks is None:
            if self.device.type == "cuda":
                torch.cuda.synchronize()
                free, _ = torch.cuda.mem_get_info(self.device)
                budget = free * kv_cache_fraction
            else:
                budget = 256 * 2 ** 20
            num_kv_blocks = PagedKVCache.blocks_for_memory(budget, cfg.layers, block_size, cfg.kv_heads // self.tp,
                                                           cfg.head_dim, torch.tensor([], dtype=self.kv_dtype).element_size())
            num_kv_blocks = min(num_kv_blocks, 1 << 20)
            num_kv_blocks = self._agree_min(num_kv_blocks)
        # each TP rank caches only its own KV heads
        self.kv_cache = PagedKVCache(cfg.layers, num_kv_blocks, block_size, cfg.kv_heads // self.tp, cfg.head_dim,
                                     self.kv_dtype, self.device)
        self.kv = make_kv_manager(num_kv_blocks, block_size)
        self.prefix_cache = PrefixCache(self.kv, block_size) if prefix_caching else None
        self.scheduler = ContinuousBatchScheduler(self.kv, max_batch_size, max_batch_tokens, self.max_model_len,
                                                  scheduler, block_size, prefix_cache=self.prefix_cache)
        self.max_batch_size = max_batch_size
        self.rope = self.model.rope_tables(self.max_model_len, self.device)
        # MoE decode on the routed-expert kernels (ops.moe_route / moe_decode_up_swiglu /
        # moe_decode_down_add_rmsnorm): per layer, the pointer tables of the expert weights
        self._moe: Optional[List[Tuple[ops.MoEExpertTable, ops.MoEExpertTable]]] = self._moe_tables()
        if self._moe is not None and self._wq is not None:
            log.info("engine: %s decode weights cover the attention projections; the experts stay bf16",
                     self.weight_dtype)
        # the eager MoE module sizes the expert segments on the host: graphs only on the routed kernels
        self.use_graphs = use_graphs and self.device.type == "cuda" and (not cfg.is_moe or self._fused_decode())
        self._graphs: Dict[int, Tuple[torch.cuda.CUDAGraph, Dict[str, torch.Tensor]]] = {}
        # batches with an extended row (penalties / logprobs, ``SamplingParams.extended``) replay a
        # second graph per bucket whose body samples with ``ops.sample_ext``; plain batches never
        # touch it.  The penalties' per-sequence state (token counts int32 + prompt mask uint8,
        # [max_batch_size, V]) lives on the device -- an asynchronous step is launched before the
        # previous step's tokens reach the host -- and is allocated on first need.
        self._graphs_ext: Dict[int, Tuple[torch.cuda.CUDAGraph, Dict[str, torch.Tensor]]] = {}
        # batches with an adapter row replay a third family, keyed (bucket, extended): the same body
        # with every projection's ``ops.LoRARows`` passed down and a static per-row ``lora_idx``
        self._graphs_lora: Dict[Tuple[int, bool], Tuple[torch.cuda.CUDAGraph, Dict[str, torch.Tensor]]] = {}
        # batches with a guided row replay a fourth family (and the LoRA family's kind 2): the body
        # samples with ``ops.sample_guided``.  The guides' tables live in an arena allocated on first
        # need: G = max_batch_size table slots (shared by sequences with the same guide, reference
        # counted) and one automaton-state word per row slot.  Addresses never change, so uploading a
        # guide is a copy into its slot and captured graphs stay valid.
        self._graphs_guided: Dict[int, Tuple[torch.cuda.CUDAGraph, Dict[str, torch.Tensor]]] = {}
        self.guide_table_words = int(guide_table_words)
        self._guide_arena: Optional[Dict[str, torch.Tensor]] = None
        self._guide_tables: Dict[Tuple, List[int]] = {}  # guide key -> [table slot, references]
        self._guide_table_free: List[int] = []
        self._sampler_state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        # row slots: one per running sequence that needs device-resident sampler state -- the
        # penalties' counts row and / or the guide's state word share the index
        self._sampler_free: List[int] = list(range(max_batch_size - 1, -1, -1))
        self._ext_step: Optional[Dict[str, np.ndarray]] = None  # the extended fields of the step being launched
        self._ext_out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None  # its logprob outputs
        self._host_lp: Optional[List] = None  # logprob rows of the last host-sampled batch
        # prompt scoring (``SamplingParams.prompt_logprobs``): the logits of at most SCORE_TILE prompt
        # rows at a time, [SCORE_TILE, V] in the model dtype (64 MB at V = 32000), allocated on
        # first need; steps without a scoring row never touch either
        self._score_scratch: Optional[torch.Tensor] = None
        self._score_out: Optional[Tuple] = None  # (segments, host results, event) of the step just run
        self.scheduler.on_release = self._release_sampler_slot
        # sampling uniforms come from the host (one H2D copy with the step's other inputs), so
        # in-graph sampling and the eager path draw the same stream
        self._np_rng = np.random.default_rng(seed)
        self._pending: Optional[Dict] = None  # an in-flight asynchronous decode step
        self._last_toks: Optional[torch.Tensor] = None  # eager path: the last step's sampled ids
        self.stats = {"steps": 0, "prefill_tokens": 0, "decode_tokens": 0, "graph_replays": 0}
        log.info("engine: %s on %s, %d KV blocks x %d tokens (%.1f GB)", cfg.name, self.device, num_kv_blocks,
                 block_size, self.kv_cache.nbytes / 1e9)

    def _fold_norm_weights(self) -> Optional[List[Tuple[torch.Tensor, torch.Tensor]]]:
        """(W_qkv * w_attn_norm, W_up * w_mlp_norm) per layer, or None when the model does not fit
        the folded prefill (GPU, TP=1, RMSNorm, RoPE, dense SwiGLU MLP without biases, gemm64 shapes)."""
        cfg, m = self.cfg, self.model
        if (self.device.type != "cuda" or self.tp != 1 or cfg.is_moe or not cfg.gated_mlp or cfg.norm != "rmsnorm"
                or cfg.position != "rope" or cfg.hidden % 128 or cfg.hidden < 256):
            return None
        out = []
        for layer in m.layers:
            if (layer.moe is not None or layer.bqkv is not None or layer.bo is not None or layer.b_up is not None
                    or layer.b_down is not None or layer.wqkv.shape[0] % 256 or layer.w_up.shape[0] % 256
                    or layer.w_down.shape[0] % 256):
                return None
            out.append(((layer.wqkv.float() * layer.attn_norm_w.float()).to(layer.wqkv.dtype).contiguous(),
                        (layer.w_up.float() * layer.mlp_norm_w.float()).to(layer.w_up.dtype).contiguous()))
        return out

    MOE_MAX_ROWS = 64  # the routed-expert decode kernels take at most 64 token rows (ops.moe_decode_ok)

    def _moe_tables(self):
        """(up, down) ``ops.MoEExpertTable`` per layer, or None when the model's MoE MLPs do not fit
        the routed-expert decode kernels (GPU, TP = 1, EP = 1, bf16, every layer routed, dimensions
        within ``ops.moe_decode_ok``)."""
        cfg = self.cfg
        if not cfg.is_moe or self.device.type != "cuda" or self.tp != 1 or self.dtype != torch.bfloat16:
            return None
        probe = torch.empty(1, cfg.hidden, dtype=self.dtype, device=self.device)
        if not ops.moe_decode_ok(probe, cfg.num_experts, cfg.experts_per_token, cfg.hidden, cfg.moe_ffn):
            return None
        out = []
        for layer in self.model.layers:
            moe = layer.moe
            if moe is None or moe.ep != 1 or moe.w_router.dtype != torch.bfloat16 or not moe.w_router.is_contiguous():
                return None
            up, down = ops.MoEExpertTable(moe.experts_up), ops.MoEExpertTable(moe.experts_down)
            if (up.dtype != torch.bfloat16 or down.dtype != torch.bfloat16 or up.E != cfg.num_experts
                    or up.shape != (2 * cfg.moe_ffn, cfg.hidden) or down.shape != (cfg.hidden, cfg.moe_ffn)):
                return None
            out.append((up, down))
        return out

    def _moe_fused(self, n: int = 1) -> bool:
        """MoE MLPs of an ``n``-row decode step on the routed-expert kernels (knob
        ``moe_decode_fused`` off: the eager ``MoEMLP`` module, A/B)."""
        return self._moe is not None and self.knobs.moe_decode_fused and n <= self.MOE_MAX_ROWS

    def _graph_ok(self, n: int) -> bool:
        """Does an ``n``-row decode step replay a captured graph?  (MoE: buckets above the routed
        kernels' row limit run eagerly through the ``MoEMLP`` module, which syncs with the host.)"""
        return self.use_graphs and (not self.cfg.is_moe or self._moe_fused(self._bucket(n)))

    def _norm_fold_ok(self, T: int, lora=None) -> bool:
        if lora is not None:  # a step with adapter rows takes the unfolded layers
            return False
        return self._nf is not None and self.knobs.prefill_norm_fold and T > 0 and T % 256 == 0

    def _prefill_layers_folded(self, x, pos, slots, fa, doc, bt, cu, ctx, work):
        """The prefill layers with each RMSNorm folded into the projection that consumes it: per layer
        rstd(h) -> QKV GEMM scaling its rows by rstd -> RoPE + cache write -> attention -> h += o W_o^T
        (hipBLASLt beta = 1) -> rstd(h) -> gate/up GEMM with row scale and SwiGLU -> h += act W_down^T
        (gemm64 accumulate epilogue).  Returns the residual stream h [T, H] after the last layer (the
        final norm is applied to the selected rows only)."""
        T = x.shape[0]
        eps = self.cfg.layer_norm_eps
        kc, vc = self.kv_cache.k, self.kv_cache.v
        h = x.contiguous()
        for li, layer in enumerate(self.model.layers):
            wqkv_f, wup_f = self._nf[li]
            qkv = ops.linear_rowscale(h, wqkv_f, ops.rms_rstd(h, eps))
            q, k, v = ops.rope_qkv_cache(qkv, self.rope[0], self.rope[1], layer.nq, layer.nkv, self.max_model_len,
                                         pos, kc[li], vc[li], slots)
            if fa:
                o = ops.flash_attention(q.view(1, T, layer.nq, layer.D), k.view(1, T, layer.nkv, layer.D),
                                        v.view(1, T, layer.nkv, layer.D), causal=True, doc_start=doc)
            else:
                o = ops.paged_prefill_attention(q.view(T, layer.nq, layer.D), kc[li], vc[li], bt, cu, ctx,
                                                work=work)
            h.addmm_(o.reshape(T, -1), layer.wo.t())
            act = ops.up_swiglu_rowscale(h, wup_f, ops.rms_rstd(h, eps))
            ops.linear_acc_(act, layer.w_down, h)
        return h

    # ------------------------------------------------------------------ TP hooks (identity at tp=1)
    def _load(self, model_path: str, dtype, seed: int):
        return load_model(model_path, device=self.device, dtype=dtype, seed=seed)

    def _agree_min(self, n: int) -> int:
        return n

    def _reduce(self, x: torch.Tensor) -> torch.Tensor:
        return x

    def _gather_vocab(self, logits: torch.Tensor) -> torch.Tensor:
        return logits

    def _fused_reduce_ok(self) -> bool:
        """TP > 1: can the row-parallel reductions fuse the bias / residual / RMSNorm (TP engine)."""
        return False

    def _reduce_add_rmsnorm(self, part, bias, res, norm_w, eps):
        """(rmsnorm(res + reduce(part) + bias) * norm_w, new residual) — TP=1: no reduction."""
        y = part if bias is None else part + bias
        return ops.add_rmsnorm(y, res, norm_w, eps)

    # ------------------------------------------------------------------ model pieces
    def _embed(self, ids: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        m = self.model
        if self.tp > 1:  # vocab-parallel table: local rows + all-reduce
            local = ids - m.vocab_start
            ok = (local >= 0) & (local < m.embed.shape[0])
            x = F.embedding(local.clamp(0, m.embed.shape[0] - 1), m.embed) * ok.unsqueeze(-1).to(m.embed.dtype)
            x = self._reduce(x)
        else:
            x = F.embedding(ids, m.embed)
        if m.pos_embed is not None:
            x = x + m.pos_embed[positions]
        return x

    def _norm(self, layer, x, res, which: str):
        w = layer.attn_norm_w if which == "attn" else layer.mlp_norm_w
        b = layer.attn_norm_b if which == "attn" else layer.mlp_norm_b
        eps = self.cfg.layer_norm_eps
        if res is None:
            return (ops.layernorm(x, w, b, eps) if b is not None else ops.rmsnorm(x, w, eps)), x
        return ops.add_layernorm(x, res, w, b, eps) if b is not None else ops.add_rmsnorm(x, res, w, eps)

    def _lin(self, x, w, b, li: int, name: str, sel):
        """``ops.decode_linear`` of projection ``name`` of layer ``li`` with the step's adapters.
        ``sel``: None (no adapter row in the step), an int32 device tensor (a slot or -1 per row:
        ``ops.lora_delta``, the decode form) or a host list of ``(row0, row1, slot)`` segments (the
        eager prefill / mixed step, whose chunks are contiguous row ranges: per segment
        ``y = x W^T + scale (x A^T) B^T`` with library GEMMs, in fp32 before the rounding)."""
        if sel is None:
            return ops.decode_linear(x, w, b)
        A, B, sc = self._lora[li][name]
        if isinstance(sel, torch.Tensor):
            return ops.decode_linear(x, w, b, lora=ops.LoRARows(sel, A, B, sc))
        # rows outside every segment keep the projection exactly as a step without adapters computes it
        covered = sum(r1 - r0 for r0, r1, _ in sel) == x.shape[0]
        y = (torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device) if covered and x.dtype != torch.float32
             else ops.decode_linear(x, w, b))
        for r0, r1, slot in sel:
            xs = x[r0:r1]
            d = self._lora_scale[slot] * ((xs.float() @ A[slot].float().t()) @ B[slot].float().t())
            if y.dtype == torch.float32:
                y[r0:r1] += d
                continue
            # the segment's product again with an fp32 result: sum + delta rounded once, like the
            # fused decode projections (a resumed sequence's prefill continues its decode steps)
            base = torch.mm(xs, w.t(), out_dtype=torch.float32)
            if b is not None:
                base = base + b.float()
            y[r0:r1] = (base + d).to(y.dtype)
        return y

    def _qkv(self, layer, xn, positions, seq_len, kc, vc, slots, li: int = 0, sel=None):
        """QKV projection, RoPE and the paged-cache write of this step's K/V rows (one fused
        pass with RoPE)."""
        qkv = self._lin(xn, layer.wqkv, layer.bqkv, li, "wqkv", sel)
        if self.rope is not None:
            return ops.rope_qkv_cache(qkv, self.rope[0], self.rope[1], layer.nq, layer.nkv, seq_len, positions,
                                      kc, vc, slots)
        T = qkv.shape[0]
        x = qkv.view(T, layer.nq + 2 * layer.nkv, layer.D)
        q, k, v = (x[:, :layer.nq].contiguous(), x[:, layer.nq:layer.nq + layer.nkv].contiguous(),
                   x[:, layer.nq + layer.nkv:].contiguous())
        ops.kv_cache_write(k, v, kc, vc, slots)
        return q, k, v

    def _mlp(self, layer, xn, li: int = 0, sel=None):
        if layer.moe is not None:  # routed experts (host-side split sizes: eager, no graphs)
            return layer.moe(xn)
        if self.cfg.gated_mlp:
            # prefill-sized (T % 256 == 0): the SwiGLU rides on the gate/up GEMM's epilogue
            act = (ops.up_swiglu(xn, layer.w_up, layer.b_up)
                   if sel is None and xn.shape[0] >= 256 and xn.shape[0] % 256 == 0
                   else ops.swiglu(self._lin(xn, layer.w_up, layer.b_up, li, "w_up", sel)))
            out = self._lin(act, layer.w_down, None, li, "w_down", sel)
        else:
            out = self._lin(ops.gelu(self._lin(xn, layer.w_up, layer.b_up, li, "w_up", sel)), layer.w_down, None, li,
                            "w_down", sel)
        out = self._reduce(out)  # row-parallel down projection
        if layer.b_down is not None:
            out = out + layer.b_down
        return out

    def _final(self, x, res):
        m = self.model
        eps = self.cfg.layer_norm_eps
        if m.final_norm_b is not None:
            xn, _ = ops.add_layernorm(x, res, m.final_norm_w, m.final_norm_b, eps)
        else:
            xn, _ = ops.add_rmsnorm(x, res, m.final_norm_w, eps)
        return self._gather_vocab(ops.decode_linear(xn, m.head_weight()))

    # ------------------------------------------------------------------ prefill
    def prefill_plan(self, chunks: List[PrefillChunk]) -> Dict:
        """Host-side description of a (chunked, packed) prefill step — what TP ranks receive."""
        ids, pos, slots, cu, ctx, last = [], [], [], [0], [], []
        score = None
        for i, c in enumerate(chunks):
            toks = c.seq.all_ids
            ids.extend(toks[c.start:c.start + c.count])
            pos.extend(range(c.start, c.start + c.count))
            slots.append(np.asarray(self.kv.slots(c.seq.seq_id, c.start, c.count), dtype=np.int64))
            if c.seq.score_pending:
                # rows still to score: prompt positions from the first unscored one, short of the
                # prompt's last (it has no target); the target of position p is prompt_ids[p + 1],
                # at a chunk's last row the next chunk's first token.  Rows of generated tokens (a
                # sequence resumed after preemption) lie past the prompt and are never scored.
                s = c.seq
                p0, p1 = max(c.start, len(s.prompt_logprobs) - 1), min(c.start + c.count, len(s.prompt_ids) - 1)
                if p0 < p1:
                    score = score or {"rows": [], "targets": [], "nlp": [], "segs": []}
                    score["rows"].extend(range(cu[-1] + p0 - c.start, cu[-1] + p1 - c.start))
                    score["targets"].extend(s.prompt_ids[p0 + 1:p1 + 1])
                    score["nlp"].extend([int(s.params.prompt_logprobs)] * (p1 - p0))
                    score["segs"].append((i, p1 - p0))
            cu.append(cu[-1] + c.count)
            ctx.append(c.start + c.count)
            if c.samples:
                last.append(cu[-1] - 1)
        bt = np.asarray(self.kv.block_tables([c.seq.seq_id for c in chunks], self.max_blocks_per_seq))
        # every chunk is a whole fresh prompt (no cached prefix): its keys are exactly the chunk's
        # own rows, so attention can run as packed-document flash attention (doc_start per token)
        fresh = bool(chunks) and all(c.start == 0 for c in chunks)
        doc = np.repeat(np.asarray(cu[:-1], dtype=np.int32), np.diff(cu)) if fresh else None
        lora = [c.seq.lora_slot for c in chunks]
        extra = {"lora": lora} if any(s >= 0 for s in lora) else {}  # adapter slot per chunk
        if score is not None:  # only a step with rows to score carries the key
            extra["score"] = score
        return {**extra, "op": "prefill", "ids": np.asarray(ids, dtype=np.int64), "pos": np.asarray(pos, dtype=np.int32),
                "slots": np.concatenate(slots) if slots else np.zeros(0, dtype=np.int64), "cu": cu, "ctx": ctx,
                "bt": bt, "last": last, "work": ops.prefill_work_list(cu), "doc": doc}

    @torch.inference_mode()
    def prefill(self, chunks) -> torch.Tensor:
        """Run prefill chunks (``PrefillChunk`` list, or sequences: whole prompts); returns the
        logits [n_final, V] of the chunks that complete their sequence, in chunk order."""
        if chunks and isinstance(chunks[0], Sequence):
            chunks = [PrefillChunk(s, 0, s.num_tokens) for s in chunks]
        return self.prefill_exec(self.prefill_plan(chunks))

    @torch.inference_mode()
    def prefill_exec(self, plan: Dict) -> torch.Tensor:
        use_knobs(self.knobs)
        d = self.device
        T = len(plan["ids"])
        ids = torch.from_numpy(plan["ids"]).to(d, non_blocking=True)
        pos = torch.from_numpy(plan["pos"]).to(d, non_blocking=True)
        slots = torch.from_numpy(plan["slots"]).to(d, non_blocking=True)
        bt = torch.from_numpy(plan["bt"]).to(d, non_blocking=True)
        cu = torch.tensor(plan["cu"], dtype=torch.int32).to(d, non_blocking=True)
        ctx = torch.tensor(plan["ctx"], dtype=torch.int32).to(d, non_blocking=True)
        work = torch.tensor(plan["work"], dtype=torch.int32).to(d, non_blocking=True)
        # fresh prompts: the training flash-attention kernel over packed documents, K/V straight
        # from the RoPE pass (16 x 2k burst TTFT p50 224.6 -> 218.6 ms, single 2k prompt 27.5 ->
        # 26.2 ms, profiles/serve_r2_session6.txt); knob prefill_fa off keeps the paged kernel
        doc = None
        fa = plan.get("doc") is not None and d.type == "cuda" and self.knobs.prefill_fa
        if fa and len(plan["cu"]) > 2:  # several prompts packed: document boundaries
            doc = torch.from_numpy(plan["doc"]).to(d, non_blocking=True).view(1, T)
        # (one prompt: plain causal attention, which also lets the kernel split the K/V range of
        # its few q-blocks over two workgroups — the split is off for packed documents)
        x = self._embed(ids, pos.long())
        # chunks of adapter sequences: contiguous row ranges, their deltas added per segment
        sel = None
        if plan.get("lora") is not None:
            sel = [(plan["cu"][i], plan["cu"][i + 1], s) for i, s in enumerate(plan["lora"]) if s >= 0]
        if self._norm_fold_ok(T, sel):
            h = self._prefill_layers_folded(x, pos, slots, fa, doc, bt, cu, ctx, work)
            self.stats["prefill_tokens"] += T
            if plan.get("score") is not None:
                self._score_rows(plan["score"], h, None)
            if not plan["last"]:
                return torch.empty(0, self.cfg.vocab_size, device=d, dtype=h.dtype)
            hl = h.index_select(0, torch.tensor(plan["last"], device=d))
            xn = ops.rmsnorm(hl, self.model.final_norm_w, self.cfg.layer_norm_eps)
            return self._gather_vocab(ops.decode_linear(xn, self.model.head_weight()))
        res = None
        kc, vc = self.kv_cache.k, self.kv_cache.v
        for li, layer in enumerate(self.model.layers):
            xn, res = self._norm(layer, x, res, "attn")
            q, k, v = self._qkv(layer, xn, pos, self.max_model_len, kc[li], vc[li], slots, li, sel)
            if fa:
                o = ops.flash_attention(q.view(1, T, layer.nq, layer.D), k.view(1, T, layer.nkv, layer.D),
                                        v.view(1, T, layer.nkv, layer.D), causal=True, doc_start=doc)
            else:
                o = ops.paged_prefill_attention(q.view(T, layer.nq, layer.D), kc[li], vc[li], bt, cu, ctx,
                                                work=work)
            a = self._reduce(self._lin(o.view(T, -1), layer.wo, None, li, "wo", sel))
            if layer.bo is not None:
                a = a + layer.bo
            xn, res = self._norm(layer, a, res, "mlp")
            x = self._mlp(layer, xn, li, sel)
        self.stats["prefill_tokens"] += T
        if plan.get("score") is not None:
            self._score_rows(plan["score"], x, res)
        if not plan["last"]:
            return torch.empty(0, self.cfg.vocab_size, device=d, dtype=x.dtype)
        last = torch.tensor(plan["last"], device=d)
        return self._final(x.index_select(0, last), res.index_select(0, last))

    # ------------------------------------------------------------------ mixed prefill + decode
    def mixed_plan(self, chunks: List[PrefillChunk], seqs: List[Sequence]) -> Dict:
        """One step's prefill chunks AND decode tokens as one token batch (decode rows last)."""
        p, d = self.prefill_plan(chunks), self.decode_plan(seqs)
        return {"op": "mixed", "prefill": p, "decode": d}

    @torch.inference_mode()
    def mixed(self, chunks: List[PrefillChunk], seqs: List[Sequence]) -> torch.Tensor:
        return self.mixed_exec(self.mixed_plan(chunks, seqs))

    @torch.inference_mode()
    def mixed_exec(self, plan: Dict) -> torch.Tensor:
        """Mixed step (continuous batching's fused step): the decode tokens of the running batch
        ride in the prefill chunks' forward — every projection / MLP GEMM streams its weights
        once for both kinds of rows — and only attention splits by row kind: prefill rows through
        the (paged or fresh-prompt flash) prefill attention, decode rows through the paged decode
        kernel.  Returns logits [n_final_chunks + n_decode, V]: the final chunks' rows first, in
        chunk order, then the decode rows (eager: the graph-captured decode step is for
        decode-only steps).  Reference batching: ``llmctl/serve/server.py:89-125, 372-386``."""
        use_knobs(self.knobs)
        d = self.device
        pp, dp = plan["prefill"], plan["decode"]
        Tp, Td = len(pp["ids"]), len(dp["ids"])
        ids = torch.cat([torch.from_numpy(pp["ids"]), torch.tensor(dp["ids"], dtype=torch.long)]).to(d, non_blocking=True)
        pos = torch.cat([torch.from_numpy(pp["pos"]), torch.tensor(dp["positions"], dtype=torch.int32)]).to(d, non_blocking=True)
        slots = torch.cat([torch.from_numpy(pp["slots"]), torch.tensor(dp["slots"], dtype=torch.long)]).to(d, non_blocking=True)
        bt = torch.from_numpy(pp["bt"]).to(d, non_blocking=True)
        cu = torch.tensor(pp["cu"], dtype=torch.int32).to(d, non_blocking=True)
        ctx = torch.tensor(pp["ctx"], dtype=torch.int32).to(d, non_blocking=True)
        work = torch.tensor(pp["work"], dtype=torch.int32).to(d, non_blocking=True)
        bt_d = torch.from_numpy(dp["bt"]).to(d, non_blocking=True)
        ctx_d = torch.tensor(dp["ctx"], dtype=torch.int32).to(d, non_blocking=True)
        fa = pp.get("doc") is not None and d.type == "cuda" and self.knobs.prefill_fa
        doc = torch.from_numpy(pp["doc"]).to(d, non_blocking=True).view(1, Tp) if fa and len(pp["cu"]) > 2 else None
        x = self._embed(ids, pos.long())
        res = None
        kc, vc = self.kv_cache.k, self.kv_cache.v
        sel = None  # adapter segments: the chunks' row ranges, then one row per decode sequence
        if pp.get("lora") is not None or dp.get("lora") is not None:
            sel = [(pp["cu"][i], pp["cu"][i + 1], s) for i, s in enumerate(pp.get("lora") or []) if s >= 0]
            sel += [(Tp + i, Tp + i + 1, s) for i, s in enumerate(dp.get("lora") or []) if s >= 0]
        for li, layer in enumerate(self.model.layers):
            xn, res = self._norm(layer, x, res, "attn")
            q, k, v = self._qkv(layer, xn, pos, self.max_model_len, kc[li], vc[li], slots, li, sel)
            if fa:
                op = ops.flash_attention(q[:Tp].reshape(1, Tp, layer.nq, layer.D),
                                         k[:Tp].reshape(1, Tp, layer.nkv, layer.D),
                                         v[:Tp].reshape(1, Tp, layer.nkv, layer.D), causal=True, doc_start=doc)
            else:
                op = ops.paged_prefill_attention(q[:Tp].reshape(Tp, layer.nq, layer.D), kc[li], vc[li], bt, cu, ctx,
                                                 work=work)
            od = ops.paged_attention_decode(q[Tp:].reshape(Td, layer.nq, layer.D).contiguous(), kc[li], vc[li], bt_d,
                                            ctx_d)
            o = torch.cat([op.reshape(Tp, -1), od.reshape(Td, -1)])
            a = self._reduce(self._lin(o, layer.wo, None, li, "wo", sel))
            if layer.bo is not None:
                a = a + layer.bo
            xn, res = self._norm(layer, a, res, "mlp")
            x = self._mlp(layer, xn, li, sel)
        self.stats["prefill_tokens"] += Tp
        self.stats["decode_tokens"] += Td
        self.stats["mixed_steps"] = self.stats.get("mixed_steps", 0) + 1
        if pp.get("score") is not None:  # the chunks' rows come first: the plan's row numbers hold
            self._score_rows(pp["score"], x, res)
        rows = torch.tensor(list(pp["last"]) + list(range(Tp, Tp + Td)), device=d)
        return self._final(x.index_select(0, rows), res.index_select(0, rows))

    def _mixed_ok(self) -> bool:
        """Knob ``mixed_steps`` off runs a step's decode and prefill as two forwards (A/B)."""
        return self.knobs.mixed_steps

    # ------------------------------------------------------------------ prompt scoring
    SCORE_TILE = 1024  # prompt rows whose logits exist at a time: the scratch is SCORE_TILE x V

    def _score_rows(self, sc: Dict, x: torch.Tensor, res: Optional[torch.Tensor]) -> None:
        """Score a prefill (or mixed) step's rows ``sc["rows"]`` against ``sc["targets"]``: final norm
        -> vocabulary projection as a many-row library GEMM into the logits scratch ->
        ``ops.prompt_logprobs``, in tiles of ``SCORE_TILE`` rows.  ``x`` / ``res``: the last layer's
        output and the residual stream; ``res`` None: ``x`` is the folded prefill's residual stream,
        with only the final RMSNorm left.  The raw logits are scored: no temperature, penalty or
        guide.  The results leave in one D2H copy (pinned on the GPU) and are read by
        :meth:`_finish_scores`, where the step's tokens are read."""
        d, m, eps = self.device, self.model, self.cfg.layer_norm_eps
        n, W = len(sc["rows"]), ops.ref.TOP_LOGPROBS
        rows = torch.tensor(sc["rows"], dtype=torch.long).to(d, non_blocking=True)
        target = torch.tensor(sc["targets"], dtype=torch.long).to(d, non_blocking=True)
        nlp = torch.tensor(sc["nlp"], dtype=torch.int32).to(d, non_blocking=True)
        w = m.head_weight()
        if self._score_scratch is None:  # on first need, as the sampler state is
            self._score_scratch = torch.empty(self.SCORE_TILE, w.shape[0], dtype=x.dtype, device=d)
            log.info("engine: prompt-logprob logits scratch: %d rows x %d tokens, %.2f MB", self.SCORE_TILE, w.shape[0],
                     self._score_scratch.numel() * self._score_scratch.element_size() / 1e6)
        out = torch.empty(n, 2 + 2 * W, dtype=torch.int32, device=d)  # logprob | rank | top ids | top logprobs
        for r0 in range(0, n, self.SCORE_TILE):
            r = rows[r0:r0 + self.SCORE_TILE]
            if res is None:
                xn = ops.rmsnorm(x.index_select(0, r), m.final_norm_w, eps)
            elif m.final_norm_b is not None:
                xn, _ = ops.add_layernorm(x.index_select(0, r), res.index_select(0, r), m.final_norm_w, m.final_norm_b, eps)
            else:
                xn, _ = ops.add_rmsnorm(x.index_select(0, r), res.index_select(0, r), m.final_norm_w, eps)
            logits = torch.mm(xn, w.t(), out=self._score_scratch[:r.shape[0]])
            lp, rank, top_ids, top_lp = ops.prompt_logprobs(logits, target[r0:r0 + self.SCORE_TILE],
                                                            nlp[r0:r0 + self.SCORE_TILE])
            o = out[r0:r0 + r.shape[0]]
            o[:, 0] = lp.view(torch.int32)
            o[:, 1] = rank
            o[:, 2:2 + W] = top_ids
            o[:, 2 + W:] = top_lp.view(torch.int32)
        ev = None
        if d.type == "cuda":
            host = torch.empty(n, 2 + 2 * W, dtype=torch.int32).pin_memory()
            host.copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        else:
            host = out
        self._score_out = (sc["segs"], host, ev)

    def _finish_scores(self, chunks: List[PrefillChunk]) -> None:
        """Append the scores of the step just run to their sequences (before any token of the step
        is appended: ``on_token`` may read them)."""
        so, self._score_out = self._score_out, None
        if so is None:
            return
        segs, host, ev = so
        if ev is not None:
            ev.synchronize()
        W = ops.ref.TOP_LOGPROBS
        a = host.numpy()
        f = a.view(np.float32)
        lp, rank, ids, tlp = f[:, 0].tolist(), a[:, 1].tolist(), a[:, 2:2 + W].tolist(), f[:, 2 + W:].tolist()
        r = 0
        for ci, cnt in segs:
            seq = chunks[ci].seq
            for j in range(r, r + cnt):
                seq.prompt_logprobs.append(lp[j])
                seq.prompt_ranks.append(rank[j])
                seq.prompt_top_logprobs.append([(t, v) for t, v in zip(ids[j], tlp[j]) if t >= 0])
            r += cnt

    def _finish_score_only(self, chunks: List[PrefillChunk]) -> None:
        """Requests that only score their prompt (``max_tokens = 0``) end with their last chunk."""
        for c in chunks:
            if c.final and c.seq.score_only and c.seq.status == "running":
                self.scheduler.finish(c.seq, "length")

    def score(self, prompts: List[List[int]], top: int = 0, lora: Optional[str] = None) -> List[Sequence]:
        """Score ``prompts`` and generate nothing: the finished sequences carry ``prompt_logprobs``,
        ``prompt_ranks`` and ``prompt_top_logprobs`` (``top`` alternatives per position)."""
        return self.generate(prompts, SamplingParams(max_tokens=0, prompt_logprobs=top, lora=lora))

    # ------------------------------------------------------------------ decode
    def _fused_decode(self, n: int = 1) -> bool:
        """Decode layers on the fused-epilogue projections (``ops.decode_qkv_rope_cache`` /
        ``decode_up_swiglu`` / ``decode_linear_add_rmsnorm``): 10 kernels per layer instead of 13
        (the RoPE/cache-write, SwiGLU and add+RMSNorm passes ride on the projections' finalize).  Needs the GPU path,
        RMSNorm, RoPE and a gated MLP; at TP > 1 the row-parallel projections' all-reduce, bias,
        residual add and next RMSNorm are one custom-all-reduce kernel
        (``_reduce_add_rmsnorm``); knob ``decode_fused`` off keeps the unfused layer (A/B).
        MoE models: the MLP half is route -> routed gate/up + SwiGLU -> routed down + combine +
        residual + RMSNorm (``_moe_fused``), for steps of at most ``MOE_MAX_ROWS`` rows."""
        cfg, m = self.cfg, self.model
        return (self.device.type == "cuda" and (self.tp == 1 or self._fused_reduce_ok()) and self.rope is not None
                and cfg.gated_mlp
                and (not cfg.is_moe or self._moe_fused(n)) and m.final_norm_b is None
                and all(l.attn_norm_b is None and l.mlp_norm_b is None for l in m.layers)
                and self.knobs.decode_fused)

    def _decode_body(self, ids, positions, slots, block_tables, ctx_lens, lora_idx=None) -> torch.Tensor:
        """``lora_idx``: int32 [rows], the adapter slot of every row (-1 = none), or None."""
        if self._fused_decode(ids.shape[0]):
            return self._decode_body_fused(ids, positions, slots, block_tables, ctx_lens, lora_idx)
        x = self._embed(ids, positions)
        res = None
        kc, vc = self.kv_cache.k, self.kv_cache.v
        for li, layer in enumerate(self.model.layers):
            xn, res = self._norm(layer, x, res, "attn")
            q, k, v = self._qkv(layer, xn, positions, self.max_model_len, kc[li], vc[li], slots, li, lora_idx)
            o = ops.paged_attention_decode(q, kc[li], vc[li], block_tables, ctx_lens)
            a = self._reduce(self._lin(o.view(o.shape[0], -1), layer.wo, None, li, "wo", lora_idx))
            if layer.bo is not None:
                a = a + layer.bo
            xn, res = self._norm(layer, a, res, "mlp")
            x = self._mlp(layer, xn, li, lora_idx)
        return self._final(x, res)

    _W8_NAMES = ("wqkv", "wo", "w_up", "w_down")

    @property
    def _w8(self):
        """The per-layer fp8 copies (``weight_dtype="fp8"``), else None."""
        return self._wq if self._wq_kind == "fp8" else None

    @property
    def _w4(self):
        """The per-layer int4 copies (``weight_dtype="int4"``), else None."""
        return self._wq if self._wq_kind == "int4" else None

    @torch.no_grad()
    def _quantize_decode_weights(self, kind: str) -> List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]]:
        """Per layer: quantised copies of the decode projection weights + their fp32 scales.  ``fp8``:
        e4m3fn + row scales (``quantizers.quantize_fp8``: absmax / 448 per output row); ``int4``:
        packed uint8 [N, K/2] + group scales [N, K/128] (``quantizers.quantize_int4_g128``).  A TP
        rank quantises its own shard; int4 groups run along K and the row-parallel shards cut K at
        multiples of 128, so the int4 values are the TP=1 engine's."""
        from llmctl.plugins.quantizers import quantize_fp8, quantize_int4_g128

        quant = quantize_fp8 if kind == "fp8" else quantize_int4_g128

        def copy(w):
            qd = quant(w.detach())
            return qd["qweight"].contiguous(), qd["scale"].float().contiguous()

        out = []
        for layer in self.model.layers:
            d = {}
            for name in self._W8_NAMES:
                w = getattr(layer, name, None)
                # only weights the fused kernels take (ops.decode_fused_ok: out % 64, in % 128)
                if w is None or w.dim() != 2 or w.shape[0] % 64 or w.shape[1] % 128:
                    continue
                d[name] = copy(w)
            out.append(d)
        hw = self.model.head_weight()
        if hw.dim() == 2 and hw.shape[0] % 64 == 0 and hw.shape[1] % 128 == 0:  # the (local shard of the) LM head
            self._wq_head = copy(hw)
        pairs = [p for d in out for p in d.values()] + ([self._wq_head] if self._wq_head is not None else [])
        nbytes = sum(t.numel() * t.element_size() for p in pairs for t in p)
        log.info("engine: %s decode weight copies of %d projections: %.3f GB (out of the KV cache budget)", kind,
                 len(pairs), nbytes / 1e9)
        return out

    W8_MAX_ROWS = 16  # the fused fp8 / int4 decode kernels take at most 16 token rows (ops.decode_fused_ok)

    def _dw(self, li: int, layer, name: str, n: int):
        """(weight, scales or None) the fused decode path streams for ``layer.name`` at ``n`` token
        rows: the fp8 / int4 copy only where the fused kernel takes it, else the bf16 weight (which
        is kept) -- never a per-step dequantised fp32 image of the copy."""
        if self._wq is not None and 1 <= n <= self.W8_MAX_ROWS and name in self._wq[li]:
            q = self._wq[li][name]
            if name not in ("wo", "w_down") or q[0].shape[0] <= 16384:  # add+RMSNorm finalize limit
                return q
        return getattr(layer, name), None

    def _decode_body_fused(self, ids, positions, slots, block_tables, ctx_lens, lora_idx=None) -> torch.Tensor:
        m = self.model
        eps = self.cfg.layer_norm_eps
        layers = m.layers
        kc, vc = self.kv_cache.k, self.kv_cache.v
        x = self._embed(ids, positions)
        xn, res = ops.rmsnorm(x, layers[0].attn_norm_w, eps), x
        tp = self.tp > 1
        def lin(x, w, s):  # a plain decode projection (TP row-parallel partial): bf16, fp8 or int4 weights
            if s is None:
                return ops.decode_linear(x, w)
            return ops.decode_linear_int4(x, w, s) if w.dtype == torch.uint8 else ops.decode_linear_fp8(x, w, s)

        def rows(li, name):  # the projection's adapters under this step's row selection
            return None if lora_idx is None else ops.LoRARows(lora_idx, *self._lora[li][name])

        n = ids.shape[0]
        for li, layer in enumerate(layers):
            (wqkv, sqkv), (wo, so) = self._dw(li, layer, "wqkv", n), self._dw(li, layer, "wo", n)
            (wu, su), (wd, sd) = self._dw(li, layer, "w_up", n), self._dw(li, layer, "w_down", n)
            o = ops.decode_attention_qkv(xn, wqkv, layer.bqkv, self.rope[0], self.rope[1], layer.nq,
                                         layer.nkv, positions, kc[li], vc[li], slots, block_tables, ctx_lens,
                                         w_scale=sqkv, lora=rows(li, "wqkv"))
            if tp:  # row-parallel o-proj partial -> one kernel: all-reduce + bias + residual + RMSNorm
                xn, res = self._reduce_add_rmsnorm(lin(o.view(o.shape[0], -1), wo, so), layer.bo,
                                                   res, layer.mlp_norm_w, eps)
            else:
                xn, res = ops.decode_linear_add_rmsnorm(o.view(o.shape[0], -1), wo, layer.bo, res,
                                                        layer.mlp_norm_w, eps, w_scale=so, lora=rows(li, "wo"))
            nw = layers[li + 1].attn_norm_w if li + 1 < len(layers) else m.final_norm_w
            if layer.moe is not None:  # routed experts: all routing stays on the device
                up_t, down_t = self._moe[li]
                topi, topw = ops.moe_route(xn, layer.moe.w_router, layer.moe.k)
                act = ops.moe_decode_up_swiglu(xn, up_t, topi)
                xn, res = ops.moe_decode_down_add_rmsnorm(act, down_t, topi, topw, res, nw, eps)
                continue
            act = ops.decode_up_swiglu(xn, wu, layer.b_up, w_scale=su, lora=rows(li, "w_up"))  # the local F shard
            if tp:
                xn, res = self._reduce_add_rmsnorm(lin(act, wd, sd), layer.b_down, res, nw, eps)
            else:
                xn, res = ops.decode_linear_add_rmsnorm(act, wd, layer.b_down, res, nw, eps, w_scale=sd,
                                                        lora=rows(li, "w_down"))
        if self._wq_head is not None and n <= self.W8_MAX_ROWS:
            return self._gather_vocab(lin(xn, *self._wq_head))
        return self._gather_vocab(ops.decode_linear(xn, m.head_weight()))

    def _bucket(self, n: int) -> int:
        b = 1
        while b < n:
            b *= 2
        return min(b, max(self.max_batch_size, n))

    _STAGED = ("ids", "positions", "slots", "block_tables", "ctx_lens", "u")

    _EXT = ("slot", "rep", "freq", "pres", "nlp")  # per-row inputs of ops.sample_ext, in argument order
    _EXT_OUT = ("lp", "top_ids", "top_lp")  # its logprob outputs

    _GUIDED = ("guide", "gslot")  # the further per-row inputs of ops.sample_guided

    def _static_ext(self, nb: int, bufs: Dict, guided: bool = False) -> None:
        """The extended graph's additional static buffers: the per-row ``sample_ext`` parameters
        (neutral defaults: no state, no penalties, no top list) and two pinned host sets for the
        logprob outputs, flipped with ``host_toks``."""
        d = self.device
        bufs["slot"] = torch.full((nb,), -1, dtype=torch.int32, device=d)
        bufs["rep"] = torch.ones(nb, dtype=torch.float32, device=d)
        bufs["freq"] = torch.zeros(nb, dtype=torch.float32, device=d)
        bufs["pres"] = torch.zeros(nb, dtype=torch.float32, device=d)
        bufs["nlp"] = torch.zeros(nb, dtype=torch.int32, device=d)
        if guided:  # the guided graph: table slot and state word of every row (-1: unguided)
            bufs["guide"] = torch.full((nb,), -1, dtype=torch.int32, device=d)
            bufs["gslot"] = torch.full((nb,), -1, dtype=torch.int32, device=d)
        W = ops.ref.TOP_LOGPROBS
        host = lambda: {"lp": torch.zeros(nb, dtype=torch.float32).pin_memory(),
                        "top_ids": torch.zeros(nb, W, dtype=torch.int32).pin_memory(),
                        "top_lp": torch.zeros(nb, W, dtype=torch.float32).pin_memory()}
        bufs["host_lp"] = [host(), host()]

    def _static(self, nb: int, lora: bool = False) -> Dict:
        d = self.device
        bufs = {"ids": torch.zeros(nb, dtype=torch.long, device=d),
                "positions": torch.zeros(nb, dtype=torch.int32, device=d),
                "slots": torch.full((nb,), -1, dtype=torch.long, device=d),
                "block_tables": torch.zeros(nb, self.max_blocks_per_seq, dtype=torch.int32, device=d),
                "ctx_lens": torch.ones(nb, dtype=torch.int32, device=d),
                # in-graph sampling: per-row parameters (rewritten when the batch's change) and uniforms
                "u": torch.zeros(nb, dtype=torch.float32, device=d),
                "temp": torch.zeros(nb, dtype=torch.float32, device=d),
                "topk": torch.zeros(nb, dtype=torch.int32, device=d),
                "topp": torch.ones(nb, dtype=torch.float32, device=d)}
        bufs["staged"] = self._STAGED
        if lora:  # the adapter slot of every row, staged with the step's other inputs
            bufs["lora_idx"] = torch.full((nb,), -1, dtype=torch.int32, device=d)
            bufs["staged"] = self._STAGED + ("lora_idx",)
        # pinned host staging of the step inputs, two sets: an asynchronous step refills one while
        # the other's H2D copies may still be queued behind the step in flight (a non_blocking
        # copy from pageable memory would be synchronous)
        pin = self.device.type == "cuda"
        stage = []
        for _ in range(2):
            # initialised from the device defaults: rows past the live batch are copied too and
            # must stay valid (block id 0, context 1) for the padded graph rows
            h = {k: bufs[k].to("cpu") for k in bufs["staged"]}
            stage.append({k: (v.pin_memory() if pin else v) for k, v in h.items()})
        bufs["stage"] = stage
        bufs["flip"] = 0
        toks = torch.zeros(nb, dtype=torch.long)
        bufs["host_toks"] = [toks.pin_memory() if pin else toks, toks.clone().pin_memory() if pin else toks.clone()]
        bufs["tflip"] = 0
        bufs["params_key"] = None
        return bufs

    def _graph_body(self, bufs: Dict) -> None:
        """Decode step + sampling; the sampled ids also become the next step's input ids (the
        asynchronous path launches step N + 1 without reading step N's tokens first)."""
        bufs["logits"] = self._decode_body(bufs["ids"], bufs["positions"], bufs["slots"], bufs["block_tables"],
                                           bufs["ctx_lens"], bufs.get("lora_idx"))
        if "guide" in bufs:  # the guided graph: also the guide's mask and the automaton step
            counts, mask = self._sampler_tensors()
            a = self._guide_arena
            bufs["toks"], bufs["lp"], bufs["top_ids"], bufs["top_lp"] = ops.sample_guided(
                bufs["logits"].contiguous(), bufs["temp"], bufs["topk"], bufs["topp"], bufs["u"],
                *(bufs[k] for k in self._EXT), counts, mask, bufs["guide"], bufs["gslot"], a["cls"], a["next"],
                a["meta"], a["state"], check_slots=False)
        elif "slot" in bufs:  # the extended graph: penalties, logprobs and the state update ride in the sampler
            counts, mask = self._sampler_state
            bufs["toks"], bufs["lp"], bufs["top_ids"], bufs["top_lp"] = ops.sample_ext(
                bufs["logits"].contiguous(), bufs["temp"], bufs["topk"], bufs["topp"], bufs["u"],
                *(bufs[k] for k in self._EXT), counts, mask, check_slots=False)
        else:
            bufs["toks"] = ops.sample(bufs["logits"].contiguous(), bufs["temp"], bufs["topk"], bufs["topp"], bufs["u"])
        bufs["ids"].copy_(bufs["toks"])

    @staticmethod
    def _sampler_kind(ext: Optional[Dict]) -> int:
        """The sampler of a step from its extended fields: 0 plain (``ops.sample``), 1 extended
        (``ops.sample_ext``), 2 guided (``ops.sample_guided``)."""
        return 0 if ext is None else 2 if "guide" in ext else 1

    def _graph_family(self, nb: int, kind: int, lora: bool):
        """(dict, key) of the graph an ``nb``-row step replays: plain, extended sampler, guided
        sampler, or -- a step with an adapter row -- the LoRA family, keyed (bucket, sampler kind)."""
        kind = int(kind)
        if lora:
            return self._graphs_lora, (nb, kind)
        return (self._graphs, self._graphs_ext, self._graphs_guided)[kind], nb

    def _capture(self, nb: int, ext: int = 0, lora: bool = False):
        """``ext``: the sampler kind (0 / False plain, 1 / True extended, 2 guided)."""
        bufs = self._static(nb, lora)
        if ext:
            self._static_ext(nb, bufs, guided=int(ext) == 2)
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(2):  # warm-up (allocator / lazy init) outside the graph
                self._graph_body(bufs)
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with graph_capture_gc_guard(), torch.cuda.graph(g):
            self._graph_body(bufs)
        graphs, key = self._graph_family(nb, ext, lora)
        graphs[key] = (g, bufs)

    def release_graphs(self) -> None:
        """Drop the captured decode graphs (they hold the RCCL communicator's captured
        collectives: release them before ``destroy_process_group``)."""
        families = (self._graphs, self._graphs_ext, self._graphs_guided, self._graphs_lora)
        if any(families) and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for graphs in families:
            for g, _ in graphs.values():
                g.reset()
            graphs.clear()

    def close(self) -> None:
        """Deterministic teardown, never left to garbage collection: drop an in-flight pipelined
        step, release the captured decode graphs (their memory pool and any captured collectives),
        drain the device and drop the KV cache / weights this engine holds.  Idempotent; the engine
        is unusable afterwards.  Also the ``with InferenceEngine(...) as e:`` exit."""
        if getattr(self, "_closed", False):
            return
        self._closed = True
        self._release_resources()

    def _release_resources(self) -> None:
        self._pending = None
        self._last_toks = None
        self._ext_out = None
        self.release_graphs()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self._sampler_state = None
        self._score_scratch = self._score_out = None
        self._sampler_free = []
        self._guide_arena = None
        self._guide_tables, self._guide_table_free = {}, []
        self.kv_cache = None
        self._wq = self._wq_head = None
        self._lora = None
        self._lora_slots, self._lora_salt, self._lora_scale = {}, {}, {}
        self._nf = None
        self._moe = None
        self.rope = None
        if self.device.type == "cuda":
            torch.cuda.empty_cache()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    @staticmethod
    def _lora_rows(seqs: List[Sequence]) -> Dict:
        """``{"lora": [slot per row]}`` for a decode plan when a row has an adapter, else nothing."""
        rows = [s.lora_slot for s in seqs]
        return {"lora": rows} if any(r >= 0 for r in rows) else {}

    def decode_plan(self, seqs: List[Sequence]) -> Dict:
        return {**self._lora_rows(seqs), "op": "decode", "ids": [s.last_id for s in seqs], "positions": [s.num_tokens - 1 for s in seqs],
                "slots": [s._decode_slot for s in seqs], "ctx": [self.kv.num_tokens(s.seq_id) for s in seqs],
                "bt": np.asarray(self.kv.block_tables([s.seq_id for s in seqs], self.max_blocks_per_seq))}

    @torch.inference_mode()
    def decode(self, seqs: List[Sequence]) -> torch.Tensor:
        return self.decode_exec(self.decode_plan(seqs))

    @torch.inference_mode()
    def decode_exec(self, plan: Dict) -> torch.Tensor:
        use_knobs(self.knobs)
        ids, positions, slots, ctx, bt = plan["ids"], plan["positions"], plan["slots"], plan["ctx"], plan["bt"]
        n = len(ids)
        self.stats["decode_tokens"] += n
        if self._graph_ok(n):
            g, b = self._stage_and_replay(plan, cont=False)
            return b["logits"][:n]
        d = self.device
        lora = torch.tensor(plan["lora"], dtype=torch.int32, device=d) if plan.get("lora") is not None else None
        return self._decode_body(torch.tensor(ids, device=d), torch.tensor(positions, dtype=torch.int32, device=d),
                                 torch.tensor(slots, device=d), torch.from_numpy(bt).to(d),
                                 torch.tensor(ctx, dtype=torch.int32, device=d), lora)

    def _stage_and_replay(self, plan: Dict, cont: bool):
        """Fill one host staging set with the step's inputs, copy them (asynchronously) into the
        graph's static buffers and replay it.  ``cont``: the input ids are already on the device
        (the previous replay of this graph sampled them), only positions / slots / block tables /
        context lengths / uniforms are copied.  A sampling plan (``decode_s``) carries its uniforms
        ``u`` and per-row ``temp`` / ``topk`` / ``topp``; a logits-only plan draws nothing (the
        in-graph sampling result is unused then, and the host RNG stream stays the one every
        engine configuration consumes: one uniform per sampled row)."""
        n = len(plan["positions"])
        nb = self._bucket(n)
        # a step with extended rows (``_launch_decode`` set ``_ext_step``) replays the bucket's
        # extended graph; its per-row penalty parameters follow the ``params_key`` rule below
        ext = self._ext_step if "temp" in plan else None
        lora = plan.get("lora")  # a step with an adapter row replays the bucket's LoRA graph
        kind = self._sampler_kind(ext)
        fields = self._EXT + (self._GUIDED if kind == 2 else ())
        graphs, gkey = self._graph_family(nb, kind, lora is not None)
        if gkey not in graphs:
            self._capture(nb, kind, lora is not None)
        g, b = graphs[gkey]
        h = b["stage"][b["flip"]]
        b["flip"] ^= 1
        hn = {k: v.numpy() for k, v in h.items()}
        if not cont:
            hn["ids"][:n] = plan["ids"]
        hn["positions"][:n] = plan["positions"]
        hn["slots"][:] = -1
        hn["slots"][:n] = plan["slots"]
        hn["block_tables"][:n] = plan["bt"]
        hn["ctx_lens"][:] = 1
        hn["ctx_lens"][:n] = plan["ctx"]
        hn["u"][:n] = plan["u"] if "u" in plan else 0.0
        if lora is not None:
            hn["lora_idx"][:] = -1
            hn["lora_idx"][:n] = lora
        if "temp" in plan:
            key = (np.asarray(plan["temp"], dtype=np.float32).tobytes(), np.asarray(plan["topk"], dtype=np.int32).tobytes(),
                   np.asarray(plan["topp"], dtype=np.float32).tobytes())
            if ext is not None:
                key += tuple(ext[k].tobytes() for k in fields)
            if ext is not None and b["params_key"] != key:
                b["slot"].fill_(-1)
                b["rep"].fill_(1.0)
                b["freq"].zero_()
                b["pres"].zero_()
                b["nlp"].zero_()
                if kind == 2:
                    b["guide"].fill_(-1)
                    b["gslot"].fill_(-1)
                for k in fields:
                    b[k][:n].copy_(torch.from_numpy(ext[k]).to(self.device))
            if b["params_key"] != key:
                d = self.device
                b["temp"].zero_()
                b["topk"].zero_()
                b["topp"].fill_(1.0)
                b["temp"][:n].copy_(torch.from_numpy(np.frombuffer(key[0], dtype=np.float32).copy()).to(d))
                b["topk"][:n].copy_(torch.from_numpy(np.frombuffer(key[1], dtype=np.int32).copy()).to(d))
                b["topp"][:n].copy_(torch.from_numpy(np.frombuffer(key[2], dtype=np.float32).copy()).to(d))
                b["params_key"] = key
        for k in b["staged"]:
            if cont and k == "ids":
                continue
            b[k].copy_(h[k], non_blocking=True)
        g.replay()
        self.stats["graph_replays"] += 1
        return g, b

    # ------------------------------------------------------------------ asynchronous decode
    @staticmethod
    def _sampling_fields(seqs: List[Sequence]) -> Dict[str, np.ndarray]:
        return {"temp": np.asarray([s.params.temperature for s in seqs], dtype=np.float32),
                "topk": np.asarray([s.params.top_k if s.params.top_k and s.params.top_k > 0 else 0 for s in seqs],
                                   dtype=np.int32),
                "topp": np.asarray([s.params.top_p for s in seqs], dtype=np.float32)}

    def _publish(self, plan: Dict) -> Dict:
        """TP hook: rank 0's plan to the other ranks (identity at TP = 1)."""
        return plan

    @torch.inference_mode()
    def _launch_decode(self, seqs: List[Sequence], plan: Dict, cont: bool) -> Dict:
        """Run a decode step with sampling (the graph replay, or the eager layer stack) and queue
        the D2H copy of its tokens; the tokens are read by :meth:`_finalize`.  ``cont``: the
        input ids are the previous step's sampled tokens, already on the device.

        TP > 1: the plan -- with the step's uniforms and sampling parameters -- goes to every rank
        first; every rank runs the same step and the same in-graph sampling on the same gathered
        logits and uniforms, so all ranks hold identical sampled ids on the device without a
        broadcast of the tokens, and a continued step (``cont``) feeds them back as its input on
        every rank.  Only rank 0 reads the tokens back."""
        n = len(seqs)
        self.stats["decode_tokens"] += n
        plan = dict(plan, op="decode_s", cont=bool(cont), u=self._np_rng.random(n, dtype=np.float32),
                    **self._sampling_fields(seqs))
        if cont:
            plan.setdefault("ids", np.zeros(n, dtype=np.int64))
        # extended rows: their fields stay on this rank (TP > 1 refuses such requests) and reach
        # the step beside the plan; slots are assigned, and their resets enqueued, here
        ext = self._ext_fields(seqs)
        self._ext_step = ext
        try:
            toks = self._decode_sample_exec(self._publish(plan))
        finally:
            self._ext_step = None
        want_lp = ext is not None and any(s.params.logprobs is not None for s in seqs)
        d = self.device
        host_lp = None
        if self._graph_ok(n):
            graphs, gkey = self._graph_family(self._bucket(n), self._sampler_kind(ext), plan.get("lora") is not None)
            b = graphs[gkey][1]
            out = b["host_toks"][b["tflip"]]
            if want_lp:  # the logprobs ride the same pinned D2H copy as the tokens
                host_lp = b["host_lp"][b["tflip"]]
                for k in self._EXT_OUT:
                    host_lp[k].copy_(b[k], non_blocking=True)
            b["tflip"] ^= 1
            out.copy_(toks, non_blocking=True)
        else:
            out = toks.to("cpu", non_blocking=True) if d.type == "cuda" else toks
            if want_lp:
                host_lp = {k: (t.to("cpu", non_blocking=True) if d.type == "cuda" else t)
                           for k, t in zip(self._EXT_OUT, self._ext_out)}
        ev = None
        if d.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        return {"seqs": list(seqs), "host": out, "host_lp": host_lp, "event": ev, "n": n}

    @torch.inference_mode()
    def _decode_sample_exec(self, plan: Dict) -> torch.Tensor:
        """Every rank's half of :meth:`_launch_decode`: the decode step + sampling of a
        ``decode_s`` plan; returns the device tensor of sampled ids (graph: the static ``toks``
        buffer, all bucket rows)."""
        use_knobs(self.knobs)
        cont = bool(plan["cont"])
        if self._graph_ok(len(plan["positions"])):
            _, b = self._stage_and_replay(plan, cont)
            return b["toks"]
        d = self.device
        n = len(plan["positions"])
        ids = self._last_toks if cont else torch.as_tensor(np.asarray(plan["ids"], dtype=np.int64)).to(d)
        logits = self._decode_body(ids, torch.as_tensor(np.asarray(plan["positions"], dtype=np.int32)).to(d),
                                   torch.as_tensor(np.asarray(plan["slots"], dtype=np.int64)).to(d),
                                   torch.from_numpy(np.asarray(plan["bt"])).to(d),
                                   torch.as_tensor(np.asarray(plan["ctx"], dtype=np.int32)).to(d),
                                   torch.as_tensor(np.asarray(plan["lora"], dtype=np.int32)).to(d)
                                   if plan.get("lora") is not None else None)
        temp = torch.from_numpy(np.asarray(plan["temp"], dtype=np.float32)).to(d)
        topk = torch.from_numpy(np.asarray(plan["topk"], dtype=np.int32)).to(d)
        topp = torch.from_numpy(np.asarray(plan["topp"], dtype=np.float32)).to(d)
        u = torch.from_numpy(np.asarray(plan["u"], dtype=np.float32)).to(d)
        ext = self._ext_step
        if ext is None:
            toks = ops.sample(logits[:n].contiguous(), temp, topk, topp, u)
        else:
            toks, lp, top_ids, top_lp = self._sample_ext_rows(logits[:n].contiguous(), temp, topk, topp, u, ext)
            self._ext_out = (lp, top_ids, top_lp)
        self._last_toks = toks
        return toks

    def _finalize(self, p: Dict) -> int:
        """Read an in-flight step's tokens (the one host sync of the pipeline) and append them."""
        if p["event"] is not None:
            p["event"].synchronize()
        toks = p["host"][: p["n"]].tolist()
        lps = None
        if p.get("host_lp") is not None:
            lps = self._lp_rows(p["seqs"], *(p["host_lp"][k][: p["n"]].tolist() for k in self._EXT_OUT))
        produced = 0
        for i, (seq, tok) in enumerate(zip(p["seqs"], toks)):
            if seq.status != "running":  # finished by the previous step's tokens: speculative row
                continue
            self.scheduler.computed(seq, 1)
            self._append(seq, tok, lps[i] if lps else None)
            produced += 1
        return produced

    def _continue_decode(self, p: Dict) -> Optional[Dict]:
        """Launch step N + 1 for the same batch before step N's tokens are known, when nothing
        else can change the batch: no request waiting for admission, every sequence of the batch
        still running and able to take two more tokens (length limits), and free KV blocks for
        one more token each (no preemption).  Its input ids are step N's sampled tokens, already
        on the device; positions / slots / context lengths advance by one."""
        seqs = p["seqs"]
        run = self.scheduler.running
        if (not self.knobs.async_decode or self.scheduler.waiting or len(run) != len(seqs)
                or any(a is not b for a, b in zip(run, seqs)) or self.kv.num_free_blocks < len(seqs)):
            return None
        for s in seqs:
            if (s.status != "running" or len(s.output_ids) + 2 > s.params.max_tokens
                    or s.num_tokens + 2 > self.max_model_len):
                return None
        for s in seqs:
            slot = self.kv.append_token(s.seq_id)
            if slot < 0:  # cannot happen with the free-block check; never launch half a batch
                raise RuntimeError("KV append failed despite free blocks")
            s._decode_slot = slot
            s.kv_len += 1
        plan = {**self._lora_rows(seqs),
                "positions": [s.num_tokens for s in seqs], "slots": [s._decode_slot for s in seqs],
                "ctx": [self.kv.num_tokens(s.seq_id) for s in seqs],
                "bt": np.asarray(self.kv.block_tables([s.seq_id for s in seqs], self.max_blocks_per_seq))}
        self.stats["async_continued"] = self.stats.get("async_continued", 0) + 1
        return self._launch_decode(seqs, plan, cont=True)

    def _async_ok(self) -> bool:
        return self.knobs.async_decode

    # ------------------------------------------------------------------ sampling
    def sample(self, logits: torch.Tensor, seqs: List[Sequence]) -> List[int]:
        return self._sample_rows(logits, seqs).tolist()

    def _sample_rows(self, logits: torch.Tensor, seqs: List[Sequence]) -> torch.Tensor:
        """Sampled token ids (device tensor) of the rows of ``logits``, one uniform per row from
        the engine's host RNG (the same stream the in-graph sampling draws from)."""
        n = len(seqs)
        d = self.device
        # per-row sampling parameters: rebuilt (3 host->device copies) only when the batch's
        # parameters change, not every decode step
        key = tuple((s.params.temperature, s.params.top_k if s.params.top_k and s.params.top_k > 0 else 0,
                     s.params.top_p) for s in seqs)
        cached = getattr(self, "_sample_params", None)
        if cached is None or cached[0] != key:
            temp = torch.tensor([k[0] for k in key], dtype=torch.float32, device=d)
            topk = torch.tensor([k[1] for k in key], dtype=torch.int32, device=d)
            topp = torch.tensor([k[2] for k in key], dtype=torch.float32, device=d)
            self._sample_params = cached = (key, temp, topk, topp)
        _, temp, topk, topp = cached
        u = torch.from_numpy(self._np_rng.random(n, dtype=np.float32)).to(d)
        self._host_lp = None
        ext = self._ext_fields(seqs)
        if ext is None:
            return ops.sample(logits.contiguous(), temp, topk, topp, u)
        toks, lp, top_ids, top_lp = self._sample_ext_rows(logits.contiguous(), temp, topk, topp, u, ext)
        if any(s.params.logprobs is not None for s in seqs):  # read with the tokens (this path syncs anyway)
            self._host_lp = self._lp_rows(seqs, lp.tolist(), top_ids.tolist(), top_lp.tolist())
        return toks

    def _take_host_lp(self) -> Optional[List]:
        """The logprob rows :meth:`_sample_rows` left for the batch just sampled (None: no row
        asked for logprobs, or an instance-level ``sample`` override did the sampling)."""
        lps, self._host_lp = self._host_lp, None
        return lps

    # ------------------------------------------------------------------ extended sampling
    def _sampler_vocab(self) -> int:
        return self.model.head_weight().shape[0] * self.tp

    def _ext_fields(self, seqs: List[Sequence]) -> Optional[Dict[str, np.ndarray]]:
        """The per-row ``ops.sample_ext`` inputs of a batch, or None when no row is extended (the
        batch then samples exactly as before).  Plain rows get the neutral values (slot -1).  A
        penalized sequence without a state slot takes one here and has it initialised from its
        prompt and the tokens generated so far -- admission and resumption after preemption alike;
        the reset is enqueued on the engine's stream, behind any speculative row of an in-flight
        step that still writes to a recycled slot."""
        guided = any(s.params.guided for s in seqs)
        if not guided and not any(s.params.extended for s in seqs):
            return None
        if self._sampler_state is None and (not guided or any(s.params.penalized for s in seqs)):
            S, V = self.max_batch_size, self._sampler_vocab()
            self._sampler_state = (torch.zeros(S, V, dtype=torch.int32, device=self.device),
                                   torch.zeros(S, V, dtype=torch.uint8, device=self.device))
            log.info("engine: sampler state for penalties: %d slots x %d tokens, %.2f MB", S, V, S * V * 5 / 1e6)
            # guided graphs captured before hold the arena's placeholder state: capture them again
            self._drop_graphs(lambda fam, key: fam is self._graphs_guided or (fam is self._graphs_lora and key[1] == 2))
        if guided:
            self._ensure_guide_arena()
        counts, mask = self._sampler_tensors() if guided else self._sampler_state
        n = len(seqs)
        ext = {"slot": np.full(n, -1, dtype=np.int32), "rep": np.ones(n, dtype=np.float32),
               "freq": np.zeros(n, dtype=np.float32), "pres": np.zeros(n, dtype=np.float32),
               "nlp": np.zeros(n, dtype=np.int32)}
        for i, s in enumerate(seqs):
            p = s.params
            if p.penalized:
                if s.sampler_slot < 0:
                    s.sampler_slot = self._row_slot(s)
                    ops.sampler_state_reset(counts, mask, s.sampler_slot, s.prompt_ids, s.output_ids)
                ext["slot"][i] = s.sampler_slot
                ext["rep"][i], ext["freq"][i], ext["pres"][i] = p.repetition_penalty, p.frequency_penalty, p.presence_penalty
            if p.logprobs is not None:
                ext["nlp"][i] = min(max(int(p.logprobs), 0), ops.ref.TOP_LOGPROBS)
        if guided:
            ext["guide"] = np.full(n, -1, dtype=np.int32)
            ext["gslot"] = np.full(n, -1, dtype=np.int32)
            for i, s in enumerate(seqs):
                if s.params.guided:
                    if s.guide_slot < 0:
                        self._pin_guide(s)
                    ext["guide"][i], ext["gslot"][i] = s.guide_table, s.guide_slot
        return ext

    def _row_slot(self, seq: Sequence) -> int:
        """The row slot of ``seq`` (its counts row and its guide-state word share the index): the one
        it holds, or a free one."""
        held = max(seq.sampler_slot, seq.guide_slot)
        if held >= 0:
            return held
        if not self._sampler_free:
            raise RuntimeError(f"no free sampler-state slot ({self.max_batch_size} penalized or guided "
                               "sequences are already running)")
        return self._sampler_free.pop()

    def _release_sampler_slot(self, seq: Sequence) -> None:
        """Scheduler hook: ``seq`` finished or was preempted; its row slot returns to the free list
        and its guide's table slot loses a reference."""
        held = max(seq.sampler_slot, seq.guide_slot)
        if held >= 0:
            self._sampler_free.append(held)
        seq.sampler_slot = seq.guide_slot = -1
        if seq.guide_table >= 0:
            ent = self._guide_tables.get(seq.guide.key)
            if ent is not None and ent[0] == seq.guide_table:
                ent[1] -= 1
                if ent[1] <= 0:
                    del self._guide_tables[seq.guide.key]
                    self._guide_table_free.append(ent[0])
            seq.guide_table = -1

    # ------------------------------------------------------------------ guided decoding
    def _sampler_tensors(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``counts`` / ``prompt_mask`` for ``ops.sample_guided``: the penalties' state when a
        penalized request has made it, else the arena's one-row placeholder (every row has slot -1)."""
        if self._sampler_state is not None:
            return self._sampler_state
        return self._guide_arena["counts0"], self._guide_arena["mask0"]

    def _drop_graphs(self, which) -> None:
        """Reset and forget the captured graphs for which ``which(family dict, key)`` holds."""
        doomed = [(fam, key) for fam in (self._graphs, self._graphs_ext, self._graphs_guided, self._graphs_lora)
                  for key in fam if which(fam, key)]
        if doomed and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for fam, key in doomed:
            fam.pop(key)[0].reset()

    def _ensure_guide_arena(self) -> Dict[str, torch.Tensor]:
        if self._guide_arena is None:
            G, V, W, d = self.max_batch_size, self._sampler_vocab(), self.guide_table_words, self.device
            i32 = dict(dtype=torch.int32, device=d)
            self._guide_arena = {"cls": torch.zeros(G, V, **i32), "next": torch.full((G, W), -1, **i32),
                                 "meta": torch.zeros(G, 2, **i32), "state": torch.zeros(G, **i32),
                                 "counts0": torch.zeros(1, V, **i32),
                                 "mask0": torch.zeros(1, V, dtype=torch.uint8, device=d)}
            self._guide_table_free = list(range(G - 1, -1, -1))
            nbytes = sum(t.numel() * t.element_size() for t in self._guide_arena.values())
            log.info("engine: guide arena: %d table slots x (%d tokens + %d table words), %.2f MB", G, V, W,
                     nbytes / 1e6)
        return self._guide_arena

    def _pin_guide(self, seq: Sequence) -> None:
        """Give a guided sequence its state word and its guide a table slot (uploading the tables
        when no running sequence holds the same guide), and set the state to where the tokens
        generated so far lead -- admission and resumption after preemption alike.  Everything is
        enqueued on the engine's stream, behind any step still in flight."""
        a = self._ensure_guide_arena()
        g = seq.guide
        ent = self._guide_tables.get(g.key)
        if ent is None:
            if not self._guide_table_free:
                raise RuntimeError(f"no free guide table slot ({self.max_batch_size} guides are in use)")
            t = self._guide_table_free.pop()
            S, C = g.next.shape
            a["cls"][t].copy_(torch.from_numpy(g.cls))
            a["next"][t, :S * C].copy_(torch.from_numpy(g.next.reshape(-1)))
            a["meta"][t].copy_(torch.tensor([S, C], dtype=torch.int32))
            ent = self._guide_tables[g.key] = [t, 0]
        ent[1] += 1
        seq.guide_table = ent[0]
        seq.guide_slot = self._row_slot(seq)
        ops.guide_state_reset(a["state"], seq.guide_slot, g.walk(seq.output_ids))

    def _sample_ext_rows(self, logits, temp, topk, topp, u, ext: Dict[str, np.ndarray]):
        """``ops.sample_ext`` -- or, for a step with a guided row, ``ops.sample_guided`` -- on the rows
        of ``logits`` with the step's extended fields."""
        d = self.device
        fields = [torch.from_numpy(ext[k]).to(d) for k in self._EXT]
        if "guide" not in ext:
            counts, mask = self._sampler_state
            return ops.sample_ext(logits, temp, topk, topp, u, *fields, counts, mask, check_slots=False)
        counts, mask = self._sampler_tensors()
        a = self._guide_arena
        return ops.sample_guided(logits, temp, topk, topp, u, *fields, counts, mask,
                                 torch.from_numpy(ext["guide"]).to(d), torch.from_numpy(ext["gslot"]).to(d),
                                 a["cls"], a["next"], a["meta"], a["state"], check_slots=False)

    @staticmethod
    def _lp_rows(seqs: List[Sequence], lp: List[float], top_ids: List[List[int]], top_lp: List[List[float]]):
        """Per row: None, or ``(logprob, [(token id, logprob), ...])`` with the sequence's
        ``logprobs`` most likely tokens."""
        return [None if s.params.logprobs is None else
                (lp[i], [(t, v) for t, v in zip(top_ids[i], top_lp[i]) if t >= 0])
                for i, s in enumerate(seqs)]

    # ------------------------------------------------------------------ step loop
    def add_request(self, prompt_ids: List[int], params: SamplingParams, request_id: str = "", on_token=None,
                    on_finish=None) -> Sequence:
        seq = Sequence(prompt_ids=list(prompt_ids), params=params, request_id=request_id, on_token=on_token,
                       on_finish=on_finish)
        name = getattr(params, "lora", None)
        if name is not None:
            if name not in self._lora_slots:
                raise ValueError(f"unknown LoRA adapter {name!r} (loaded: {sorted(self._lora_slots) or 'none'})")
            seq.lora_slot, seq.lora_salt = self._lora_slots[name], self._lora_salt[name]
        if getattr(params, "prompt_logprobs", None) is not None:
            if self.tp > 1:  # the vocabulary projection is sharded and the plan channel carries no targets
                raise ValueError(f"prompt_logprobs not supported with tensor parallelism > 1 (TP = {self.tp})")
            seq.prompt_logprobs, seq.prompt_ranks, seq.prompt_top_logprobs = [None], [None], [None]
        if getattr(params, "guided", False):  # compiled (or taken from the cache) on the caller's thread
            from . import guided

            kind, spec = guided.params_guide(params)
            if self.tp > 1:
                raise ValueError(f"guided_{kind} not supported with tensor parallelism > 1 (TP = {self.tp})")
            seq.guide = guided.compile_guide(kind, spec, self.tokenizer, self._sampler_vocab(),
                                             table_words=self.guide_table_words)
        self.scheduler.add(seq)
        return seq

    # ------------------------------------------------------------------ LoRA adapters
    def _lora_projections(self, layer) -> Dict[str, torch.Tensor]:
        from .lora import PROJECTIONS

        return {n: getattr(layer, n) for n in PROJECTIONS
                if isinstance(getattr(layer, n, None), torch.Tensor) and getattr(layer, n).dim() == 2}

    def _alloc_lora(self):
        """Per layer and projection the resident stacked adapters ``(A_all [slots, R, K], B_all
        [slots, N, R], scale_all [slots] fp32)``, all zeros: loading an adapter is a ``copy_`` into
        its slot, the addresses never change, so captured graphs stay valid across loads."""
        from .lora import LORA_RANKS

        S, R = self.max_loras, self.max_lora_rank
        if R not in LORA_RANKS:
            raise ValueError(f"max_lora_rank must be one of {LORA_RANKS}, got {R}")
        out, nbytes = [], 0
        for li, layer in enumerate(self.model.layers):
            d = {}
            for name, w in self._lora_projections(layer).items():
                N, K = w.shape
                if self.device.type == "cuda" and (N % 64 or K % 64):
                    raise ValueError(f"LoRA: layer {li} {name} [{N}, {K}] does not fit the adapter kernels "
                                     "(out and in features multiples of 64)")
                d[name] = (torch.zeros(S, R, K, dtype=self.dtype, device=self.device),
                           torch.zeros(S, N, R, dtype=self.dtype, device=self.device),
                           torch.zeros(S, dtype=torch.float32, device=self.device))
                nbytes += sum(t.numel() * t.element_size() for t in d[name])
            out.append(d)
        log.info("engine: LoRA adapter slots: %d x rank %d on %d projections: %.3f GB (out of the KV cache budget)",
                 S, R, sum(len(d) for d in out), nbytes / 1e9)
        return out

    def _lora_refusal(self) -> Optional[str]:
        if self.cfg.is_moe:
            return "LoRA adapters not supported with MoE models (routed-expert adapters are out of scope)"
        if self.tp > 1:
            return f"LoRA adapters not supported with tensor parallelism > 1 (TP = {self.tp})"
        return None

    @torch.no_grad()
    def load_lora(self, name: str, adapter) -> int:
        """Make ``adapter`` (a ``LoRAAdapter``, or the path of an adapter directory) selectable as
        ``SamplingParams(lora=name)``; returns its slot.  Ranks below ``max_lora_rank`` are
        zero-padded, larger ones refused.  Every load draws a fresh prefix-cache salt: K/V blocks
        computed under an earlier adapter of the same name are never re-attached."""
        import os

        from .lora import LoRAAdapter

        why = self._lora_refusal()
        if why is not None:
            raise ValueError(why)
        if self._lora is None:
            raise ValueError("this engine has no LoRA slots (max_loras = 0)")
        if name in self._lora_slots:
            raise ValueError(f"LoRA adapter {name!r} is already loaded (unload_lora first)")
        if len(self._lora_slots) >= self.max_loras:
            raise ValueError(f"cannot load LoRA adapter {name!r}: max_loras = {self.max_loras} adapters are loaded")
        if not isinstance(adapter, LoRAAdapter):
            adapter = LoRAAdapter.load(str(adapter), self.cfg)
        R = self.max_lora_rank
        staged = []  # everything validated and padded before a slot is touched
        known = set()
        for li, d in enumerate(self._lora):
            for pname, (A_all, B_all, _) in d.items():
                known.add((li, pname))
                staged.append((li, pname, adapter.padded(li, pname, R, B_all.shape[1], A_all.shape[2])))
        stray = sorted(set(adapter.tensors) - known)
        if stray:
            raise ValueError(f"LoRA adapter {name!r} targets projections the model does not have: {stray[:4]}")
        slot = min(set(range(self.max_loras)) - set(self._lora_slots.values()))
        for li, pname, ab in staged:
            A_all, B_all, sc = self._lora[li][pname]
            if ab is None:  # a missing (layer, projection) means a zero delta
                A_all[slot].zero_()
                B_all[slot].zero_()
            else:
                A_all[slot].copy_(ab[0].to(A_all.dtype))
                B_all[slot].copy_(ab[1].to(B_all.dtype))
            sc[slot] = adapter.scale
        self._lora_slots[name] = slot
        self._lora_salt[name] = os.urandom(16)
        self._lora_scale[slot] = adapter.scale
        return slot

    @torch.no_grad()
    def unload_lora(self, name: str) -> None:
        """Free ``name``'s slot (zeroed).  Raises while a live sequence uses the adapter."""
        if name not in self._lora_slots:
            raise ValueError(f"unknown LoRA adapter {name!r}")
        slot = self._lora_slots[name]
        live = [s for s in list(self.scheduler.running) + list(self.scheduler.waiting)
                if s.lora_slot == slot and s.status != "finished"]
        if live:
            raise RuntimeError(f"LoRA adapter {name!r} is in use by {len(live)} live sequence(s)")
        for d in self._lora:
            for A_all, B_all, sc in d.values():
                A_all[slot].zero_()
                B_all[slot].zero_()
                sc[slot] = 0.0
        del self._lora_slots[name], self._lora_salt[name]
        self._lora_scale.pop(slot, None)

    @property
    def loras(self) -> List[str]:
        return sorted(self._lora_slots)

    def _append(self, seq: Sequence, tok: int, lp=None) -> None:
        """``lp``: the token's row of :meth:`_lp_rows` (a sequence with ``logprobs`` set)."""
        now = time.time()
        if seq.first_token_time is None:
            seq.first_token_time = now
        seq.output_ids.append(tok)
        if seq.params.logprobs is not None:  # kept in step with output_ids (before on_token reads them)
            seq.output_logprobs.append(lp[0] if lp is not None else float("nan"))
            seq.output_top_logprobs.append(lp[1] if lp is not None else [])
        if seq.on_token:
            seq.on_token(seq, tok)
        eos = getattr(self.tokenizer, "eos_token_id", None)
        if not seq.params.ignore_eos and eos is not None and tok == eos:
            self.scheduler.finish(seq, "stop")
        elif len(seq.output_ids) >= seq.params.max_tokens:
            self.scheduler.finish(seq, "length")
        elif seq.num_tokens >= self.max_model_len:
            self.scheduler.finish(seq, "length")
        elif seq.params.stop:
            text = self.tokenizer.decode(seq.output_ids)
            if any(st and st in text for st in seq.params.stop):
                self.scheduler.finish(seq, "stop")

    def step(self) -> int:
        """One scheduling iteration; returns the number of tokens produced.  Pure decode steps
        run asynchronously (knob ``async_decode``): the step is launched and its tokens are read
        by the NEXT call, which first launches the following step when the batch cannot change."""
        use_knobs(self.knobs)
        produced = 0
        if self._pending is not None:
            p, self._pending = self._pending, None
            nxt = self._continue_decode(p)
            produced = self._finalize(p)
            if nxt is not None:
                self._pending = nxt
                self.stats["steps"] += 1
                return produced
            if not self.scheduler.has_work():
                return produced
        out = self.scheduler.schedule()
        if out.decode and out.prefill and self._mixed_ok():
            logits = self.mixed(out.prefill, out.decode)
            final = [c.seq for c in out.prefill if c.samples]
            toks = self.sample(logits, final + list(out.decode))
            lps = self._take_host_lp()
            self._finish_scores(out.prefill)
            for c in out.prefill:
                self.scheduler.computed(c.seq, c.count)
                self.stats["prefix_hit_tokens"] = self.stats.get("prefix_hit_tokens", 0) + (
                    c.seq.cached_tokens if c.start == c.seq.cached_tokens else 0)
            self._finish_score_only(out.prefill)
            for seq in out.decode:
                self.scheduler.computed(seq, 1)
            for i, (seq, tok) in enumerate(zip(final + list(out.decode), toks)):
                self._append(seq, tok, lps[i] if lps else None)
                produced += 1
            self.stats["steps"] += 1
            return produced
        if out.decode and not out.prefill and "sample" not in self.__dict__:
            # sampling in the decode step (inside the graph); asynchronous: tokens read next call.
            # (an instance-level ``sample`` override -- teacher forcing, logit capture -- keeps
            # the host-sampling path below)
            pend = self._launch_decode(out.decode, self.decode_plan(out.decode), cont=False)
            self.stats["steps"] += 1
            if self._async_ok():
                self._pending = pend
                return produced
            return produced + self._finalize(pend)
        if out.decode:
            logits = self.decode(out.decode)
            toks = self.sample(logits, out.decode)
            lps = self._take_host_lp()
            for i, (seq, tok) in enumerate(zip(out.decode, toks)):
                self.scheduler.computed(seq, 1)
                self._append(seq, tok, lps[i] if lps else None)
                produced += 1
        if out.prefill:
            logits = self.prefill(out.prefill)
            final = [c.seq for c in out.prefill if c.samples]
            self._finish_scores(out.prefill)
            for c in out.prefill:
                self.scheduler.computed(c.seq, c.count)
                self.stats["prefix_hit_tokens"] = self.stats.get("prefix_hit_tokens", 0) + (
                    c.seq.cached_tokens if c.start == c.seq.cached_tokens else 0)
            self._finish_score_only(out.prefill)
            if final:
                toks = self.sample(logits, final)
                lps = self._take_host_lp()
                for i, (seq, tok) in enumerate(zip(final, toks)):
                    self._append(seq, tok, lps[i] if lps else None)
                    produced += 1
        self.stats["steps"] += 1
        return produced

    def generate(self, prompts: List[List[int]], params: SamplingParams) -> List[Sequence]:
        seqs = [self.add_request(p, params) for p in prompts]
        while any(s.status != "finished" for s in seqs):
            self.step()
        return seqs
