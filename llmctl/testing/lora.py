"""Serving scenarios of per-request LoRA adapters on the tiny model, shared by the CPU suite (the
fp32 oracle behind ``ops``) and the GPU suite (``csrc/lora_decode.hip`` behind the fused decode
projections, the captured LoRA graphs, the asynchronous pipeline).  Every function asserts its
scenario on ``device``.

The end-to-end oracle is a base-only fp32 CPU engine whose weights had the adapter merged
(``merge_into``).  All engines of a process share one model: built on the CPU, every parameter
rounded to a bf16 value (so the bf16 GPU copy holds the same numbers), adapters likewise."""

from __future__ import annotations

import copy
from typing import Dict, List, Optional

import torch

from llmctl.serve.engine import InferenceEngine
from llmctl.serve.lora import LoRAAdapter, merge_into, random_adapter
from llmctl.serve.scheduler import SamplingParams
from llmctl.testing.numerics import row_err, snap_int4_grid
from llmctl.testing.sampling_ext import MODES

ENGINE = dict(max_batch_size=4, num_kv_blocks=128, block_size=16, max_model_len=512)
PROMPTS = [[1, 2, 3, 4, 5], [9] * 37, [7, 7], [3] * 70]
ADAPTERS = ["a", None, "b", "a"]  # the mixed batch: adapter of each request
STEPS = 8
MIN_MOVE = 0.15  # 5 x the engine bound 3e-2: what an adapter must move the logits by, so a dropped one cannot pass
CPU_TOL = 1e-4  # the oracle against itself (fp32, two summation orders)

_CACHE: Dict = {}


def _model(grid: bool = False):
    """The shared tiny model (CPU, fp32 storage, bf16 values); ``grid``: its int4-eligible weights
    and LM head snapped onto the lossless int4 grid."""
    key = "grid" if grid else "model"
    if key not in _CACHE:
        from llmctl.models import build_model, get_model_config

        cfg = get_model_config("tiny")
        model = build_model(cfg, device="cpu", dtype=torch.float32, seed=3)
        with torch.no_grad():
            for p in model.parameters():
                p.copy_(p.bfloat16().float())
            if grid:
                ws = [getattr(layer, n) for layer in model.layers for n in InferenceEngine._W8_NAMES] + [model.head_weight()]
                for w in ws:
                    if w.dim() == 2 and w.shape[0] % 64 == 0 and w.shape[1] % 128 == 0:
                        w.copy_(snap_int4_grid(w))
        _CACHE[key] = (model.eval(), cfg)
    return _CACHE[key]


def adapter(name: str) -> LoRAAdapter:
    """Adapters ``a``, ``b``, ``c``: rank 8, std 0.02, alpha 16 (scale 2), bf16 values."""
    if ("adapter", name) not in _CACHE:
        _, cfg = _model()
        ad = random_adapter(cfg, rank=8, seed=11 + "abc".index(name), std=0.02, alpha=16.0)
        ad.tensors = {k: (A.bfloat16().float(), B.bfloat16().float()) for k, (A, B) in ad.tensors.items()}
        _CACHE[("adapter", name)] = ad
    return _CACHE[("adapter", name)]


def engine(device: str, model=None, loras=("a", "b"), **kw) -> InferenceEngine:
    """An engine on a copy of the shared model (or ``model``), adapters ``loras`` loaded."""
    src, cfg = (model, _model()[1]) if model is not None else _model()

    class SharedModelEngine(InferenceEngine):
        def _load(self, model_path, dtype, seed):
            return copy.deepcopy(src).to(device=self.device, dtype=dtype), cfg, None

    kw = dict(ENGINE, max_loras=2, max_lora_rank=16, **kw)
    e = SharedModelEngine("tiny", device=device, seed=3, **kw)
    for name in loras:
        e.load_lora(name, adapter(name))
    return e


def run_forced(eng, prompts, loras, max_tokens=STEPS, forced=None, **params):
    """Greedy (or teacher-forced) generation recording every step's logits per sequence; returns
    ``(token ids, logits [requests, steps, V], sequences)``."""
    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, lora=l, **params))
            for p, l in zip(prompts, loras)]
    idx = {s.seq_id: i for i, s in enumerate(seqs)}
    rec: Dict[int, List[torch.Tensor]] = {}
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
    try:
        while any(s.status != "finished" for s in seqs):
            eng.step()
    finally:
        del eng.sample
    return [s.output_ids for s in seqs], torch.stack([torch.stack(rec[i]) for i in range(len(seqs))]), seqs


def run_free(eng, prompts, loras, max_tokens=16, **params):
    """Greedy generation through the engine's own sampling (in-graph, asynchronous where enabled)."""
    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True, lora=l, **params))
            for p, l in zip(prompts, loras)]
    while any(s.status != "finished" for s in seqs):
        eng.step()
    return seqs


def _flat(lg):
    return lg.reshape(-1, lg.shape[-1])


def oracle() -> Dict:
    """Computed once per process on the CPU in fp32: the base engine's greedy tokens on PROMPTS and,
    teacher-forced on them, the logits of the base model and of the model with ``a`` / ``b`` / ``c``
    merged.  Asserts that every adapter moves the decode logits by at least MIN_MOVE."""
    if "oracle" not in _CACHE:
        out: Dict = {}
        with engine("cpu", loras=()) as e:
            out["toks"], out["base"], _ = run_forced(e, PROMPTS, [None] * 4)
        for name in "abc":
            merged = merge_into(copy.deepcopy(_model()[0]), adapter(name))
            with engine("cpu", model=merged, loras=()) as e:
                _, out[name], _ = run_forced(e, PROMPTS, [None] * 4, forced=out["toks"])
            move = row_err(_flat(out[name][:, 1:]), _flat(out["base"][:, 1:]))
            print(f"adapter {name}: merged vs base decode logits row_err {move:.3f}")
            out["move_" + name] = move
        _CACHE["oracle"] = out
    out = _CACHE["oracle"]
    for name in "abc":
        assert out["move_" + name] >= MIN_MOVE, (name, out["move_" + name])
    return out


def want_logits(names=ADAPTERS) -> torch.Tensor:
    """The oracle's logits of the mixed batch: request ``i`` under adapter ``names[i]``."""
    o = oracle()
    return torch.stack([o[n if n is not None else "base"][i] for i, n in enumerate(names)])


def bound(device: str) -> float:
    """What adapter logits may differ from the merged oracle by.  CPU: CPU_TOL.  GPU: measured here,
    once: 2 x ``err_base``, the row_err of the GPU base engine against the CPU fp32 base engine on
    the same tokens (the factor 2 covers the two extra bf16-input products per projection and the
    changed activations)."""
    if device == "cpu":
        return CPU_TOL
    if ("bound", device) not in _CACHE:
        o = oracle()
        with engine(device, loras=()) as e:
            _, lg, _ = run_forced(e, PROMPTS, [None] * 4, forced=o["toks"])
        err_base = row_err(_flat(lg[:, 1:]), _flat(o["base"][:, 1:]))
        print(f"err_base ({device} base engine vs CPU fp32 base engine, decode logits) {err_base:.3e}")
        assert 0 < err_base < 3e-2, err_base
        _CACHE[("bound", device)] = 2 * err_base
    return _CACHE[("bound", device)]


def _err_rows(lg, want, names=ADAPTERS) -> float:
    """row_err over the decode logits of the adapter requests."""
    rows = [i for i, n in enumerate(names) if n is not None]
    return row_err(_flat(lg[rows][:, 1:]), _flat(want[rows][:, 1:]))


# ------------------------------------------------------------------------------------- scenarios
def check_merged_oracle(device: str) -> None:
    """1. Four concurrent requests on adapters a, none, b, a: every adapter row's decode logits are
    those of the base-only engine with that adapter merged."""
    o, tol = oracle(), bound(device)
    with engine(device) as e:
        toks, lg, _ = run_forced(e, PROMPTS, ADAPTERS, forced=o["toks"])
        assert toks == o["toks"]
        if e.use_graphs:
            assert e._graphs_lora and e.stats["graph_replays"] > 0
    want = want_logits()
    err_lora = _err_rows(lg, want)
    err_all = row_err(_flat(lg), _flat(want))  # the prefill step and the adapter-less request included
    print(f"merged oracle on {device}: err_lora {err_lora:.3e} (bound {tol:.3e}), all rows and steps {err_all:.3e}")
    assert err_lora <= tol, (err_lora, tol)
    assert err_all <= max(tol, 3e-2 if device != "cpu" else tol), err_all
    # the adapters are told apart: request 0 (a) is not b's
    assert _err_rows(lg, want_logits(["b", None, "a", "b"])) >= MIN_MOVE / 2


def check_modes(device: str) -> None:
    """2. The three engine modes agree on the mixed batch's logits; graph modes replay the LoRA graph
    family and the asynchronous pipeline continues through adapter batches."""
    o, tol, want = oracle(), bound(device), want_logits()
    runs, free = [], []
    for mode in MODES:
        with engine(device, **mode) as e:
            _, lg, _ = run_forced(e, PROMPTS, ADAPTERS, forced=o["toks"])
            err = _err_rows(lg, want)
            print(f"mode {mode}: err_lora {err:.3e} (bound {tol:.3e})")
            assert err <= tol, (mode, err, tol)
            runs.append(lg)
            seqs = run_free(e, PROMPTS, ADAPTERS)
            free.append([s.output_ids for s in seqs])
            if e.use_graphs:
                assert e._graphs_lora and e.stats["graph_replays"] > 0
                if mode["perf_knobs"]["async_decode"]:
                    assert e.stats.get("async_continued", 0) > 5
            else:
                assert not e._graphs_lora and not e._graphs
    for lg in runs[1:]:
        assert _err_rows(lg, runs[0]) <= tol
    assert free[1] == free[0] and free[2] == free[0]


def check_base_rows_untouched(device: str) -> None:
    """3. In the mixed batch the request without an adapter produces exactly the tokens it produces
    when the same four requests run with no adapters at all, in the same mode."""
    oracle()
    for mode in MODES:
        with engine(device, **mode) as e:
            plain = run_free(e, PROMPTS, [None] * 4)
            assert not e._graphs_lora
            mixed = run_free(e, PROMPTS, ADAPTERS)
        assert mixed[1].output_ids == plain[1].output_ids, mode
        assert any(mixed[i].output_ids != plain[i].output_ids for i in (0, 2, 3)), mode


def check_prefix_cache(device: str) -> None:
    """4. K/V depend on the adapter: a cached prefix is re-attached only under the adapter (and the
    load) it was computed with."""
    oracle()
    tol = bound(device)
    prompt = [[(7 * i) % 200 + 1 for i in range(40)]]
    with engine(device) as e:
        cached, logits, toks = [], [], None
        for name in (None, "a", "b", "a"):
            t, lg, seqs = run_forced(e, prompt, [name], forced=toks if name == "a" else None)
            if name == "a" and toks is None:
                toks = t
            cached.append(seqs[0].cached_tokens)
            logits.append(lg)
        assert cached[:3] == [0, 0, 0] and cached[3] > 0, cached
        err = row_err(_flat(logits[3]), _flat(logits[1]))
        print(f"prefix-cache hit under adapter a: logits row_err {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (err, tol)
        assert row_err(_flat(logits[1]), _flat(logits[0])) >= MIN_MOVE / 2
        e.unload_lora("a")
        e.load_lora("a", adapter("c"))  # a different adapter under the old name
        _, _, seqs = run_forced(e, prompt, ["a"])
        assert seqs[0].cached_tokens == 0


def check_slot_reuse(device: str) -> None:
    """5. Unload a, load c: c takes a's slot, the captured LoRA graphs are the same objects (no
    recapture) and c's logits are c's merged oracle's."""
    o, tol = oracle(), bound(device)
    with engine(device) as e:
        slot_a = e._lora_slots["a"]
        run_forced(e, PROMPTS, ["a"] * 4, forced=o["toks"])
        graphs = dict(e._graphs_lora)
        e.unload_lora("a")
        assert e.load_lora("c", adapter("c")) == slot_a
        _, lg, _ = run_forced(e, PROMPTS, ["c"] * 4, forced=o["toks"])
        assert set(e._graphs_lora) == set(graphs) and all(e._graphs_lora[k][0] is g for k, (g, _) in graphs.items())
        if e.use_graphs:
            assert graphs
    err = _err_rows(lg, want_logits(["c"] * 4), ["c"] * 4)
    print(f"slot reuse: c in a's slot, err_lora {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (err, tol)


def check_preemption(device: str) -> None:
    """6. An adapter sequence preempted after 9 tokens finishes with the ids of an undisturbed run."""
    oracle()
    base = [(7 * i) % 200 + 1 for i in range(40)]
    p = SamplingParams(max_tokens=20, temperature=0.0, ignore_eos=True, lora="a")
    with engine(device, perf_knobs={"async_decode": False}) as e:  # the scheduler state is read between steps
        seq = e.add_request(base, p)
        for _ in range(9):
            e.step()
        assert len(seq.output_ids) == 9 and seq.lora_slot >= 0
        e.scheduler._preempt(seq)
        while seq.status != "finished":
            e.step()
        assert seq.preemptions == 1 and len(seq.output_ids) == 20
    with engine(device, perf_knobs={"async_decode": False}) as e:
        ref = run_free(e, [base], ["a"], max_tokens=20)[0]
        plain = run_free(e, [base], [None], max_tokens=20)[0]
    assert seq.output_ids == ref.output_ids
    assert plain.output_ids != ref.output_ids


def check_structure(device: str) -> None:
    """7. Plain batches never touch the LoRA graphs; an adapter in use cannot be unloaded; loads stop
    at ``max_loras``; unknown names are refused; close() empties everything; no slots, no tensors."""
    e = engine(device)
    run_free(e, PROMPTS, [None] * 4)
    assert e._graphs_lora == {}
    graphs = dict(e._graphs)
    seq = e.add_request(PROMPTS[0], SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True, lora="a"))
    try:
        e.unload_lora("a")
        raise AssertionError("unload_lora of an adapter in use did not raise")
    except RuntimeError as ex:
        assert "in use" in str(ex)
    while seq.status != "finished":
        e.step()
    assert dict(e._graphs) == graphs
    if e.use_graphs:
        assert e._graphs_lora and graphs
    for bad, exc in ((lambda: e.load_lora("c", adapter("c")), "max_loras = 2"),
                     (lambda: e.add_request([1, 2], SamplingParams(lora="nope")), "unknown LoRA adapter 'nope'"),
                     (lambda: e.unload_lora("nope"), "unknown LoRA adapter")):
        try:
            bad()
            raise AssertionError(f"no refusal: {exc}")
        except ValueError as ex:
            assert exc in str(ex), ex
    e.unload_lora("a")
    e.load_lora("c", adapter("c"))
    assert e.loras == ["b", "c"]
    e.close()
    assert e._graphs == {} and e._graphs_lora == {} and e._lora is None and e.loras == []
    with InferenceEngine("tiny", device=device, **ENGINE) as e0:
        assert e0._lora is None and e0.max_loras == 0
        try:
            e0.load_lora("a", adapter("a"))
            raise AssertionError("load_lora without slots did not raise")
        except ValueError as ex:
            assert "max_loras = 0" in str(ex)


def check_extended_sampler(device: str) -> None:
    """8. An adapter request with a huge presence penalty under greedy decoding never repeats a
    token, through the LoRA graph family's extended member."""
    oracle()
    with engine(device) as e:
        s = run_free(e, PROMPTS[:1], ["a"], max_tokens=24, presence_penalty=1e4)[0]
        assert len(s.output_ids) == 24 and len(set(s.output_ids)) == 24, s.output_ids
        if e.use_graphs:
            assert (e._bucket(1), True) in e._graphs_lora and not e._graphs_ext


def check_int4_base(device: str) -> None:
    """9. (GPU) int4 decode weights on the lossless-grid model with adapter a follow the bf16-weight
    engine with a on the same tokens, within the project's 3e-2."""
    oracle()
    grid = _model(grid=True)[0]
    with engine(device, model=grid) as e:
        toks, lg_ref, _ = run_forced(e, PROMPTS, ["a"] * 4)
        _, lg_base, _ = run_forced(e, PROMPTS, [None] * 4, forced=toks)
    assert row_err(_flat(lg_ref[:, 1:]), _flat(lg_base[:, 1:])) >= MIN_MOVE
    with engine(device, model=grid, weight_dtype="int4") as e:
        assert e.weight_dtype == "int4" and e._w4 is not None
        _, lg4, _ = run_forced(e, PROMPTS, ["a"] * 4, forced=toks)
        assert e._graphs_lora and e.stats["graph_replays"] > 0
    err = row_err(_flat(lg4[:, 1:]), _flat(lg_ref[:, 1:]))
    print(f"int4 base + adapter a vs bf16 base + adapter a: decode logits row_err {err:.3e}")
    assert err < 3e-2, err
