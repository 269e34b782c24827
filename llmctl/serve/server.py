"""HTTP inference server (FastAPI + uvicorn) around :class:`InferenceEngine`.

Routes (same as the reference, ``server.py:286-311``): ``POST /v1/completions``,
``GET /v1/models``, ``GET /health``; plus ``GET /metrics`` (Prometheus) and SSE streaming
when ``stream=true`` (ignored by the reference).  Request/response schemas keep the
reference fields (``GenerationRequest`` / ``GenerationResponse``, ``server.py:25-37``) and add
OpenAI-style ``choices``.

Concurrency model (fixes SURVEY App. C #1): the engine runs on its own thread, looping
``engine.step()`` while there is work; HTTP handlers enqueue a request and await an
``asyncio.Future`` (or an async token queue for streaming) that the engine thread resolves
via ``loop.call_soon_threadsafe`` — no polling, the event loop is never blocked by model
compute, and unfinished sequences stay scheduled until they finish.
"""

from __future__ import annotations

import asyncio
import json
import logging
import os
import threading
import time
import uuid
from typing import Any, Dict, List, Optional, Union

from pydantic import BaseModel, Field

log = logging.getLogger("llmctl.serve.server")


class GenerationRequest(BaseModel):
    prompt: Union[str, List[int]]
    max_tokens: int = 100
    temperature: float = 1.0
    top_p: float = 1.0
    top_k: int = -1
    stream: bool = False
    stop: Optional[Union[str, List[str]]] = None
    ignore_eos: bool = False
    model: Optional[str] = None
    # the extended sampler: OpenAI's presence / frequency penalties (over the generated tokens),
    # the HF-style repetition penalty (over prompt and generated tokens), per-token logprobs with
    # the ``logprobs`` most likely alternatives
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
    logprobs: Optional[int] = None
    # name of a loaded LoRA adapter (``InferenceEngine.load_lora``); a ``model`` value that equals a
    # loaded adapter's name selects it too, any other ``model`` value is served by the base
    lora: Optional[str] = None
    # guided decoding (at most one): the completion is a full match of ``guided_regex``, one of
    # ``guided_choice``, or an instance of the ``guided_json`` schema (a subset, see the README);
    # OpenAI's ``response_format`` of type ``json_schema`` maps to ``guided_json``, ``text`` to nothing
    guided_regex: Optional[str] = None
    guided_choice: Optional[List[str]] = None
    guided_json: Optional[Union[Dict[str, Any], str]] = None
    response_format: Optional[Dict[str, Any]] = None
    # prompt scoring, in the prefill pass.  OpenAI form: ``echo`` with ``logprobs = k`` returns the
    # prompt's text and tokens in front of the completion's, each prompt token with its logprob and
    # the k most likely alternatives.  vLLM form: ``prompt_logprobs = k`` adds
    # ``choices[0].prompt_logprobs``.  Only with either may ``max_tokens`` be 0 (score, generate
    # nothing).  ``echo`` without ``logprobs`` only prepends the prompt text.  Not with ``stream``.
    echo: bool = False
    prompt_logprobs: Optional[int] = None


def prompt_logprobs_of(req: GenerationRequest) -> Optional[int]:
    """The ``SamplingParams.prompt_logprobs`` a request asks for: its ``prompt_logprobs`` field, or
    ``logprobs`` under ``echo`` (the larger of the two when both are given); None: no scoring."""
    ks = [k for k in (req.prompt_logprobs, req.logprobs if req.echo else None) if k is not None]
    return max(ks) if ks else None


def guide_fields(req: GenerationRequest) -> Dict[str, Any]:
    """The request's guide as ``SamplingParams`` fields (empty: unguided).  ``ValueError`` for more
    than one guide, a guide with ``ignore_eos`` and a ``response_format`` that cannot be served."""
    from .guided import response_format_to_guide

    given = {n: getattr(req, n) for n in ("guided_regex", "guided_choice", "guided_json") if getattr(req, n) is not None}
    rf = response_format_to_guide(req.response_format)
    if rf is not None:
        if given:
            raise ValueError(f"at most one guide per request, got response_format and {', '.join(given)}")
        given = {"guided_json": rf[1]}
    if len(given) > 1:
        raise ValueError(f"at most one guide per request, got {', '.join(given)}")
    if given and req.ignore_eos:
        raise ValueError(f"ignore_eos cannot be combined with {next(iter(given))} (a guided request ends with EOS)")
    return given


def validate_request(req: GenerationRequest, tokenizer=None, vocab_size: Optional[int] = None,
                     table_words: Optional[int] = None) -> None:
    """Range checks of the extended sampling fields and the guide (``ValueError``: answered with
    400).  With a ``tokenizer`` the guide is compiled here (and cached for ``add_request``), so an
    unsupported construct or a guide over the limits is refused before a stream starts."""
    g = guide_fields(req)
    if g and tokenizer is not None:
        from .guided import compile_guide

        (name, spec), = g.items()
        compile_guide(name[len("guided_"):], spec, tokenizer, vocab_size, table_words=table_words)
    for name in ("presence_penalty", "frequency_penalty"):
        v = getattr(req, name)
        if not -2.0 <= v <= 2.0:
            raise ValueError(f"{name} must be in [-2, 2], got {v}")
    if not 0.0 < req.repetition_penalty <= 10.0:
        raise ValueError(f"repetition_penalty must be in (0, 10], got {req.repetition_penalty}")
    if req.logprobs is not None and not 0 <= req.logprobs <= 8:
        raise ValueError(f"logprobs must be in 0..8, got {req.logprobs}")
    if req.prompt_logprobs is not None and not 0 <= req.prompt_logprobs <= 8:
        raise ValueError(f"prompt_logprobs must be in 0..8, got {req.prompt_logprobs}")
    if req.stream and (req.echo or req.prompt_logprobs is not None):
        raise ValueError(f"{'echo' if req.echo else 'prompt_logprobs'} is not supported with stream=true")


class GenerationResponse(BaseModel):
    id: str
    text: str
    finish_reason: str
    usage: Dict[str, int]
    object: str = "text_completion"
    created: int = 0
    model: str = ""
    choices: List[Dict[str, Any]] = Field(default_factory=list)
    timing: Dict[str, float] = Field(default_factory=dict)


class InferenceServer:
    def __init__(self, model_path: str, host: str = "0.0.0.0", port: int = 8080, max_batch_size: int = 8,
                 max_batch_tokens: int = 8192, max_concurrent: int = 128, scheduler: str = "dynamic",
                 device: str = "auto", kv_cache_fraction: float = 0.85, block_size: int = 16, use_graphs: bool = True,
                 tensor_parallel: int = 1, engine=None, kv_cache_dtype: str = "auto", weight_dtype: str = "auto",
                 loras: Optional[Dict[str, str]] = None, max_loras: int = 0, max_lora_rank: int = 16,
                 guide_table_words: int = 1 << 18):
        from fastapi import FastAPI, HTTPException
        from fastapi.middleware.cors import CORSMiddleware
        from fastapi.responses import PlainTextResponse, StreamingResponse

        self.model_path, self.host, self.port = model_path, host, port
        self.max_concurrent = max_concurrent
        self.engine_kwargs = dict(model_path=model_path, device=device, max_batch_size=max_batch_size,
                                  max_batch_tokens=max_batch_tokens, kv_cache_fraction=kv_cache_fraction,
                                  block_size=block_size, scheduler=scheduler, use_graphs=use_graphs,
                                  kv_cache_dtype=kv_cache_dtype, weight_dtype=weight_dtype,
                                  max_loras=max(max_loras, len(loras or {})), max_lora_rank=max_lora_rank,
                                  guide_table_words=guide_table_words)
        self.loras = dict(loras or {})  # adapter name -> directory, loaded when the engine starts
        if tensor_parallel != 1 and engine is None:
            raise ValueError("TP serving runs one engine per rank under torchrun: use llmctl.serve.tp "
                             "(`llmctl serve start --tensor-parallel N` launches it)")
        self.engine = engine
        self.active_requests: Dict[str, Any] = {}
        self._lock = threading.Lock()
        self._wake = threading.Event()
        self._stop = False
        self._thread: Optional[threading.Thread] = None
        self.loop: Optional[asyncio.AbstractEventLoop] = None
        from llmctl.metrics.observability import ObservabilityManager

        self.obs = ObservabilityManager(enable_prometheus=True, prometheus_port=0, collection_interval=5.0)
        from llmctl.metrics.health import HealthManager

        self.health = HealthManager(check_interval=30.0)

        app = FastAPI(title="llmctl inference server", version="0.2.0")
        app.add_middleware(CORSMiddleware, allow_origins=["*"], allow_credentials=True, allow_methods=["*"],
                           allow_headers=["*"])
        self.app = app

        @app.on_event("startup")
        async def _startup():
            self.loop = asyncio.get_running_loop()
            self.start_engine()

        @app.on_event("shutdown")
        async def _shutdown():
            self.stop_engine()
            if getattr(self, "_own_engine", False) and self.engine is not None:
                self.engine.close()
                self.engine = None

        @app.post("/v1/completions")
        async def completions(req: GenerationRequest):
            if len(self.active_requests) >= self.max_concurrent:
                raise HTTPException(status_code=503, detail="Server at capacity")
            try:
                e = self.engine
                if e is not None:
                    validate_request(req, e.tokenizer, e._sampler_vocab(), e.guide_table_words)
                else:
                    validate_request(req)
                self._lora_name(req)  # an unknown adapter is refused before a stream starts
                if e is not None and e.tp > 1 and prompt_logprobs_of(req) is not None:
                    name = "prompt_logprobs" if req.prompt_logprobs is not None else "echo with logprobs (prompt_logprobs)"
                    raise ValueError(f"{name} not supported with tensor parallelism > 1 (TP = {e.tp})")
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            if req.stream:
                return StreamingResponse(self._stream(req), media_type="text/event-stream")
            try:
                return await self.handle_generation_request(req)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))

        @app.get("/v1/models")
        async def models():
            now = int(time.time())
            data = [{"id": self.model_name, "object": "model", "created": now, "owned_by": "llmctl"}]
            for name in (self.engine.loras if self.engine is not None else []):  # adapters: children of the base
                data.append({"id": name, "object": "model", "created": now, "owned_by": "llmctl",
                             "parent": self.model_name})
            return {"object": "list", "data": data}

        @app.get("/health")
        async def health():
            e = self.engine
            sched = e.scheduler if e else None
            return {"status": "healthy" if e is not None else "loading",
                    "active_requests": len(self.active_requests),
                    "pending_requests": sched.num_waiting if sched else 0,
                    "running_sequences": sched.num_running if sched else 0,
                    "kv_cache_usage": round(e.kv.usage(), 4) if e else 0.0,
                    "device": str(e.device) if e else None}

        @app.get("/metrics")
        async def metrics():
            return PlainTextResponse(self.obs.prometheus_exporter.render().decode())

    # ------------------------------------------------------------------ engine thread
    @property
    def model_name(self) -> str:
        return self.engine.cfg.name if self.engine is not None else str(self.model_path)

    def start_engine(self):
        if self.engine is None:
            from .engine import InferenceEngine

            self.engine = InferenceEngine(**self.engine_kwargs)
            self._own_engine = True  # closed by this server's shutdown (a passed-in engine is the caller's)
            for name, path in self.loras.items():
                self.engine.load_lora(name, path)
        if self._thread is None:
            self._stop = False
            self._thread = threading.Thread(target=self._engine_loop, name="llmctl-engine", daemon=True)
            self._thread.start()

    def stop_engine(self):
        self._stop = True
        self._wake.set()
        if self._thread:
            self._thread.join(timeout=10)
            self._thread = None

    def _engine_loop(self):
        e = self.engine
        while not self._stop:
            with self._lock:
                busy = e.scheduler.has_work()
            if not busy:
                self._wake.wait(timeout=0.05)
                self._wake.clear()
                continue
            try:
                with self._lock:
                    e.step()
            except Exception as ex:  # fail all in-flight requests loudly instead of hanging
                with self._lock:
                    for seq in list(e.scheduler.running) + list(e.scheduler.waiting):
                        e.scheduler.finish(seq, f"error: {ex}") if seq.status == "running" else None
                        seq.status = "finished"
                        seq.finish_reason = f"error: {ex}"
                        if seq.on_finish:
                            seq.on_finish(seq)
                    e.scheduler.waiting.clear()
                from .control import PeerLostError

                if isinstance(ex, PeerLostError):
                    # a TP rank is gone: the group cannot serve again.  Give the failed requests a
                    # moment to be answered, then leave non-zero so the launcher tears down the job
                    log.error("TP peer lost, server exiting: %s", ex)
                    threading.Timer(0.5, os._exit, (70,)).start()
                    return

    # ------------------------------------------------------------------ request handling
    def _lora_name(self, req: GenerationRequest) -> Optional[str]:
        """The adapter a request selects: its ``lora`` field (unknown: ``ValueError``), else a
        ``model`` value that names a loaded adapter, else None (the base model)."""
        loaded = self.engine.loras if self.engine is not None else []
        if req.lora is not None:
            if req.lora not in loaded:
                raise ValueError(f"unknown LoRA adapter {req.lora!r} (loaded: {list(loaded) or 'none'})")
            return req.lora
        return req.model if req.model is not None and req.model in loaded else None

    def _make_params(self, req: GenerationRequest):
        from .scheduler import SamplingParams

        stop = [req.stop] if isinstance(req.stop, str) else (req.stop or [])
        plp = prompt_logprobs_of(req)  # only a scoring request may generate nothing
        return SamplingParams(max_tokens=max(0 if plp is not None else 1, req.max_tokens), prompt_logprobs=plp,
                              temperature=req.temperature, top_p=req.top_p,
                              top_k=req.top_k, stop=stop, ignore_eos=req.ignore_eos,
                              repetition_penalty=req.repetition_penalty, presence_penalty=req.presence_penalty,
                              frequency_penalty=req.frequency_penalty, logprobs=req.logprobs,
                              lora=self._lora_name(req), **guide_fields(req))

    def _logprobs_payload(self, seq) -> Dict[str, Any]:
        """``choices[0]["logprobs"]`` in the OpenAI completions shape: four lists, one entry per
        generated token (``top_logprobs``: token text -> logprob of the most likely alternatives)."""
        dec = self.engine.tokenizer.decode
        return {"tokens": [dec([t]) for t in seq.output_ids], "token_ids": list(seq.output_ids),
                "token_logprobs": list(seq.output_logprobs),
                "top_logprobs": [{dec([t]): v for t, v in top} for top in seq.output_top_logprobs]}

    def _echo_logprobs_payload(self, seq) -> Dict[str, Any]:
        """``choices[0]["logprobs"]`` of an ``echo`` request: the prompt tokens, then the generated
        ones.  The first prompt token has no logprob (``null``); ``text_offset`` is every token's
        offset in ``choices[0].text``."""
        dec = self.engine.tokenizer.decode
        k = seq.params.logprobs
        ids = list(seq.prompt_ids) + list(seq.output_ids)
        toks = [dec([t]) for t in ids]
        tops = [None if top is None else {dec([t]): v for t, v in top[:k]} for top in seq.prompt_top_logprobs]
        offs, at = [], 0
        for t in toks:
            offs.append(at)
            at += len(t)
        return {"tokens": toks, "token_ids": ids, "token_logprobs": list(seq.prompt_logprobs) + list(seq.output_logprobs),
                "top_logprobs": tops + [{dec([t]): v for t, v in top} for top in seq.output_top_logprobs],
                "text_offset": offs}

    def _prompt_logprobs_payload(self, seq, k: int) -> List[Optional[Dict[str, Any]]]:
        """``choices[0]["prompt_logprobs"]`` (the vLLM shape): per prompt position ``null`` (the
        first) or token id (a string) -> ``{logprob, rank, decoded_token}`` for the prompt token and
        the ``k`` most likely alternatives."""
        dec = self.engine.tokenizer.decode
        out: List[Optional[Dict[str, Any]]] = []
        for tok, lp, rank, top in zip(seq.prompt_ids, seq.prompt_logprobs, seq.prompt_ranks, seq.prompt_top_logprobs):
            if lp is None:
                out.append(None)
                continue
            ent = {str(t): {"logprob": v, "rank": i + 1, "decoded_token": dec([t])} for i, (t, v) in enumerate(top[:k])}
            ent[str(tok)] = {"logprob": lp, "rank": rank, "decoded_token": dec([tok])}
            out.append(ent)
        return out

    def _encode(self, prompt) -> List[int]:
        if isinstance(prompt, list):
            return [int(t) for t in prompt]
        return self.engine.tokenizer.encode(prompt)

    async def handle_generation_request(self, req: GenerationRequest) -> GenerationResponse:
        loop = asyncio.get_running_loop()
        fut: asyncio.Future = loop.create_future()
        rid = f"cmpl-{uuid.uuid4().hex[:16]}"
        t0 = time.time()
        ids = self._encode(req.prompt)

        def on_finish(seq):
            loop.call_soon_threadsafe(lambda: fut.done() or fut.set_result(seq))

        with self._lock:
            self.active_requests[rid] = True
            try:
                seq = self.engine.add_request(ids, self._make_params(req), rid, on_finish=on_finish)
            except ValueError:
                self.active_requests.pop(rid, None)
                raise
        self._wake.set()
        try:
            seq = await fut
        finally:
            self.active_requests.pop(rid, None)
        text = self.engine.tokenizer.decode(seq.output_ids)
        lat = time.time() - t0
        ttft = (seq.first_token_time - seq.arrival_time) if seq.first_token_time else lat
        n = len(seq.output_ids)
        tpot = (seq.finish_time - seq.first_token_time) / max(n - 1, 1) if seq.first_token_time and seq.finish_time else 0.0
        self.obs.record_inference_request(lat, ttft=ttft, tpot=tpot)
        self.health.record_inference_request(lat, success=not str(seq.finish_reason).startswith("error"))
        usage = {"prompt_tokens": len(ids), "completion_tokens": n, "total_tokens": len(ids) + n}
        if req.echo:  # the prompt's text in front of the completion's
            text = self.engine.tokenizer.decode(list(seq.prompt_ids)) + text
        choice = {"index": 0, "text": text, "finish_reason": seq.finish_reason}
        if req.logprobs is not None:
            choice["logprobs"] = self._echo_logprobs_payload(seq) if req.echo else self._logprobs_payload(seq)
        if req.prompt_logprobs is not None:
            choice["prompt_logprobs"] = self._prompt_logprobs_payload(seq, req.prompt_logprobs)
        return GenerationResponse(id=rid, text=text, finish_reason=seq.finish_reason or "stop", usage=usage,
                                  created=int(t0), model=self.model_name,
                                  choices=[choice],
                                  timing={"latency_s": lat, "ttft_s": ttft, "tpot_s": tpot})

    async def _stream(self, req: GenerationRequest):
        loop = asyncio.get_running_loop()
        q: asyncio.Queue = asyncio.Queue()
        rid = f"cmpl-{uuid.uuid4().hex[:16]}"

        def on_token(seq, tok):
            lp = seq.output_logprobs[-1] if seq.params.logprobs is not None else None
            loop.call_soon_threadsafe(q.put_nowait, ("tok", (tok, lp)))

        def on_finish(seq):
            loop.call_soon_threadsafe(q.put_nowait, ("end", seq.finish_reason))

        with self._lock:
            self.active_requests[rid] = True
            self.engine.add_request(self._encode(req.prompt), self._make_params(req), rid, on_token=on_token,
                                    on_finish=on_finish)
        self._wake.set()
        try:
            while True:
                kind, val = await q.get()
                if kind == "tok":
                    val, lp = val
                    payload = {"id": rid, "object": "text_completion", "model": self.model_name,
                               "choices": [{"index": 0, "text": self.engine.tokenizer.decode([val]), "token": val,
                                            "finish_reason": None}]}
                    if lp is not None:
                        payload["choices"][0]["logprob"] = lp
                    yield f"data: {json.dumps(payload)}\n\n"
                else:
                    payload = {"id": rid, "choices": [{"index": 0, "text": "", "finish_reason": val}]}
                    yield f"data: {json.dumps(payload)}\n\n"
                    yield "data: [DONE]\n\n"
                    break
        finally:
            self.active_requests.pop(rid, None)

    # ------------------------------------------------------------------ run
    def run(self):
        import uvicorn

        uvicorn.run(self.app, host=self.host, port=self.port, log_level="info")

    async def start_server(self):
        import uvicorn

        config = uvicorn.Config(self.app, host=self.host, port=self.port, log_level="info")
        await uvicorn.Server(config).serve()


def create_inference_server(model_path: str, **kwargs) -> InferenceServer:
    return InferenceServer(model_path, **kwargs)
