"""Group-128 int4 decode weights (W4A16) on the GPU: ``decode_gemm_w4_kernel`` behind
``decode_linear_int4`` and the fused decode ops, against the fp32 oracle on the dequantised weight
(``ops.ref.dequant_int4_g128``), and the serving engine's ``weight_dtype="int4"``."""

import pytest
import torch

from llmctl.ops import ref
from llmctl.plugins.quantizers import quantize_int4_g128
from llmctl.testing.numerics import int4_grid, row_err as _row_err, snap_int4_grid

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def _w4(N, K, seed):
    """(qweight, scale, fp32 image of the dequantised weight) of a random bf16 weight."""
    qd = quantize_int4_g128(_bf(N, K, scale=0.05, seed=seed))
    return qd["qweight"], qd["scale"], ref.dequant_int4_g128(qd["qweight"], qd["scale"])


@pytest.mark.parametrize("M,N,K,bias", [(1, 64, 128, False), (16, 64, 1024, False), (3, 256, 1152, False),
                                        (7, 128, 2176, False), (16, 1024, 384, True), (5, 16384, 1152, True)])
def test_decode_linear_int4(native_lib, M, N, K, bias):
    """int4 decode projection == fp32 ``x @ dequant(W)^T (+ b)``: one K block, exactly one chunk, a
    chunk + a one-block tail, two chunks + a tail, a short single chunk with bias, and a wide
    projection (>= 16384 out features: two 16-row tiles per wave) with a tail chunk."""
    x = _bf(M, K, seed=301)
    w4, sc, wd = _w4(N, K, 302)
    assert w4.shape == (N, K // 2) and sc.shape == (N, K // 128)
    b = _bf(N, seed=303) if bias else None
    y = native_lib.decode_linear_int4(x, w4, sc, b)
    yr = x.float() @ wd.t() + (b.float() if bias else 0.0)
    err = _row_err(y, yr)
    print(f"decode_linear_int4 {M}x{N}x{K} row_err {err:.3e}")
    assert y.shape == (M, N) and y.dtype == torch.bfloat16 and err < 1e-2, err


def test_decode_linear_int4_lossless_grid(native_lib):
    """Weights int4 holds exactly, with a power-of-two step that differs per row and per group (a
    scale taken from another row or group is off by a factor >= 2): the int4 result and the bf16
    decode path on the same weights are both within 1e-2 of the fp32 product."""
    M, N, K = 5, 192, 2176
    wf, e = int4_grid(N, K, seed=311)
    assert (e[:, 1:] != e[:, :-1]).any() and (e[1:] != e[:-1]).any()
    wf = wf.to(DEV)
    qd = quantize_int4_g128(wf)
    assert torch.equal(ref.dequant_int4_g128(qd["qweight"], qd["scale"]), wf)
    x = _bf(M, K, seed=312)
    yr = x.float() @ wf.t()
    y4 = native_lib.decode_linear_int4(x, qd["qweight"], qd["scale"], None)
    yb = native_lib.skinny_linear_cfg(x, wf.to(torch.bfloat16), None, 25)
    errs = (_row_err(y4, yr), _row_err(yb, yr))
    print(f"lossless grid row_err int4 {errs[0]:.3e} bf16 {errs[1]:.3e}")
    assert max(errs) < 1e-2, errs


@pytest.mark.parametrize("M", [16, 5])
def test_decode_fused_ops_int4_weights(native_lib, M):
    """QKV + RoPE + cache write, up + SwiGLU and row projection + residual + RMSNorm with int4
    weights against the fp32 oracles on the dequantised weight."""
    K = 384
    nq, nkv, D, bs, nb = 4, 2, 64, 16, 4
    x = _bf(M, K, seed=321)
    # QKV: the last token row has no cache slot
    w4, sc, wd = _w4((nq + 2 * nkv) * D, K, 322)
    cos, sin = ref.rope_tables(256, D, base=10000.0, device=DEV)
    gen = torch.Generator().manual_seed(326)
    pos = torch.randint(0, 256, (M,), generator=gen, dtype=torch.int32).to(DEV)
    slots = torch.randperm(nb * bs, generator=gen)[:M].to(DEV)
    slots[M - 1] = -1
    kc = _bf(nb, bs, nkv, D, seed=327)
    vc = _bf(nb, bs, nkv, D, seed=328)
    kc0, vc0 = kc.clone(), vc.clone()
    q = native_lib.decode_qkv_rope_cache(x, w4, None, cos, sin, nq, nkv, pos, kc, vc, slots, sc)
    qo, ko, vo = ref.rope_qkv_fwd(x.float() @ wd.t(), cos, sin, nq, nkv, 256, pos)
    kflat, vflat = kc.view(nb * bs, nkv, D), vc.view(nb * bs, nkv, D)
    live = slots >= 0
    errs = (_row_err(q.reshape(M, -1), qo.float().reshape(M, -1)),
            _row_err(kflat[slots[live]].reshape(M - 1, -1), ko.float()[live].reshape(M - 1, -1)),
            _row_err(vflat[slots[live]].reshape(M - 1, -1), vo.float()[live].reshape(M - 1, -1)))
    print(f"int4 qkv+rope+cache M={M} row_err {errs}")
    assert max(errs) < 2e-2, errs
    untouched = torch.ones(nb * bs, dtype=torch.bool, device=DEV)
    untouched[slots[live]] = False
    assert torch.equal(kflat[untouched], kc0.view(nb * bs, nkv, D)[untouched])
    assert torch.equal(vflat[untouched], vc0.view(nb * bs, nkv, D)[untouched])
    # up + SwiGLU
    F = 256
    w4, sc, wd = _w4(2 * F, K, 323)
    act = native_lib.decode_up_swiglu(x, w4, None, sc)
    gu = x.float() @ wd.t()
    err = _row_err(act, torch.nn.functional.silu(gu[:, :F]) * gu[:, F:])
    print(f"int4 up+swiglu M={M} row_err {err:.3e}")
    assert act.shape == (M, F) and err < 2e-2, err
    # row projection + residual + RMSNorm
    N = 256
    w4, sc, wd = _w4(N, K, 324)
    res = _bf(M, N, seed=325)
    nw = (1.0 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16)
    y, res_out = native_lib.decode_linear_add_rmsnorm(x, w4, None, res, nw, 1e-5, sc)
    s_ = x.float() @ wd.t() + res.float()
    errs = (_row_err(res_out, s_), _row_err(y, s_ * torch.rsqrt(s_.pow(2).mean(-1, keepdim=True) + 1e-5) * nw.float()))
    print(f"int4 o-proj+residual+rmsnorm M={M} row_err {errs}")
    assert errs[0] < 1.5e-2 and errs[1] < 2e-2, errs


# ---------------------------------------------------------------------------------------- engine
_GRID_MODEL = {}


def _grid_engine(**kw):
    """The tiny model with every projection the int4 path can take (and the LM head) snapped onto
    the lossless int4 grid, so int4 and bf16 decode stream the same weight values."""
    from llmctl.models import build_model, get_model_config
    from llmctl.serve.engine import InferenceEngine

    class GridEngine(InferenceEngine):
        def _load(self, model_path, dtype, seed):
            if "m" not in _GRID_MODEL:
                cfg = get_model_config("tiny")
                model = build_model(cfg, device=self.device, dtype=dtype, seed=seed)
                with torch.no_grad():
                    ws = [getattr(layer, n) for layer in model.layers for n in self._W8_NAMES] + [model.head_weight()]
                    for w in ws:
                        if w.dim() == 2 and w.shape[0] % 64 == 0 and w.shape[1] % 128 == 0:
                            w.copy_(snap_int4_grid(w))
                _GRID_MODEL["m"] = (model, cfg)
            model, cfg = _GRID_MODEL["m"]
            return model, cfg, None

    return GridEngine("tiny", device="cuda", block_size=16, max_model_len=256, seed=0, use_graphs=True, **kw)


def _run_forced(eng, prompts, max_tokens, forced=None):
    """Greedy (or teacher-forced) generation recording every step's logits per sequence."""
    from llmctl.serve.scheduler import SamplingParams

    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, temperature=0.0, ignore_eos=True)) for p in prompts]
    idx = {s.seq_id: i for i, s in enumerate(seqs)}
    rec = {}
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


def test_engine_int4_decode_weights(native_lib):
    """weight_dtype="int4" on a model whose eligible weights int4 holds exactly: on the bf16
    engine's token stream the decode logits follow the bf16 weights' (fused path, captured graphs)."""
    prompts = [[(7 * i + 3 * r) % 500 + 1 for i in range(6 + 5 * r)] for r in range(3)]
    ref_eng = _grid_engine(max_batch_size=4, num_kv_blocks=64)
    assert ref_eng.weight_dtype == "auto" and ref_eng._w4 is None
    toks, lg_ref = _run_forced(ref_eng, prompts, 8)
    ref_eng.release_graphs()
    eng = _grid_engine(max_batch_size=4, num_kv_blocks=64, weight_dtype="int4")
    assert eng.weight_dtype == "int4" and eng._w8 is None
    for d in eng._w4:
        assert {"wqkv", "wo", "w_up"} <= set(d)
        for name, (q, s) in d.items():
            w = getattr(eng.model.layers[0], name)
            assert q.dtype == torch.uint8 and q.shape == (w.shape[0], w.shape[1] // 2)
            assert s.dtype == torch.float32 and s.shape == (w.shape[0], w.shape[1] // 128)
    assert eng._wq_head is not None
    w, s = eng._dw(0, eng.model.layers[0], "wqkv", 16)
    assert s is not None and w.dtype == torch.uint8
    w, s = eng._dw(0, eng.model.layers[0], "wqkv", 17)
    assert s is None and w.dtype == torch.bfloat16
    toks4, lg4 = _run_forced(eng, prompts, 8, forced=toks)
    assert toks4 == toks
    assert eng._fused_decode() and eng.stats["graph_replays"] > 0
    # step 0 of every sequence is the (bf16) prefill's; the rest are decode steps
    err = _row_err(lg4[:, 1:].reshape(-1, lg4.shape[-1]), lg_ref[:, 1:].reshape(-1, lg_ref.shape[-1]))
    print(f"int4 engine decode logits row_err {err:.3e}")
    assert err < 3e-2, err
    eng.release_graphs()
    eng.close()
    assert eng._w4 is None and eng._wq_head is None


def test_int4_weights_large_batch_uses_bf16(native_lib):
    """More than 16 decode rows (the fused kernels' limit): the decode layers stream the kept bf16
    weights, so the greedy tokens equal the bf16-weight engine's exactly."""
    from llmctl.serve.engine import InferenceEngine
    from llmctl.serve.scheduler import SamplingParams

    prompts = [[(11 * i + r) % 400 + 1 for i in range(5 + r)] for r in range(20)]
    p = SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True)
    outs = {}
    for wd in ("auto", "int4"):
        e = InferenceEngine("tiny", device="cuda", max_batch_size=32, num_kv_blocks=256, block_size=16,
                            max_model_len=256, use_graphs=True, weight_dtype=wd)
        assert (e._w4 is not None) == (wd == "int4")
        outs[wd] = [s.output_ids for s in e.generate(prompts, p)]
        e.release_graphs()
    assert outs["int4"] == outs["auto"]


def test_tp2_serving_int4_weights(native_lib):
    """TP=2 with int4 decode weights: each rank quantises its own shard, groups run along K and the
    shards cut K at multiples of 128, so both ranks hold the TP=1 engine's quantised values and the
    logits differ by the per-rank bf16 rounding of the partial sums only."""
    from llmctl.testing.harness import run_ranks
    from llmctl.testing.workers import serve_forced_gpu

    kw = {"weight_dtype": "int4"}
    w4 = serve_forced_gpu(0, 1, 8, "tiny", None, None, kw)
    assert w4["fused_decode"] and w4["graph_replays"] > 0
    tp = run_ranks(serve_forced_gpu, 2, 8, "tiny", w4["tokens"], None, kw, timeout=300)
    assert tp[0]["graph_replays"] > 0 and tp[0]["fused_decode"]
    lg, lg1 = tp[0]["logits"], w4["logits"]
    err = _row_err(lg.reshape(-1, lg.shape[-1]), lg1.reshape(-1, lg1.shape[-1]))
    print(f"TP=2 int4 vs TP=1 int4 logits row_err {err:.3e}")
    assert err < 3e-2, err
