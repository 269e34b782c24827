"""fp8 / int4 decode weights at 17-64 token rows (``csrc/decode_gemm_mid.hip``) behind the decode ops
and the engine's ``weight_max_rows``, against fp64 products on the dequantised weight."""

import pytest
import torch

from llmctl.config import knobs
from llmctl.ops import ref
from llmctl.plugins.quantizers import quantize_fp8, quantize_int4_g128
from llmctl.testing.decode_wq import grid_engine, run_forced
from llmctl.testing.numerics import int4_grid, row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ("int4", "fp8")


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def _wq(kind, N, K, seed):
    """(qweight, scale, fp64 image of the dequantised weight) of a random bf16 weight."""
    w = _bf(N, K, scale=0.05, seed=seed)
    if kind == "int4":
        qd = quantize_int4_g128(w)
        return qd["qweight"], qd["scale"], ref.dequant_int4_g128(qd["qweight"], qd["scale"]).double()
    qd = quantize_fp8(w)
    q, s = qd["qweight"].contiguous(), qd["scale"].float().contiguous()
    return q, s, q.double() * s.double()[:, None]


# second token tile with one live row; three tiles, ragged; exactly three; four full + bias; three
# workgroups, the last half full; the smallest N on the 8-wave int4 kernel; that kernel at three
# token tiles with a half-full last workgroup
SHAPES = [(17, 64, 128, False), (33, 256, 1152, False), (48, 128, 2176, False), (64, 192, 384, True),
          (40, 320, 640, False), (64, 8192, 128, False), (48, 8256, 384, True)]


@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("M,N,K,bias", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_linear_wq_mid(native_lib, kind, M, N, K, bias, splits):
    """Plain projection, automatic and forced split-K (3 slices leave a shorter last one at K = 1152
    and 640; a K of one or two chunks caps the count)."""
    x = _bf(M, K, seed=401)
    q, s, wd = _wq(kind, N, K, 402)
    b = _bf(N, seed=403) if bias else None
    op = native_lib.decode_linear_int4 if kind == "int4" else native_lib.decode_linear_fp8
    with knobs.override(decode_mid_splits=splits):
        y = op(x, q, s, b)
        parts = native_lib.decode_linear_partials(x, q, s)
    if splits:
        chunks = -(-K // 256)
        per = -(-chunks // min(splits, chunks))
        assert parts.shape == (-(-chunks // per), M, N), parts.shape
    yr = x.double() @ wd.t() + (b.double() if bias else 0.0)
    err = row_err(y, yr)
    print(f"decode_linear_{kind} {M}x{N}x{K} splits {splits} -> {parts.shape[0]} row_err {err:.3e}")
    assert y.shape == (M, N) and y.dtype == torch.bfloat16 and err < 1e-2, err


def test_decode_linear_int4_mid_lossless_grid(native_lib):
    """Exponents that differ per row and per group: a scale or group sum of x taken from the wrong
    row, group or token tile is off by >= 2x."""
    M, N, K = 40, 192, 2176
    wf, e = int4_grid(N, K, seed=411)
    assert (e[:, 1:] != e[:, :-1]).any() and (e[1:] != e[:-1]).any()
    qd = quantize_int4_g128(wf.to(DEV))
    assert torch.equal(ref.dequant_int4_g128(qd["qweight"], qd["scale"]), wf.to(DEV))
    x = _bf(M, K, seed=412)
    err = row_err(native_lib.decode_linear_int4(x, qd["qweight"], qd["scale"], None), x.double() @ wf.to(DEV).double().t())
    print(f"lossless grid M={M} row_err {err:.3e}")
    assert err < 1e-2, err


@pytest.mark.parametrize("M", [17, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_decode_fused_ops_wq_mid(native_lib, kind, M):
    """QKV + RoPE + cache write (one row without a slot), up + SwiGLU, projection + residual + RMSNorm."""
    K = 384
    nq, nkv, D, bs, nb = 4, 2, 64, 16, 8
    x = _bf(M, K, seed=421)
    q4, sc, wd = _wq(kind, (nq + 2 * nkv) * D, K, 422)
    cos, sin = ref.rope_tables(256, D, base=10000.0, device=DEV)
    gen = torch.Generator().manual_seed(426)
    pos = torch.randint(0, 256, (M,), generator=gen, dtype=torch.int32).to(DEV)
    slots = torch.randperm(nb * bs, generator=gen)[:M].to(DEV)
    slots[M - 1] = -1
    kc, vc = _bf(nb, bs, nkv, D, seed=427), _bf(nb, bs, nkv, D, seed=428)
    kc0, vc0 = kc.clone(), vc.clone()
    q = native_lib.decode_qkv_rope_cache(x, q4, None, cos, sin, nq, nkv, pos, kc, vc, slots, sc)
    qo, ko, vo = ref.rope_qkv_fwd((x.double() @ wd.t()).float(), cos, sin, nq, nkv, 256, pos)
    kflat, vflat = kc.view(nb * bs, nkv, D), vc.view(nb * bs, nkv, D)
    live = slots >= 0
    errs = (row_err(q.reshape(M, -1), qo.float().reshape(M, -1)),
            row_err(kflat[slots[live]].reshape(M - 1, -1), ko.float()[live].reshape(M - 1, -1)),
            row_err(vflat[slots[live]].reshape(M - 1, -1), vo.float()[live].reshape(M - 1, -1)))
    print(f"{kind} qkv+rope+cache M={M} row_err {errs}")
    assert max(errs) < 2e-2, errs
    untouched = torch.ones(nb * bs, dtype=torch.bool, device=DEV)
    untouched[slots[live]] = False
    assert torch.equal(kflat[untouched], kc0.view(nb * bs, nkv, D)[untouched])
    assert torch.equal(vflat[untouched], vc0.view(nb * bs, nkv, D)[untouched])
    F = 256
    q4, sc, wd = _wq(kind, 2 * F, K, 423)
    act = native_lib.decode_up_swiglu(x, q4, None, sc)
    gu = x.double() @ wd.t()
    err = row_err(act, torch.nn.functional.silu(gu[:, :F]) * gu[:, F:])
    print(f"{kind} up+swiglu M={M} row_err {err:.3e}")
    assert act.shape == (M, F) and err < 2e-2, err
    N = 256
    q4, sc, wd = _wq(kind, N, K, 424)
    res = _bf(M, N, seed=425)
    nw = (1.0 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16)
    y, res_out = native_lib.decode_linear_add_rmsnorm(x, q4, None, res, nw, 1e-5, sc)
    s_ = x.double() @ wd.t() + res.double()
    errs = (row_err(res_out, s_), row_err(y, s_ * torch.rsqrt(s_.pow(2).mean(-1, keepdim=True) + 1e-5) * nw.double()))
    print(f"{kind} proj+residual+rmsnorm M={M} row_err {errs}")
    assert errs[0] < 1.5e-2 and errs[1] < 2e-2, errs


@pytest.mark.parametrize("kind", KINDS)
def test_engine_weight_max_rows(native_lib, kind):
    """20 decode rows with ``weight_max_rows=32``: the layers stream the quantised copies (captured
    graphs); int4 on the lossless grid follows the bf16 engine's logits on the same token stream."""
    prompts = [[(11 * i + r) % 400 + 1 for i in range(5 + r)] for r in range(20)]
    eng = grid_engine(max_batch_size=32, num_kv_blocks=256, use_graphs=True, weight_dtype=kind, weight_max_rows=32)
    layer = eng.model.layers[0]
    w, s = eng._dw(0, layer, "wqkv", 20)
    assert s is not None and w.dtype == (torch.uint8 if kind == "int4" else torch.float8_e4m3fn)
    w, s = eng._dw(0, layer, "wqkv", 33)
    assert s is None and w.dtype == torch.bfloat16
    if kind == "int4":
        ref_eng = grid_engine(max_batch_size=32, num_kv_blocks=256, use_graphs=True)
        toks, lg_ref = run_forced(ref_eng, prompts, 6)
        ref_eng.release_graphs()
        toks4, lg = run_forced(eng, prompts, 6, forced=toks)
        assert toks4 == toks
        err = row_err(lg[:, 1:].reshape(-1, lg.shape[-1]), lg_ref[:, 1:].reshape(-1, lg_ref.shape[-1]))
        print(f"int4 engine decode logits at 20 rows row_err {err:.3e}")
        assert err < 3e-2, err
    else:
        run_forced(eng, prompts, 6)
    assert eng._fused_decode(20) and eng.stats["graph_replays"] > 0
    eng.release_graphs()
    eng.close()
