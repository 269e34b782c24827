"""Per-row LoRA adapters on the GPU: ``lora_delta`` (``csrc/lora_decode.hip``) against the fp64
oracle, and the fused decode projections carrying the delta as one more fp32 slice of their
partials, on bf16, fp8 and int4 base weights."""

import pytest
import torch

from llmctl.ops import ref
from llmctl.plugins.quantizers import quantize_fp8, quantize_int4_g128
from llmctl.testing.numerics import row_err as _row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS = 4
PATTERN = [3, -1, 0, 3, 1, 2, -1, 0]  # slot 3 is the last slot


def _bf(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def _row_err64(got, want):
    """``row_err`` kept in fp64 (the shared helper compares in fp32, the size of the errors here);
    rows whose reference is all zero are skipped."""
    rows = want.abs().amax(1) > 0
    g, w = got.double()[rows], want.double()[rows]
    return ((g - w).abs().amax(1) / w.abs().amax(1)).max().item()


def _idx(M):
    return torch.tensor([PATTERN[i % len(PATTERN)] for i in range(M)], dtype=torch.int32, device=DEV)


def _adapters(N, K, R, seed, std=0.05):
    """4 slots whose adapters differ by a factor 2^slot in magnitude (a wrong slot or stride is off
    by at least 2x): A [S, R, K], B [S, N, R] bf16, scale [S] fp32."""
    mag = torch.exp2(torch.arange(SLOTS, device=DEV, dtype=torch.float32)).view(SLOTS, 1, 1)
    A = (_bf(SLOTS, R, K, scale=std, seed=seed).float() * mag).to(torch.bfloat16)
    B = _bf(SLOTS, N, R, scale=std, seed=seed + 1)
    scale = torch.tensor([2.0, 0.5, 1.0, 1.5], device=DEV)
    return A, B, scale


@pytest.mark.parametrize("M,N,K,R", [(1, 64, 128, 16), (16, 512, 256, 16), (5, 1408, 256, 32), (7, 256, 704, 16),
                                     (33, 256, 1152, 64), (3, 22016, 4096, 16)])
def test_lora_delta(native_lib, M, N, K, R):
    """The kernel against the fp64 oracle, within 4x the error of the same chain done with torch's
    fp32 matmuls on the GPU; rows without an adapter are exactly zero."""
    x = _bf(M, K, seed=401)
    idx = _idx(M)
    A, B, scale = _adapters(N, K, R, 402)
    want = ref.lora_delta(x.double(), idx, A.double(), B.double(), scale.double())
    fp32 = ref.lora_delta(x.float(), idx, A.float(), B.float(), scale)  # torch fp32 GEMMs on the GPU
    assert want.dtype == torch.float64 and fp32.dtype == torch.float32
    got = native_lib.lora_delta(x, idx, A, B, scale)
    assert got.shape == (M, N) and got.dtype == torch.float32
    rows = idx >= 0
    assert bool((want[rows].abs().amax(1) > 0).all())
    err_t, err_k = _row_err64(fp32, want), _row_err64(got, want)
    print(f"lora_delta {M}x{N}x{K} R={R}: kernel row_err {err_k:.3e}, torch fp32 row_err {err_t:.3e}")
    assert err_t > 0
    assert (got[~rows] == 0).all()
    assert err_k <= 4 * err_t, (err_k, err_t)


def test_lora_delta_bad_operands(native_lib):
    x, idx = _bf(3, 128, seed=1), _idx(3)
    A, B, scale = _adapters(64, 128, 16, 2)
    native_lib.lora_delta(x, idx, A, B, scale)
    bad = [
        (_bf(3, 96, seed=1), idx, A[:, :, :96].contiguous(), B, scale),  # K % 64
        (x, idx, A, _bf(SLOTS, 96, 16, seed=4), scale),  # N % 64
        (x, idx, A[:, :8].contiguous(), B[:, :, :8].contiguous(), scale),  # rank 8
        (x, idx.long(), A, B, scale),  # idx dtype
        (x, idx[:2].contiguous(), A, B, scale),  # idx length
        (x, idx, A.float(), B, scale),  # A dtype
        (x.float(), idx, A, B, scale),  # x dtype
        (x, idx, A, B, scale[:3].contiguous()),  # scale length
        (x, idx, A[:, :, :64].contiguous(), B, scale),  # K mismatch
        (x, idx, A, B.transpose(1, 2), scale),  # B layout
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            native_lib.lora_delta(*args)
    w = _bf(64, 128, seed=3)
    with pytest.raises(RuntimeError):  # LoRA tensors without lora_idx
        native_lib.decode_up_swiglu(x, w, None, None, None, A, B, scale)
    with pytest.raises(RuntimeError):  # lora_idx without the tensors
        native_lib.decode_up_swiglu(x, w, None, None, idx, None, None, None)


def _weights(kind, N, K, seed):
    """(weight as the op takes it, scales or None, fp32 image) of a random bf16 weight."""
    w = _bf(N, K, scale=0.05, seed=seed)
    if kind == "bf16":
        return w, None, w.float()
    if kind == "fp8":
        qd = quantize_fp8(w)
        q, s = qd["qweight"].contiguous(), qd["scale"].float().contiguous()
        return q, s, q.float() * s.unsqueeze(1)
    qd = quantize_int4_g128(w)
    return qd["qweight"], qd["scale"], ref.dequant_int4_g128(qd["qweight"], qd["scale"])


@pytest.mark.parametrize("kind", ["bf16", "fp8", "int4"])
@pytest.mark.parametrize("M", [16, 5])
def test_decode_fused_ops_lora(native_lib, M, kind):
    """QKV + RoPE + cache write, up + SwiGLU, row projection + residual + RMSNorm and the plain
    fp8 / int4 projections with per-row adapters: the fp32 ``x W^T + delta`` through the oracle
    epilogues; with every row at -1 the outputs (and caches) equal the calls without ``lora``."""
    K, R = 384, 16
    nq, nkv, D, bs, nb = 4, 2, 64, 16, 4
    x = _bf(M, K, seed=421)
    idx = _idx(M)
    none = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    # QKV: the last token row has no cache slot
    Nq = (nq + 2 * nkv) * D
    w, sc, wd = _weights(kind, Nq, K, 422)
    A, B, ls = _adapters(Nq, K, R, 430)
    cos, sin = ref.rope_tables(256, D, base=10000.0, device=DEV)
    gen = torch.Generator().manual_seed(426)
    pos = torch.randint(0, 256, (M,), generator=gen, dtype=torch.int32).to(DEV)
    slots = torch.randperm(nb * bs, generator=gen)[:M].to(DEV)
    slots[M - 1] = -1
    kc0, vc0 = _bf(nb, bs, nkv, D, seed=427), _bf(nb, bs, nkv, D, seed=428)
    kc, vc = kc0.clone(), vc0.clone()
    q = native_lib.decode_qkv_rope_cache(x, w, None, cos, sin, nq, nkv, pos, kc, vc, slots, sc, idx, A, B, ls)
    delta = ref.lora_delta(x, idx, A, B, ls)
    assert delta[idx >= 0].abs().amax(1).min() > 0.05  # the adapters are visible at the test's bounds
    qo, ko, vo = ref.rope_qkv_fwd(x.float() @ wd.t() + delta, cos, sin, nq, nkv, 256, pos)
    kflat, vflat = kc.view(nb * bs, nkv, D), vc.view(nb * bs, nkv, D)
    live = slots >= 0
    errs = (_row_err(q.reshape(M, -1), qo.float().reshape(M, -1)),
            _row_err(kflat[slots[live]].reshape(M - 1, -1), ko.float()[live].reshape(M - 1, -1)),
            _row_err(vflat[slots[live]].reshape(M - 1, -1), vo.float()[live].reshape(M - 1, -1)))
    print(f"{kind} lora qkv+rope+cache M={M} row_err {errs}")
    assert max(errs) < 2e-2, errs
    untouched = torch.ones(nb * bs, dtype=torch.bool, device=DEV)
    untouched[slots[live]] = False
    assert torch.equal(kflat[untouched], kc0.view(nb * bs, nkv, D)[untouched])
    assert torch.equal(vflat[untouched], vc0.view(nb * bs, nkv, D)[untouched])
    ka, va, kb, vb = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    qa = native_lib.decode_qkv_rope_cache(x, w, None, cos, sin, nq, nkv, pos, ka, va, slots, sc)
    qb = native_lib.decode_qkv_rope_cache(x, w, None, cos, sin, nq, nkv, pos, kb, vb, slots, sc, none, A, B, ls)
    assert torch.equal(qa, qb) and torch.equal(ka, kb) and torch.equal(va, vb)
    assert not torch.equal(ka, kc)
    # up + SwiGLU
    F = 256
    w, sc, wd = _weights(kind, 2 * F, K, 423)
    A, B, ls = _adapters(2 * F, K, R, 432)
    act = native_lib.decode_up_swiglu(x, w, None, sc, idx, A, B, ls)
    gu = x.float() @ wd.t() + ref.lora_delta(x, idx, A, B, ls)
    err = _row_err(act, torch.nn.functional.silu(gu[:, :F]) * gu[:, F:])
    print(f"{kind} lora up+swiglu M={M} row_err {err:.3e}")
    assert act.shape == (M, F) and err < 2e-2, err
    assert torch.equal(native_lib.decode_up_swiglu(x, w, None, sc),
                       native_lib.decode_up_swiglu(x, w, None, sc, none, A, B, ls))
    # row projection + residual + RMSNorm
    N = 256
    w, sc, wd = _weights(kind, N, K, 424)
    A, B, ls = _adapters(N, K, R, 434)
    res = _bf(M, N, seed=425)
    nw = (1.0 + 0.1 * torch.randn(N, device=DEV)).to(torch.bfloat16)
    y, res_out = native_lib.decode_linear_add_rmsnorm(x, w, None, res, nw, 1e-5, sc, idx, A, B, ls)
    delta = ref.lora_delta(x, idx, A, B, ls)
    s_ = x.float() @ wd.t() + delta + res.float()
    errs = (_row_err(res_out, s_), _row_err(y, s_ * torch.rsqrt(s_.pow(2).mean(-1, keepdim=True) + 1e-5) * nw.float()))
    print(f"{kind} lora o-proj+residual+rmsnorm M={M} row_err {errs}")
    assert errs[0] < 1.5e-2 and errs[1] < 2e-2, errs
    ya, ra = native_lib.decode_linear_add_rmsnorm(x, w, None, res, nw, 1e-5, sc)
    yb, rb = native_lib.decode_linear_add_rmsnorm(x, w, None, res, nw, 1e-5, sc, none, A, B, ls)
    assert torch.equal(ya, yb) and torch.equal(ra, rb)
    # the plain quantised projections
    if kind != "bf16":
        op = native_lib.decode_linear_fp8 if kind == "fp8" else native_lib.decode_linear_int4
        yl = op(x, w, sc, None, idx, A, B, ls)
        err = _row_err(yl, x.float() @ wd.t() + delta)
        print(f"{kind} lora plain projection M={M} row_err {err:.3e}")
        assert err < 2e-2, err
        assert torch.equal(op(x, w, sc, None), op(x, w, sc, None, none, A, B, ls))
