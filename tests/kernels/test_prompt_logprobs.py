"""``ops.prompt_logprobs`` (csrc/prompt_logprobs.hip) against ``ref.prompt_logprobs`` (GPU only).

bf16 -> fp32 is exact, so ranks, listed ids and the padding are compared exactly; only the logprob
values get a tolerance (``lp_tol``)."""

import math

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
W = ref.TOP_LOGPROBS
RS = (1, 3, 130)
VS = (1, 5, 8, 257, 1000, 4099, 32000, 50257)  # the odd ones leave row bases unaligned for 16-byte loads


def _inputs(R, V, dtype=torch.bfloat16, seed=0, rounded=False):
    """``randn * 3`` logits (as ``test_sampling_ext._inputs``), random targets, nlp cycling 0, 1, 5, 8."""
    torch.manual_seed(seed)
    logits = (torch.randn(R, V, device=DEV) * 3)
    if rounded:  # dense ties
        logits = logits.round()
    logits = logits.to(dtype)
    target = torch.randint(0, V, (R,), device=DEV)
    nlp = torch.tensor([0, 1, 5, 8], dtype=torch.int32, device=DEV).repeat((R + 3) // 4)[:R].contiguous()
    return logits, target, nlp


@pytest.fixture(scope="module")
def lp_tol():
    """4 x the max abs error of torch's own fp32 ``log_softmax`` on the GPU against fp64, on this
    module's R = 130, V = 32000 bf16 inputs: the margin the kernel's fast exp and its summation order
    get (the convention of ``test_sampling_ext.py::lp_tol``).  Measured on MI355X: 1.244e-06, so
    the kernel is allowed 4.975e-06 (its own error on these rows: 1.907e-06, profiles/prompt_logprobs.txt)."""
    x = _inputs(130, 32000)[0].float()
    err = (torch.log_softmax(x, dim=-1).double() - torch.log_softmax(x.double(), dim=-1)).abs().max().item()
    print(f"torch fp32 log_softmax vs fp64 on 130 x 32000: max abs err {err:.3e}; lp_tol {4 * err:.3e}")
    assert err > 0
    return 4 * err


def _check(logits, target, nlp, tol, what=""):
    """Kernel outputs against the oracle's: exact rank / ids / padding, logprobs within ``tol``, a
    listed target's logprob bit-equal to its list entry.  Returns the largest logprob error."""
    lp, rank, ids, tlp = ops.prompt_logprobs(logits, target, nlp)
    rlp, rrank, rids, rtlp = ref.prompt_logprobs(logits, target, nlp)
    R, V = logits.shape
    assert lp.shape == (R,) and rank.shape == (R,) and ids.shape == (R, W) and tlp.shape == (R, W)
    assert lp.dtype == torch.float32 and rank.dtype == torch.int32 and ids.dtype == torch.int32 and tlp.dtype == torch.float32
    assert torch.equal(rank, rrank), (what, rank.tolist()[:8], rrank.tolist()[:8])
    assert torch.equal(ids, rids), (what, (ids != rids).nonzero()[:4].tolist())
    pad = rids < 0
    assert torch.equal(torch.isneginf(tlp), pad), what
    ok = (target >= 0) & (target < V)
    assert torch.equal(torch.isnan(lp), ~ok), what
    err = 0.0
    if ok.any():
        err = (lp[ok].double() - rlp[ok].double()).abs().max().item()
    if (~pad).any():
        err = max(err, (tlp[~pad].double() - rtlp[~pad].double()).abs().max().item())
    assert err <= tol, (what, err, tol)
    # rank <= nlp exactly when the target is listed, and then the two logprobs are one value
    listed = (ids == target.view(R, 1).to(torch.int32)) & ~pad
    assert torch.equal(listed.any(1), ok & (rank <= nlp.clamp(0, min(W, V)))), what
    r, c = listed.nonzero(as_tuple=True)
    assert torch.equal(tlp[r, c], lp[r]) and torch.equal(c.to(torch.int32) + 1, rank[r]), what
    return err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("R", RS)
def test_against_oracle(R, V, dtype, lp_tol):
    err = _check(*_inputs(R, V, dtype, seed=R + V), lp_tol, f"R {R} V {V} {dtype}")
    if (R, V) == (130, 32000):
        print(f"prompt_logprob_kernel {dtype} 130 x 32000: max abs logprob err {err:.3e} (lp_tol {lp_tol:.3e})")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [5, 257, 4099, 32000])
def test_dense_ties(V, dtype, lp_tol):
    logits, target, nlp = _inputs(130, V, dtype, seed=7, rounded=True)
    assert logits.unique().numel() < 40
    _check(logits, target, nlp, lp_tol, f"ties V {V}")
    # and targets that are themselves among the tied maxima
    _check(logits, logits.float().argmax(1) if V < 8 else logits.float().topk(8, dim=1).indices[:, 5].contiguous(),
           nlp, lp_tol, f"ties at the top V {V}")


@pytest.mark.parametrize("stride", [1, 256, 1024, 2048])
def test_adversarial_placement(stride, lp_tol):
    """The 8 largest entries at 8 indices ``stride`` apart (from several first indices): however the
    kernel shares a row among its threads, some case puts all of them into one thread's share."""
    V = 32000
    firsts = [0, 1, 7, 8, 2047, 2048, 12345, V - 7 * stride - 1]
    logits, _, _ = _inputs(len(firsts) * 2, V, seed=3)
    logits = logits.float().clamp(max=6.0)
    target = torch.empty(len(firsts) * 2, dtype=torch.long, device=DEV)
    for r, f in enumerate(firsts):
        idx = torch.arange(8, device=DEV) * stride + f
        logits[2 * r, idx] = torch.tensor([9.0, 16.0, 10.0, 15.0, 11.0, 14.0, 12.0, 13.0], device=DEV)  # distinct
        logits[2 * r + 1, idx] = 12.0  # tied: listed in index order
        target[2 * r], target[2 * r + 1] = idx[6], idx[7]
    nlp = torch.full((len(firsts) * 2,), 8, dtype=torch.int32, device=DEV)
    for dtype in (torch.bfloat16, torch.float32):
        lg = logits.to(dtype)
        _check(lg, target, nlp, lp_tol, f"stride {stride} {dtype}")
        ids = ops.prompt_logprobs(lg, target, nlp)[2]
        for r, f in enumerate(firsts):
            assert sorted(ids[2 * r].tolist()) == ids[2 * r + 1].tolist() == [f + k * stride for k in range(8)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_flat_and_peaked_rows(dtype, lp_tol):
    V = 32000
    logits = torch.zeros(4, V, device=DEV)
    logits[1] = -3.25
    logits[2] = _inputs(1, V, seed=5)[0][0].float()
    logits[2, 777] = logits[2].max() + 80.0  # one entry 80 above the rest
    logits[3] = logits[2]
    target = torch.tensor([V - 1, 0, 777, 778], device=DEV)
    nlp = torch.tensor([8, 3, 8, 2], dtype=torch.int32, device=DEV)
    logits = logits.to(dtype)
    _check(logits, target, nlp, lp_tol, "flat / peaked")
    lp, rank, ids, tlp = ops.prompt_logprobs(logits, target, nlp)
    assert ids[0].tolist() == list(range(8)) and rank.tolist()[:3] == [V, 1, 1]
    assert abs(lp[0].item() + math.log(V)) <= lp_tol and lp[2].item() == 0.0 and tlp[2, 0].item() == 0.0
    assert lp[3].item() < -70.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [5, 4099, 32000])
def test_invalid_targets(V, dtype, lp_tol):
    """Targets of -1 and V: NaN / 0, the row's lists intact, the other rows as without them."""
    logits, target, nlp = _inputs(6, V, dtype, seed=11)
    nlp[:] = torch.tensor([8, 8, 1, 5, 8, 0], dtype=torch.int32)
    good = ops.prompt_logprobs(logits, target, nlp)
    bad_t = target.clone()
    bad_t[1], bad_t[4] = -1, V
    _check(logits, bad_t, nlp, lp_tol, f"invalid V {V}")
    lp, rank, ids, tlp = ops.prompt_logprobs(logits, bad_t, nlp)
    assert torch.isnan(lp[[1, 4]]).all() and rank[[1, 4]].tolist() == [0, 0]
    keep = [0, 2, 3, 5]
    assert torch.equal(lp[keep], good[0][keep]) and torch.equal(rank[keep], good[1][keep])
    assert torch.equal(ids, good[2]) and torch.equal(tlp, good[3])  # every list, the invalid rows' too
    for far in (-(1 << 40), (1 << 31) + 3, (1 << 32) + 1):  # beyond 32 bits: still only a range check
        bad_t[4] = far
        assert math.isnan(ops.prompt_logprobs(logits, bad_t, nlp)[0][4].item())


def test_nlp_beyond_v_and_range(lp_tol):
    logits, target, _ = _inputs(4, 5, seed=2)
    nlp = torch.tensor([8, 5, 6, 0], dtype=torch.int32, device=DEV)
    _check(logits, target, nlp, lp_tol, "nlp > V")
    ids = ops.prompt_logprobs(logits, target, nlp)[2]
    assert ((ids[:3] >= 0).sum(1) == 5).all() and (ids[3] == -1).all()
    empty = ops.prompt_logprobs(logits[:0], target[:0], nlp[:0])
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, W), (0, W)]


def test_rows_past_2_31_elements(lp_tol):
    """R x V beyond 2^31 elements: the row offset is 64-bit."""
    V, R = 32000, (1 << 31) // 32000 + 40
    logits = torch.empty(R, V, dtype=torch.bfloat16, device=DEV)
    logits[:4], logits[-4:] = _inputs(4, V, seed=1)[0], _inputs(4, V, seed=2)[0]
    logits[4:-4] = 0
    target = torch.randint(0, V, (R,), device=DEV)
    nlp = torch.full((R,), 8, dtype=torch.int32, device=DEV)
    lp, rank, ids, tlp = ops.prompt_logprobs(logits, target, nlp)
    assert (R - 4) * V > 1 << 31
    for sl in (slice(0, 4), slice(R - 4, R)):
        rlp, rrank, rids, _ = ref.prompt_logprobs(logits[sl], target[sl], nlp[sl])
        assert torch.equal(rank[sl], rrank) and torch.equal(ids[sl], rids)
        assert (lp[sl].double() - rlp.double()).abs().max().item() <= lp_tol
    assert (ids[4:-4] == torch.arange(8, device=DEV, dtype=torch.int32)).all()
