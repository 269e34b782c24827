"""``sample_ext`` (csrc/sampling.hip): penalties, logprobs and device-resident sampler state
against ``ref.sample_ext`` and against ``sample`` on the oracle's penalized rows (GPU only).

Penalty values are dyadic (rep in {1, 2, 0.5}; freq, pres in {0, 0.25, 0.5, 1}; counts 0..8), so
with the fixed order of the three steps the penalized fp32 logits do not depend on FMA
contraction and are bit-equal to the oracle's."""

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
W = ref.TOP_LOGPROBS


def _inputs(N, V, dtype=torch.bfloat16, seed=0, rounded=False):
    """The inputs of ``test_kernels.py::test_sampling`` (at N = 64, V = 32000 exactly those) plus a
    random sampler state: S = N + 3 slots, a shuffled slot map with a third of the rows stateless."""
    torch.manual_seed(seed)
    logits = (torch.randn(N, V, device=DEV) * 3).to(torch.bfloat16)
    temp = torch.rand(N, device=DEV) + 0.3
    temp[:(N + 7) // 8] = 0.0  # greedy rows
    topk = torch.randint(0, 100, (N,), device=DEV, dtype=torch.int32)
    topp = torch.rand(N, device=DEV) * 0.6 + 0.4
    topp[::3] = 1.0
    u = torch.rand(N, device=DEV)
    if rounded:  # dense ties
        logits = logits.float().round().to(torch.bfloat16)
    logits = logits.to(dtype)
    S = N + 3
    slot = torch.randperm(S, device=DEV)[:N].to(torch.int32)
    slot[2::3] = -1
    pick = lambda vals: torch.tensor(vals, device=DEV)[torch.randint(0, len(vals), (N,), device=DEV)]
    rep, freq, pres = pick([1.0, 2.0, 0.5]), pick([0.0, 0.25, 0.5, 1.0]), pick([0.0, 0.25, 0.5, 1.0])
    nlp = torch.tensor([0, 1, 5, 8], dtype=torch.int32, device=DEV).repeat((N + 3) // 4)[:N].contiguous()
    counts = (torch.randint(0, 9, (S, V), device=DEV) * (torch.rand(S, V, device=DEV) < 0.3)).to(torch.int32)
    mask = (torch.rand(S, V, device=DEV) < 0.2).to(torch.uint8)
    return dict(logits=logits, temp=temp, topk=topk, topp=topp, u=u, slot=slot, rep=rep, freq=freq, pres=pres,
                nlp=nlp, counts=counts, mask=mask)


def _call(fn, c, counts):
    return fn(c["logits"], c["temp"], c["topk"], c["topp"], c["u"], c["slot"], c["rep"], c["freq"], c["pres"],
              c["nlp"], counts, c["mask"])


def _penalized(c):
    return ref.penalize(c["logits"], c["slot"], c["rep"], c["freq"], c["pres"], c["counts"], c["mask"])


def _counts_after(c, toks):
    exp = c["counts"].clone()
    for i, s in enumerate(c["slot"].tolist()):
        if s >= 0:
            exp[s, int(toks[i])] += 1
    return exp


@pytest.fixture(scope="module")
def lp_tol():
    """4 x the max abs error of torch's own fp32 ``log_softmax`` on the GPU against the fp64 oracle,
    on the penalized rows of the N = 64, V = 32000 case: the kernel's fast exp and its summation
    order get that margin.  Measured on MI355X: 2.006e-06, so the kernel is allowed 8.02e-06 (its
    own error on such rows: 5.8e-07, profiles/sampling_ext.txt)."""
    x = _penalized(_inputs(64, 32000))
    err = (torch.log_softmax(x, dim=-1).double() - torch.log_softmax(x.double(), dim=-1)).abs().max().item()
    print(f"torch fp32 log_softmax max abs error vs fp64: {err:.3e}")
    assert err > 0
    return 4 * err


@pytest.mark.parametrize("V", [37, 1000, 32000])
def test_neutral_parameters_match_sample(native_lib, V):
    """slot = -1, or a slot with rep = 1 and freq = pres = 0: the tokens of ``sample``."""
    c = _inputs(6, V)
    c["rep"].fill_(1.0)
    c["freq"].zero_()
    c["pres"].zero_()
    counts = c["counts"].clone()
    toks, lp, top_ids, top_lp = _call(native_lib.sample_ext, c, counts)
    assert torch.equal(toks, native_lib.sample(c["logits"], c["temp"], c["topk"], c["topp"], c["u"]))
    assert torch.equal(counts, _counts_after(c, toks))  # -1 rows: nothing changed anywhere
    c["slot"].fill_(-1)
    counts = c["counts"].clone()
    toks2 = _call(native_lib.sample_ext, c, counts)[0]
    assert torch.equal(toks2, toks) and torch.equal(counts, c["counts"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [37, 1000, 50257, 32000])
@pytest.mark.parametrize("N", [1, 5, 64])
def test_penalties(native_lib, lp_tol, N, V, dtype):
    c = _inputs(N, V, dtype)
    counts = c["counts"].clone()
    toks, lp, top_ids, top_lp = _call(native_lib.sample_ext, c, counts)
    x = _penalized(c)
    # the draw: exactly ``sample`` on the oracle's penalized fp32 rows
    assert torch.equal(toks, native_lib.sample(x, c["temp"], c["topk"], c["topp"], c["u"]))
    rcounts = c["counts"].clone()
    rtoks, rlp, rtop_ids, rtop_lp = _call(ref.sample_ext, c, rcounts)
    greedy = c["temp"] <= 0
    assert torch.equal(toks[greedy], rtoks[greedy])
    if (N, V) == (64, 32000):  # test_sampling's allowance: summation order at an inverse-CDF boundary
        assert (toks != rtoks).sum().item() <= 2
    # state: plus one at (slot, token) of the stateful rows and nothing else
    assert torch.equal(counts, _counts_after(c, toks))
    if torch.equal(toks, rtoks):
        assert torch.equal(counts, rcounts)
    # logprobs against the fp64 oracle (at the kernel's tokens), top lists against the stable sort
    lp64 = torch.log_softmax(x.double(), dim=-1)
    err = (lp.double() - lp64.gather(1, toks.view(N, 1)).view(N)).abs().max().item()
    assert err <= lp_tol, (err, lp_tol)
    assert torch.equal(top_ids, rtop_ids)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for i, k in enumerate(c["nlp"].tolist()):
        assert torch.equal(top_ids[i, :k].long(), order[i, :k])
        assert (top_ids[i, k:] == -1).all() and (top_lp[i, k:] == -float("inf")).all()
        if k:
            e = (top_lp[i, :k].double() - lp64[i, order[i, :k]]).abs().max().item()
            assert e <= lp_tol, (i, e, lp_tol)
            assert (top_lp[i, :k - 1] >= top_lp[i, 1:k]).all()
        hit = (top_ids[i, :k] == toks[i]).nonzero()
        if hit.numel():  # the chosen token's logprob is its top-list entry, bit for bit
            assert lp[i].item() == top_lp[i, int(hit[0])].item()


def test_state_chain(native_lib):
    """Three greedy calls, each seeing the counts the previous ones left."""
    N, V = 5, 1000
    c = _inputs(N, V)
    c["temp"].zero_()
    c["pres"].fill_(1.0)  # every pick moves the next step's arg-max candidates
    counts, rcounts = c["counts"].clone(), c["counts"].clone()
    for step in range(3):
        c["logits"] = _inputs(N, V, seed=step)["logits"].float().round().to(torch.bfloat16)
        toks = _call(native_lib.sample_ext, c, counts)[0]
        rtoks = _call(ref.sample_ext, c, rcounts)[0]
        assert torch.equal(toks, rtoks), step
    assert torch.equal(counts, rcounts)
    assert (counts - c["counts"]).sum().item() == 3 * int((c["slot"] >= 0).sum())


def test_strong_penalties(native_lib):
    V = 300
    c = _inputs(2, V)
    c["temp"].zero_()
    c["slot"] = torch.tensor([1, 3], dtype=torch.int32, device=DEV)
    c["counts"].zero_()
    c["mask"].zero_()
    logits = torch.randn(2, V, device=DEV).clamp_(-3, -0.5)
    # row 0: the arg-max was generated before; presence 64 pushes it below everything else
    logits[0, 17], logits[0, 200] = 9.0, 5.0
    c["counts"][1, 17] = 1
    c["rep"][0], c["freq"][0], c["pres"][0] = 1.0, 0.0, 64.0
    # row 1: the arg-max occurs in the prompt; rep = 2 halves it to 2.0, below the runner-up's 3.0
    logits[1, 40], logits[1, 7] = 4.0, 3.0
    c["mask"][3, 40] = 1
    c["rep"][1], c["freq"][1], c["pres"][1] = 2.0, 0.0, 0.0
    c["logits"] = logits.to(torch.bfloat16)
    counts = c["counts"].clone()
    toks = _call(native_lib.sample_ext, c, counts)[0]
    assert toks.tolist() == [200, 7]
    c["slot"].fill_(-1)  # without the state: the plain arg-max
    assert _call(native_lib.sample_ext, c, counts.clone())[0].tolist() == [17, 40]


@pytest.mark.parametrize("V", [5, 8, 1000])
def test_top_ids_dense_ties(native_lib, lp_tol, V):
    """Rounded logits (many equal values): the top list is the stable descending sort, ties to the
    lowest index; a vocabulary smaller than nlp pads with -1 / -inf."""
    N = 8
    c = _inputs(N, V, rounded=True)
    c["nlp"] = torch.tensor([0, 1, 5, 8, 8, 8, 3, 2], dtype=torch.int32, device=DEV)
    toks, lp, top_ids, top_lp = _call(native_lib.sample_ext, c, c["counts"].clone())
    x = _penalized(c)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for i, k in enumerate(c["nlp"].tolist()):
        k = min(k, V)
        assert torch.equal(top_ids[i, :k].long(), order[i, :k]), i
        assert (top_ids[i, k:] == -1).all() and (top_lp[i, k:] == -float("inf")).all()
    if V == 8:  # a full row's logprobs are a normalised distribution
        full = c["nlp"] == 8
        z = torch.logsumexp(top_lp[full].double(), dim=1).abs().max().item()
        assert z <= lp_tol, (z, lp_tol)
        for i in full.nonzero().view(-1).tolist():  # the token is in the list: the same number
            j = int((top_ids[i] == toks[i]).nonzero()[0])
            assert lp[i].item() == top_lp[i, j].item()


def test_slot_check(native_lib):
    c = _inputs(4, 37)
    c["slot"] = torch.tensor([2, -1, 2, -1], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="distinct"):
        _call(ops.sample_ext, c, c["counts"].clone())
    c["slot"] = torch.tensor([2, -1, 7, -1], dtype=torch.int32, device=DEV)  # S = 7
    with pytest.raises(ValueError, match="below 7"):
        _call(ops.sample_ext, c, c["counts"].clone())


def test_graph_capture(native_lib):
    """Captured in a graph and replayed twice on fresh logits, the state carrying over: the
    tokens and counts of two eager calls."""
    N, V = 5, 1000
    c = _inputs(N, V)
    c["temp"][1] = 0.0
    steps = [_inputs(N, V, seed=10 + i)["logits"] for i in range(2)]
    ecounts = c["counts"].clone()
    etoks = []
    for l in steps:
        etoks.append(_call(ops.sample_ext, dict(c, logits=l), ecounts)[0].clone())
    static = dict(c, logits=steps[0].clone())
    counts = c["counts"].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(ops.sample_ext, static, counts)  # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _call(ops.sample_ext, static, counts)
    counts.copy_(c["counts"])  # the warm-up call counted: start over
    for l, e in zip(steps, etoks):
        static["logits"].copy_(l)
        g.replay()
        assert torch.equal(out[0], e)
    assert torch.equal(counts, ecounts)
    torch.cuda.synchronize()
    g.reset()
