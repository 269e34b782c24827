"""``sample_guided`` (csrc/sampling.hip): the guide's mask, the draw on rows that hold -inf, the
logprobs over the allowed set and the device-resident automaton state, against ``ref.sample_guided``
(GPU only).  The guides are random tables (``llmctl.testing.guided.random_arena``), no regex, so the
kernel is tested alone; the inputs are made on the CPU and are the same on every machine
(``tests/unit/test_guided_cpu.py`` checks the oracle's fp32 draw against an fp64 one on them)."""

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref
from llmctl.testing import guided as tg
from llmctl.testing.sampling_ext import lp_tolerance

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = -float("inf")


@pytest.fixture(scope="module")
def lp_tol():
    """4 x the max abs error of torch's own fp32 ``log_softmax`` on the GPU against fp64 on 64 x
    32000 logits: the margin ``test_sampling_ext.py`` gives the kernel's fast exp and summation order."""
    return lp_tolerance(DEV)


def _masked_rows(c):
    """The oracle's penalized and masked fp32 rows and the allowed mask."""
    x = ref.penalize(c["logits"], c["slot"], c["rep"], c["freq"], c["pres"], c["counts"], c["mask"])
    ok = ref.guide_mask(c["guide"], c["gslot"], c["cls"], c["next"], c["meta"], c["state"])
    return torch.where(ok, x, torch.full_like(x, NEG)), ok


def _clone(c):
    return {k: v.clone() for k, v in c.items()}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [257, 512, 32000])
@pytest.mark.parametrize("N", [1, 3, 16])
def test_against_oracle(native_lib, lp_tol, N, V, dtype):
    c = tg.to_device(tg.kernel_inputs(N, V, dtype), DEV)
    r = _clone(c)
    x, ok = _masked_rows(c)
    toks, lp, top_ids, top_lp = tg.call(ops.sample_guided, c)
    rtoks, rlp, rtop_ids, rtop_lp = tg.call(ref.sample_guided, r)
    rows = torch.arange(N, device=DEV)
    assert ok[rows, toks].all()  # every token is allowed
    greedy = c["temp"] <= 0
    for i in greedy.nonzero().view(-1).tolist():  # the arg-max over the allowed set, lowest index on ties
        assert int(toks[i]) == int((x[i] == x[i].max()).nonzero()[0])
    diff = (toks != rtoks)
    print(f"N={N} V={V}: {int(diff.sum())} rows differ from the oracle")
    if (N, V) == (16, 32000):  # test_sampling_ext's allowance: summation order at an inverse-CDF boundary
        assert diff.sum().item() <= 2 and not diff[greedy].any()
    else:
        assert torch.equal(toks, rtoks)
    # state: counts plus one at (slot, token); the automaton state follows the kernel's own token
    exp_counts, exp_state = r["counts"], r["state"]
    if diff.any():
        exp_counts, exp_state = tg.kernel_inputs(N, V, dtype)["counts"].to(DEV), tg.kernel_inputs(N, V, dtype)["state"].to(DEV)
        for i in range(N):
            if c["slot"][i] >= 0:
                exp_counts[c["slot"][i], toks[i]] += 1
            g = int(c["guide"][i])
            if g >= 0:
                C = int(c["meta"][g, 1])
                gs = int(c["gslot"][i])
                exp_state[gs] = c["next"][g, int(exp_state[gs]) * C + int(c["cls"][g, toks[i]])]
    assert torch.equal(c["counts"], exp_counts) and torch.equal(c["state"], exp_state)
    assert (c["state"] >= 0).all()
    # logprobs against the fp64 oracle on the masked row (at the kernel's tokens): renormalised over
    # the allowed set; top lists against the stable sort over the allowed entries
    lp64 = torch.log_softmax(x.double(), dim=-1)
    err = (lp.double() - lp64[rows, toks]).abs().max().item()
    assert err <= lp_tol, (err, lp_tol)
    assert torch.equal(top_ids, rtop_ids)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for i, k in enumerate(c["nlp"].tolist()):
        k = min(k, int(ok[i].sum()))
        assert torch.equal(top_ids[i, :k].long(), order[i, :k]) and ok[i, top_ids[i, :k].long()].all()
        assert (top_ids[i, k:] == -1).all() and (top_lp[i, k:] == NEG).all()
        if k:
            e = (top_lp[i, :k].double() - lp64[i, order[i, :k]]).abs().max().item()
            assert e <= lp_tol, (i, e, lp_tol)
        hit = (top_ids[i, :k] == toks[i]).nonzero()
        if hit.numel():
            assert lp[i].item() == top_lp[i, int(hit[0])].item()


@pytest.mark.parametrize("V", [257, 512, 32000])
def test_unguided_rows_are_sample_ext(native_lib, V):
    """guide = -1 everywhere: the four outputs and ``counts`` of ``sample_ext``, bit for bit, and
    ``guide_state`` untouched."""
    for dtype in (torch.bfloat16, torch.float32):
        c = tg.to_device(tg.kernel_inputs(5, V, dtype), DEV)
        c["guide"].fill_(-1)
        c["gslot"].fill_(-1)
        c["state"] = torch.arange(7, dtype=torch.int32, device=DEV)
        e = _clone(c)
        out = tg.call(ops.sample_guided, c)
        exp = native_lib.sample_ext(*(e[k] for k in tg.ARGS[:12]))
        for a, b in zip(out, exp):
            assert torch.equal(a, b)
        assert torch.equal(c["counts"], e["counts"]) and not torch.equal(c["counts"], tg.kernel_inputs(5, V, dtype)["counts"].to(DEV))
        assert c["state"].tolist() == list(range(7))


def _trap_logits(V, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, V, generator=g).clamp_(-3, 1)


def _uniforms(n=64):
    return (torch.arange(n, dtype=torch.float32) + 0.5) / n


@pytest.mark.parametrize("V", [257, 32000])
def test_top_k_cuts_on_masked_rows(native_lib, V):
    """T = 1 and the 10 largest logits masked.  From a minimum of -inf the bisection's midpoints are
    all -inf and top-k keeps every token; over the finite entries it keeps the k best allowed."""
    l = _trap_logits(V)
    top = torch.randperm(V, generator=torch.Generator().manual_seed(1))[:12]
    l[0, top[:10]] = 5.0 + torch.arange(10) * 0.25  # masked, and larger than everything allowed
    l[0, top[10]], l[0, top[11]] = 2.0, 1.75  # the two best allowed
    allowed = torch.ones(V, dtype=torch.bool)
    allowed[top[:10]] = False
    for k, want in ((1, {int(top[10])}), (2, {int(top[10]), int(top[11])})):
        c = tg.to_device(tg.neutral_case(l.expand(64, V).contiguous(), 1.0, k, 1.0, _uniforms(), allowed), DEV)
        toks = tg.call(ops.sample_guided, c)[0]
        assert set(toks.tolist()) == want, (k, sorted(set(toks.tolist())))


@pytest.mark.parametrize("V", [257, 32000])
def test_top_p_cuts_on_masked_rows(native_lib, V):
    """One allowed token holds 0.9 of the allowed mass: top_p = 0.5 always returns it."""
    l = torch.zeros(1, V)
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(2))
    masked, star = perm[:V // 4], int(perm[V // 4])
    l[0, masked] = 30.0
    n_rest = V - masked.numel() - 1
    l[0, star] = float(torch.log(torch.tensor(9.0 * n_rest)))  # e^l / (e^l + n_rest) = 0.9
    allowed = torch.ones(V, dtype=torch.bool)
    allowed[masked] = False
    c = tg.to_device(tg.neutral_case(l.expand(64, V).contiguous(), 1.0, 0, 0.5, _uniforms(), allowed), DEV)
    assert set(tg.call(ops.sample_guided, c)[0].tolist()) == {star}
    c = tg.to_device(tg.neutral_case(l.expand(64, V).contiguous(), 1.0, 0, 1.0, _uniforms(), allowed), DEV)
    assert len(set(tg.call(ops.sample_guided, c)[0].tolist())) > 1  # without the cut the others are drawn too


@pytest.mark.parametrize("V", [257, 512, 32000])
def test_rounding_fallback_returns_an_allowed_token(native_lib, V):
    """The top quarter of the vocabulary is masked.  With the largest uniform below 1 the draw ends
    on an allowed token; with r at the very top (u = 1: no entry's running sum exceeds it) the
    fallback returns the last kept entry -- with a threshold of -inf that is the last *allowed*
    token, where "the last token with x >= thr" would be the masked token V - 1."""
    last = (3 * V) // 4 - 1
    allowed = torch.arange(V) <= last
    below1 = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    u = torch.tensor([below1, below1, 1.0, 1.0])
    l = _trap_logits(V, seed=3).expand(4, V).contiguous()
    temp = torch.tensor([1.0, 0.5, 1.0, 2.0])
    for k, p in ((0, 1.0), (40, 0.9)):
        c = tg.to_device(tg.neutral_case(l, temp, k, p, u, allowed), DEV)
        toks = tg.call(ops.sample_guided, c)[0]
        assert allowed.to(DEV)[toks].all(), (k, p, toks.tolist())
        if k == 0:
            assert toks[2:].tolist() == [last, last]


def test_one_allowed_token(native_lib, lp_tol):
    V = 512
    allowed = torch.zeros(V, dtype=torch.bool)
    allowed[333] = True
    temp = torch.tensor([0.0, 0.3, 1.0, 5.0])
    l = _trap_logits(V, seed=4).expand(4, V).contiguous()
    for k, p in ((0, 1.0), (5, 0.7)):
        c = tg.to_device(tg.neutral_case(l, temp, k, p, torch.tensor([0.0, 0.5, 0.99, 0.2]), allowed, nlp=8), DEV)
        toks, lp, top_ids, top_lp = tg.call(ops.sample_guided, c)
        assert toks.tolist() == [333] * 4 and lp.abs().max().item() <= lp_tol
        assert top_ids[:, 0].tolist() == [333] * 4 and (top_ids[:, 1:] == -1).all() and (top_lp[:, 1:] == NEG).all()


def test_short_top_lists(native_lib, lp_tol):
    """nlp = 8 with 3 allowed tokens: 3 entries, then (-1, -inf); their probabilities sum to 1."""
    V = 1000
    allowed = torch.zeros(V, dtype=torch.bool)
    allowed[[5, 600, 999]] = True
    l = _trap_logits(V, seed=5).expand(2, V).contiguous()
    c = tg.to_device(tg.neutral_case(l, torch.tensor([0.0, 1.0]), 0, 1.0, torch.tensor([0.1, 0.6]), allowed, nlp=8), DEV)
    toks, lp, top_ids, top_lp = tg.call(ops.sample_guided, c)
    assert sorted(top_ids[0, :3].tolist()) == [5, 600, 999] and torch.equal(top_ids[0], top_ids[1])
    assert (top_ids[:, 3:] == -1).all() and (top_lp[:, 3:] == NEG).all()
    assert (top_lp[:, :2] >= top_lp[:, 1:3]).all()
    assert torch.logsumexp(top_lp[:, :3].double(), dim=1).abs().max().item() <= lp_tol


def test_state_chain(native_lib):
    """Three chained launches on fresh logits: the oracle's trajectory of tokens, counts and states."""
    N, V = 6, 512
    c = tg.to_device(tg.kernel_inputs(N, V), DEV)
    r = _clone(c)
    start = c["state"].clone()
    for step in range(3):
        c["logits"] = r["logits"] = tg.kernel_inputs(N, V, seed=step + 1)["logits"].to(DEV)
        c["u"] = r["u"] = tg.kernel_inputs(N, V, seed=step + 1)["u"].to(DEV)
        toks = tg.call(ops.sample_guided, c)[0]
        rtoks = tg.call(ref.sample_guided, r)[0]
        assert torch.equal(toks, rtoks), step
        assert torch.equal(c["state"], r["state"]) and torch.equal(c["counts"], r["counts"]), step
    assert not torch.equal(c["state"], start)
    free = torch.ones(N + 2, dtype=torch.bool, device=DEV)
    free[c["gslot"][c["gslot"] >= 0].long()] = False
    assert torch.equal(c["state"][free], start[free])  # words no row owns are untouched


def test_lds_edge_last_class(native_lib):
    """C = 8192 (the whole LDS row) in a state whose only allowed class is the last one."""
    V, C, S = 32000, 8192, 3
    gen = torch.Generator().manual_seed(6)
    cls = torch.randint(0, C - 1, (1, V), generator=gen, dtype=torch.int32)
    last = torch.randperm(V, generator=gen)[:5]
    cls[0, last] = C - 1
    nxt = torch.full((1, S * C), -1, dtype=torch.int32)
    nxt[0, :C] = 1  # state 0: everything allowed
    nxt[0, 2 * C - 1] = 2  # state 1: only the last class, to state 2
    nxt[0, 2 * C:3 * C - 1] = 0  # state 2: everything but the last class
    l = _trap_logits(V, seed=7).expand(3, V).contiguous()
    c = tg.neutral_case(l, torch.tensor([0.0, 1.0, 1.0]), 0, 1.0, torch.tensor([0.3, 0.6, 0.9]), torch.ones(V, dtype=torch.bool))
    c.update(cls=cls, next=nxt, meta=torch.tensor([[S, C]], dtype=torch.int32), state=torch.tensor([1, 1, 2], dtype=torch.int32))
    c = tg.to_device(c, DEV)
    r = _clone(c)
    toks = tg.call(ops.sample_guided, c)[0]
    assert torch.equal(toks, tg.call(ref.sample_guided, r)[0])
    assert set(toks[:2].tolist()) <= set(last.tolist()) and int(toks[2]) not in last.tolist()
    assert c["state"].tolist() == [2, 2, 0]


def test_graph_capture(native_lib):
    """One call captured and replayed three times on fresh logits: the state advances with every
    replay and the tokens follow the oracle step by step."""
    N, V = 5, 1000
    c = tg.to_device(tg.kernel_inputs(N, V), DEV)
    r = _clone(c)
    steps = [tg.kernel_inputs(N, V, seed=10 + i)["logits"].to(DEV) for i in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tg.call(ops.sample_guided, c)  # warm-up outside the graph
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = tg.call(ops.sample_guided, c)
    c["counts"].copy_(r["counts"])  # the warm-up call advanced the state: start over
    c["state"].copy_(r["state"])
    trail = []
    for l in steps:
        c["logits"].copy_(l)
        r["logits"] = l
        g.replay()
        rtoks = tg.call(ref.sample_guided, r)[0]
        assert torch.equal(out[0], rtoks)
        assert torch.equal(c["state"], r["state"]) and torch.equal(c["counts"], r["counts"])
        trail.append(c["state"].tolist())
    assert len({tuple(t) for t in trail}) == 3  # the state moved with every replay
    torch.cuda.synchronize()
    g.reset()


def test_slot_check(native_lib):
    c = tg.to_device(tg.kernel_inputs(4, 257), DEV)
    c["guide"] = torch.tensor([1, -1, 2, 0], dtype=torch.int32, device=DEV)
    c["state"].zero_()
    c["gslot"] = torch.tensor([2, -1, 2, 0], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="gslot.*distinct"):
        tg.call(ops.sample_guided, c)
    c["gslot"] = torch.tensor([2, -1, 6, 0], dtype=torch.int32, device=DEV)  # Sg = 6
    with pytest.raises(ValueError, match="below 6"):
        tg.call(ops.sample_guided, c)
    c["gslot"] = torch.tensor([2, -1, -1, 0], dtype=torch.int32, device=DEV)  # guided row without a state word
    with pytest.raises(ValueError, match="gslot"):
        tg.call(ops.sample_guided, c)
    c["gslot"] = torch.tensor([2, -1, 1, 0], dtype=torch.int32, device=DEV)
    c["guide"][0] = 5  # G = 5
    with pytest.raises(ValueError, match="guide must be below 5"):
        tg.call(ops.sample_guided, c)
    c["guide"][0] = 1
    c["slot"] = torch.tensor([3, 3, -1, -1], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="state slots"):
        tg.call(ops.sample_guided, c)
