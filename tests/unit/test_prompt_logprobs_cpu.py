"""``ref.prompt_logprobs`` -- the specification of ``ops.prompt_logprobs`` -- against a direct fp64
``log_softmax`` and a stable sort on small rows (CPU)."""

import math

import pytest
import torch

from llmctl import ops
from llmctl.ops import ref

W = ref.TOP_LOGPROBS


def _direct(logits, target, nlp):
    """Row by row, in plain Python on top of fp64 log_softmax and a stable descending sort."""
    R, V = logits.shape
    lsm = torch.log_softmax(logits.double(), dim=-1)
    out = []
    for r in range(R):
        x = logits[r].double().tolist()
        order = sorted(range(V), key=lambda i: (-x[i], i))
        t, k = int(target[r]), min(max(int(nlp[r]), 0), W, V)
        ok = 0 <= t < V
        lp = float(lsm[r, t].float()) if ok else float("nan")
        rank = order.index(t) + 1 if ok else 0
        ids = order[:k] + [-1] * (W - k)
        tlp = [float(lsm[r, i].float()) for i in order[:k]] + [-math.inf] * (W - k)
        out.append((lp, rank, ids, tlp))
    return out


def _assert_same(logits, target, nlp, fn=ref.prompt_logprobs):
    lp, rank, ids, tlp = fn(logits, target, nlp)
    assert lp.dtype == torch.float32 and rank.dtype == torch.int32 and ids.dtype == torch.int32 and tlp.dtype == torch.float32
    assert tuple(ids.shape) == tuple(tlp.shape) == (logits.shape[0], W)
    for r, (wlp, wrank, wids, wtlp) in enumerate(_direct(logits, target, nlp)):
        got = lp[r].item()
        assert (math.isnan(got) and math.isnan(wlp)) or abs(got - wlp) <= 1e-6, (r, got, wlp)
        assert rank[r].item() == wrank and ids[r].tolist() == wids, r
        assert all(a == b or abs(a - b) <= 1e-6 for a, b in zip(tlp[r].tolist(), wtlp)), r  # (-inf == -inf)
        # rank <= nlp exactly when the target is listed; its entry is the logprob, bit for bit
        listed = int(target[r]) in [i for i in wids if i >= 0]
        assert listed == (0 < wrank <= min(max(int(nlp[r]), 0), W))
        if listed:
            assert tlp[r, wrank - 1].item() == got and ids[r, wrank - 1].item() == int(target[r])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [1, 5, 8, 9, 257])
def test_random_rows(V, dtype):
    torch.manual_seed(V)
    R = 18
    logits = (torch.randn(R, V) * 3).to(dtype)
    _assert_same(logits, torch.randint(0, V, (R,)), torch.arange(R, dtype=torch.int32) % 9)  # nlp 0..8


def test_ties_edge_targets_and_nlp_beyond_v():
    logits = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0],
                           [0.0, 0.0, 0.0, 0.0, 0.0],
                           [5.0, 4.0, 3.0, 2.0, 1.0],
                           [1.0, 2.0, 3.0, 4.0, 5.0]])
    for target in ([4, 4, 0, 0], [2, 0, 4, 4], [1, 2, 3, 1]):
        for nlp in ([8, 8, 8, 8], [0, 1, 2, 5], [3, 6, 4, 1]):
            _assert_same(logits, torch.tensor(target), torch.tensor(nlp, dtype=torch.int32))
    lp, rank, ids, tlp = ref.prompt_logprobs(logits, torch.tensor([4, 4, 0, 0]), torch.full((4,), 8, dtype=torch.int32))
    assert ids[0].tolist() == [1, 2, 4, 0, 3, -1, -1, -1] and rank.tolist() == [3, 5, 1, 5]  # lower index first on ties
    assert ids[1].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and torch.isneginf(tlp[:, 5:]).all()
    assert lp[1].item() == pytest.approx(-math.log(5), abs=1e-7)


def test_dense_ties():
    torch.manual_seed(1)
    logits = (torch.randn(12, 64) * 2).round()
    _assert_same(logits, torch.randint(0, 64, (12,)), torch.full((12,), 8, dtype=torch.int32))


def test_invalid_targets():
    torch.manual_seed(2)
    logits = torch.randn(4, 7)
    nlp = torch.tensor([8, 2, 0, 7], dtype=torch.int32)
    target = torch.tensor([-1, 7, 3, 1 << 40])
    _assert_same(logits, target, nlp)
    lp, rank, ids, tlp = ref.prompt_logprobs(logits, target, nlp)
    assert torch.isnan(lp[[0, 1, 3]]).all() and rank.tolist()[:2] == [0, 0] and rank[3].item() == 0
    good = ref.prompt_logprobs(logits, torch.tensor([0, 0, 3, 0]), nlp)
    assert torch.equal(ids, good[2]) and torch.equal(tlp, good[3]) and lp[2] == good[0][2] and rank[2] == good[1][2]


def test_ops_dispatches_to_the_oracle_on_cpu():
    torch.manual_seed(3)
    logits = torch.randn(5, 33)
    _assert_same(logits, torch.randint(0, 33, (5,)), torch.tensor([0, 1, 5, 8, 3], dtype=torch.int32),
                 fn=ops.prompt_logprobs)
