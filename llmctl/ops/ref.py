"""Pure-PyTorch fp32 oracles for every HIP kernel in ``llmctl/ops/csrc``.

These are (a) the numerics reference the kernel tests compare against and (b) the compute
path on CPU (the gloo/CPU distributed tests and the GPT-2-125M CPU plumbing config run
through them).  They are deliberately written in plain fp32 math, not for speed.

Reference parity: the reference runs all of these as stock HF/PyTorch ops
(attention, RMSNorm, RoPE, SwiGLU, AdamW, clip, CE are library calls there).
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------- norms
def rmsnorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
    y = (xf * rstd.unsqueeze(-1)) * w.float()
    return y.to(x.dtype), rstd


def rmsnorm_bwd(dy, x, w, rstd, dres: Optional[torch.Tensor] = None):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    r = rstd.unsqueeze(-1)
    xhat = xf * r
    g = dyf * wf
    dx = r * (g - xhat * (g * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.float()
    dw = (dyf * xhat).reshape(-1, x.shape[-1]).sum(0)
    return dx.to(x.dtype), dw.to(w.dtype)


def layernorm_fwd(x, w, b, eps):
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = (xf - mu).pow(2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    y = (xf - mu) * rstd * w.float() + b.float()
    return y.to(x.dtype), mu.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(dy, x, w, mu, rstd, dres=None):
    xf, dyf, wf = x.float(), dy.float(), w.float()
    r = rstd.unsqueeze(-1)
    xhat = (xf - mu.unsqueeze(-1)) * r
    g = dyf * wf
    dx = r * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.float()
    H = x.shape[-1]
    dw = (dyf * xhat).reshape(-1, H).sum(0)
    db = dyf.reshape(-1, H).sum(0)
    return dx.to(x.dtype), dw.to(w.dtype), db.to(w.dtype)


# ----------------------------------------------------------------------------- rope
def rope_tables(seq_len: int, head_dim: int, base: float = 10000.0, scaling: str = "linear",
                factor: float = 1.0, short_factor=None, long_factor=None,
                original_max_position: Optional[int] = None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin tables [seq_len, head_dim/2] fp32 (host-precomputed, per the CDNA guide's
    'precompute trig tables' rule for RoPE).  ``su`` = LongRoPE-style per-dim rescale."""
    half = head_dim // 2
    inv = 1.0 / (base ** (torch.arange(0, half, dtype=torch.float64) * 2.0 / head_dim))
    pos = torch.arange(seq_len, dtype=torch.float64)
    mscale = 1.0
    if scaling == "linear" and factor and factor != 1.0:
        pos = pos / factor
    elif scaling == "su":
        orig = original_max_position or seq_len
        fac = long_factor if (seq_len > orig and long_factor) else short_factor
        if fac:
            inv = inv / torch.tensor(fac, dtype=torch.float64)
        if seq_len > orig:
            s = seq_len / orig
            mscale = math.sqrt(1 + math.log(s) / math.log(orig))
    ang = torch.outer(pos, inv)
    cos = (torch.cos(ang) * mscale).float()
    sin = (torch.sin(ang) * mscale).float()
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return cos.contiguous(), sin.contiguous()


def _rot(x, cos, sin):
    # x [..., D] rotate-half convention (Llama/NeoX): (x1, x2) -> (x1 c - x2 s, x2 c + x1 s)
    d = x.shape[-1] // 2
    x1, x2 = x[..., :d], x[..., d:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_qkv_fwd(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, nq: int, nkv: int,
                 seq_len: int, positions: Optional[torch.Tensor] = None):
    """qkv [T, (nq+2nkv)*D] -> q [T, nq, D], k [T, nkv, D], v [T, nkv, D] (q,k rotated)."""
    T = qkv.shape[0]
    D = qkv.shape[1] // (nq + 2 * nkv)
    x = qkv.float().view(T, nq + 2 * nkv, D)
    pos = positions.long() if positions is not None else torch.arange(T, device=qkv.device) % seq_len
    c = cos[pos].unsqueeze(1)
    s = sin[pos].unsqueeze(1)
    q = _rot(x[:, :nq], c, s)
    k = _rot(x[:, nq:nq + nkv], c, s)
    v = x[:, nq + nkv:]
    dt = qkv.dtype
    return q.to(dt).contiguous(), k.to(dt).contiguous(), v.to(dt).contiguous()


def rope_qkv_bwd(dq, dk, dv, cos, sin, seq_len: int, positions=None):
    T = dq.shape[0]
    pos = positions.long() if positions is not None else torch.arange(T, device=dq.device) % seq_len
    c = cos[pos].unsqueeze(1)
    s = sin[pos].unsqueeze(1)
    dqf = _rot(dq.float(), c, -s)  # inverse rotation = transpose
    dkf = _rot(dk.float(), c, -s)
    out = torch.cat([dqf, dkf, dv.float()], dim=1).reshape(T, -1)
    return out.to(dq.dtype)


# ----------------------------------------------------------------------------- attention
def _doc_mask(doc_start, S: int, device):
    """[B,1,S,S] visibility of packed documents: key j visible to query i iff doc_start[i] <= j."""
    j = torch.arange(S, device=device)
    return (j.view(1, 1, 1, S) >= doc_start.to(device).long().view(doc_start.shape[0], 1, S, 1))


def document_starts(input_ids: torch.Tensor, separator: int) -> torch.Tensor:
    """[B,S] position where each token's document begins; a document ends with (includes) the
    ``separator`` token, the next one starts right after it."""
    B, S = input_ids.shape
    pos = torch.arange(S, device=input_ids.device).expand(B, S)
    is_start = torch.zeros_like(input_ids, dtype=torch.bool)
    is_start[:, 0] = True
    is_start[:, 1:] = input_ids[:, :-1] == separator
    starts = torch.where(is_start, pos, torch.zeros_like(pos))
    return torch.cummax(starts, dim=1).values.to(torch.int32).contiguous()


def attention_fwd(q, k, v, scale: float, causal: bool = True, doc_start=None):
    """q [B,S,Hq,D], k/v [B,S,Hkv,D] -> o [B,S,Hq,D], lse [B,Hq,S] (natural log)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    Sk = k.shape[1]
    if causal:
        mask = torch.ones(S, Sk, dtype=torch.bool, device=q.device).tril(Sk - S)
        s = s.masked_fill(~mask, float("-inf"))
    if doc_start is not None:
        s = s.masked_fill(~_doc_mask(doc_start, S, q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    o = torch.matmul(p, vf).transpose(1, 2)
    return o.to(q.dtype).contiguous(), lse


def attention_bwd(do, q, k, v, o, lse, scale: float, causal: bool = True, doc_start=None):
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(rep, dim=1)
    dof = do.float().transpose(1, 2)
    of = o.float().transpose(1, 2)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    Sk = k.shape[1]
    if causal:
        mask = torch.ones(S, Sk, dtype=torch.bool, device=q.device).tril(Sk - S)
        s = s.masked_fill(~mask, float("-inf"))
    if doc_start is not None:
        s = s.masked_fill(~_doc_mask(doc_start, S, q.device), float("-inf"))
    p = torch.exp(s - lse.unsqueeze(-1))
    dv = torch.matmul(p.transpose(-1, -2), dof)
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * of).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    dq = torch.matmul(ds, kf)
    dk = torch.matmul(ds.transpose(-1, -2), qf)
    dk = dk.view(B, Hkv, rep, Sk, D).sum(2)
    dv = dv.view(B, Hkv, rep, Sk, D).sum(2)
    return (dq.transpose(1, 2).to(q.dtype).contiguous(), dk.transpose(1, 2).to(k.dtype).contiguous(),
            dv.transpose(1, 2).to(v.dtype).contiguous())


def paged_attention_decode(q, k_cache, v_cache, block_tables, context_lens, scale: float):
    """q [N, Hq, D]; caches [num_blocks, block_size, Hkv, D]; block_tables [N, max_blocks]."""
    N, Hq, D = q.shape
    bs = k_cache.shape[1]
    Hkv = k_cache.shape[2]
    rep = Hq // Hkv
    out = torch.empty_like(q)
    for i in range(N):
        L = int(context_lens[i])
        nb = (L + bs - 1) // bs
        blocks = block_tables[i, :nb].long()
        kk = k_cache[blocks].reshape(nb * bs, Hkv, D)[:L].float()
        vv = v_cache[blocks].reshape(nb * bs, Hkv, D)[:L].float()
        kk = kk.repeat_interleave(rep, dim=1)
        vv = vv.repeat_interleave(rep, dim=1)
        s = torch.einsum("hd,lhd->hl", q[i].float(), kk) * scale
        p = torch.softmax(s, dim=-1)
        out[i] = torch.einsum("hl,lhd->hd", p, vv).to(q.dtype)
    return out


def attn_merge_(o_acc, lse_acc, o_j, lse_j) -> None:
    """In-place log-sum-exp merge: o_acc [B,S,H,D] fp32 / lse_acc [B,H,S] fp32 absorb the
    partial (o_j, lse_j); a fresh accumulator is (0, -inf)."""
    ln = torch.logaddexp(lse_acc, lse_j)
    dead = torch.isinf(ln) & (ln < 0)
    wa = torch.where(dead, torch.zeros_like(ln), torch.exp(lse_acc - ln)).transpose(1, 2).unsqueeze(-1)
    wj = torch.where(dead, torch.zeros_like(ln), torch.exp(lse_j - ln)).transpose(1, 2).unsqueeze(-1)
    o_acc.mul_(wa).add_(o_j.float() * wj)
    lse_acc.copy_(ln)


def paged_prefill_attention(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, scale: float):
    """Packed new tokens q [T, Hq, D] of N sequences (rows cu_q[n]:cu_q[n+1]) attending, causally,
    every cached key of their sequence: after the chunk's cache write sequence n holds
    ctx_lens[n] tokens and its new tokens sit at positions ctx - qlen .. ctx - 1."""
    T, Hq, D = q.shape
    bs, Hkv = k_cache.shape[1], k_cache.shape[2]
    rep = Hq // Hkv
    out = torch.empty_like(q)
    cu = [int(x) for x in cu_q]
    for n in range(len(cu) - 1):
        q0, q1 = cu[n], cu[n + 1]
        qlen, L = q1 - q0, int(ctx_lens[n])
        if qlen == 0:
            continue
        nb = (L + bs - 1) // bs
        blocks = block_tables[n, :nb].long()
        kk = k_cache[blocks].reshape(nb * bs, Hkv, D)[:L].float().repeat_interleave(rep, dim=1)
        vv = v_cache[blocks].reshape(nb * bs, Hkv, D)[:L].float().repeat_interleave(rep, dim=1)
        s = torch.einsum("qhd,lhd->hql", q[q0:q1].float(), kk) * scale
        pos = torch.arange(L - qlen, L, device=q.device).view(1, qlen, 1)
        keys = torch.arange(L, device=q.device).view(1, 1, L)
        s = s.masked_fill(keys > pos, float("-inf"))
        out[q0:q1] = torch.einsum("hql,lhd->qhd", torch.softmax(s, dim=-1), vv).to(q.dtype)
    return out


def kv_cache_write(k, v, k_cache, v_cache, slot_mapping):
    """k/v [N, Hkv, D] written at flat slots (block*block_size + offset) of the caches."""
    nb, bs = k_cache.shape[:2]
    kc = k_cache.view(nb * bs, *k_cache.shape[2:])
    vc = v_cache.view(nb * bs, *v_cache.shape[2:])
    idx = slot_mapping.long()
    valid = idx >= 0
    if kc.dtype == torch.float8_e4m3fn:  # saturating, like the kernels (torch's cast maps > 448 to NaN)
        k, v = k.float().clamp(-448.0, 448.0), v.float().clamp(-448.0, 448.0)
    kc[idx[valid]] = k[valid].to(kc.dtype)
    vc[idx[valid]] = v[valid].to(vc.dtype)


# ----------------------------------------------------------------------------- MLP
def swiglu_fwd(gu: torch.Tensor) -> torch.Tensor:
    f = gu.shape[-1] // 2
    g, u = gu[..., :f].float(), gu[..., f:].float()
    return (F.silu(g) * u).to(gu.dtype)


def swiglu_bwd(dact: torch.Tensor, gu: torch.Tensor) -> torch.Tensor:
    f = gu.shape[-1] // 2
    g, u = gu[..., :f].float(), gu[..., f:].float()
    d = dact.float()
    sg = torch.sigmoid(g)
    silu = g * sg
    dg = d * u * (sg * (1 + g * (1 - sg)))
    du = d * silu
    return torch.cat([dg, du], dim=-1).to(gu.dtype)


def gelu_fwd(x: torch.Tensor) -> torch.Tensor:
    return F.gelu(x.float(), approximate="tanh").to(x.dtype)


def gelu_bwd(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    xf = x.float().requires_grad_(True)
    with torch.enable_grad():
        y = F.gelu(xf, approximate="tanh")
        (g,) = torch.autograd.grad(y, xf, dy.float())
    return g.to(x.dtype)


# ----------------------------------------------------------------------------- loss
def cross_entropy_fwd(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100):
    """Per-row loss (fp32, 0 where ignored) and lse (fp32)."""
    lf = logits.float()
    lse = torch.logsumexp(lf, dim=-1)
    valid = labels != ignore_index
    tgt = torch.where(valid, labels, torch.zeros_like(labels)).long()
    picked = lf.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    return loss, lse


def cross_entropy_bwd(dloss: torch.Tensor, logits: torch.Tensor, lse: torch.Tensor, labels: torch.Tensor,
                      ignore_index: int = -100) -> torch.Tensor:
    """dloss per row (fp32) -> dlogits (dtype of logits)."""
    lf = logits.float()
    p = torch.exp(lf - lse.unsqueeze(-1))
    valid = labels != ignore_index
    tgt = torch.where(valid, labels, torch.zeros_like(labels)).long()
    p.scatter_add_(-1, tgt.unsqueeze(-1), -torch.ones_like(p[..., :1]))
    g = p * (dloss * valid.float()).unsqueeze(-1)
    return g.to(logits.dtype)


# ----------------------------------------------------------------------------- optimizer
def adamw_step_(param, master, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
                grad_scale: float = 1.0):
    """Decoupled-weight-decay Adam on an fp32 master copy; writes the bf16 param.  A
    non-finite ``grad_scale`` skips the update (same policy as the HIP kernel)."""
    if not math.isfinite(grad_scale):
        return
    g = grad.float() * grad_scale
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    master.mul_(1 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
    master.addcdiv_(exp_avg, denom, value=-lr / bc1)
    param.copy_(master.to(param.dtype))


def l2norm_sq(t: torch.Tensor) -> torch.Tensor:
    return t.float().pow(2).sum()


# ----------------------------------------------------------------------------- sampling
def sample(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
           uniform: torch.Tensor) -> torch.Tensor:
    """Batched temperature / top-k / top-p sampling driven by caller-supplied uniforms
    (so the kernel and this oracle pick the same token).  temperature<=0 => greedy.

    Semantics (shared with ``csrc/sampling.hip``): x = logits / T; the kept set is
    {x >= max(T_k, T_p)} where T_k is the k-th largest x and T_p the smallest value of the
    minimal descending prefix whose softmax mass reaches top_p; the token is drawn by
    inverse CDF over the kept tokens *in vocabulary order* with r = u * kept_mass."""
    N, V = logits.shape
    out = torch.empty(N, dtype=torch.long, device=logits.device)
    for i in range(N):
        l = logits[i].float()
        t = float(temperature[i])
        if t <= 0:
            out[i] = int(torch.argmax(l))
            continue
        x = l / t
        e = torch.exp(x - x.max())
        thr = -float("inf")
        k = int(top_k[i])
        if 0 < k < V:
            thr = float(torch.topk(x, k).values[-1])
        tp = float(top_p[i])
        if tp < 1.0:
            sx, si = torch.sort(x, descending=True)
            cum = torch.cumsum(e[si], 0)
            n = int(torch.searchsorted(cum, torch.tensor([tp * float(e.sum())], device=cum.device), right=False)[0])
            thr = max(thr, float(sx[min(n, V - 1)]))
        keep = x >= thr
        w = torch.where(keep, e, torch.zeros_like(e))
        cum = torch.cumsum(w, 0)
        r = float(uniform[i]) * float(cum[-1])
        j = int(torch.searchsorted(cum, torch.tensor([r], device=cum.device, dtype=cum.dtype), right=True)[0])
        out[i] = min(j, V - 1)
    return out


TOP_LOGPROBS = 8  # width of the top-logprob outputs of ``sample_ext``


def penalize(logits: torch.Tensor, slot: torch.Tensor, rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor,
             counts: torch.Tensor, prompt_mask: torch.Tensor) -> torch.Tensor:
    """Step 1 of :func:`sample_ext`: the penalized fp32 rows ``x [N, V]`` (``counts`` is only read)."""
    x = logits.float().clone()
    for i in range(x.shape[0]):
        s = int(slot[i])
        if s < 0:
            continue
        c = counts[s]
        xi = x[i]
        seen = (prompt_mask[s] != 0) | (c > 0)
        xi = torch.where(seen, torch.where(xi > 0, xi / rep[i], xi * rep[i]), xi)
        xi = xi - freq[i] * c.float()
        xi = xi - pres[i] * (c > 0).float()
        x[i] = xi
    return x


def sample_ext(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
               uniform: torch.Tensor, slot: torch.Tensor, rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor,
               nlp: torch.Tensor, counts: torch.Tensor, prompt_mask: torch.Tensor):
    """:func:`sample` with repetition / frequency / presence penalties, logprobs and per-sequence
    state; returns ``(tokens int64 [N], logprob f32 [N], top_ids int32 [N, 8], top_lp f32 [N, 8])``
    and MUTATES ``counts``.

    Per row: logits ``l [V]`` (bf16 or fp32), a state slot ``s`` (``-1``: no state, no penalties,
    no update), ``rep > 0``, ``freq``, ``pres`` (fp32) and ``nlp`` in 0..8.  The state is ``counts
    int32 [S, V]`` (occurrences among the generated tokens) and ``prompt_mask uint8 [S, V]`` (the
    token occurs in the prompt).  Semantics (shared with ``csrc/sampling.hip``):

    1. ``x = float(l)``; for a row with ``s >= 0``, in fp32 and in exactly this order:
       a. if ``prompt_mask[s, v] or counts[s, v] > 0``: ``x = x / rep if x > 0 else x * rep``;
       b. ``x = x - freq * counts[s, v]``;
       c. ``x = x - pres * (counts[s, v] > 0)``
       (the HF / vLLM convention: repetition sees prompt and output, frequency and presence the
       output only);
    2. the token is drawn from ``x`` by the rule of :func:`sample` (temperature, top-k, top-p, the
       caller's uniform, greedy at ``T <= 0``, lowest index on ties), with the arithmetic of
       ``sample`` on an fp32 row holding ``x``;
    3. ``logprob = x[tok] - logsumexp(x)``: after the penalties, before the temperature (the
       logsumexp is taken in fp64 here and returned as fp32);
    4. the ``nlp`` largest ``x`` as ``(id, x - logsumexp)`` in descending order, ties to the lowest
       index; entries past ``nlp`` hold id ``-1`` and logprob ``-inf``;
    5. for a row with ``s >= 0``: ``counts[s, tok] += 1``, after everything above.  No two rows of
       a call may share a slot."""
    N, V = logits.shape
    x = penalize(logits, slot, rep, freq, pres, counts, prompt_mask)
    toks = sample(x, temperature, top_k, top_p, uniform)
    lp = x.double() - torch.logsumexp(x.double(), dim=1, keepdim=True)
    logprob = lp.gather(1, toks.view(N, 1)).view(N).float()
    top_ids = torch.full((N, TOP_LOGPROBS), -1, dtype=torch.int32, device=logits.device)
    top_lp = torch.full((N, TOP_LOGPROBS), -float("inf"), dtype=torch.float32, device=logits.device)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices  # stable: lowest index first on ties
    for i in range(N):
        k = min(max(int(nlp[i]), 0), TOP_LOGPROBS, V)
        top_ids[i, :k] = order[i, :k].to(torch.int32)
        top_lp[i, :k] = lp[i, order[i, :k]].float()
        s = int(slot[i])
        if s >= 0:
            counts[s, int(toks[i])] += 1
    return toks, logprob, top_ids, top_lp


def prompt_logprobs(logits: torch.Tensor, target: torch.Tensor, nlp: torch.Tensor):
    """Score every row of ``logits [R, V]`` (bf16 or fp32, finite) against ``target int64 [R]``;
    returns ``(logprob f32 [R], rank int32 [R], top_ids int32 [R, 8], top_lp f32 [R, 8])``.
    Semantics (shared with ``csrc/prompt_logprobs.hip``), in fp64 internally:

    1. ``logprob[r] = x[r, target[r]] - logsumexp(x[r])`` over the raw row;
    2. ``rank[r]``: the 1-based position of the target in the row's stable descending order (larger
       value first, lower index on ties -- the order of :func:`sample_ext`'s lists), so ``rank <=
       nlp`` exactly when the target is listed;
    3. the first ``nlp[r]`` (0..8, at most V) entries of that order as ``(id, logprob)``; the rest
       of the lists hold id ``-1`` and logprob ``-inf``.  A listed target's entry equals
       ``logprob[r]`` bit for bit;
    4. ``target[r]`` outside ``0..V-1``: ``logprob = NaN``, ``rank = 0``; the lists are produced."""
    R, V = logits.shape
    dev = logits.device
    x = logits.double()
    lp = x - torch.logsumexp(x, dim=1, keepdim=True)
    t = target.to(dev).long()
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1).view(R, 1)
    xt = x.gather(1, tc)
    idx = torch.arange(V, device=dev).view(1, V)
    ahead = ((x > xt) | ((x == xt) & (idx < tc))).sum(dim=1)
    logprob = torch.where(ok, lp.gather(1, tc).view(R).float(), torch.full((R,), float("nan"), device=dev))
    rank = torch.where(ok, ahead + 1, torch.zeros_like(ahead)).to(torch.int32)
    W = min(TOP_LOGPROBS, V)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :W]  # stable: lowest index first on ties
    keep = torch.arange(W, device=dev).view(1, W) < nlp.to(dev).long().clamp(0, TOP_LOGPROBS).view(R, 1)
    top_ids = torch.full((R, TOP_LOGPROBS), -1, dtype=torch.int32, device=dev)
    top_lp = torch.full((R, TOP_LOGPROBS), -float("inf"), dtype=torch.float32, device=dev)
    top_ids[:, :W] = torch.where(keep, order, torch.full_like(order, -1)).to(torch.int32)
    top_lp[:, :W] = torch.where(keep, lp.gather(1, order).float(), top_lp[:, :W])
    return logprob, rank, top_ids, top_lp


def guide_mask(guide: torch.Tensor, gslot: torch.Tensor, guide_cls: torch.Tensor, guide_next: torch.Tensor,
               guide_meta: torch.Tensor, guide_state: torch.Tensor) -> torch.Tensor:
    """bool [N, V]: the tokens each row's guide allows in its current state (all True for a row
    with ``guide = -1``)."""
    N, V = guide.shape[0], guide_cls.shape[1]
    ok = torch.ones(N, V, dtype=torch.bool, device=guide_cls.device)
    for i in range(N):
        g = int(guide[i])
        if g < 0:
            continue
        C = int(guide_meta[g, 1])
        st = int(guide_state[int(gslot[i])])
        ok[i] = guide_next[g, st * C:(st + 1) * C][guide_cls[g].long()] >= 0
    return ok


def sample_guided(logits: torch.Tensor, temperature: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                  uniform: torch.Tensor, slot: torch.Tensor, rep: torch.Tensor, freq: torch.Tensor, pres: torch.Tensor,
                  nlp: torch.Tensor, counts: torch.Tensor, prompt_mask: torch.Tensor, guide: torch.Tensor,
                  gslot: torch.Tensor, guide_cls: torch.Tensor, guide_next: torch.Tensor, guide_meta: torch.Tensor,
                  guide_state: torch.Tensor, draw_dtype: torch.dtype = torch.float32):
    """:func:`sample_ext` with a token-class automaton per guided row; returns the same four
    tensors and MUTATES ``counts`` and ``guide_state``.

    Per row: ``guide`` (a table slot, ``-1``: unguided) and ``gslot`` (the row's word of
    ``guide_state int32 [Sg]``: its current automaton state; ``-1`` with ``guide = -1``).  Table slot
    ``g`` is ``guide_cls[g] int32 [V]`` (the class of every token), ``guide_next[g] int32 [W]``
    holding ``next[s * C_g + c]`` (``-1``: not allowed) and ``guide_meta[g] = (S_g, C_g)``.
    Semantics (shared with ``csrc/sampling.hip``):

    1. ``x`` = the penalized row of :func:`sample_ext`; for a guided row in state ``s``, ``x[v] =
       -inf`` wherever ``next[s * C + cls[v]] < 0``.  Every state of a well-formed guide allows at
       least one token;
    2. the token is drawn from ``x`` by the rule of :func:`sample` with the masked entries never
       kept: the top-k and top-p cut-offs are taken over the allowed tokens (the k-th largest
       allowed value; the minimal descending prefix reaching ``top_p`` of the allowed mass), and
       -- ONE CORRECTION to :func:`sample` -- an inverse-CDF result past the end (``r`` at the very
       top, by rounding) is clamped to the last *kept* entry, not to ``V - 1``, which may be masked;
    3. ``logprob`` and the top lists as in :func:`sample_ext`, over the masked row: the logprobs are
       renormalised over the allowed set, ``-inf`` entries are never listed, and with fewer allowed
       tokens than ``nlp`` the remaining entries are ``(-1, -inf)``;
    4. ``counts[slot, tok] += 1`` as in :func:`sample_ext`, then for a guided row ``guide_state[gslot] =
       next[s * C + cls[tok]]`` (left alone if negative, which a well-formed guide cannot give).
       No two rows of a call share a ``gslot``; they may share a ``guide``.

    ``draw_dtype``: the arithmetic of step 2 (fp32 as the kernel; fp64 to see how far summation
    order can move an inverse-CDF boundary)."""
    N, V = logits.shape
    x = penalize(logits, slot, rep, freq, pres, counts, prompt_mask)
    ok = guide_mask(guide, gslot, guide_cls, guide_next, guide_meta, guide_state)
    x = torch.where(ok, x, torch.full_like(x, -float("inf")))
    toks = torch.empty(N, dtype=torch.long, device=logits.device)
    for i in range(N):
        l = x[i].to(draw_dtype)
        t = float(temperature[i])
        if t <= 0:
            toks[i] = int(torch.argmax(l))
            continue
        xs = l / t
        e = torch.exp(xs - xs.max())
        thr = -float("inf")
        k = int(top_k[i])
        if 0 < k < V:
            thr = float(torch.topk(xs, k).values[-1])
        tp = float(top_p[i])
        if tp < 1.0:
            sx, si = torch.sort(xs, descending=True)
            cum = torch.cumsum(e[si], 0)
            n = int(torch.searchsorted(cum, torch.tensor([tp * float(e.sum())], device=cum.device, dtype=cum.dtype),
                                       right=False)[0])
            thr = max(thr, float(sx[min(n, V - 1)]))
        keep = (xs >= thr) & torch.isfinite(xs)
        cum = torch.cumsum(torch.where(keep, e, torch.zeros_like(e)), 0)
        r = float(uniform[i].to(draw_dtype)) * float(cum[-1])
        j = int(torch.searchsorted(cum, torch.tensor([r], device=cum.device, dtype=cum.dtype), right=True)[0])
        toks[i] = j if j < V else int(keep.nonzero()[-1])
    lp = x.double() - torch.logsumexp(x.double(), dim=1, keepdim=True)
    logprob = lp.gather(1, toks.view(N, 1)).view(N).float()
    top_ids = torch.full((N, TOP_LOGPROBS), -1, dtype=torch.int32, device=logits.device)
    top_lp = torch.full((N, TOP_LOGPROBS), -float("inf"), dtype=torch.float32, device=logits.device)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    for i in range(N):
        k = min(max(int(nlp[i]), 0), TOP_LOGPROBS, int(torch.isfinite(x[i]).sum()))
        top_ids[i, :k] = order[i, :k].to(torch.int32)
        top_lp[i, :k] = lp[i, order[i, :k]].float()
        s = int(slot[i])
        if s >= 0:
            counts[s, int(toks[i])] += 1
        g = int(guide[i])
        if g >= 0:
            C = int(guide_meta[g, 1])
            gs = int(gslot[i])
            nxt = int(guide_next[g, int(guide_state[gs]) * C + int(guide_cls[g, int(toks[i])])])
            if nxt >= 0:
                guide_state[gs] = nxt
    return toks, logprob, top_ids, top_lp


def sampler_state_reset(counts: torch.Tensor, prompt_mask: torch.Tensor, slot: int, prompt_ids, output_ids) -> None:
    """Slot ``slot`` of the ``sample_ext`` state as it stands after ``prompt_ids`` were given and
    ``output_ids`` generated: both rows zeroed, then the prompt's tokens marked and the generated
    ones counted."""
    counts[slot].zero_()
    prompt_mask[slot].zero_()
    d = counts.device
    if len(prompt_ids):
        prompt_mask[slot].index_fill_(0, torch.as_tensor(list(prompt_ids), dtype=torch.long).to(d), 1)
    if len(output_ids):
        idx = torch.as_tensor(list(output_ids), dtype=torch.long).to(d)
        counts[slot].index_add_(0, idx, torch.ones(len(output_ids), dtype=counts.dtype, device=d))


# ----------------------------------------------------------------------------- int4 decode weights
def dequant_int4_g128(qweight: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 ``[N, K]`` image of a group-128 int4 weight (``quantizers.quantize_int4_g128``):
    ``qweight`` uint8 ``[N, K/2]``, byte ``j`` = ``u[2j] | u[2j+1] << 4`` with ``u = q + 8`` in
    0..15; ``scale`` fp32 ``[N, K/128]``; ``w[n, k] = (u[n, k] - 8) * scale[n, k // 128]``."""
    N, K = qweight.shape[0], qweight.shape[1] * 2
    if qweight.dtype != torch.uint8 or K % 128 or tuple(scale.shape) != (N, K // 128):
        raise ValueError(f"dequant_int4_g128: need uint8 [N, K/2] and scales [N, K/128], got "
                         f"{qweight.dtype} {tuple(qweight.shape)} and {tuple(scale.shape)}")
    p = qweight.to(torch.int16)
    u = torch.stack([p & 0xF, p >> 4], dim=2).reshape(N, K)
    return (u - 8).float() * scale.float().repeat_interleave(128, dim=1)


def decode_linear_int4(x, qweight, scale, b=None) -> torch.Tensor:
    """fp32 ``x @ dequant(W)^T (+ b)``: the spec of the int4 decode projection."""
    y = x.float() @ dequant_int4_g128(qweight, scale).t()
    return y if b is None else y + b.float()


# ----------------------------------------------------------------------------- routed-expert decode MLP
def moe_route(x: torch.Tensor, w_router: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k routing of ``x [M, h]`` over ``w_router [E, h]``: ``(topi int32 [M, k], topw fp32 [M, k])``.

    The model's definition (``MoEMLP.forward``): the logits are ``linear(x, w_router)`` -- fp32
    accumulation rounded to the activation dtype (bf16 on the GPU) -- then softmax in fp32, the k
    largest probabilities in descending order, weights renormalised over the picks.  On equal
    probabilities the lowest expert index wins (a stable descending sort; ``torch.topk`` leaves the
    tie order unspecified)."""
    logits = (x.float() @ w_router.float().t()).to(x.dtype).float()
    probs = logits.softmax(-1)
    vals, idx = torch.sort(probs, dim=-1, descending=True, stable=True)
    topw = vals[:, :k]
    return idx[:, :k].to(torch.int32), topw / topw.sum(-1, keepdim=True)


def moe_decode_up_swiglu(x, experts_up, topi) -> torch.Tensor:
    """fp32 ``act [M k, F]``: row ``t k + j`` = ``silu(g) * u`` of ``x[t] @ experts_up[topi[t, j]]^T``
    (each ``[2F, h]``, gate rows first)."""
    M, k = topi.shape
    F_ = experts_up[0].shape[0] // 2
    flat = topi.reshape(-1).long()
    xf = x.float()
    act = torch.zeros(M * k, F_, dtype=torch.float32, device=x.device)
    for e, w in enumerate(experts_up):
        c = (flat == e).nonzero().flatten()
        if c.numel():
            gu = xf[torch.div(c, k, rounding_mode="floor")] @ w.float().t()
            act[c] = F.silu(gu[:, :F_]) * gu[:, F_:]
    return act


def moe_decode_down_add_rmsnorm(act, experts_down, topi, topw, residual, norm_w, eps: float):
    """fp32 ``(xn, res_out)``: ``res_out[t] = sum_j topw[t, j] act[t k + j] @ experts_down[topi[t, j]]^T
    + residual[t]`` (slot order), ``xn = rmsnorm(res_out) * norm_w``."""
    M, k = topi.shape
    flat = topi.reshape(-1).long()
    af = act.float()
    d = torch.zeros(M * k, experts_down[0].shape[0], dtype=torch.float32, device=act.device)
    for e, w in enumerate(experts_down):
        c = (flat == e).nonzero().flatten()
        if c.numel():
            d[c] = af[c] @ w.float().t()
    d = d.view(M, k, -1)
    y = torch.zeros_like(d[:, 0])
    for j in range(k):
        y = y + topw[:, j].float().unsqueeze(-1) * d[:, j]
    s = y + residual.float()
    xn = s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps) * norm_w.float()
    return xn, s


def moe_decode_mlp(x, experts_up, experts_down, topi, topw, residual, norm_w, eps: float):
    """The whole routed MLP of a decode step in fp32 with no intermediate rounding: expert SwiGLU
    MLPs of the routed copies, weighted combine, residual add and RMSNorm -> ``(xn, res_out)``."""
    act = moe_decode_up_swiglu(x, experts_up, topi)
    return moe_decode_down_add_rmsnorm(act, experts_down, topi, topw, residual, norm_w, eps)


# ----------------------------------------------------------------------------- per-row LoRA adapters
def lora_delta(x, lora_idx, lora_a, lora_b, lora_scale) -> torch.Tensor:
    """``delta[m, n] = scale[s] * sum_j (sum_k x[m, k] A[s, j, k]) B[s, n, j]`` with ``s = lora_idx[m]``;
    rows with ``s < 0`` are exact zeros.  ``lora_a [slots, R, K]``, ``lora_b [slots, N, R]``,
    ``lora_scale [slots]``.  fp32 throughout, the inner sum not rounded (fp64 inputs: fp64)."""
    dt = torch.float64 if x.dtype == torch.float64 else torch.float32
    M, N = x.shape[0], lora_b.shape[1]
    out = torch.zeros(M, N, dtype=dt, device=x.device)
    idx = lora_idx.long()
    for s in range(lora_a.shape[0]):
        rows = (idx == s).nonzero().flatten()
        if rows.numel():
            t = x[rows].to(dt) @ lora_a[s].to(dt).t()
            out[rows] = lora_scale[s].to(dt) * (t @ lora_b[s].to(dt).t())
    return out
