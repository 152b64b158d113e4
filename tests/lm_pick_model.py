"""The fp64 model of rgn_lm_pick (csrc/decode.hip), plain torch on the CPU: what the new sampling tests compare the kernel and `generate`
against.  The stages transformers computes in fp32 (the repetition penalty, the division by the temperature, the top-k mask) are computed
in fp32 here too, with the same torch expressions, so they can be compared bit for bit with the installed processors; the softmax masses,
the top-p threshold and the CDF of the draw are fp64.

Top-p treats equal scores as ONE group, judged by the mass up to and including all of them (TopPLogitsWarper's sort splits a group that
straddles the boundary; the kernel and this model keep all of it).  `group_mass` returns that cumulative mass per token, so a test can
tell which tokens lie within a rounding bound of the threshold 1 - top_p."""
import math

import torch


def seen_mask(V, ids):
    m = torch.zeros(V, dtype=torch.bool)
    m[torch.as_tensor(ids, dtype=torch.int64).flatten()] = True
    return m


def scores_before_top_p(z, seen, penalty=1.0, sample=False, temperature=1.0, top_k=0):
    """fp32 [V]: the penalty over the bool map `seen`, then (sampling only) the temperature and the top-k mask."""
    s = z.detach().float().cpu().clone()
    if penalty != 1.0:
        t = s[seen]
        s[seen] = torch.where(t < 0, t * penalty, t / penalty)
    if not sample:
        return s
    s = s / temperature
    if top_k and top_k < s.numel():
        kth = torch.topk(s, top_k)[0][-1]
        s = s.masked_fill(s < kth, -math.inf)
    return s


def group_mass(s):
    """fp64 [V]: for every token the softmax mass of all tokens whose score is <= its own (equal scores included); 0 mass for -inf."""
    p = torch.softmax(s.double(), 0)
    vals, order = torch.sort(s.double())
    c = p[order].cumsum(0)
    _, inverse, counts = torch.unique_consecutive(vals, return_inverse=True, return_counts=True)
    ends = counts.cumsum(0) - 1
    out = torch.empty_like(c)
    out[order] = c[ends][inverse]
    return out


def top_p_keep(s, top_p):
    """bool [V]: what TopPLogitsWarper(top_p, min_tokens_to_keep=1) keeps, groups of equal scores taken whole."""
    if top_p >= 1.0:
        return s > -math.inf
    keep = group_mass(s) > 1.0 - top_p
    keep[s == s.max()] = True                                                    # the largest is never dropped
    return keep & (s > -math.inf)


def cdf(s, keep):
    """(kept indices ascending, fp64 cumulative q over them): q = softmax over the kept tokens."""
    idx = torch.nonzero(keep).flatten()
    q = torch.softmax(s.double()[idx], 0)
    return idx, q.cumsum(0)


def draw(idx, C, us):
    """int64 [len(us)]: per uniform the lowest kept index whose cumulative q exceeds u; the last kept token if none does."""
    j = torch.searchsorted(C, torch.as_tensor(us).double().flatten(), right=True).clamp(max=idx.numel() - 1)
    return idx[j]


def pick(z, seen, penalty=1.0, sample=False, temperature=1.0, top_k=0, top_p=1.0, us=None):
    """Everything at once: dict(scores fp32 [V] with -inf where filtered, keep, idx, C, tokens)."""
    s = scores_before_top_p(z, seen, penalty, sample, temperature, top_k)
    if not sample:
        first = int(torch.nonzero(s == s.max())[0])
        return dict(scores=s, keep=torch.ones_like(s, dtype=torch.bool), idx=None, C=None, tokens=torch.tensor([first]))
    keep = top_p_keep(s, top_p)
    idx, C = cdf(s, keep)
    return dict(scores=s.masked_fill(~keep, -math.inf), keep=keep, idx=idx, C=C, tokens=None if us is None else draw(idx, C, us),
                before_top_p=s)
