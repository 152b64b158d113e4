"""A numpy model of a verification step under sampling and a repetition penalty (`lookup_sampling=True`; csrc/decode.hip:
lm_pick_verify_kernel, lm_lookup_step_mark_kernel), with the defects such kernels and their host loop can have as switches:

  penalised(V, seen, drafts, r)     how often the penalty is applied to each id in row r of a step: once for the members of
                                    seen U {drafts[i] : i < r, 0 <= drafts[i] < V}, never otherwise (rgn_lm_pick_verify's map rule)
  pick_verify(...)                  the R processed score rows, greedy tokens and the map afterwards (which the pick never writes)
  marks(seen, seq, n, a, R, V)      the map after rgn_lm_lookup_step_mark: seen U seq[n .. n + a], ids outside [0, V) ignored
  replay(lm, prompt, u, ...)        a drafted sampled generate over a toy language model whose pick at new-token position k is a function
                                    of (the previous token, the map, u[k]): the token run and the stats the loop reports, against
  plain(lm, prompt, u, T)           the one-token-a-step loop: the run every drafted generate must equal

The layout is the kernels': `seq` is ONE run of ids (prompt, then new tokens); seq[0, n) is settled, seq[n - 1] was row 0 of the step,
seq[n, n + R - 1) are the drafts that were rows 1..R-1.  Not a model of transformers and not bit-exact to the kernels' sums: the GPU tests
compare the kernels with rgn_lm_pick itself; this file says WHICH ids, WHICH uniform and WHICH marks."""
import numpy as np

DEFECTS = ("sees_own_draft", "misses_last_draft", "repeat_twice", "seen_and_draft_twice", "marks_rejected", "own_token_unmarked",
           "uniform_from_zero", "pick_writes_seen")


# ---- the map rule -----------------------------------------------------------------------------------------------------------------------
def penalised(V, seen, drafts, r, defect=None):
    """int [V]: the number of applications of the penalty per id in row r (the rule: 0 or 1)."""
    seen = np.asarray(seen).astype(np.int64)
    upto = r + 1 if defect == "sees_own_draft" else max(r - 1, 0) if defect == "misses_last_draft" else r
    hits = np.zeros(V, dtype=np.int64)
    for t in list(drafts)[:upto]:
        if 0 <= int(t) < V:
            hits[int(t)] += 1
    if defect == "repeat_twice":
        return np.maximum(seen, hits)
    if defect == "seen_and_draft_twice":
        return seen + (hits > 0)
    return np.maximum(seen, (hits > 0).astype(np.int64))


def penalise(z, times, penalty):
    """transformers' RepetitionPenaltyLogitsProcessor in fp32, `times[v]` applications on id v."""
    s = np.asarray(z, dtype=np.float32).copy()
    p = np.float32(penalty)
    for _ in range(int(times.max()) if times.size else 0):
        on = times > 0
        s[on] = np.where(s[on] < 0, s[on] * p, s[on] / p).astype(np.float32)
        times = times - on
    return s


def pick_verify(z, seen, drafts, penalty, defect=None):
    """(scores [R, V] fp32, greedy tokens [R], the map afterwards) of one rgn_lm_pick_verify call with sample = 0 over z [R, V]."""
    z = np.asarray(z, dtype=np.float32)
    R, V = z.shape
    after = np.asarray(seen).astype(np.uint8).copy()
    scores = np.stack([penalise(z[r], penalised(V, seen, drafts, r, defect), penalty) for r in range(R)])
    toks = [int(np.argmax(scores[r])) for r in range(R)]                       # the lowest index among equal values
    if defect == "pick_writes_seen":
        after[toks] = 1
    return scores, toks, after


def probe(V=16):
    """The exact probe of the map rule: logits of 8.0 (odd ids) and -8.0 (even ids), so both branches of the penalty are met, with
    penalty 2, where one application gives 4.0 / -16.0 and two give 2.0 / -32.0 exactly.  R = 9 rows over the drafts
    [1, 3, 3, 5, 4, 6, -1, V] with ids 5, 6 and 9 already seen: the argmax of row 0 (1) and of row 1 (3) drafted, so the penalty moves
    the next row's token; a duplicate (3, 3); ids both seen and drafted (5, 6); ids outside the vocabulary.
    Returns (z [R, V], seen [V] uint8, drafts [R - 1], penalty)."""
    R = 9
    z = np.where(np.arange(V) % 2 == 0, -8.0, 8.0).astype(np.float32)
    z = np.tile(z, (R, 1))
    seen = np.zeros(V, dtype=np.uint8)
    seen[[5, 6, 9]] = 1
    return z, seen, [1, 3, 3, 5, 4, 6, -1, V], 2.0


# Hand-computed for probe(16): the ids row r is penalised for (once each), and its greedy token - the lowest odd id left at 8.0
PROBE_MEMBERS = [[5, 6, 9], [1, 5, 6, 9], [1, 3, 5, 6, 9], [1, 3, 5, 6, 9], [1, 3, 5, 6, 9], [1, 3, 4, 5, 6, 9], [1, 3, 4, 5, 6, 9],
                 [1, 3, 4, 5, 6, 9], [1, 3, 4, 5, 6, 9]]
PROBE_TOKENS = [1, 3, 7, 7, 7, 7, 7, 7, 7]


def probe_holds(defect=None):
    z, seen, drafts, pen = probe()
    scores, toks, after = pick_verify(z, seen, drafts, pen, defect)
    want = z.copy()
    for r, ids in enumerate(PROBE_MEMBERS):
        want[r, ids] = np.where(z[r, ids] < 0, -16.0, 4.0)
    return bool(np.array_equal(scores, want)) and toks == PROBE_TOKENS and bool(np.array_equal(after, seen))


# ---- the marks --------------------------------------------------------------------------------------------------------------------------
def marks(seen, seq, n, a, R, V, defect=None):
    """The map after the step: seq[n .. n + a] (the a accepted drafts and the step's own token, already written at seq[n + a])."""
    out = np.asarray(seen).astype(np.uint8).copy()
    ids = [int(t) for t in seq[n:n + a + 1]]
    if defect == "marks_rejected":                                               # every draft still in the run, and the own token
        ids = [int(t) for t in seq[n:n + R - 1]] + [int(seq[n + a])]
    if defect == "own_token_unmarked":
        ids = [int(t) for t in seq[n:n + a]]
    for t in ids:
        if 0 <= t < V:
            out[t] = 1
    return out


# Hand-computed: (name, seen ids, seq, n, a, R, V, the ids set afterwards)
MARK_CASES = [
    ("nothing accepted: the own token alone", [1], [1, 2, 7, 8, 9], 2, 0, 3, 16, [1, 7]),      # seq[2] = 7 is the pick; 8, 9 rejected
    ("two of three accepted", [0], [0, 4, 5, 6, 7], 1, 2, 4, 16, [0, 4, 5, 6]),                 # seq[3] = 6 replaced the third draft
    ("all accepted", [], [3, 4, 5, 6], 1, 2, 3, 16, [4, 5, 6]),
    ("one row", [2], [2, 9], 1, 0, 1, 16, [2, 9]),
    ("ids outside the vocabulary mark nothing", [], [1, 16, -1, 3, 99], 1, 2, 4, 16, [3]),       # 16 and -1 accepted, 3 the own token
]


def mark_case_holds(c, defect=None):
    name, ids, seq, n, a, R, V, want = c
    seen = np.zeros(V, dtype=np.uint8)
    seen[ids] = 1
    return sorted(np.flatnonzero(marks(seen, seq, n, a, R, V, defect)).tolist()) == sorted(want)


# ---- a position-indexed replay ----------------------------------------------------------------------------------------------------------
def toy_lm(V=12, seed=0):
    """pick(prev, k, seen, u) -> token: logits that depend on the previous token and the position, the penalty 1.5 over `seen`,
    temperature 1, then the inverse CDF of the softmax at u in fp64 - deterministic given (logits row, map, uniform)."""
    def pick(prev, k, seen, u):
        z = np.random.default_rng([seed, int(prev), int(k)]).normal(0, 2, V).astype(np.float32)
        s = penalise(z, np.asarray(seen).astype(np.int64), 1.5).astype(np.float64)
        p = np.exp(s - s.max())
        c = np.cumsum(p)
        return int(min(np.searchsorted(c, u * c[-1], side="right"), V - 1))
    pick.V = V
    return pick


def _seen_of(ids, V):
    seen = np.zeros(V, dtype=np.uint8)
    for t in ids:
        if 0 <= int(t) < V:
            seen[int(t)] = 1
    return seen


def plain(lm, prompt, u, T):
    """The plain sampled loop: new token k is picked under the map of the prompt and new tokens 0..k-1, with u[k]."""
    seen, prev, out = _seen_of(prompt, lm.V), prompt[-1], []
    for k in range(T):
        prev = lm(prev, k, seen, u[k])
        seen[prev] = 1
        out.append(prev)
    return out


def replay(lm, prompt, u, guess, K, T, defect=None):
    """The drafted loop under a caller's guess of the continuation: (tokens, dict(steps, drafted, accepted, tokens))."""
    V, L = lm.V, len(prompt)
    seq = [int(t) for t in prompt] + [0] * T
    seen = _seen_of(prompt, V)
    guess = [int(t) for t in guess]

    def step(n, R, k):
        """Rows 0..R-1 at settled length n (k new tokens settled): picks, accept, the own token, the marks."""
        nonlocal seen
        drafts = seq[n:n + R - 1]
        heads = []
        for r in range(R):
            m = penalised(V, seen, drafts, r, defect if defect in DEFECTS[:4] else None)
            heads.append(lm(seq[n - 1 + r], k + r, m, u[r] if defect == "uniform_from_zero" else u[k + r]))
        if defect == "pick_writes_seen":
            seen[heads] = 1
        a = 0
        while a < R - 1 and seq[n + a] == heads[a]:
            a += 1
        seq[n + a] = heads[a]
        seen = marks(seen, seq, n, a, R, V, defect if defect in ("marks_rejected", "own_token_unmarked") else None)
        return a

    step(L, 1, 0)                                                                # the prefill's pick: a step of one row
    k, steps, drafted, accepted = 1, 0, 0, 0
    while k < T:
        kd = len(guess[k:k + max(0, min(K, T - k - 1))])
        seq[L + k:L + k + kd] = guess[k:k + kd]
        a = step(L + k, kd + 1, k)
        steps, drafted, accepted, k = steps + 1, drafted + kd, accepted + a, k + a + 1
    return seq[L:L + T], dict(steps=steps, drafted=drafted, accepted=accepted, tokens=k)
