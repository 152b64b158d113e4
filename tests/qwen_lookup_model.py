"""A numpy model of rgn_lm_lookup_step (csrc/decode.hip: lm_lookup_step_kernel) - the end of a generate step that carried drafted tokens:
accept the drafts the argmaxes confirm, write the token after them, propose the next drafts - with the defects such a kernel can have as
switches, the hand-computed cases that tell each defect from the rule, and a host simulation of the speculative loop under a caller's
guess (the step / accepted counts a generate must report).

The layout is the kernel's: `seq` is ONE run of ids (prompt, then new tokens); seq[0, n) is settled, seq[n - 1] was row 0 of the step,
seq[n, n + R - 1) are the R - 1 drafts that were rows 1..R-1, head[r] is the argmax after row r.  `limit` is the end of the run."""
import numpy as np

DEFECTS = ("highest_match", "trailing_self_match", "no_end_clip", "small_ngram_first", "later_coincidence", "no_bonus", "clamp_off_by_one")


def accept(seq, n, head, defect=None):
    """a = the number of leading drafts that equal the argmax before them: the FIRST mismatch ends the run."""
    R = len(head)
    if defect == "later_coincidence":                                            # counts up to the LAST coincidence
        hits = [i for i in range(R - 1) if seq[n + i] == head[i]]
        return hits[-1] + 1 if hits else 0
    a = 0
    while a < R - 1 and seq[n + a] == head[a]:
        a += 1
    return a


def propose(seq, n1, kcap, max_ngram, defect=None):
    """transformers' PromptLookupCandidateGenerator over seq[0, n1): the draft ids (possibly none)."""
    if kcap <= 0:
        return []
    top = min(max_ngram, n1 - 1)
    sizes = range(1, top + 1) if defect == "small_ngram_first" else range(top, 0, -1)
    for size in sizes:
        run = np.asarray(seq[:n1])
        same = np.ones(n1 - size + 1, dtype=bool)                                # window i equals the trailing n-gram
        for j in range(size):
            same &= run[j:j + n1 - size + 1] == run[n1 - size + j]
        hits = [int(i) for i in np.flatnonzero(same)]
        for idx in (reversed(hits) if defect == "highest_match" else hits):
            start = idx + size
            end = start + kcap if defect == "no_end_clip" else min(start + kcap, n1)
            if start < end or (defect == "trailing_self_match" and start == n1):
                if start == n1:                                                  # the defect: whatever lies past the settled run
                    end = start + kcap
                return [int(v) for v in seq[start:end]]
    return []


def step(seq, n, head, limit, K, max_ngram=2, guess=None, L=0, defect=None):
    """One call of the kernel on a copy of `seq`: returns (a, drafts, accepted tokens, seq after the call)."""
    seq = np.array(seq, dtype=np.int64).copy()
    head = [int(h) for h in head]
    a = accept(seq, n, head, defect)
    if defect != "no_bonus":
        seq[n + a] = head[a]
    n1 = n + a + 1
    kcap = max(0, min(K, limit - n1 - (0 if defect == "clamp_off_by_one" else 1)))
    if guess is not None:
        at = n1 - L
        drafts = [int(v) for v in list(guess)[at:at + kcap]] if at >= 0 else []
    else:
        drafts = propose(seq, n1, kcap, max_ngram, defect)
    room = len(seq) - n1
    drafts = drafts[:max(room, 0)]
    seq[n1:n1 + len(drafts)] = drafts
    return a, drafts, head[:a + 1], seq


def _case(name, settled, drafts, head, limit, K, max_ngram, want_a, want_drafts, guess=None, L=0, pad=8):
    """seq = settled ids, the step's drafts, then `pad` ids of 777 (what a defect that reads past the run would pick up)."""
    seq = list(settled) + list(drafts)
    seq = seq + [777] * (max(limit, len(seq) + 1) - len(seq) + pad)
    return dict(name=name, seq=seq, n=len(settled), head=list(head), limit=limit, K=K, max_ngram=max_ngram, guess=guess, L=L,
                want_a=want_a, want_drafts=list(want_drafts))


# Hand-computed: every `want` below was worked out from the rule on paper, not by running this file.
CASES = [
    # [5,6,7,5,6,8,5] + 6: the 2-gram (5,6) sits at 0, 3 and 6 (itself); the lowest, 0, continues with 7, 5
    _case("lowest of several matches", [5, 6, 7, 5, 6, 8, 5], [], [6], 100, 2, 2, 0, [7, 5]),
    # [1,2,3,4] + 9: (4,9) and (9) match only themselves, and the continuation of the trailing n-gram is empty
    _case("only the trailing match", [1, 2, 3, 4], [], [9], 100, 3, 2, 0, []),
    # [3,4,3] + 4: (3,4) at 0 continues at 2, and only 2 ids are left before the end although K = 5
    _case("continuation cut by the end", [3, 4, 3], [], [4], 100, 5, 2, 0, [3, 4]),
    # [2,7,1,2,9,1] + 2: the 2-gram (1,2) at 2 continues with 9; the 1-gram (2) at 0 would continue with 7
    _case("a larger n-gram beats a smaller one", [2, 7, 1, 2, 9, 1], [], [2], 100, 1, 2, 0, [9]),
    # drafts 10, 11, 12 against argmaxes 10, 99, 12: the second draft is wrong, the third coincidence does not count; 99 is written
    _case("the first mismatch decides", [1, 2, 3, 4], [10, 11, 12], [10, 99, 12, 13], 100, 3, 2, 1, []),
    # the bonus token takes part in the lookup: [8,9,8] with draft 5 refused for 9 -> [8,9,8,9]: (8,9) at 0 continues with 8, 9
    _case("the bonus token is written", [8, 9, 8], [5], [9, 4], 100, 2, 2, 0, [8, 9]),
    _case("every draft accepted", [1, 2, 3], [4, 5, 6], [4, 5, 6, 7], 100, 3, 2, 3, []),
    # [5,5,5,5] + 5 = five 5s, n' = 5: limit - n' = 2 leaves room for ONE draft (the step's own token comes after it)
    _case("the clamp at limit - n' = 2", [5, 5, 5, 5], [], [5], 7, 3, 2, 0, [5]),
    _case("the clamp at limit - n' = 1", [5, 5, 5, 5], [], [5], 6, 3, 2, 0, []),
    _case("the clamp at limit - n' = 0", [5, 5, 5, 5], [], [5], 5, 3, 2, 0, []),
    # guess mode, L = 2: after the step 2 new tokens are settled, so the drafts are guess[2], guess[3]
    _case("a guess of the continuation", [1, 2, 3], [], [4], 100, 2, 2, 0, [5, 6], guess=[3, 4, 5, 6, 7], L=2),
    _case("the guess runs out", [1, 2, 3], [], [4], 100, 2, 2, 0, [5], guess=[3, 4, 5], L=2),
    _case("the guess is over", [1, 2, 3], [], [4], 100, 2, 2, 0, [], guess=[3, 4], L=2),
    _case("a guess under the clamp", [1, 2, 3], [], [4], 6, 2, 2, 0, [5], guess=[3, 4, 5, 6, 7], L=2),
]


def run_case(c, defect=None):
    return step(c["seq"], c["n"], c["head"], c["limit"], c["K"], c["max_ngram"], c["guess"], c["L"], defect)


def case_holds(c, defect=None):
    a, drafts, toks, seq = run_case(c, defect)
    n1 = c["n"] + c["want_a"] + 1
    want_seq = list(c["seq"][:c["n"] + c["want_a"]]) + [c["head"][c["want_a"]]] + c["want_drafts"]
    return a == c["want_a"] and drafts == c["want_drafts"] and toks == c["head"][:c["want_a"] + 1] and \
        [int(v) for v in seq[:n1 + len(drafts)]] == want_seq


def simulate_guess(greedy_new, guess, K, T):
    """The speculative loop under a caller's guess, on the host: `greedy_new` are the T tokens plain greedy search decodes (no EOS cut).
    Returns dict(steps, drafted, accepted, tokens) as HipQwen25VLTextEncoder.last_lookup_stats counts them: the prefill's pick settles
    token 0 and is not a step."""
    G, guess = [int(v) for v in greedy_new], [int(v) for v in guess]
    k, steps, drafted, accepted = 1, 0, 0, 0
    kd = len(guess[1:1 + max(0, min(K, T - 1 - 1))])
    while k < T:
        drafts = guess[k:k + kd]
        a = 0
        while a < len(drafts) and drafts[a] == G[k + a]:
            a += 1
        steps, drafted, accepted, k = steps + 1, drafted + len(drafts), accepted + a, k + a + 1
        kd = len(guess[k:k + max(0, min(K, T - k - 1))])
    return dict(steps=steps, drafted=drafted, accepted=accepted, tokens=k)
