"""rgn_lm_lookup_step_mark on the GPU (csrc/decode.hip: lm_lookup_step_mark_kernel): rgn_lm_lookup_step over the picks of a step that
also marks the tokens the step settles in the byte map.  Every comparison is torch.equal: `seq` and `result` against rgn_lm_lookup_step
on the same inputs, the map against map U accepted tokens (tests/qwen_lookup_sampling_model.py), for every accept pattern up to 8 rows
and at 32 rows, in both propose modes; seen = NULL is rgn_lm_lookup_step; ids outside [0, V) mark nothing."""
import itertools
import os
import sys

import numpy as np
import torch
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qwen_lookup_sampling_model as SM  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 32


def _step(seq, n, head, limit, K, ngram, guess, L, hs, seen, V):
    """One call on copies of the inputs: (seq after, result, map after).  seen is None: rgn_lm_lookup_step; "null": the new entry with
    seen = NULL; else a uint8 [V] map, sentinels on both sides of it."""
    h = _lib.lib()
    R = len(head)
    sb = torch.tensor([-7] * 8 + list(seq) + [-7] * 8, dtype=torch.int64).cuda()
    hb = torch.full((R * hs + 1,), -5, dtype=torch.int64)
    hb[:R * hs:hs] = torch.tensor(head, dtype=torch.int64)
    hb = hb.cuda()
    rb = torch.full((4 + 2 + R + 4,), -9, dtype=torch.int64).cuda()
    gb = torch.tensor(list(guess), dtype=torch.int64).cuda() if guess is not None else None
    args = (sb.data_ptr() + 64, n, R, hb.data_ptr(), hs, limit, K, ngram, None if gb is None else gb.data_ptr(), 0 if gb is None else gb.numel(),
            L, rb.data_ptr() + 32)
    mb = None
    if seen is None:
        _lib.check(h.rgn_lm_lookup_step(*args, ops._stream()), "rgn_lm_lookup_step")
    elif isinstance(seen, str):
        _lib.check(h.rgn_lm_lookup_step_mark(*args, None, 0, ops._stream()), "rgn_lm_lookup_step_mark")
    else:
        mb = torch.full((V + 2 * GUARD,), 7, dtype=torch.uint8)
        mb[GUARD:GUARD + V] = torch.as_tensor(seen)
        mb = mb.cuda()
        _lib.check(h.rgn_lm_lookup_step_mark(*args, mb.data_ptr() + GUARD, V, ops._stream()), "rgn_lm_lookup_step_mark")
        assert bool((mb[:GUARD] == 7).all()) and bool((mb[GUARD + V:] == 7).all()), "the bytes around the map"
        mb = mb[GUARD:GUARD + V].cpu()
    return sb.cpu(), rb.cpu(), mb


def _check(seq, n, head, limit, K, ngram, seen, V, guess=None, L=0, hs=1, tag=None):
    """The three calls agree on seq and result; the marks are the model's.  Returns a."""
    s0, r0, _ = _step(seq, n, head, limit, K, ngram, guess, L, hs, None, V)
    s1, r1, _ = _step(seq, n, head, limit, K, ngram, guess, L, hs, "null", V)
    s2, r2, m2 = _step(seq, n, head, limit, K, ngram, guess, L, hs, seen, V)
    assert torch.equal(s1, s0) and torch.equal(r1, r0), (tag, "seen = NULL")
    assert torch.equal(s2, s0) and torch.equal(r2, r0), (tag, "with a map")
    a = int(r0[4])
    after = s0[8:-8].tolist()
    want = SM.marks(seen, after, n, a, len(head), V)
    assert torch.equal(m2, torch.from_numpy(want)), (tag, "marks", np.flatnonzero(m2.numpy() != want).tolist())
    settled = [t for t in after[n:n + a + 1] if 0 <= t < V]
    assert int(m2.sum()) == len(set(np.flatnonzero(np.asarray(seen)).tolist()) | set(settled)), (tag, "map U accepted tokens")
    return a


V = 152064
IDS = [152063, 7, 151000, 152062, 0]                                             # up to V - 1 of Qwen2.5-VL


def _run(rng, n, vocab):
    return [IDS[i] for i in rng.integers(0, vocab, n)]


def _map(rng):
    seen = np.zeros(V, dtype=np.uint8)
    seen[rng.integers(0, V, 50)] = 1
    seen[IDS[int(rng.integers(0, 5))]] = 1                                        # one of the ids in play is already seen
    return seen


def test_every_accept_pattern_up_to_8_rows_marks_the_accepted_tokens_only():
    rng = np.random.default_rng(8)
    for R in range(1, 9):
        for mask in itertools.product((0, 1), repeat=R - 1):                     # which drafts coincide with the pick before them
            n = int(rng.integers(3, 70))
            settled, head = _run(rng, n, 4), _run(rng, R, 5)
            drafts = [head[i] if m else head[i] ^ 1 for i, m in enumerate(mask)]  # a rejected draft is an id of its own: 152062, 6, ...
            limit = n + R + int(rng.integers(0, 12))
            seq = settled + drafts + [777] * (limit - n - (R - 1))
            want_a = mask.index(0) if 0 in mask else R - 1
            seen = _map(rng)
            assert _check(seq, n, head, limit, 7, int(rng.integers(1, 9)), seen, V, tag=(R, mask)) == want_a
            guess = _run(rng, int(rng.integers(1, 30)), 5)
            assert _check(seq, n, head, limit, int(rng.integers(0, 8)), 2, seen, V, guess, int(rng.integers(0, n + 1)), hs=3,
                          tag=(R, mask, "guess")) == want_a


def test_32_rows():
    rng = np.random.default_rng(32)
    R, n = 32, 40
    for want_a in (0, 1, 17, 30, 31):
        head = [int(t) for t in rng.integers(0, V, R)]
        drafts = [head[i] if i < want_a else (head[i] + 1) % V for i in range(R - 1)]
        limit = n + R + 5
        seq = _run(rng, n, 4) + drafts + [777] * (limit - n - (R - 1))
        assert _check(seq, n, head, limit, 31, 2, _map(rng), V, tag=(32, want_a)) == want_a
        assert _check(seq, n, head, limit, 31, 2, np.zeros(V, dtype=np.uint8), V, [5] * 90, 3, tag=(32, want_a, "guess")) == want_a


def test_ids_outside_the_vocabulary_mark_nothing():
    rng = np.random.default_rng(5)
    small = 100                                                                   # of IDS only 7 and 0 are ids of this vocabulary
    for head, drafts in (([152063, 151000, 7], [152063, 151000]), ([-1, 2 ** 40, 100, 99], [-1, 2 ** 40, 100]), ([100], [])):
        n, R = 6, len(head)
        seq = _run(rng, n, 5) + drafts + [777] * 6
        seen = np.zeros(small, dtype=np.uint8)
        seen[3] = 1
        assert _check(seq, n, head, n + R + 5, 3, 2, seen, small, tag=head) == R - 1


def test_the_hand_computed_mark_cases():
    for name, ids, seq, n, a, R, v, want in SM.MARK_CASES:
        seen = np.zeros(v, dtype=np.uint8)
        seen[ids] = 1
        # the run BEFORE the step: the a accepted drafts as they are, then drafts that differ from the picks; head = the run after
        head = list(seq[n:n + a + 1]) + [555] * (R - a - 1)
        before = list(seq[:n + a]) + [444] * (R - 1 - a) + [777] * 8
        s, r, m = _step(before, n, head, n + R + 4, 0, 2, None, 0, 1, seen, v)
        assert int(r[4]) == a and sorted(np.flatnonzero(m.numpy()).tolist()) == sorted(want), name
