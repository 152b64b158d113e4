"""rgn_lm_pick_verify on the GPU: the picks of a verification step (csrc/decode.hip: lm_pick_verify_kernel).  Every comparison is
torch.equal.  Row r - token and processed scores - against rgn_lm_pick on that row with a copy of the map on which rgn_lm_seen_mark
marked drafts[:r]; the exact probe of tests/qwen_lookup_sampling_model.py against its hand-computed scores; `seen`, the logits and the
sentinel-filled frames around the strided token slots and score rows unchanged; a repeated call identical."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qwen_lookup_sampling_model as SM  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

RS = (1, 2, 8, 9, 32)
VS = (1, 2, 1000, 4097, 152064)
PENALTIES = (1.0, 1.3)
# (sample, temperature, top_k, top_p): greedy; the three filters together; top-p alone; top-k alone
CONFIGS = ((0, 1.0, 0, 1.0), (1, 0.7, 20, 0.8), (1, 1.0, 0, 0.9), (1, 1.0, 50, 1.0))
RMAX, GUARD, TS = 32, 64, 3                                                      # token slots 3 int64 apart
ROW, TOP, NEXT = 4, 9.0, 8.5                                                     # row 4's two planted logits (V >= 1000)


def _st():
    return ops._stream()


def _p(t):
    return t.data_ptr()


class Case:
    """One vocabulary's inputs, shared by every R, penalty and configuration: 32 logits rows (row stride V + 3, NaN beside them), a map
    with every 7th id and a few others seen, 31 drafts and 32 uniforms."""

    def __init__(self, V):
        g = torch.Generator().manual_seed(V)
        self.V, self.ldl, self.lds = V, V + 3, V + 5
        z = torch.full((RMAX, self.ldl), float("nan"))
        z[:, :V] = torch.randn(RMAX, V, generator=g)
        seen = torch.zeros(V, dtype=torch.uint8)
        seen[::7] = 1
        d = torch.randint(0, V, (RMAX - 1,), generator=g)
        d[1] = d[0]                                                              # a duplicate
        d[2] = 7 * int(torch.randint(0, (V + 6) // 7, (1,), generator=g))        # an id already seen
        self.top = self.next = None
        if V >= 1000:
            self.top, self.next = 501, 17                                        # neither seen (501 = 7 x 71 + 4, 17 = 7 x 2 + 3)
            assert not seen[self.top] and not seen[self.next]
            d[d == self.top] = self.top + 1                                      # drafted once, at index 3 only
            d[d == self.next] = self.next + 1
            z[ROW, self.top], z[ROW, self.next] = TOP, NEXT                      # 9 / 1.3 < 8.5: the penalty moves row 4's argmax
            d[3] = self.top                                                      # the argmax of row 4, drafted before it
        for i, t in zip((5, 6, 7, 8, 9), (-1, V, V + 5, -2 ** 40, 2 ** 40)):     # no ids of the vocabulary
            d[i] = t
        self.z, self.drafts = z.cuda(), d.cuda()
        self.seen_buf = torch.full((V + 2 * GUARD,), 7, dtype=torch.uint8).cuda()
        self.seen = self.seen_buf[GUARD:GUARD + V]
        self.seen.copy_(seen.cuda())
        self.u = torch.rand(RMAX, generator=g).cuda()
        self.lib = _lib.lib()
        self.nb = self.lib.rgn_lm_pick_workspace_bytes(V)
        self.ws = torch.empty(RMAX * self.nb // 4, dtype=torch.float32, device="cuda")

    def verify(self, R, pen, cfg, scores=True, drafts=None):
        """(tokens [R], scores [R, V]) of one call; asserts that nothing outside them was written."""
        sample, T, k, p = cfg
        tok = torch.full(((RMAX + 2) * TS,), -5, dtype=torch.int64, device="cuda")
        sc = torch.full((RMAX + 2, self.lds), -77.0, dtype=torch.float32, device="cuda")
        z0, seen0 = self.z.clone(), self.seen_buf.clone()
        d = self.drafts if drafts is None else drafts
        rc = self.lib.rgn_lm_pick_verify(_p(self.z), self.ldl, R, self.V, _p(self.seen), None if R == 1 and drafts is None else _p(d), pen, sample,
                                         T, k, p, _p(self.u) if sample else None, _p(tok) + 8 * TS, TS, _p(sc[1]) if scores else None, self.lds,
                                         _p(self.ws), R * self.nb, _st())
        _lib.check(rc, "rgn_lm_pick_verify")
        assert torch.equal(self.seen_buf, seen0), "the map was written"
        assert torch.equal(self.z.view(torch.int32), z0.view(torch.int32)), "the logits were written"
        frame = tok.clone()
        frame[TS:TS * (R + 1):TS] = -5
        assert bool((frame == -5).all()), "a token slot outside the R rows was written"
        assert bool((sc[0] == -77.0).all()) and bool((sc[R + 1:] == -77.0).all()) and bool((sc[:, self.V:] == -77.0).all()), \
            "scores outside the R rows and V columns were written"
        if not scores:
            assert bool((sc == -77.0).all())
        return tok[TS:TS * (R + 1):TS].clone(), sc[1:R + 1, :self.V].clone()

    @functools.lru_cache(maxsize=None)
    def reference(self, pen, cfg):
        """rgn_lm_pick on each of the 32 rows with a copy of the map on which rgn_lm_seen_mark marked drafts[:r]."""
        sample, T, k, p = cfg
        toks = torch.empty(RMAX, dtype=torch.int64, device="cuda")
        sc = torch.empty(RMAX, self.V, dtype=torch.float32, device="cuda")
        for r in range(RMAX):
            seen = self.seen.clone()
            _lib.check(self.lib.rgn_lm_seen_mark(_p(self.drafts), r, _p(seen), self.V, _st()), "rgn_lm_seen_mark")
            row = self.z[r, :self.V].clone()
            _lib.check(self.lib.rgn_lm_pick(_p(row), self.V, _p(seen), pen, sample, T, k, p, _p(self.u) + 4 * r if sample else None,
                                            _p(toks) + 8 * r, _p(sc[r]), _p(self.ws), self.nb, _st()), "rgn_lm_pick")
        return toks, sc


@functools.lru_cache(maxsize=None)
def _case(V):
    return Case(V)


@pytest.mark.parametrize("V", VS)
def test_every_row_is_the_one_row_pick_under_the_map_with_the_drafts_before_it(V):
    c = _case(V)
    for pen in PENALTIES:
        for ci, cfg in enumerate(CONFIGS):
            want_t, want_s = c.reference(pen, cfg)
            for R in RS:
                got_t, got_s = c.verify(R, pen, cfg)
                assert torch.equal(got_t, want_t[:R]), (V, pen, ci, R, "tokens")
                assert torch.equal(got_s.view(torch.int32), want_s[:R].view(torch.int32)), (V, pen, ci, R, "scores")
            got_t, _ = c.verify(9, pen, cfg, scores=False)                       # the scores in the workspace
            assert torch.equal(got_t, want_t[:9]), (V, pen, ci, "no scores_out")
    a, b = c.verify(32, 1.3, CONFIGS[1]), c.verify(32, 1.3, CONFIGS[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "a repeated call"


@pytest.mark.parametrize("V", [1000, 4097, 152064])
def test_a_drafted_argmax_moves_the_token_of_the_rows_after_it_only_under_a_penalty(V):
    c = _case(V)
    for pen, want in ((1.0, c.top), (1.3, c.next)):
        toks, sc = c.verify(9, pen, CONFIGS[0])
        assert int(toks[ROW]) == want, (pen, int(toks[ROW]))
        assert float(sc[ROW, c.top]) == float(np.float32(TOP) / np.float32(pen)) and float(sc[ROW, c.next]) == NEXT
    # row 3 is the row the draft itself sits in: the draft at index 3 is not in its map (rows see the drafts BEFORE them)
    z3 = c.z[3, c.top].clone()
    toks, sc = c.verify(9, 1.3, CONFIGS[0])
    assert float(sc[3, c.top]) == float(z3), "row 3 was penalised for its own draft"


def test_the_exact_probe_gives_the_hand_computed_scores_and_tokens():
    """Logits of 8.0 / -8.0 under penalty 2: one application is 4.0 / -16.0, two would be 2.0 / -32.0 - a duplicate draft, an id both
    seen and drafted, and ids outside the vocabulary, against tests/qwen_lookup_sampling_model.py's hand-computed members."""
    z, seen, drafts, pen = SM.probe()
    R, V = z.shape
    lib = _lib.lib()
    zd, sd, dd = torch.from_numpy(z).cuda(), torch.from_numpy(seen).cuda(), torch.tensor(drafts, dtype=torch.int64).cuda()
    tok = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    sc = torch.full((R, V), -77.0, dtype=torch.float32, device="cuda")
    nb = lib.rgn_lm_pick_workspace_bytes(V)
    ws = torch.empty(R * nb // 4, dtype=torch.float32, device="cuda")
    _lib.check(lib.rgn_lm_pick_verify(_p(zd), V, R, V, _p(sd), _p(dd), pen, 0, 1.0, 0, 1.0, None, _p(tok), 1, _p(sc), V, _p(ws), R * nb, _st()),
               "rgn_lm_pick_verify")
    want = z.copy()
    for r, ids in enumerate(SM.PROBE_MEMBERS):
        want[r, ids] = np.where(z[r, ids] < 0, -16.0, 4.0)
    assert torch.equal(sc.cpu(), torch.from_numpy(want)) and tok.tolist() == SM.PROBE_TOKENS
    assert torch.equal(sd.cpu(), torch.from_numpy(seen))
    model_scores, model_toks, _ = SM.pick_verify(z, seen, drafts, pen)
    assert torch.equal(sc.cpu(), torch.from_numpy(model_scores)) and tok.tolist() == model_toks


def test_one_row_reads_no_draft():
    c = _case(1000)
    want_t, want_s = c.reference(1.3, CONFIGS[1])
    got_t, got_s = c.verify(1, 1.3, CONFIGS[1])                                  # drafts = NULL
    assert torch.equal(got_t, want_t[:1]) and torch.equal(got_s.view(torch.int32), want_s[:1].view(torch.int32))
