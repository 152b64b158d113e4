"""GPU: the 64-query-row attention kernel writes the bits of the 8-wave kernel it replaces.

tools/attn_w64_bits.py launches rgn_attention_bounded on seeded inputs - the full-step shape (8704^2 x 24 x 128), the region-step query sets
(Sq 1536, 708), rows whose scores reach +-score_bound, every launch class that changed kernel (whole rounds in front of a split or stream-K
remainder, one partial round, rounds plus an unsplit tail), 1 / 2 / 3 / 65-tile KV lengths - and prints one sha256 per case.
tests/golden/attn_w64_bits_parent.txt is that listing from the PARENT commit's library on an MI355X.  Every digest has to be equal: there is no
tolerance.  The launch plan is part of each line, so a planner change that moves a case to another launch class shows as well.

Limit: equal digests do not show WHICH kernel wrote them - a build that kept the 8-wave kernel on these launches would pass too.  That the
64-row kernel is the one dispatched is shown by the kernel traces (profiles/r10_attn_w64_ab.txt) and by launch_attention_asm in attn.hip."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_w64_bits_parent.txt")


@pytest.mark.gpu
def test_every_digest_equals_the_parent_librarys():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import attn_w64_bits as B
    want = [l.rstrip("\n") for l in open(GOLDEN) if not l.startswith("#")]
    assert len(want) == len(B.CASES)
    got = B.listing()
    for g, w in zip(got, want):
        print(g)
    assert got == want
