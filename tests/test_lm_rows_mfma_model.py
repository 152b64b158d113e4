"""The model of the wide decode step (tests/lm_rows_mfma_model.py) meets its own probes, and every named defect of it fails at least one:
the probes of tests/test_gpu_lm_rows_mfma.py are sharp enough to see each of them.  CPU only."""
import pytest
import torch

import lm_rows_mfma_model as M


def _run(mutant=None):
    return lambda p, B, Y: M.emulate(p, B, Y, mutant)


def _head(mutant=None):
    return lambda p, B: M.emulate_head(p, B, mutant)


def _probes(mutant=None):
    """name -> met, over the tiny shapes (the probes of the GPU test at the sizes a CPU loop affords)."""
    run, head = _run(mutant), _head(mutant)
    N, K = M.TINY[-1]
    out = {}
    for w8 in (False, True):
        t = "w8" if w8 else "bf16"
        out[f"integer_{t}"] = all(M.check_integer(run, n, k, w8, B) for n, k in M.TINY for B in (1, 15, 17, 32))
        out[f"index_{t}"] = M.check_index(run, 17, K, w8)
        out[f"invariance_{t}"] = M.check_invariance(run, N, K, w8, rows=(0, 31))
    out["codes"] = M.check_codes(run)
    out["scale_once"] = M.check_scale(run)
    out["head_invariance"] = M.check_head_invariance(head, 33, K, rows=(0, 31))
    out["head_ties"] = all(M.check_head_ties(head, V) for V in (17, 97))
    return out


def test_the_model_meets_every_probe():
    got = _probes()
    assert all(got.values()), got


CAUGHT_BY = dict(k_halves_swapped=("integer_bf16", "integer_w8", "index_bf16", "index_w8"), scale_per_partial=("scale_once",),
                 resid_before_rounding=("integer_bf16", "integer_w8"), tail_writes_column_n=("integer_bf16", "integer_w8"),
                 row_b_written=("integer_bf16", "integer_w8"), tie_to_higher_index=("head_ties",),
                 fold_order_reads_b=("invariance_bf16", "invariance_w8", "head_invariance"))


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_named_defect_fails_the_probe_that_is_there_for_it(mutant):
    got = _probes(mutant)
    failed = {k for k, ok in got.items() if not ok}
    assert failed, mutant
    assert set(CAUGHT_BY[mutant]) <= failed, (mutant, failed)


def test_the_k_maps_cover_a_waves_256_k_once():
    for w8 in (False, True):
        ks = torch.cat([M.kmap(m, w8).flatten() for m in range(M.KW // 32)])
        assert torch.equal(torch.sort(ks).values, torch.arange(M.KW))


def test_the_split_of_the_uneven_shape_is_256_256_64_0():
    N, K = M.TINY[-1]
    p = M.integer_case(N, K, False)
    p.X[:] = 1
    p.W[:] = 1
    acc = M.partial_sums(p, 1)
    assert [int(acc[w, 0, 0]) for w in range(4)] == [256, 256, 64, 0]


def test_the_bound_holds_for_the_model_and_the_fp8_codes_are_a_subset_of_bf16():
    for fam in ("randn", "cancel"):
        for w8 in (False, True):
            p = M.with_pad(M.bound_case(33, 576, fam, w8))
            Y = M.emulate(p, 32, M.frames(p, 32))
            assert M.bound_ratio(p, 32, Y) <= 1.0, (fam, w8)
    t = M.G.e4m3fn_table()
    fin = t[[c for c in range(256) if (c & 0x7f) != 0x7f]]
    assert torch.equal(fin.float().to(torch.bfloat16).double(), fin)
