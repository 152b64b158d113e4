"""The CPU model of the LoRA merge kernel (tests/lora_merge_model.py): the exact probes and the fp64 bound the GPU test applies accept
the contract and reject every named defect - so a kernel that passes tests/test_gpu_lora_merge.py has none of them.  Also the argument
validation of rgn_lora_merge_bf16 (codes and messages, no launch: null or never-dereferenced pointers)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_merge_model as M  # noqa: E402


def test_bf16_rounding_is_round_to_nearest_even():
    import torch
    x = np.array([1.0, 257.0, 255.0, 1.00390625, 1.01171875, -3.3, 1e-40, 0.0, 65535.0])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(M.bf16_rne(x), want)
    assert M.bf16_rne(257.0) == 256.0 and M.bf16_rne(259.0) == 260.0          # ties to even, both directions


def test_probes_are_exact_and_the_model_meets_them():
    for p in M.probes():
        ref = M.reference(p.w_rows(), p.terms)
        assert np.array_equal(M.bf16_rne(ref), ref), p.name                    # the fp64 result IS a bf16 value
        got = np.stack([p.expected[n * p.ldd:n * p.ldd + p.K] for n in range(p.N)])
        assert np.array_equal(got, ref), p.name
        assert M.accepted(got, p.w_rows(), p.terms).all()
        keep = np.ones(len(p.dst), bool)
        for n in range(p.N):
            keep[n * p.ldd:n * p.ldd + p.K] = False
        assert np.array_equal(p.expected[keep], p.dst[keep])                   # pad columns untouched


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_named_defect_changes_a_probe_element(defect):
    hit = [p.name for p in M.probes() if not np.array_equal(M.merge(p.dst, p.ldd, p.W, p.ldw, p.N, p.K, p.terms, defect), p.expected)]
    assert hit, f"no probe sees {defect}"


def _random_case(seed, N, K, ranks, scales):
    rng = np.random.default_rng(seed)
    bf = lambda a: M.bf16_rne(a)
    W = bf(rng.standard_normal((N, K)) * 0.05)
    terms = [(rng.standard_normal((r, K)).astype(np.float32) * 0.2, rng.standard_normal((N, r)).astype(np.float32) * 0.2, s)
             for r, s in zip(ranks, scales)]
    return W, terms


@pytest.mark.parametrize("defect", [d for d in M.DEFECTS if d not in ("ldd_ignored", "last_partial_row_tile_skipped")])
def test_the_fp64_bound_accepts_the_contract_and_rejects_the_arithmetic_defects(defect):
    """Seeded random data at the GPU test's shapes: the correct model lies inside the bound everywhere; each arithmetic defect leaves it
    somewhere (the two addressing defects are the probes' business: they write right values to wrong places)."""
    N, K = 67, 72
    W, terms = _random_case(5, N, K, (4, 16), (0.75, -1.5))
    flat = lambda a: np.asarray(a, np.float64).reshape(-1)
    good = M.merge(np.zeros(N * K), K, flat(W), K, N, K, terms).reshape(N, K)
    assert M.accepted(good, W, terms).all()
    bad = M.merge(np.zeros(N * K), K, flat(W), K, N, K, terms, defect).reshape(N, K)
    assert not M.accepted(bad, W, terms).all()


@pytest.mark.parametrize("N,K,ranks", [(1, 8, (1,)), (5, 72, (130,)), (67, 520, (16, 4)), (5, 8, (1, 4, 16, 130, 1, 4, 16, 130))])
def test_the_bound_holds_for_the_model_over_the_shape_grid(N, K, ranks):
    scales = [(-1.0) ** i * (0.5 + 0.25 * i) for i in range(len(ranks))]
    W, terms = _random_case(N * 1000 + K, N, K, ranks, scales)
    got = M.merge(np.zeros(N * K), K, W.reshape(-1), K, N, K, terms).reshape(N, K)
    assert M.accepted(got, W, terms).all()
    zero = M.merge(np.zeros(N * K), K, W.reshape(-1), K, N, K, [(A, B, 0.0) for A, B, _ in terms]).reshape(N, K)
    assert np.array_equal(zero, W)                                              # scale = 0 returns W bit for bit


def test_argument_validation_returns_codes_and_messages_without_touching_the_gpu():
    from regione_amd import _lib
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address

    def msg():
        return h.rgn_last_error().decode()

    def call(dst=P, ldd=64, W=P, ldw=64, N=4, K=64, terms=((P, P, 4, 1.0),), n_terms=None, null_terms=False):
        arr = (_lib.LoraTerm * max(len(terms), 1))(*[_lib.LoraTerm(*t) for t in terms])
        return h.rgn_lora_merge_bf16(dst, ldd, W, ldw, N, K, None if null_terms else arr, len(terms) if n_terms is None else n_terms, None)
    assert call(N=0) == 0 and call(N=0, dst=None, null_terms=True) == 0                                # N = 0: nothing to do
    assert call(dst=None) == -1 and "non-null" in msg()
    assert call(W=None) == -1 and call(null_terms=True) == -1
    assert call(terms=((None, P, 4, 1.0),)) == -1 and "non-null" in msg()
    assert call(terms=((P, None, 4, 1.0),)) == -1
    assert call(n_terms=0) == -1 and "1..8" in msg()
    assert call(terms=((P, P, 4, 1.0),) * 9) == -1 and "1..8" in msg()
    assert call(terms=((P, P, 4, 1.0),) * 8, N=-1) == -1
    assert call(terms=((P, P, 0, 1.0),)) == -1 and "1..1024" in msg()
    assert call(terms=((P, P, 1025, 1.0),)) == -1 and "1..1024" in msg()
    assert call(K=60, ldd=64, ldw=64) == -1 and "multiple of 8" in msg()
    assert call(ldd=56) == -1 and call(ldw=56) == -1 and call(ldd=68) == -1
    assert call(dst=P + 2) == -1 and "aligned" in msg()
    assert call(terms=((P + 4, P, 4, 1.0),)) == -1 and "aligned" in msg()
    assert call(ldd=128, ldw=64) == -1 and "in-place" in msg()                                          # dst == W needs equal strides


def test_ops_wrapper_checks_tensors_before_the_library_sees_them():
    import torch
    from regione_amd import _lib, ops
    W = torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError):                       # CPU tensors: there is no CPU fallback
        ops.lora_merge(W, W, [(torch.zeros(2, 16), torch.zeros(4, 2), 1.0)])
    with pytest.raises(_lib.RegionEHipError, match="bf16"):
        ops.lora_merge(W.float(), W, [(torch.zeros(2, 16), torch.zeros(4, 2), 1.0)])
    with pytest.raises(_lib.RegionEHipError, match="term 0 B"):
        ops.lora_merge(W, W, [(torch.zeros(2, 16), torch.zeros(2, 4), 1.0)])
    with pytest.raises(_lib.RegionEHipError, match="term 0 A"):
        ops.lora_merge(W, W, [(torch.zeros(2, 16, dtype=torch.bfloat16), torch.zeros(4, 2), 1.0)])
