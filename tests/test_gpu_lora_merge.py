"""rgn_lora_merge_bf16 on the GPU (csrc/lora.hip) against the CPU model of tests/lora_merge_model.py: exact probes (`torch.equal` with the
fp64 result - tests/test_lora_merge_model.py shows that every named defect changes one of them), the element-wise fp64 bound on seeded
random data over the shapes that reach every code path (rows 1 / 5 / 67: below, inside and past one 64-row tile; columns 8 / 72 / 520:
one partial, one partial, two full + a partial 256-column tile; ranks 1 / 4 / 16 / 130: below, at and past the 16-rank LDS chunk),
a destination inside a packed tensor with canaries, the in-place form and repeatability."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lora_merge_model as M  # noqa: E402
from regione_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu


def _bf(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).cuda()


def _terms_dev(terms):
    return [(torch.from_numpy(np.ascontiguousarray(A, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(B, np.float32)).cuda(), s)
            for A, B, s in terms]


def _strided(flat, N, K, ld):
    """[N, K] view with row stride ld of a flat device buffer of (N - 1) * ld + K elements."""
    return flat.as_strided((N, K), (ld, 1))


@pytest.mark.parametrize("probe", M.probes(), ids=lambda p: p.name)
def test_exact_probes_equal_the_fp64_model(probe):
    p = probe
    dst, W = _bf(p.dst), _bf(p.W)
    assert torch.equal(dst.float().cpu().double(), torch.from_numpy(p.dst))            # the probe's values ARE bf16 values
    ops.lora_merge(_strided(dst, p.N, p.K, p.ldd), _strided(W, p.N, p.K, p.ldw), _terms_dev(p.terms))
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), _bf(p.expected).cpu()), p.name
    assert torch.equal(W.cpu(), _bf(p.W).cpu())                                        # W is read only


def _random_case(seed, N, K, ranks, scales):
    rng = np.random.default_rng(seed)
    W = M.bf16_rne(rng.standard_normal((N, K)) * 0.05)
    terms = [(rng.standard_normal((r, K)).astype(np.float32) * 0.2, rng.standard_normal((N, r)).astype(np.float32) * 0.2, float(s))
             for r, s in zip(ranks, scales)]
    return W, terms


_TERM_SETS = {"one": lambda r: ((r,), (-0.75,)),
              "two": lambda r: ((r, 3 if r != 3 else 5), (1.5, -0.5)),
              "eight": lambda r: ((r, 1, 4, 16, 2, 7, 1, 4), (0.5, -0.25, 1.0, -1.0, 0.0, 2.0, -2.0, 0.125))}


@pytest.mark.parametrize("n_terms", ["one", "two", "eight"])
@pytest.mark.parametrize("r", [1, 4, 16, 130])
def test_fp64_bound_on_random_data(r, n_terms):
    """Every (N, K) of the grid for one (rank, term set): one launch each, all tiny."""
    ranks, scales = _TERM_SETS[n_terms](r)
    for N in (1, 5, 67):
        for K in (8, 72, 520):
            W, terms = _random_case(N * 100000 + K * 100 + r, N, K, ranks, scales)
            Wd = _bf(W)
            out = ops.lora_merge(torch.empty_like(Wd), Wd, _terms_dev(terms)).float().cpu().double().numpy()
            ok = M.accepted(out, W, terms)
            assert ok.all(), (N, K, ranks, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
            # and it is not W: the delta is far above the bound
            assert not np.array_equal(out, W)


@pytest.mark.parametrize("N,K,r", [(1, 8, 1), (67, 520, 130)])
def test_scale_zero_returns_w_bit_for_bit(N, K, r):
    W, terms = _random_case(7, N, K, (r, 4), (0.0, 0.0))
    Wd = _bf(W)
    out = ops.lora_merge(torch.empty_like(Wd), Wd, _terms_dev(terms))
    assert torch.equal(out, Wd)


def test_destination_rows_5_to_9_of_a_16_row_tensor_leave_canaries_and_pad_columns_alone():
    K, ld = 72, 96
    W, terms = _random_case(11, 5, K, (4, 12), (1.25, -0.5))
    g = torch.Generator().manual_seed(3)
    packed = torch.randn(16, ld, generator=g).to(torch.bfloat16).cuda()
    before = packed.clone()
    Wd = _bf(W)
    ops.lora_merge(packed[5:10, :K], Wd, _terms_dev(terms))
    alone = ops.lora_merge(torch.empty_like(Wd), Wd, _terms_dev(terms))
    assert torch.equal(packed[5:10, :K], alone)
    assert torch.equal(packed[:5], before[:5]) and torch.equal(packed[10:], before[10:]) and torch.equal(packed[5:10, K:], before[5:10, K:])
    assert M.accepted(alone.float().cpu().double().numpy(), W, terms).all()


@pytest.mark.parametrize("N,K,ld", [(67, 520, 520), (5, 72, 96)])
def test_in_place_equals_out_of_place_and_a_repeated_call_is_bit_identical(N, K, ld):
    W, terms = _random_case(13, N, K, (16, 5), (0.5, -1.0))
    td = _terms_dev(terms)
    buf = torch.zeros(N, ld, dtype=torch.bfloat16, device="cuda")
    buf[:, :K] = _bf(W)
    Wd = buf.clone()
    a = ops.lora_merge(torch.empty(N, K, dtype=torch.bfloat16, device="cuda"), Wd[:, :K], td)
    b = ops.lora_merge(torch.empty(N, K, dtype=torch.bfloat16, device="cuda"), Wd[:, :K], td)
    assert torch.equal(a, b)
    view = buf[:, :K]
    ops.lora_merge(view, view, td)                                   # dst is W, ldd == ldw
    assert torch.equal(view, a)
    assert torch.equal(buf[:, K:], Wd[:, K:])
