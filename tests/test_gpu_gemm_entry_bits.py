"""GPU: every way to the GEMM kernel writes the bits, and picks the launch plan, it did before the nine C entry points became one.

tools/gemm_entry_bits.py runs a fixed list of calls through the public op names - ops.gemm (bf16 / fp8, M = 8 / 200 / 520, every epilogue, a
row scatter, a strided W), ops.gemm_pair (one problem empty included), ops.gemm_qkv / gemm_qkv_pair (with and without the MLP half, identity
and permuted cache rows, fp16 round trip, row_base), ops.gemm_group and, with the C++ registration, torch.ops.regione_mi.kv_partial_update_ /
_pair_ - on inputs drawn on the CPU with a fixed seed, and prints per case the launch plan and a sha256 of every output buffer (C, K slab,
V^T slab).  tests/golden/gemm_entry_bits_parent.txt is that listing from the PARENT commit (eight fixed-arity C calls beside the descriptor call)
on an MI355X.  Every line has to be equal: there is no tolerance.

A process that holds the Python registration (RGN_TORCH_OPS=py) compares the lines of the op wrappers only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_entry_bits_parent.txt")


@pytest.mark.gpu
def test_every_line_equals_the_parent_commits():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gemm_entry_bits as B
    want = [l.rstrip("\n") for l in open(GOLDEN) if not l.startswith("#")]
    assert len(want) == len(B.CASES), "the golden listing was written with the C++ registration: one line per case"
    if not B.CPP:
        want = [l for l in want if not l.startswith(B.CPP_PREFIX)]
    got = B.listing()
    for g in got:
        print(g)
    assert got == want
