"""rgn_mmdit_double_block / rgn_mmdit_single_block and `torch.ops.regione_mi.mmdit_*_block_` without a GPU: both registrations define
the two ops with the same schemas, the mutation annotations are there, the fake kernels do nothing, a CPU tensor fails loudly, and the
C entries validate every argument before anything could launch."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import regione_amd.torch_ops as T
from regione_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmdit_double_block_", "mmdit_single_block_")


def test_both_registrations_define_the_block_ops_with_identical_schemas():
    """The C++ library loaded alone (nothing of regione_amd imported) and the Python registration (RGN_TORCH_OPS=py), each in a child
    process: the same two schema strings, which are the ones of `torch_ops.BLOCK_SCHEMAS`."""
    assert T.registered_block_ops() == tuple(sorted(NAMES)) and set(T.BLOCK_SCHEMAS) == set(NAMES)
    code = ("import json, sys, torch; torch.ops.load_library(sys.argv[1]); names = sys.argv[2].split(','); "
            "assert 'regione_amd' not in sys.modules; "
            "print(json.dumps({n: str(getattr(torch.ops.regione_mi, n).default._schema) for n in names}))")
    r = subprocess.run([sys.executable, "-c", code, T.CPP_LIB, ",".join(NAMES)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cpp = json.loads(r.stdout.strip().splitlines()[-1])
    code = ("import json, torch, regione_amd.torch_ops as T; assert T.REGISTRATION == 'py'; "
            "print(json.dumps({n: str(getattr(torch.ops.regione_mi, n).default._schema) for n in T.BLOCK_SCHEMAS}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, RGN_TORCH_OPS="py"))
    assert r.returncode == 0, r.stderr[-3000:]
    py = json.loads(r.stdout.strip().splitlines()[-1])
    assert cpp == py and set(cpp) == set(NAMES)
    here = {n: str(getattr(torch.ops.regione_mi, n).default._schema) for n in NAMES}
    assert here == cpp


def test_the_region_op_table_keeps_its_eleven_names():
    """The block ops live in a table of their own, beside the unchanged region-op table."""
    assert T.registered_block_ops() == tuple(sorted(NAMES)) and set(T.BLOCK_SCHEMAS) == set(NAMES)
    assert len(T.registered()) == 11 and len(T.SCHEMAS) == 11 and not set(NAMES) & set(T.registered())
    assert not set(NAMES) & set(T.registered_row_ops())


def test_mutation_annotations_lists_and_defaults():
    for n in NAMES:
        s = str(getattr(torch.ops.regione_mi, n).default._schema)
        for part in ("Tensor(a!) x", "Tensor(b!) nrm", "Tensor(c!) wide", "Tensor(d!) k_cache", "Tensor(e!) vt_cache", "Tensor[] weights",
                     "Tensor?[] scales", "Tensor?[] biases", "Tensor[] norms", "Tensor? kv_rows", "int T", "int M", "int heads", "int skv",
                     "float score_bound", "bool rowbands=False", "-> ()"):
            assert part in s, (n, part, s)
    assert "Tensor adaln_img, Tensor adaln_txt" in str(torch.ops.regione_mi.mmdit_double_block_.default._schema)


def _args(single, device, d=256, heads=2, ff=1024, T=8, M=24, rows=None):
    bf = dict(dtype=torch.bfloat16, device=device)
    R = T + M
    x, nrm, wide = torch.zeros(R, d, **bf), torch.zeros(R, d, **bf), torch.zeros(R, 3 * d + ff, **bf)
    shapes = ((3 * d + ff, d), (d, d + ff)) if single else ((3 * d, d), (3 * d, d), (d, d), (d, d), (ff, d), (ff, d), (d, ff), (d, ff))
    weights = [torch.zeros(*s, **bf) for s in shapes]
    biases = [torch.zeros(s[0], **bf) for s in shapes]
    norms = [torch.ones(128, **bf) for _ in range(2 if single else 4)]
    rope = [torch.zeros(R, 128, dtype=torch.float32, device=device) for _ in range(4)]
    k, vt = torch.zeros(64, d, **bf), torch.zeros(d, 64, **bf)
    ada = [torch.zeros(3 * d, **bf)] if single else [torch.zeros(6 * d, **bf), torch.zeros(6 * d, **bf)]
    return [x, nrm, wide, *ada, weights, [], biases, norms, *rope, rows, k, vt, T, M, heads, R, 0.0, False]


@pytest.mark.parametrize("single", [False, True])
def test_fake_kernels_return_none_and_touch_nothing(single):
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = getattr(torch.ops.regione_mi, NAMES[single])
    with FakeTensorMode():
        assert op(*_args(single, "cuda")) is None


@pytest.mark.parametrize("single", [False, True])
def test_a_cpu_tensor_fails_loudly(single):
    with pytest.raises((NotImplementedError, RuntimeError)):
        getattr(torch.ops.regione_mi, NAMES[single])(*_args(single, "cpu"))


def test_struct_size_matches_the_ctypes_mirror():
    h = _lib.lib()
    assert h.rgn_mmdit_block_bytes() == ctypes.sizeof(_lib.MmditBlock)
    assert h.rgn_version() >= 115                       # the ABI version that introduced the block entries


P = 0x10000             # a plausible, 16-byte aligned, never dereferenced address


def _desc(**kw):
    b = _lib.MmditBlock()
    for n in ("x", "nrm", "wide", "adaln", "adaln_txt", "norm_q", "norm_k", "norm_added_q", "norm_added_k", "k_slab", "vt_slab", "cos_q", "sin_q",
              "cos_k", "sin_k"):
        setattr(b, n, P)
    for n in T.DOUBLE_WEIGHTS + T.SINGLE_WEIGHTS:
        setattr(b, n, _lib.BlockWeight(P, None, P))
    b.ldx, b.ldnrm, b.ldwide = 256, 256, 3 * 256 + 1024
    b.T, b.M, b.d, b.d_ff, b.heads = 8, 24, 256, 1024, 2
    b.skv, b.skv_pad, b.score_bound, b.rowbands, b.out_rows, b.branches = 32, 64, 0.0, 0, 0, 1
    for k, v in kw.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("entry", ["rgn_mmdit_double_block", "rgn_mmdit_single_block"])
def test_argument_validation_returns_codes_and_messages_without_touching_the_gpu(entry):
    """Every refusal comes back before the first launch: the addresses in the descriptor are never dereferenced (there is no GPU here, and
    a launch would fail with a HIP error code > 0 instead of the negative RGN_E_* the assertions ask for)."""
    h = _lib.lib()
    fn = getattr(h, entry)
    single = entry.endswith("single_block")

    def run(**kw):
        rc = fn(ctypes.byref(_desc(**kw)), None)
        return rc, h.rgn_last_error().decode()
    BAD, UNSUP = -1, -2
    assert fn(None, None) == BAD
    for buf in ("x", "nrm", "wide", "k_slab", "vt_slab", "cos_q", "sin_k", "adaln", "norm_q", "norm_k"):
        rc, msg = run(**{buf: None})
        assert rc == BAD and "null" in msg.lower(), (buf, rc, msg)
    if not single:
        for buf in ("adaln_txt", "norm_added_q", "norm_added_k"):
            assert run(**{buf: None})[0] == BAD, buf
    assert run(**{("w_po" if single else "ff_w2"): _lib.BlockWeight(None, None, P)})[0] == BAD
    rc, msg = run(d=288, heads=2)
    assert rc == BAD and "64" in msg                                        # d % 64 != 0
    rc, msg = run(d=512, heads=2)
    assert rc == BAD and "heads * 128" in msg
    assert run(T=-1)[0] == BAD and run(M=0)[0] == BAD and run(M=-3)[0] == BAD
    for buf in ("x", "wide", "adaln", "k_slab", "cos_k"):
        rc, msg = run(**{buf: P + 2})
        assert rc == BAD and "aligned" in msg, (buf, rc, msg)
    assert run(**{("w_kvqm" if single else "w_out"): _lib.BlockWeight(P + 8, None, P)})[0] == BAD
    for ld in ("ldx", "ldnrm", "ldwide"):
        rc, msg = run(**{ld: getattr(_desc(), ld) + 4})
        assert rc == BAD and "strides" in msg, (ld, rc, msg)
    rc, msg = run(skv=65, skv_pad=64)
    assert rc == BAD and "skv_pad" in msg
    assert run(skv_pad=0)[0] == BAD and run(T=48, M=24)[0] == BAD          # identity rows past the slab
    # what stays with the caller
    rc, msg = run(d=384, heads=3, ldx=384, ldnrm=384, ldwide=3 * 384 + 1024)
    assert rc == UNSUP and "odd head count" in msg
    rc, msg = run(out_rows=16)
    assert rc == UNSUP and "out_rows" in msg
    rc, msg = run(branches=2)
    assert rc == UNSUP and "CFG branches" in msg
    mixed = {("w_po" if single else "w_out"): _lib.BlockWeight(P, P, P)}
    rc, msg = run(**mixed)
    assert rc == UNSUP and "same format" in msg


def test_block_ops_option_is_off_by_default_and_declared_per_trunk():
    """`harness.flux.BLOCK_OPS` is a plain module attribute, default False; the FLUX and Step1X trunks declare their blocks covered, the
    Qwen trunk (its double-stream block is out of scope) does not, and a context no forward has marked never takes the op path."""
    from regione_amd.harness import flux as H, qwen as HQ, step1x as HS
    assert H.BLOCK_OPS is False
    assert H.FluxTransformer2DModel.block_ops is True and HS.Step1XEditTransformer2DModel.block_ops is True
    assert HQ.QwenImageTransformer2DModel.block_ops is False
    assert H.FwdCtx(None, 0, 1, None).block_ops is False
