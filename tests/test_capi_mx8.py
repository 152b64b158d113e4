"""CPU-side checks of the mx8 boundary: include/regione_hip.h declares rgn_quantize_rows_mx8, the built library exports it, _lib.py types
it, the dispatcher knows `regione_mi.quantize_rows_mx8` with a fake kernel, and the entry validates before it launches (no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

from regione_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "rgn_quantize_rows_mx8"


def test_header_library_and_ctypes_table_agree_on_the_entry():
    text = open(os.path.join(ROOT, "include", "regione_hip.h")).read()
    decl = re.search(r"\bint\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert decl, f"{ENTRY} is not declared in include/regione_hip.h"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["x", "ldx", "q", "ldq", "s", "lds", "col0", "M", "K", "stream"]
    assert '"mx8 rows"' in text                                  # the format is stated in the header, once
    h = ctypes.CDLL(build.build_lib())
    assert hasattr(h, ENTRY), f"{ENTRY} declared but not exported"
    sig = _lib.SIGNATURES[ENTRY]
    assert len(sig) == len(params)
    for p, c in zip(params, sig):                                # pointers as void*, the rest as int
        assert c is (ctypes.c_void_p if "*" in p else ctypes.c_int), p
    assert int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 120


def test_the_entry_validates_before_it_launches():
    h = _lib.lib()
    P = 0x10000                                                  # plausible, 16-byte aligned, never dereferenced

    def call(x=P, ldx=256, q=P, ldq=256, s=P, lds=8, col0=0, M=4, K=256):
        return h.rgn_quantize_rows_mx8(x, ldx, q, ldq, s, lds, col0, M, K, None)

    def msg():
        return h.rgn_last_error().decode()
    assert call(M=0) == 0 and call(M=0, x=None) == 0             # nothing to do
    assert call(K=192) == -1 and "multiple of 128" in msg()      # RGN_E_BADARG
    assert call(K=0) < 0 and call(M=-1) < 0 and call(x=None) < 0 and call(x=P + 8) < 0 and call(ldx=128) < 0 and call(ldx=260) < 0
    assert call(col0=64) < 0 and "column offset" in msg()
    assert call(col0=-128) < 0 and call(col0=2 ** 31 - 128) < 0
    assert call(q=None) < 0 and call(q=P + 8) < 0 and call(ldq=264) < 0 and "16-byte" in msg()
    assert call(col0=128, ldq=256) < 0                           # the offset rows do not fit the destination
    assert call(s=None) < 0 and call(s=P + 2) < 0 and call(lds=6) < 0 and call(lds=4) < 0 and "4-byte" in msg()
    assert call(col0=128, ldq=384, lds=8) < 0                    # (col0 + K) / 32 = 12 scale bytes per row


def test_the_op_is_registered_with_a_fake_kernel():
    import regione_amd.torch_ops as T
    assert "quantize_rows_mx8" in T.A8_SCHEMAS and T.A8_SCHEMAS["quantize_rows_mx8"] == "(Tensor x) -> (Tensor, Tensor)"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty((7, 384), dtype=torch.bfloat16, device="cuda")
        q, s = torch.ops.regione_mi.quantize_rows_mx8(x)
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (7, 384)
    assert s.dtype == torch.uint8 and tuple(s.shape) == (7, 12)


def test_the_wrapper_refuses_before_it_reaches_the_library():
    from regione_amd import ops
    with pytest.raises(_lib.RegionEHipError, match="bf16"):
        ops.quantize_rows_mx8(torch.zeros(4, 128))
    with pytest.raises(_lib.RegionEHipError, match="multiple of 128"):
        ops.quantize_rows_mx8(torch.zeros(4, 96, dtype=torch.bfloat16))
    with pytest.raises(_lib.RegionEHipError, match="multiple of 128"):
        ops.mx8_rows(4, 96, "cpu")
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="needs the `out`"):
        ops.quantize_rows_mx8(x, col=128)
    bare = torch.zeros(4, 256, dtype=torch.uint8).view(ops.FP8)
    with pytest.raises(_lib.RegionEHipError, match="_rgn_mx_scale"):
        ops.quantize_rows_mx8(x, out=bare)
    with pytest.raises(_lib.RegionEHipError, match="_rgn_mx_scale"):
        ops.mx8_arows(bare, 0, 2)
    out = ops.mx8_rows(4, 256, "cpu")
    assert out._rgn_mx_scale.shape == (4, 8) and not hasattr(out, "_rgn_scale")
    with pytest.raises(_lib.RegionEHipError, match=">= 384"):
        ops.quantize_rows_mx8(x, out=out, col=256)               # columns [256, 384) of a 256-column buffer
    band = ops.mx8_arows(out, 1, 3)
    assert band.data_ptr() == out[1:3].data_ptr() and band._rgn_mx_scale.data_ptr() == out._rgn_mx_scale[1:3].data_ptr()
