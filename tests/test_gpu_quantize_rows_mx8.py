"""rgn_quantize_rows_mx8 against the numpy specification (tests/gemm_mx8_model.py), bit for bit, bytes and scales:

  * every finite bf16 exponent (subnormals included) as block amax, at the mantissas around the 1.75 threshold, with the amax in the
    first, the last and a middle slot of its block; zero blocks, -0, values that round up to 448, every e4m3fn tie, ordinary data;
  * M in {1, 63, 130}: one row; a ragged last workgroup and a ragged last pass of 512 columns; the whole pool, two passes per row;
  * x with a row stride above K, a destination wider than K (ldq > K), a destination column offset - and every byte around what the
    launch owns (columns left and right of it, the rows past M, the scale bytes alike) still holds its sentinel;
  * a second call writes the same bytes; the ctypes wrapper, the registered op and a launch per row band agree.
The mutants of the model (tests/test_gemm_mx8_model.py) each change these inputs' outputs, so none of those defects passes here."""
import numpy as np
import pytest
import torch

import gemm_mx8_model as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
QS, SS = 0xA5, 0x5A                              # sentinels: a finite fp8 code, an in-range scale - neither is special to the kernel


@pytest.fixture(scope="module")
def ops():
    from regione_amd import ops as o
    import regione_amd.torch_ops                                 # noqa: F401 - registers torch.ops.regione_mi.*
    return o


_ref = {}


def reference(M, K, off):
    """(bf16 bits, codes, scales) of a probe shape - computed once, never written to."""
    if (M, K, off) not in _ref:
        x = X.rows(M, K, off)
        q, s = X.quantize_rows(x)
        for a in (x, q, s):
            a.setflags(write=False)
        _ref[(M, K, off)] = (x, q, s)
    return _ref[(M, K, off)]


def bf16_tensor(bits, ldx=None):
    """bf16 bits [M, K] -> a bf16 device tensor [M, K] with row stride ldx (elements)."""
    M, K = bits.shape
    buf = torch.zeros((M, ldx or K), dtype=torch.int16)
    buf[:, :K] = torch.from_numpy(bits.view(np.int16).copy())
    return buf.view(torch.bfloat16).to(DEV)[:, :K]


def framed(ops, M, W, extra_rows=2):
    """An mx8 buffer [M, W] that is the top-left part of sentinel-filled allocations with `extra_rows` more rows."""
    qa = torch.full((M + extra_rows, W), QS, dtype=torch.uint8, device=DEV)
    sa = torch.full((M + extra_rows, W // 32), SS, dtype=torch.uint8, device=DEV)
    out = qa[:M].view(ops.FP8)
    out._rgn_mx_scale = sa[:M]
    return out, qa, sa


def same(got, want, what):
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}"


@pytest.mark.parametrize("M,K,off", X.SHAPES)
def test_the_kernel_equals_the_model_bit_for_bit(ops, M, K, off):
    x, q, s = reference(M, K, off)
    xd = bf16_tensor(x)
    got = ops.quantize_rows_mx8(xd)
    assert got.dtype == ops.FP8 and tuple(got.shape) == (M, K) and tuple(got._rgn_mx_scale.shape) == (M, K // 32)
    same(got.view(torch.uint8), q, "codes")
    same(got._rgn_mx_scale, s, "scales")
    again = ops.quantize_rows_mx8(xd)                            # a repeated call is identical
    assert torch.equal(again.view(torch.uint8), got.view(torch.uint8)) and torch.equal(again._rgn_mx_scale, got._rgn_mx_scale)
    tq, ts = torch.ops.regione_mi.quantize_rows_mx8(xd)          # the registered op
    assert torch.equal(tq.view(torch.uint8), got.view(torch.uint8)) and torch.equal(ts, got._rgn_mx_scale)


@pytest.mark.parametrize("M,K,off", X.SHAPES)
def test_strides_column_offset_and_untouched_surroundings(ops, M, K, off):
    x, q, s = reference(M, K, off)
    xd = bf16_tensor(x, ldx=K + 24)                              # ldx > K, rows still 16-byte aligned
    assert xd.stride(0) == K + 24
    for col, W in ((0, K + 128), (256, K + 256 + 128), (128, K + 128)):     # ldq > K each time; left / right / both neighbours present
        out, qa, sa = framed(ops, M, W)
        assert ops.quantize_rows_mx8(xd, out=out, col=col) is out
        want_q = np.full((M + 2, W), QS, np.uint8)
        want_q[:M, col:col + K] = q
        want_s = np.full((M + 2, W // 32), SS, np.uint8)
        want_s[:M, col // 32:(col + K) // 32] = s
        same(qa, want_q, f"codes, col {col}")
        same(sa, want_s, f"scales, col {col}")
        ops.quantize_rows_mx8(xd, out=out, col=col)              # and again: the same bytes, the same surroundings
        same(qa, want_q, f"codes, col {col}, second call")
        same(sa, want_s, f"scales, col {col}, second call")


def test_row_bands_write_what_one_launch_writes(ops):
    M, K, off = X.SHAPES[0]
    x, q, s = reference(M, K, off)
    xd = bf16_tensor(x)
    out, qa, sa = framed(ops, M, K + 128)
    for lo, hi in ((0, 47), (47, 48), (48, M)):                  # bands that start on no multiple of the 4 rows of a workgroup
        ops.quantize_rows_mx8(xd[lo:hi], out=ops.mx8_arows(out, lo, hi), col=128)
    same(qa[:M, 128:], q, "codes")
    same(sa[:M, 4:], s, "scales")
    assert bool((qa[:, :128] == QS).all()) and bool((qa[M:] == QS).all()) and bool((sa[:, :4] == SS).all()) and bool((sa[M:] == SS).all())


def test_the_device_result_dequantises_to_the_input_within_the_format(ops):
    """Independent of the model's rounding: what the kernel wrote, decoded by torch, is the input within three mantissa bits, nothing
    above 448 X, and no smaller scale would have held the block's amax."""
    M, K, off = X.SHAPES[0]
    x, _, _ = reference(M, K, off)
    got = ops.quantize_rows_mx8(bf16_tensor(x))
    assert not bool(((got.view(torch.uint8) & 0x7f) == 0x7f).any()) and not bool((got._rgn_mx_scale == 255).any())
    sc = torch.exp2(got._rgn_mx_scale.double() - 127).repeat_interleave(32, dim=1).cpu()
    d = got.cpu().double() * sc
    v = torch.from_numpy(X.bf16_to_f64(x))
    assert bool(((d - v).abs() <= torch.maximum(2.0 ** -4 * v.abs(), 2.0 ** -10 * sc)).all())
    amax = v.abs().view(M, K // 32, 32).amax(dim=2)
    s1 = sc.view(M, K // 32, 32)[:, :, 0]
    b = got._rgn_mx_scale.cpu()
    assert bool((amax <= 448 * s1).all()) and bool(((amax > 224 * s1) | (b == 0) | (amax == 0)).all())
    assert bool((b[amax == 0] == 127).all())


def test_argument_checks(ops):
    from regione_amd import _lib
    x = torch.zeros(4, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_mx8(x[:, :192])                        # K % 128
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_mx8(x, out=ops.mx8_rows(4, 256, DEV), col=64)
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_mx8(x, out=ops.mx8_rows(3, 256, DEV))
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_mx8(x, out=ops.mx8_rows(4, 256, DEV), col=128)
    odd = torch.zeros(4, 264, dtype=torch.bfloat16, device=DEV)[:, 4:260]        # rows 8-byte aligned only
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_mx8(odd)
    assert tuple(ops.quantize_rows_mx8(x[:0]).shape) == (0, 256)
