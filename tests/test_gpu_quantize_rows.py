"""-m gpu: the fp8 row quantiser (csrc/norm.hip) bit for bit.

  * rgn_quantize_rows_a8 equals the torch expression evaluated on the CPU - scale = max(amax|x|, 1e-12) / 448 per row in fp32,
    q = e4m3fn(f32(x) / scale) - in every code and every scale, on the rows of A.quant_rows (randn, all-zero, a single non-zero, values
    at every e4m3fn rounding tie after scaling, subnormal results, amax in the last column, amax below the clamp), d in {128, 3072},
    M in {1, 65} (one wave of a block / a last block of one row), ld > K on both sides, through ops and through torch.ops.regione_mi;
  * rgn_ln_modulate_a8 (plain, split_row, four segments) equals rgn_quantize_rows_a8(rgn_ln_modulate(...)) bit for bit, on both
    LN kernels (d = 3072: one wave per row; d = 128: one block per row), dense and with ld > d;
  * the destination keeps its sentinel outside the rows and columns named."""
import pytest
import torch

import gemm_a8_model as A
from regione_amd import _lib, ops
from regione_amd import torch_ops  # noqa: F401  (registers torch.ops.regione_mi)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5a


def _rows(M, d, seed=0):
    """[M, d] bf16 on the CPU: the named rows of A.quant_rows first, N(0, 1) rows of mixed magnitude behind them."""
    named = list(A.quant_rows(d, seed).values())
    g = torch.Generator().manual_seed(5 + seed)
    rest = [torch.randn(d, generator=g) * 4.0 ** (i % 5 - 2) for i in range(max(0, M - len(named)))]
    return torch.stack((named + [r.to(torch.bfloat16) for r in rest])[:M]).contiguous()


def _want(x):
    q, s = A.quantize_rows(x.cpu())
    return q, s


def _framed_out(M, d, pad):
    """fp8 [M, d] view (row stride d + pad) into a sentinel-filled buffer 3 rows longer, with a sentinel-framed scale vector."""
    buf = torch.full((M + 3, d + pad), SENT, dtype=torch.uint8, device=DEV)
    sc = torch.full((M + 16,), -7.0, dtype=torch.float32, device=DEV)
    out = buf[:M, :d].view(ops.FP8)
    out._rgn_scale = sc[:M]
    return buf, sc, out


def _check(buf, sc, M, d, q, s, what):
    assert torch.equal(buf[:M, :d].cpu(), q), f"{what}: codes differ in {int((buf[:M, :d].cpu() != q).sum())} places"
    assert torch.equal(sc[:M].cpu().view(torch.int32), s.view(torch.int32)), f"{what}: scales differ"
    frame = buf.clone()
    frame[:M, :d] = SENT
    assert bool((frame == SENT).all()) and bool((sc[M:] == -7.0).all()), f"{what}: wrote outside the named rows / columns"


@pytest.mark.parametrize("d", [128, 3072])
@pytest.mark.parametrize("M", [1, 65])
def test_quantize_rows_a8_is_the_torch_expression(M, d):
    x = _rows(M, d)
    q, s = _want(x)
    got = ops.quantize_rows_a8(x.to(DEV))
    assert got.dtype == ops.FP8 and torch.equal(got.view(torch.uint8).cpu(), q)
    assert torch.equal(got._rgn_scale.cpu().view(torch.int32), s.view(torch.int32))
    # ld > K on both sides, sentinel frame
    wide = torch.full((M + 2, d + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:M, :d] = x.to(DEV)
    buf, sc, out = _framed_out(M, d, 40)
    assert ops.quantize_rows_a8(wide[:M, :d], out=out) is out
    _check(buf, sc, M, d, q, s, "strided")
    # the registered op
    tq, ts = torch.ops.regione_mi.quantize_rows_a8(x.to(DEV))
    assert torch.equal(tq.view(torch.uint8).cpu(), q) and torch.equal(ts.cpu().view(torch.int32), s.view(torch.int32))
    # slices keep their scales
    if M > 1:
        part = ops.arows(got, 3, 20)
        assert torch.equal(part._rgn_scale, got._rgn_scale[3:20]) and part.data_ptr() == got[3:20].data_ptr()


def test_quantize_rows_a8_argument_checks():
    x = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_a8(x.float())
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_a8(x, out=torch.zeros(4, 128, dtype=torch.uint8, device=DEV).view(ops.FP8))          # no `_rgn_scale`
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_a8(x[:, :100].contiguous())                                                           # K % 8
    bad = torch.zeros(4, 128, dtype=torch.uint8, device=DEV).view(ops.FP8)
    bad._rgn_scale = torch.zeros(3, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.RegionEHipError):
        ops.quantize_rows_a8(x, out=bad)


def _mods(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return [((torch.randn(d, generator=g) * 0.5).to(torch.bfloat16).to(DEV), (torch.randn(d, generator=g) * 0.5).to(torch.bfloat16).to(DEV)) for _ in range(n)]


@pytest.mark.parametrize("d", [128, 3072])
@pytest.mark.parametrize("M", [1, 65])
def test_ln_modulate_a8_is_quantize_rows_of_ln_modulate(M, d):
    g = torch.Generator().manual_seed(11 * M + d)
    x = (torch.randn(M, d, generator=g) * 3 + 0.5).to(torch.bfloat16)
    x[0, :] = 0                                                       # a constant row: LN output 0, the quantised row is the shift alone
    xw = torch.zeros(M + 1, d + 16, dtype=torch.bfloat16, device=DEV)
    xw[:M, :d] = x.to(DEV)
    (sh0, sc0), (sh1, sc1), (sh2, sc2), (sh3, sc3) = _mods(4, d, 3)
    variants = {"plain": lambda xx, out: ops.ln_modulate(xx, out, sh1, sc1),
                "split_row": lambda xx, out: ops.ln_modulate(xx, out, sh1, sc1, split_row=M // 3, shift0=sh0, scale0=sc0)}
    if M >= 4:
        ends = [M // 5, M // 2, M // 2 + 1, M]
        variants["four_segments"] = lambda xx, out: ops.ln_modulate_segs(xx, out, list(zip(ends, (sh0, sh1, sh2, sh3), (sc0, sc1, sc2, sc3))))
    for name, fn in variants.items():
        for xx in (x.to(DEV), xw[:M, :d]):
            ref = fn(xx, torch.empty(M, d, dtype=torch.bfloat16, device=DEV))
            want = ops.quantize_rows_a8(ref)
            buf, sc, out = _framed_out(M, d, 16)
            fn(xx, out)
            _check(buf, sc, M, d, want.view(torch.uint8).cpu(), want._rgn_scale.cpu(), f"{name} d={d}")
            # and the two-step result is the torch expression of the bf16 rows
            q, s = _want(ref)
            assert torch.equal(want.view(torch.uint8).cpu(), q) and torch.equal(want._rgn_scale.cpu().view(torch.int32), s.view(torch.int32))
