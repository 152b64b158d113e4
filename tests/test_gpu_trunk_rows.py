"""-m gpu: the trunk's row kernels (csrc/norm.hip) and the fused Q/K/V epilogue (csrc/gemm.hip) against the CPU model of
tests/trunk_rows_model.py - tests/test_trunk_rows_model.py shows that every named defect fails one of these checks.

  AdaLN   exact probes (bits) through ops.ln_modulate (plain, split_row at 1 and M - 1) and ops.ln_modulate_segs (1 - 4 segments, eps = 0)
          at every width of T.D_ALL: the block-per-row kernel at d = 8 / 256 / 520 / 2560 / 4808 / 8192 (1 - 4 column passes, a partial
          last one, the d <= 8192 limit) and ln_modulate_wave_kernel<1, 2, 3, 4, 6, 8> at d = 512 / 1024 / 1536 / 2048 / 3072 / 4096;
          the element-wise interval on seeded random rows (M = 1 / 5 / 67, centred and offset rows, four segments, strided, canaries);
          the fp8 form == quantize_rows_a8 of the bf16 rows at the same widths (both `_a8` kernels, every instantiation).
  Q/K/V   exact probes (bits, whole buffers: Q in place, the K slab, the V^T slab, every canary) for H = 1 / 3, M = 1 / 63 / 64 / 65 / 130,
          identity and gathered cache rows, split_row, unpaired tables, moved column blocks; separate roundings versus fma; the interval
          on a random case; the same probes through ops.gemm_qkv with an identity weight, on each of the three tile variants."""
import faulthandler
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_a8_model as A  # noqa: E402
import plan_helpers as P  # noqa: E402
import trunk_rows_model as T  # noqa: E402
from oracle import regione_oracle as O  # noqa: E402
from regione_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5a


@pytest.fixture(autouse=True)
def _time_limit():
    """Each test here is a handful of tiny launches: one that has not returned after a minute hangs - end the process, with a traceback."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(DEV)


def _f64(t):
    return t.float().cpu().double().numpy()


def _f32dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _same_bits(got, want_f64):
    return torch.equal(got.cpu().view(torch.int16), _bf(want_f64).cpu().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------------------
# AdaLN
# ------------------------------------------------------------------------------------------------------------------------------------
def _run_ln(api, xv, ov, seg_end, shift, scale, eps):
    if api == "plain":
        ops.ln_modulate(xv, ov, shift[0], scale[0], eps=eps)
    elif api == "split":
        ops.ln_modulate(xv, ov, shift[1], scale[1], split_row=seg_end[0], shift0=shift[0], scale0=scale[0], eps=eps)
    else:
        ops.ln_modulate_segs(xv, ov, list(zip(seg_end, shift, scale)), eps=eps)


@pytest.mark.parametrize("d", T.D_ALL)
def test_ln_exact_probes_equal_the_model_bit_for_bit(d):
    for p in T.ln_probes(d):
        x, out = _bf(p.x), _bf(p.out0)
        assert _same_bits(x, p.x) and _same_bits(out, p.out0)                        # the probe's values ARE bf16 values
        _run_ln(p.api, x.as_strided((p.M, d), (p.ldx, 1)), out.as_strided((p.M, d), (p.ldo, 1)), p.seg_end,
                [_bf(v) for v in p.shift], [_bf(v) for v in p.scale], p.eps)
        torch.cuda.synchronize()
        diff = (_f64(out) != p.expected)
        assert not diff.any(), (p.name, int(diff.sum()), np.flatnonzero(diff)[:8].tolist())
        assert _same_bits(out, p.expected) and _same_bits(x, p.x), p.name          # signed zeros too; x is read only


@pytest.mark.parametrize("d", T.D_ALL)
def test_ln_interval_on_seeded_random_rows(d):
    for dd, M, fam in T.ln_random_grid():
        if dd != d:
            continue
        x, seg_end, shift, scale = T.ln_random_case(d, M, fam)
        xw = torch.full((M + 1, d + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        xw[:M, :d] = _bf(x)
        buf = torch.full((M + 2, d + 16), 77.0, dtype=torch.bfloat16, device=DEV)
        ops.ln_modulate_segs(xw[:M, :d], buf[:M, :d], list(zip(seg_end, [_bf(v) for v in shift], [_bf(v) for v in scale])))
        torch.cuda.synchronize()
        out = _f64(buf[:M, :d])
        lo, hi = T.ln_interval(x, seg_end, shift, scale)
        bad = (out < lo) | (out > hi) | ~np.isfinite(out)
        assert not bad.any(), (d, M, fam, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        buf[:M, :d] = 77.0
        assert bool((buf == 77.0).all()), (d, M, fam, "wrote outside its rows / columns")
        # the two-segment entry point on the same rows: the same interval
        if M > 1:
            o2 = torch.empty(M, d, dtype=torch.bfloat16, device=DEV)
            ops.ln_modulate(xw[:M, :d], o2, _bf(shift[3]), _bf(scale[3]), split_row=seg_end[0], shift0=_bf(shift[0]), scale0=_bf(scale[0]))
            lo2, hi2 = T.ln_interval(x, [seg_end[0], M], [shift[0], shift[3]], [scale[0], scale[3]])
            o2 = _f64(o2)
            assert ((lo2 <= o2) & (o2 <= hi2)).all(), (d, M, fam, "split_row")


def _framed_out(M, d, pad):
    buf = torch.full((M + 3, d + pad), SENT, dtype=torch.uint8, device=DEV)
    sc = torch.full((M + 16,), -7.0, dtype=torch.float32, device=DEV)
    out = buf[:M, :d].view(ops.FP8)
    out._rgn_scale = sc[:M]
    return buf, sc, out


@pytest.mark.parametrize("d", T.D_ALL)
def test_ln_fp8_form_is_quantize_rows_a8_of_the_bf16_rows(d):
    for M in (1, 67):
        x, seg_end, shift, scale = T.ln_random_case(d, M, "centred")
        xd, sh, sc = _bf(x), [_bf(v) for v in shift], [_bf(v) for v in scale]
        for name, fn in (("plain", lambda o: ops.ln_modulate(xd, o, sh[1], sc[1])),
                         ("segs", lambda o: ops.ln_modulate_segs(xd, o, list(zip(seg_end, sh, sc))))):
            ref = fn(torch.empty(M, d, dtype=torch.bfloat16, device=DEV))
            want = ops.quantize_rows_a8(ref)
            buf, rs, out = _framed_out(M, d, 16)
            fn(out)
            torch.cuda.synchronize()
            what = f"{name} d={d} M={M}"
            assert torch.equal(buf[:M, :d], want.view(torch.uint8)), f"{what}: codes differ in {int((buf[:M, :d] != want.view(torch.uint8)).sum())} places"
            assert torch.equal(rs[:M].view(torch.int32), want._rgn_scale.view(torch.int32)), f"{what}: scales differ"
            buf[:M, :d] = SENT
            assert bool((buf == SENT).all()) and bool((rs[M:] == -7.0).all()), f"{what}: wrote outside the named rows / columns"
            q, s = A.quantize_rows(ref.cpu())                                         # and both are the torch expression of the bf16 rows
            assert torch.equal(want.view(torch.uint8).cpu(), q) and torch.equal(want._rgn_scale.cpu().view(torch.int32), s.view(torch.int32)), what


# ------------------------------------------------------------------------------------------------------------------------------------
# Q/K/V
# ------------------------------------------------------------------------------------------------------------------------------------
def _qk_device(p):
    w = [None if v is None else _bf(v) for v in (p.wq0, p.wk0, p.wq1, p.wk1)]
    rope_q, rope_k = tuple(_f32dev(t) for t in p.rope_q), tuple(_f32dev(t) for t in p.rope_k)
    kv_rows = None if p.kv_rows is None else torch.from_numpy(p.kv_rows).to(DEV)
    return w, rope_q, rope_k, kv_rows


def _run_qk(p):
    """The stand-alone kernels on a probe's buffers -> (qkv, k_slab, vt_slab) as fp64 arrays."""
    (wq0, wk0, wq1, wk1), rope_q, rope_k, kv_rows = _qk_device(p)
    # every index the kernels will use lies inside its table / slab (checked here: the values of kv_rows are device data to them)
    rows = np.arange(p.M) if p.kv_rows is None else p.kv_rows
    assert rows.max() < min(p.rope_k[0].shape[0], p.k0.shape[0]) and p.rope_q[0].shape[0] >= p.M and len(rows) >= p.M
    assert max(p.k_col, p.v_col, p.q_col) + p.H * 128 <= p.ld == p.qkv0.shape[1]
    qkv, k, vt = _bf(p.qkv0), _bf(p.k0), _bf(p.vt0)
    ops.qk_norm_rope_store(qkv, p.k_col, p.v_col, p.q_col, p.H, wq1, wk1, rope_q, rope_k, k, vt, kv_rows, split_row=p.split_row,
                           wq0=wq0, wk0=wk0, eps=p.eps)
    torch.cuda.synchronize()
    return qkv, k, vt


def _assert_bits(p, got, what=""):
    for name, g, e in zip(("qkv", "k_slab", "vt_slab"), got, p.expected):
        diff = _f64(g) != e
        assert not diff.any(), (p.name, what, name, int(diff.sum()), np.argwhere(diff)[:6].tolist())
        assert _same_bits(g, e), (p.name, what, name, "signed zero")


_QK_PROBES = {H: T.qk_probes(H) for H in T.QK_PROBE_H}


@pytest.mark.parametrize("H,i", [(H, i) for H in T.QK_PROBE_H for i in range(len(_QK_PROBES[H]))],
                         ids=[p.name for H in T.QK_PROBE_H for p in _QK_PROBES[H]])
def test_qk_exact_probes_and_canaries_equal_the_model_bit_for_bit(H, i):
    """Whole-buffer comparison: Q in place, K rows kv_rows[:M], V^T columns kvpos(kv_rows[:M]) hold the model's bits; the K / V columns and
    the pad columns of `qkv`, every other slab row / column ([skv, skv_pad) included) hold the non-zero prefill."""
    p = _QK_PROBES[H][i]
    _assert_bits(p, _run_qk(p))


def test_qk_rotation_rounds_each_product_and_the_sum_separately():
    p = T.qk_fma_probe()
    _assert_bits(p, _run_qk(p))


@pytest.mark.parametrize("tables", ["uniform_angles", "flux_pos_embed"])
def test_qk_interval_on_a_random_case_with_gathered_rows_split_row_and_distinct_tables(tables):
    """Real tables: the oracle's flux_pos_embed on synthetic ids (a text prefix, then image grids that differ between the queries and
    the cache), and tables of uniform random angles; the cap on ambiguous elements is checked on both by test_trunk_rows_model.py."""
    p = T.qk_random_case()
    if tables == "flux_pos_embed":
        p = T.qk_random_case(*(tuple(t.numpy() for t in O.flux_pos_embed(torch.from_numpy(ids))) for ids in T.qk_random_ids()))
    qkv, k, vt = _run_qk(p)
    assert T.qk_accept(p, _f64(qkv), _f64(k), _f64(vt)) == 0


@pytest.mark.parametrize("variant", ["128", "256c", "256"])
def test_fused_qkv_epilogue_on_the_exact_probes_equals_the_model(variant):
    """ops.gemm_qkv with A = the probe rows, W = the identity, zero bias: the GEMM result IS the probe, the epilogue must produce the
    model's bits (not merely the stand-alone kernel's): Q in C, K and V^T in the slabs; the K / V columns of C and the rest of the slabs
    keep their prefill."""
    H = 2
    D, N = H * 128, 3 * H * 128
    W = torch.eye(N, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    for p in (T.qk_probe(65, H, True, standard=True), T.qk_probe(130, H, False, standard=True), T.qk_fma_probe(H, standard=True)):
        P.geometry(variant)
        (_, _, wq, wk), rope_q, rope_k, kv_rows = _qk_device(p)
        Ad, k, vt = _bf(p.qkv0), _bf(p.k0), _bf(p.vt0)
        out = torch.full((p.M, N), 99.0, dtype=torch.bfloat16, device=DEV)
        epi = ops.qkv_epilogue(wq=wq, wk=wk, rope_q=rope_q, rope_k=rope_k, k_slab=k, vt_slab=vt, H=H, k_col=p.k_col, v_col=p.v_col,
                               q_col=p.q_col, kv_rows=kv_rows, eps=p.eps, rows=p.M)
        ops.gemm_qkv(Ad, W, bias, out, epi)
        torch.cuda.synchronize()
        eq, ek, ev = p.expected
        dq = _f64(out[:, p.q_col:]) != eq[:, p.q_col:]
        assert not dq.any(), (p.name, variant, "Q", int(dq.sum()), np.argwhere(dq)[:6].tolist())
        assert bool((out[:, :p.q_col] == 99.0).all()), (p.name, variant, "K / V columns of C written")
        for name, g, e in (("k_slab", k, ek), ("vt_slab", vt, ev)):
            diff = _f64(g) != e
            assert not diff.any(), (p.name, variant, name, int(diff.sum()), np.argwhere(diff)[:6].tolist())
        assert _same_bits(Ad, p.qkv0)
