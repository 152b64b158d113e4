"""The CPU model of the trunk's row kernels (tests/trunk_rows_model.py): the exact probes are exact (sums exactly representable in any
order, the one inexact stage >= 16 half-widths from a bf16 tie), the restated kernels meet them and lie inside the interval on the seeded
random cases, every NAMED DEFECT changes a probe or leaves the interval (CAUGHT_BY tabulates which), the share of ambiguous elements stays
under its cap on the very inputs tests/test_gpu_trunk_rows.py uses, and the model agrees with the oracle's eager op sequence."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trunk_rows_model as T  # noqa: E402
from oracle import regione_oracle as O  # noqa: E402

# which check sees which defect: "probe" = an exact probe changes, "bound" = a seeded random case leaves the interval
CAUGHT_BY = {
    "y0_not_rounded": {"probe", "bound"}, "one_plus_scale_not_rounded": {"probe", "bound"}, "y1_not_rounded": {"probe", "bound"},
    "variance_unbiased": {"probe", "bound"}, "eps_dropped": {"probe"}, "segment_end_inclusive": {"probe", "bound"},
    "chunk_modulation_offset_dropped": {"probe", "bound"}, "last_pass_skipped": {"probe"}, "ldo_ignored": {"probe"},
    "rms_over_row": {"probe", "bound"}, "norm_not_rounded_before_weight": {"probe", "bound"},
    "odd_lane_uses_even_table_entry": {"probe"}, "sin_sign_flipped": {"probe", "bound"}, "k_rotated_with_row_m": {"probe", "bound"},
    "k_stored_at_row_m": {"probe", "bound"}, "split_row_inclusive": {"probe", "bound"}, "fused_multiply_add": {"probe"},
    "vt_kvpos_identity": {"probe", "bound"}, "vt_tail_rows_written": {"probe", "bound"},
}


def _low_bit(values):
    """The largest power of two that divides every value (fp64 values with few significant bits)."""
    q = None
    for v in np.unique(np.abs(values[values != 0])):
        m, e = np.frexp(v)
        i = int(m * 2 ** 53)
        b = e - 53 + ((i & -i).bit_length() - 1)
        q = b if q is None else min(q, b)
    return 2.0 ** q


def _exact_in_any_order(v):
    """Every partial sum of v, in any order, is an integer below 2^24 times one power of two: exact in fp32."""
    return float(np.abs(v).sum() / _low_bit(v)) < 2 ** 24


def test_bf16_helpers():
    x = np.array([1.0, 257.0, 255.0, 1.00390625, 1.01171875, -3.3, 1e-40, 0.0, 65535.0, 0.447, -1.3416])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).double().numpy()
    assert np.array_equal(T.bf16_rne(T.f32(x)), want)
    assert T.bf16_tie_distance(1.0 + 2.0 ** -8) == 0.0 and T.bf16_tie_distance(1.0) == 2.0 ** -9       # the tie below 1 is nearer
    assert T.bf16_tie_distance(1.0 - 2.0 ** -9) == 0.0 and T.bf16_tie_distance(0.75) == 2.0 ** -9
    r = np.arange(64)
    assert np.array_equal(T.kvpos(T.kvpos(r)), r) and T.kvpos(4) == 8 and T.kvpos(12) == 12 and T.kvpos(21) == 25


# ------------------------------------------------------------------------------------------------------------------------------------
# AdaLN
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", T.D_ALL)
def test_ln_probes_are_exact_keep_their_margin_and_the_model_meets_them(d):
    worst = np.inf
    for p in T.ln_probes(d):
        X = p.rows()
        assert np.array_equal(T.bf16_rne(X), X) and all(np.array_equal(T.bf16_rne(v), v) for v in p.shift + p.scale)
        for r in range(p.M):
            assert _exact_in_any_order(X[r]), (p.name, r)
            mean = X[r].sum() / d
            assert T.f32(mean) == mean and _exact_in_any_order((X[r] - mean) ** 2), (p.name, r)
        ref, lo, hi = T.ln_y0_interval(X, p.eps)
        half = np.maximum(hi - ref, ref - lo)
        assert (T.bf16_tie_distance(ref) >= T.MARGIN * half).all(), p.name
        worst = min(worst, float((T.bf16_tie_distance(ref) / half).min()))
        # 1 + scale: more than 8 bits, never a tie
        for s in p.scale:
            assert (T.bf16_rne(1 + s) != 1 + s).all() and (T.bf16_tie_distance(1 + s) > 0).all()
        # expected bits = the fp64 chain, rounded where the contract rounds
        seg = T.ln_segment_of_rows(p.M, p.seg_end)
        want = T._ln_tail(T.bf16_rne(ref), np.stack(p.scale)[seg], np.stack(p.shift)[seg])
        got = np.stack([p.expected[r * p.ldo:r * p.ldo + d] for r in range(p.M)])
        assert np.array_equal(got, want), p.name
        lo_o, hi_o = T.ln_interval(X, p.seg_end, p.shift, p.scale, p.eps)
        assert np.array_equal(lo_o, hi_o) and np.array_equal(lo_o, got), p.name          # the interval is one bf16 value, this one
        keep = np.ones(len(p.out0), bool)
        for r in range(p.M):
            keep[r * p.ldo:r * p.ldo + d] = False
        assert np.array_equal(p.expected[keep], p.out0[keep])
        if len(p.seg_end) > 1:                                # the segments' vectors differ in every 8-column group
            for a, b in zip(p.shift[:-1] + p.scale[:-1], p.shift[1:] + p.scale[1:]):
                assert (a.reshape(-1, 8) != b.reshape(-1, 8)).any(1).all()
    print(f"d={d}: smallest tie distance / half-width over the probes = {worst:.1f}")


def _ln_inside(d, M, fam, defect=None):
    x, seg_end, shift, scale = T.ln_random_case(d, M, fam)
    out = T.ln_modulate(x.reshape(-1), d, np.zeros(M * d), d, M, d, T.EPS, seg_end, shift, scale, defect).reshape(M, d)
    lo, hi = T.ln_interval(x, seg_end, shift, scale)
    return ((lo <= out) & (out <= hi)).all(), int((lo != hi).sum()), lo.size


def test_ln_interval_holds_the_model_and_ambiguity_stays_under_its_cap_on_the_gpu_tests_inputs():
    amb, tot = {}, {}
    for d, M, fam in T.ln_random_grid():
        ok, a, n = _ln_inside(d, M, fam)
        assert ok, (d, M, fam)
        amb[fam, d], tot[fam, d] = amb.get((fam, d), 0) + a, tot.get((fam, d), 0) + n
    for fam in T.LN_FAMILIES:
        per_d = {d: amb[f, d] / tot[f, d] for (f, d) in amb if f == fam}
        share = sum(amb[f, d] for (f, d) in amb if f == fam) / sum(tot[f, d] for (f, d) in tot if f == fam)
        print(f"{fam}: ambiguous share {share:.4%}; per d: " + ", ".join(f"{d}: {s:.3%}" for d, s in sorted(per_d.items())))
        assert share <= T.AMBIGUITY_CAP[fam], (fam, share)
        assert all(s <= T.AMBIGUITY_CAP[fam] for s in per_d.values()), (fam, per_d)


_LN_DEFECT_CASES = [(520, 67, "centred"), (1024, 5, "centred"), (4808, 5, "centred"), (8, 67, "centred"), (2560, 5, "offset")]


@pytest.mark.parametrize("defect", T.LN_DEFECTS)
def test_every_named_ln_defect_is_caught(defect):
    seen = set()
    if any(not np.array_equal(p.run(defect), p.expected) for d in (8, 520, 1024, 4808) for p in T.ln_probes(d)):
        seen.add("probe")
    if defect not in ("ldo_ignored", "last_pass_skipped"):        # addressing defects: the probes' canaries are their check
        if any(not _ln_inside(d, M, fam, defect)[0] for d, M, fam in _LN_DEFECT_CASES):
            seen.add("bound")
    assert seen, f"nothing sees {defect}"
    assert seen == CAUGHT_BY[defect], (defect, seen)


@pytest.mark.parametrize("defect", ["chunk_modulation_offset_dropped", "last_pass_skipped"])
@pytest.mark.parametrize("d", [x for x in T.D_ALL if x > (512 if x in T.LN_WAVE_D else 2048)])
def test_pass_defects_are_seen_at_every_multi_pass_width(d, defect):
    assert any(not np.array_equal(p.run(defect), p.expected) for p in T.ln_probes(d))


@pytest.mark.parametrize("fam,d,M", [("centred", 520, 67), ("centred", 3072, 5), ("offset", 1024, 5)])
def test_ln_model_agrees_with_the_oracles_eager_sequence(fam, d, M):
    """O.layer_norm in fp32 on the CPU, then the eager bf16 ops (y0 to bf16, times bf16(1 + scale), plus shift): inside the interval."""
    x, seg_end, shift, scale = T.ln_random_case(d, M, fam)
    seg = T.ln_segment_of_rows(M, seg_end)
    bf = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16)
    y0 = O.layer_norm(bf(x).float(), T.EPS).to(torch.bfloat16)
    y = y0 * (1 + bf(np.stack(scale)[seg])) + bf(np.stack(shift)[seg])
    lo, hi = T.ln_interval(x, seg_end, shift, scale)
    out = y.double().numpy()
    assert ((lo <= out) & (out <= hi)).all(), int(((out < lo) | (out > hi)).sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# Q/K/V
# ------------------------------------------------------------------------------------------------------------------------------------
def _all_qk_probes():
    return [p for H in T.QK_PROBE_H for p in T.qk_probes(H)] + [T.qk_fma_probe(), T.qk_probe(65, 2, True, standard=True),
                                                                 T.qk_probe(130, 2, False, standard=True), T.qk_fma_probe(standard=True)]


def test_qk_probes_are_exact_keep_their_margin_and_the_model_meets_them():
    worst = np.inf
    for p in _all_qk_probes():
        D = p.H * 128
        for t in p.rope_q + p.rope_k:
            assert np.array_equal(T.f32(t), t)
        if not p.name.startswith("fma"):
            for tab in (p.rope_q, p.rope_k):                 # unpaired, Q tables differ from K tables
                assert (tab[0][:, 0::2] != tab[0][:, 1::2]).mean() > 0.9 and (tab[1][:, 0::2] != tab[1][:, 1::2]).mean() > 0.9
            assert not np.array_equal(p.rope_q[0], p.rope_k[0][:p.M])
        for col in (p.q_col, p.k_col):
            X = p.heads(col)
            assert all(_exact_in_any_order(X[m, h] ** 2) for m in range(p.M) for h in range(p.H)), p.name
            ref, lo, hi = T.qk_n_interval(X, p.eps)
            half = np.maximum(hi - ref, ref - lo)
            assert (T.bf16_tie_distance(ref) >= T.MARGIN * half).all(), p.name
            worst = min(worst, float((T.bf16_tie_distance(ref) / half).min()))
        # the rotation's two products and their sum are exact in fp32 (the fma probe: one product is inexact, by design - both operand
        # values are fixed, so is its single rounding): the final bf16 rounding sees one value whatever the implementation
        kr = np.arange(p.M) if p.kv_rows is None else p.kv_rows
        for col, tab, rows, w0, w1 in ((p.q_col, p.rope_q, np.arange(p.M), p.wq0, p.wq1), (p.k_col, p.rope_k, kr, p.wk0, p.wk1)):
            n = T._norm(p.heads(col), T._row_weights(p.M, p.split_row, w0, w1), p.eps)
            a, b, c, s = n[..., 0::2], n[..., 1::2], tab[0][rows][:, None, :], tab[1][rows][:, None, :]
            for t0, t1 in ((a * c[..., 0::2], -b * s[..., 0::2]), (b * c[..., 1::2], a * s[..., 1::2])):
                exact = np.array_equal(T.f32(t0), t0) and np.array_equal(T.f32(t1), t1) and np.array_equal(T.f32(t0 + t1), t0 + t1)
                assert exact != p.name.startswith("fma"), p.name
        # the restated kernel lies in the interval; everything else is untouched / a copy
        assert T.qk_accept(p, *p.expected) == 0, p.name
        q, k, vt = p.expected
        assert np.array_equal(vt[:, T.kvpos(kr)], p.qkv0[:, p.v_col:p.v_col + D].T)
        keep = np.ones(p.qkv0.shape, bool)
        keep[:, p.q_col:p.q_col + D] = False
        assert np.array_equal(q[keep], p.qkv0[keep])
        rows = np.ones(k.shape[0], bool)
        rows[kr] = False
        assert np.array_equal(k[rows], p.k0[rows]) and rows[p.skv:].all()
        cols = np.ones(vt.shape[1], bool)
        cols[T.kvpos(kr)] = False
        assert np.array_equal(vt[:, cols], p.vt0[:, cols])
        if p.kv_rows is not None and p.M > 2:
            assert (p.kv_rows >= p.M).any() and (np.diff(p.kv_rows) < 0).any()
    print(f"Q/K probes: smallest tie distance / half-width = {worst:.1f}")


def _flux_tables():
    return tuple(tuple(t.numpy() for t in O.flux_pos_embed(torch.from_numpy(ids))) for ids in T.qk_random_ids())


def _qk_random_case(tables):
    return T.qk_random_case(*_flux_tables()) if tables == "flux_pos_embed" else T.qk_random_case()


@pytest.mark.parametrize("tables", ["uniform_angles", "flux_pos_embed"])
def test_qk_interval_holds_the_model_and_ambiguity_stays_under_its_cap(tables):
    p = _qk_random_case(tables)
    assert not np.array_equal(p.rope_q[0], p.rope_k[0][:p.M]) and not np.array_equal(p.rope_q[0][47:], p.rope_k[0][p.kv_rows][47:])
    assert T.qk_accept(p, *p.expected) == 0
    qlo, qhi, klo, khi = T.qk_case_intervals(p)
    share = float(((qlo != qhi).sum() + (klo != khi).sum()) / (qlo.size + klo.size))
    print(f"Q/K random case, {tables}: ambiguous share {share:.4%}")
    assert share <= T.AMBIGUITY_CAP["qk"]


@pytest.mark.parametrize("defect", T.QK_DEFECTS)
def test_every_named_qk_defect_is_caught(defect):
    seen = set()
    if any(any(not np.array_equal(a, b) for a, b in zip(p.run(defect), p.expected)) for p in _all_qk_probes()):
        seen.add("probe")
    if any(T.qk_accept(p, *p.run(defect)) != 0 for p in (_qk_random_case("uniform_angles"), _qk_random_case("flux_pos_embed"))):
        seen.add("bound")
    assert seen, f"nothing sees {defect}"
    assert seen == CAUGHT_BY[defect], (defect, seen)
    if defect == "fused_multiply_add":                        # both forms of the probe see it, in every Q and K element of the even rows
        for f in (T.qk_fma_probe(), T.qk_fma_probe(standard=True)):
            D = f.H * 128
            assert (f.run(defect)[0][0::2, f.q_col:f.q_col + D] != f.expected[0][0::2, f.q_col:f.q_col + D]).all()


@pytest.mark.parametrize("tables", ["uniform_angles", "flux_pos_embed"])
def test_qk_model_agrees_with_the_oracles_rms_norm_and_rope(tables):
    p = _qk_random_case(tables)
    M, H, D = p.M, p.H, p.H * 128
    bf = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    qlo, qhi, klo, khi = T.qk_case_intervals(p)
    for col, tab, rows, w0, w1, lo, hi in ((p.q_col, p.rope_q, np.arange(M), p.wq0, p.wq1, qlo, qhi),
                                           (p.k_col, p.rope_k, p.kv_rows, p.wk0, p.wk1, klo, khi)):
        x = bf(p.heads(col)).permute(1, 0, 2)[None]                                    # [1, H, M, 128]
        n = torch.cat([O.rms_norm(x[:, :, :p.split_row], bf(w0), T.EPS), O.rms_norm(x[:, :, p.split_row:], bf(w1), T.EPS)], 2)
        out = O.apply_rope(n, f(tab[0][rows]), f(tab[1][rows]))[0].permute(1, 0, 2).reshape(M, D).double().numpy()
        assert ((lo <= out) & (out <= hi)).all(), int(((out < lo) | (out > hi)).sum())
