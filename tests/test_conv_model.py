"""CPU: the convolution probes of tests/conv_model.py against the model's own emulation - every check passes on `emulate`, every named
defect of MUTANTS fails at least one of them, every table row's instantiation and tile count follow from the restated dispatch rule, the
layouts the model restates are the ones regione_amd/vae.py builds, and every closed-form expectation is its own bf16 rounding (the
"exact" claim of tests/test_gpu_conv_probes.py, checked where it can be checked without a GPU)."""
import pytest
import torch

import conv_model as C
from regione_amd import vae as V

ROWS = C.TABLE_BY_NAME


def _exact_cases(row):
    """Every exact probe case of a row (name, case)."""
    out = [("shift%d%d" % t, C.shift_case(row, t)) for t in C.taps_of(row)]
    out += [("ints%d%d" % t, C.shift_case(row, t, ints=True)) for t in (C.taps_of(row)[0], C.taps_of(row)[-1])]
    out += [("sig%d" % p, C.signature_case(row, p)) for p in range(C.signature_passes(row))]
    out += [("count", C.count_case(row)), ("count_bias", C.count_case(row, with_bias=True))]
    if row.resid:
        out.append(("epilogue", C.epilogue_case(row)))
    return out


@pytest.mark.parametrize("name", [r.name for r in C.TABLE])
def test_table_row_follows_from_the_dispatch_rule(name):
    row = ROWS[name]
    geom, av, per, nprob = C.dispatch(row)
    assert (geom, av) == (row.geom, row.av)
    g = C.geo(row)
    assert per == -(-g.M // geom) * -(-g.N // geom) and nprob == (4 if row.kind == "up2" else 1)
    assert g.K % 64 == 0 and (g.crt == 0 or g.K == 3 * g.crt * 64 or (row.kind == "up2" and g.K == 2 * g.crt * 64))
    if row.gn:
        assert g.gn_c in (128, 256, 512)


def test_tile_counts_at_the_geometry_thresholds():
    assert C.nblk(ROWS["thr_above"]) == 102 and C.nblk(ROWS["thr_below"]) == 380           # 51 x 2 of 256; 95 x 4 of 128
    assert C.nblk(ROWS["up2_thr_above"]) == 104 and C.nblk(ROWS["up2_thr_below"]) == 384   # 4 x 13 x 2; 4 x 24 x 4
    r = ROWS["a_1x1_k128_f256"]
    assert r.geometry == 256 and C.dispatch(r)[0] == 128 and C.nblk(r) == 4                # K = 128 < 256 stays on the 128 geometry


def test_features_are_spread_over_the_table():
    rows = [r for r in C.TABLE if not r.feat.get("huge")]
    assert {C.geo(r).gn_c for r in rows if r.gn} == {128, 256, 512}
    for geom in (128, 256):
        sel = [r for r in rows if r.geom == geom]
        assert any(r.resid for r in sel) and any(not r.resid for r in sel) and any(not r.gn for r in sel)
        assert any(r.group == 2 for r in sel) and any(r.group == 8 and r.ldy == 8 for r in sel)
        assert {r.kind for r in sel} == {"conv", "s2", "up2"}
    assert any(r.ldy > r.cout and r.group == 1 for r in rows)
    assert {C.geo(r).crt for r in rows if r.av == 3} >= {2, 3, 6, 8, 9, 20, 24}


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_model_layouts_are_the_librarys(name):
    row = ROWS[name]
    c = C.bound_case(row, "randn")
    if row.kind == "up2":
        uw = V.UpConvWeights(c.w4, c.bias)
        assert torch.equal(uw.w.view(4, row.cout, 2, 2, row.cin), C.phase_fold(c.w4, torch.float32).to(C.BF16))
        # the host's rounding of the tap sums: one bf16 rounding of the exact (fp64) sum
        assert torch.equal(uw.w.view(4, row.cout, 2, 2, row.cin), C.phase_fold(c.w4).float().to(C.BF16))
        assert torch.equal(V.upsample_rows(row.H, row.W, "cpu"), C.row_table(row))
    else:
        cw = V.ConvWeights(c.w4, c.bias, group=row.group, ldy=row.ldy)
        W, b = C.toeplitz(row, c.w4, c.bias)
        assert torch.equal(cw.w, W) and torch.equal(cw.b, b) and W.shape == (C.geo(row).N, C.geo(row).K)
        if row.kind == "s2":
            assert torch.equal(V.downsample_rows(row.H, row.W, "cpu"), C.row_table(row)[0])
    g = C.geo(row)
    img = V.PaddedImage(row.H, row.W, row.cin, "cpu")
    assert img.storage.shape[0] == g.rows + 2 * g.gin and g.gin >= g.Wp + 1 + row.group


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_every_expectation_is_exact_and_emulate_passes(name):
    row = ROWS[name]
    for what, case in _exact_cases(row):
        assert case.img.dtype == C.BF16 and bool(torch.isfinite(case.img.float()).all()), what
        if case.lin is not None:                                 # the closed form in fp64 is its own bf16 rounding
            assert torch.equal(case.lin, case.img.double()), what
        res = C.emulate(row, case)
        assert C.check_store(row, case, res) == 0, what
        if row.gn and case.exact_stats:
            assert C.check_partials(row, case, res) == 0, what
    if row.resid:
        e = C.epilogue_case(row)
        assert int((C.bits(e.img) != C.bits(e.once)).sum()) > e.img.numel() // 20          # two roundings are not one


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_emulate_is_inside_the_fp64_bound(name):
    row = ROWS[name]
    for fam in C.FAMILIES:
        case = C.bound_case(row, fam)
        r = C.bound_ratio(row, case, C.emulate(row, case))
        assert r <= 1.0, (fam, r)


def _fails(row, case, mutant):
    res = C.emulate(row, case, mutant)
    bad = C.check_store(row, case, res)
    if row.gn and case.exact_stats:
        bad += C.check_partials(row, case, res)
    return bad


# the rows on which a defect can show: where the feature it breaks exists
MUTANT_ROWS = {
    "jump_one_tile_late": ["a_g1", "r_c512", "a_s2", "r_up2_c64"], "jump_of_wp": ["a_g1", "r_g2", "a_s2", "a_up2"],
    "kx_reversed": ["a_g1", "a_g2"], "origin_off_by_one": ["a_g1", "a_up2", "a_s2"],
    "mask_missing_last_column": ["a_g1", "a_g2", "a_up2"], "mask_missing_last_row": ["a_g1", "a_rgb"], "mask_before_skip": ["a_g1", "p_1x1"],
    "stats_before_mask": ["a_g1", "a_up2"], "stats_shift_of_wrong_channel_count": ["a_g1", "r_c128"],
    "slot_of_neighbour_tile": ["a_m33", "r_up2_c64"], "up2_slot_base_restarted": ["a_up2", "r_up2_c64_tiles"],
    "group_pixels_swapped": ["a_g2", "a_rgb", "a_1x1_g2"], "hanging_row_dropped": ["a_g2", "r_g8", "a_rgb"],
    "s2_origin_without_offset": ["a_s2", "a_s2_2x2"], "s2_pad_top": ["a_s2"], "s2_pad_left": ["a_s2"],
    "phases_exchanged": ["a_up2", "a_up2_2x2"], "up2_border_not_zeroed": ["a_up2", "r_up2_c256"],
    "skip_before_rounding": ["a_g1", "r_c512", "p_1x1"], "group_m_tiles_swapped": ["a_m33", "r_m33"],
}


@pytest.mark.parametrize("mutant", C.MUTANTS)
def test_every_mutant_fails_a_check(mutant):
    assert set(MUTANT_ROWS) == set(C.MUTANTS)
    for name in MUTANT_ROWS[mutant]:
        row = ROWS[name]
        hits = [what for what, case in _exact_cases(row) if _fails(row, case, mutant)]
        assert hits, (mutant, name)


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_guard_rows_that_reach_interior_outputs(name):
    """The contract probe f holds: group = 1, 1 x 1, stride-2 and phase launches read no guard row with an effect on a stored output;
    a 3 x 3 pixel-group launch reads at most group - 1 rows in front of the image and group - 1 behind it through zero weights."""
    row = ROWS[name]
    g, reads = C.geo(row), C.guard_reads(row)
    if name not in C.GROUP_ROWS:
        assert not reads
        return
    assert reads and min(reads) >= -(row.group - 1) and max(reads) <= g.rows + row.group - 2
    case = C.count_case(row)
    want, _ = C.expected_storage(row, case.img)
    for r in reads:
        res = C.emulate(row, case, nan_rows=[r])
        got = res.Y[g.gout:g.gout + g.rows]
        hit = C.poisoned_pixels(row, r)
        assert bool(hit.any()) and torch.equal(torch.isnan(got.float()).all(1), hit)
        assert torch.equal(C.bits(got[~hit]), C.bits(want[g.gout:g.gout + g.rows][~hit]))
