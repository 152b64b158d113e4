"""-m gpu: rgn_conv_bf16, rgn_conv_s2_bf16 and rgn_conv_up2_bf16 on every launch path of tests/conv_model.py's table against closed forms
and float64 - one test is one row of the table.  Probes a (one-hot taps: the shifted image), b (K-tile signature, tap count), c (the
two-rounding ResNet skip, the zero border, the sentinel around the image), d (GroupNorm partials per tile) and f (NaN outside the
problem, the guard rows a pixel-group launch reads through zero weights) bit for bit, e (|out - ref64| <= 2^-8 |ref64| + K 2^-23 sum|a w|,
one more bf16 ulp where a skip is added) as a ratio <= 1.  The entries are called through the C ABI on raw buffers, so that guard rows,
the partial workspace and the rows behind the image are the test's to poison and to read.  Every launch runs with NaN in every place
the contract of include/regione_hip.h says it does not read: the input's guard rows (but the group - 1 rows next to the image of a 3 x 3
pixel-group launch), the skip's border and guard rows, the weight and bias tails, the scratch row of a table launch.  tests/
test_conv_model.py shows on the CPU that each of these checks rejects the named defects.  Measured margins: profiles/r32_conv_probes.txt."""
import contextlib
import ctypes

import pytest
import torch

import conv_model as C
from regione_amd import _lib, ops, vae as V

pytestmark = pytest.mark.gpu
ROWS = C.TABLE_BY_NAME
DEV = "cuda"


def _nan_tail(t):
    """`t` in front of 4096 NaN elements (what lies behind the weights and the bias is not read)."""
    buf = torch.full((t.numel() + 4096,), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf


def _launch(row, case, nan_rows=()):
    g = C.geo(row)
    X, Y = C.build_input(row, case.x, True, nan_rows), C.new_output(row, DEV)
    R = None if case.resid is None else C.build_resid(row, case.resid)
    if row.kind == "up2":
        cw = V.UpConvWeights(case.w4, case.bias)
        if getattr(case, "wph", None) is not None:                  # e: the reference used the phase weights as stored
            assert torch.equal(cw.w.view(4, row.cout, 2, 2, row.cin), case.wph)
    else:
        cw = V.ConvWeights(case.w4, case.bias, group=row.group, ldy=row.ldy)
    w, b = _nan_tail(cw.w), _nan_tail(cw.b)
    ws = None
    if row.gn:                                                       # the whole workspace, so that a wrong tile count stays inside it
        ws = torch.full((_lib.lib().rgn_groupnorm_workspace_bytes() // 4,), C.WS_SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    nblk = ctypes.c_int(-1)
    x, y = X[g.gin:].data_ptr(), Y[g.gout:].data_ptr()
    wsp, nb = (ws.data_ptr(), ctypes.byref(nblk)) if row.gn else (None, None)
    L, st = _lib.lib(), ops._stream()
    if g.table:
        Y[g.gout + g.rows_out] = float("nan")                        # the scratch row's previous content
        tab = (V.upsample_rows if row.kind == "up2" else V.downsample_rows)(row.H, row.W, DEV)
        assert torch.equal(tab.reshape(g.nprob, -1), C.row_table(row, DEV))
    with _lib.plan_override(gemm_geometry=row.geometry) if row.geometry else contextlib.nullcontext():
        if row.kind == "conv":
            rc = L.rgn_conv_bf16(x, row.cin, w.data_ptr(), b.data_ptr(), None if R is None else R[g.gout:].data_ptr(), y, row.ldy, g.Hp, g.Wp,
                                 row.cin, row.cout, row.taps, row.group, wsp, nb, st)
        elif row.kind == "s2":
            rc = L.rgn_conv_s2_bf16(x, w.data_ptr(), b.data_ptr(), y, row.ldy, g.Hp, g.Wp, row.cin, row.cout, tab.data_ptr(), st)
        else:
            rc = L.rgn_conv_up2_bf16(x, w.data_ptr(), b.data_ptr(), y, row.ldy, g.Hp, g.Wp, row.cin, row.cout, tab.data_ptr(), wsp, nb, st)
    _lib.check(rc, "rgn_conv*")
    torch.cuda.synchronize()
    return C.NS(Y=Y, ws=ws, nblk=nblk.value)


def _exact(row, case, what):
    res = _launch(row, case)
    assert C.check_store(row, case, res) == 0, (row.name, what)
    if row.gn:
        assert res.nblk == C.nblk(row), (row.name, what, res.nblk)
        if case.exact_stats:
            assert C.check_partials(row, case, res) == 0, (row.name, what)
    return res


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_a_shift(name):
    """a + d: every tap on arbitrary finite bf16 values; the first and the last tap on small integers with an integer bias and skip, where
    every partial slot is exact."""
    row = ROWS[name]
    for tap in C.taps_of(row):
        _exact(row, C.shift_case(row, tap, DEV), ("shift", tap))
    for tap in (C.taps_of(row)[0], C.taps_of(row)[-1]):
        _exact(row, C.shift_case(row, tap, DEV, ints=True), ("ints", tap))


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_b_signature_and_count(name):
    row = ROWS[name]
    for ps in range(C.signature_passes(row)):
        _exact(row, C.signature_case(row, ps, DEV), ("signature", ps))
    _exact(row, C.count_case(row, DEV), "count")
    _exact(row, C.count_case(row, DEV, with_bias=True), "count + bias")


@pytest.mark.parametrize("name", C.RESID_ROWS)
def test_c_skip_rounds_twice(name):
    row = ROWS[name]
    _exact(row, C.epilogue_case(row, DEV), "epilogue")


@pytest.mark.parametrize("name", C.HUGE_ROWS)
def test_d_geometry_left_to_the_library(name):
    """No override: the tile count *gn_blocks_host reports is the geometry's (256 from 100 tiles of 256 on, 4 x the tiles for the four
    phases), every slot exact."""
    row = ROWS[name]
    assert row.geometry is None
    res = _exact(row, C.shift_case(row, (1, 1), DEV, ints=True), "ints")
    print(f"CONV_PROBE_TILES {name} geometry {row.geom} tiles {res.nblk}")
    _exact(row, C.count_case(row, DEV, with_bias=True), "count + bias")


@pytest.mark.parametrize("name", C.SMALL_ROWS)
def test_e_fp64_bound(name):
    row = ROWS[name]
    for fam in C.FAMILIES:
        case = C.bound_case(row, fam, DEV)
        res = _launch(row, case)
        r = C.bound_ratio(row, case, res)
        host = C.bound_case(row, fam)
        print(f"CONV_PROBE_E {name} {fam} {r:.3f} emulate {C.bound_ratio(row, host, C.emulate(row, host)):.3f}")
        assert r <= 1.0, (name, fam, r)
        again, g = _launch(row, case), C.geo(row)
        keep = torch.ones(res.Y.shape[0], dtype=torch.bool, device=DEV)
        keep[g.gout + g.rows_out] = row.kind != "s2"                 # the stride-2 scratch row: many GEMM rows, the last store wins
        assert torch.equal(C.bits(res.Y)[keep], C.bits(again.Y)[keep])
        if row.gn:
            assert torch.equal(res.ws.view(torch.int32), again.ws.view(torch.int32))


@pytest.mark.parametrize("name", C.GROUP_ROWS)
def test_f_guard_rows_a_pixel_group_reads(name):
    """The exact set: a NaN in a guard row guard_reads names shows in every unmasked pixel of the GEMM rows that read it and nowhere else;
    every other guard row holds NaN in all launches of this file, this one included."""
    row = ROWS[name]
    g, case = C.geo(row), C.count_case(row, DEV)
    want, _ = C.expected_storage(row, case.img)
    for r in sorted(C.guard_reads(row)):
        res = _launch(row, case, nan_rows=[r])
        hit = C.poisoned_pixels(row, r).to(DEV)
        got = res.Y[g.gout:g.gout + g.rows]
        assert torch.equal(torch.isnan(got.float()).all(1), hit) and not bool(torch.isnan(got[~hit].float()).any()), (name, r)
        frame = res.Y.clone()
        frame[g.gout:g.gout + g.rows][hit] = want[g.gout:g.gout + g.rows][hit]
        assert C.mismatches(frame, want) == 0, (name, r)


@pytest.mark.parametrize("name", ["a_g2", "r_c64", "a_s2", "r_up2_c256"])
def test_vae_wrappers_launch_the_probed_entries(name):
    """V.conv / V.conv_s2 / V.conv_up2 on PaddedImages store the image the raw launch stores and hand the same tile count on."""
    row = ROWS[name]
    g, case = C.geo(row), C.shift_case(row, C.taps_of(row)[-1], DEV, ints=True)
    x, out = V.PaddedImage(row.H, row.W, row.cin, DEV), V.PaddedImage(g.Ho, g.Wo, row.ldy, DEV)
    assert x.storage.shape[0] == g.rows + 2 * g.gin and out.storage.shape[0] == g.rows_out + 2 * g.gout
    x.t.view(g.Hp, g.Wp, row.cin)[1:-1, 1:-1] = case.x
    with _lib.plan_override(gemm_geometry=row.geometry):
        if row.kind == "conv":
            r = None
            if case.resid is not None:
                r = V.PaddedImage(g.Ho, g.Wo, row.ldy, DEV)
                r.t.view(g.Hq, g.Wq, row.ldy)[1:-1, 1:-1, :row.cout] = case.resid
            V.conv(x, V.ConvWeights(case.w4, case.bias, group=row.group, ldy=row.ldy), out, resid=r, gn=row.gn)
        elif row.kind == "s2":
            V.conv_s2(x, V.ConvWeights(case.w4, case.bias), out, V.downsample_rows(row.H, row.W, DEV))
        else:
            V.conv_up2(x, V.UpConvWeights(case.w4, case.bias), out, V.upsample_rows(row.H, row.W, DEV), gn=row.gn)
    torch.cuda.synchronize()
    t = out.t.view(g.Hq, g.Wq, row.ldy)
    assert C.mismatches(t[1:-1, 1:-1, :row.cout], case.img) == 0
    assert not bool(t[0].any() or t[-1].any() or t[:, 0].any() or t[:, -1].any())      # the zero border: written, or the buffer's own
    if row.gn:
        owner, nblk = V.gn_handoff(out.t.device)
        assert owner is out and nblk == C.nblk(row)


def test_pixel_group_wider_than_the_image_is_refused():
    row = C.NS(**{**ROWS["a_1x1img"].__dict__, "group": 2})
    case = C.count_case(ROWS["a_1x1img"], DEV)
    g = C.geo(ROWS["a_1x1img"])
    X, Y = C.build_input(ROWS["a_1x1img"], case.x), C.new_output(ROWS["a_1x1img"], DEV)
    cw = V.ConvWeights(case.w4, case.bias, group=2)
    rc = _lib.lib().rgn_conv_bf16(X[g.gin:].data_ptr(), row.cin, cw.w.data_ptr(), cw.b.data_ptr(), None, Y[g.gout:].data_ptr(), row.ldy, g.Hp, g.Wp,
                                  row.cin, row.cout, 9, 2, None, None, ops._stream())
    with pytest.raises(_lib.RegionEHipError):
        _lib.check(rc, "rgn_conv_bf16")
    torch.cuda.synchronize()
    assert C.mismatches(Y, C.new_output(ROWS["a_1x1img"], DEV)) == 0
