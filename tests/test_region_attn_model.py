"""CPU: the checks of tests/test_gpu_region_attn_probes.py separate a correct region-attention arithmetic from a subtly wrong one.

rgn_attention / rgn_attention_bounded (csrc/attn.hip) were held to Frobenius ratios (1e-2 against fp32, 2e-3 / 5e-3 between schedules)
and to an element-wise 2^-7 |ref| + 6e-3.  tests/region_attn_model.py emulates the region scheme - one launch, equal pieces, stream-K
runs - with named defects; this file shows, at the shapes and plans of the GPU file (query rows sampled by 32-row groups):
  * the emulation WITHOUT a defect passes every check the GPU tests apply (exact probes, the element-wise fp64 bound), with the
    deferred-max decision taken per 32-row group (the kernels) and per row, with and without the static shift;
  * every defect fails the probes aimed at it, and at least one probe of a short sweep;
  * the gap: the last key never counted in one item of 120, and a counted pad key at Skv = 2533, pass the old thresholds on N(0, 1)
    inputs - and both fail the counting probe;
  * the plan table of the GPU file is what attention_schedule chooses (rgn_attention_plan_query: host arithmetic, no GPU).
"""
import functools

import pytest
import torch.nn.functional as F

import region_attn_model as R
from regione_amd import _lib


def _sample(row):
    """(heads, groups) the emulation looks at for a row of the table: the first and last 32-row group, the groups around the first
    256-row block edge, and for a split launch the heads and blocks of its first item and of the items around a run boundary."""
    ng, nQ = (row.Sq + 31) // 32, (row.Sq + row.QB - 1) // row.QB
    groups, heads = {0, 7, 8, ng - 2, ng - 1}, {0, row.H - 1}
    items = [row.first_item]
    if row.streamk:
        b = R.streamk_boundary(row.left, (row.Skv + 63) // 64, row.slots)
        items += [row.first_item + b[0], row.first_item + b[2]] if b else []
    for it in items:
        heads.add(it // nQ)
        groups |= {(it % nQ) * (row.QB // 32), (it % nQ) * (row.QB // 32) + row.QB // 32 - 1}
    return sorted(h for h in heads if 0 <= h < row.H), sorted(g for g in groups if 0 <= g < ng)


def _emulate(row, case, static, any_row=True, defect=None):
    """(the case restricted to what was emulated, out)."""
    heads, groups = _sample(row)
    rows, out = R.emulate_region(case.q, case.k, case.v, case.scale, R.plan_of(row), defect, static_shift=static and row.asm,
                                 any_row=any_row, groups=groups, heads=heads, first_item=row.first_item, QB=row.QB)
    return R.sub_case(case, heads, rows), out


@functools.lru_cache(maxsize=None)
def _exact_cases(name):
    row = R.TABLE_BY_NAME[name]
    cases = [("counting", R.counting_case(row.Sq, row.Skv, row.H))]
    cases += [(f"spike j={j}", R.spike_case(row.Sq, row.Skv, row.H, j)) for j in R.spike_keys(row)]
    if name in R.CLASS_ROWS:
        cases.append(("wrong head", R.wrong_head_case(row.Sq, row.Skv, row.H)))
    return cases


@pytest.mark.parametrize("any_row", [True, False])
def test_the_correct_emulation_passes_every_exact_probe(any_row):
    for row in R.TABLE:
        for what, case in _exact_cases(row.name):
            for static in row.bounded:
                sub, out = _emulate(row, case, static, any_row)
                assert R.CHECKS[case.kind](sub, out) == 0, (row.name, what, static)


@pytest.mark.parametrize("any_row", [True, False])
def test_the_correct_emulation_stays_inside_the_fp64_bound(any_row):
    worst = {}
    for row in R.TABLE:
        cls = "asm" if row.asm else "c8" if row.waves8 else "c4"
        plan = "stream-K" if row.streamk else "pieces" if row.pieces > 1 else "unsplit"
        for family in R.FAMILIES:
            case = R.bound_case(family, row.Sq, row.Skv, row.H)
            for static in row.bounded:
                sub, out = _emulate(row, case, static, any_row)
                R.check_stress_shape(sub)
                r = R.bound_ratio(sub, out)
                assert r <= 1.0, (row.name, family, static, r)
                key = (cls + ("/static" if static else ""), family, plan)
                worst[key] = max(worst.get(key, 0.0), r)
    for (cls, family, plan), r in sorted(worst.items()):
        print(f"emulation any_row={any_row} {cls:10s} {family:9s} {plan:8s}: worst err / bound {r:.3f}")


# ---- every defect is rejected -----------------------------------------------------------------------------------------------------------
SK = ("streamk", 3, 4)            # 3 items (H = 3, one query block each) x 5 tiles in 4 runs: [0, 3) [3, 7) [7, 11) [11, 15)


def _run(case, plan, defect=None, **kw):
    kw.setdefault("QB", 256)
    return R.emulate_region(case.q, case.k, case.v, case.scale, plan, defect, **kw)[1]


def _fails(case, plan, defect, **kw):
    out = _run(case, plan, defect, **kw)
    if case.kind == "bound":
        return R.bound_ratio(case, out) > 1.0
    return R.CHECKS[case.kind](case, out) > 0


# the probes meant to catch each defect (case, plan, emulation arguments): every one of them must fail
CATCHERS = {
    "drop_last_key": [
        lambda: (R.counting_case(64, 65, 2), None, {}),
        lambda: (R.counting_case(33, 192, 2), ("pieces", 3), {}),
        lambda: (R.counting_case(64, 320, 3), SK, {}),
        lambda: (R.spike_case(64, 200, 2, 199), None, {}),
        lambda: (R.spike_case(64, 320, 2, 319), None, dict(static_shift=True)),
        lambda: (R.bound_case("late_max", 64, 320, 2), None, {}),
    ],
    "count_one_padded_key": [
        lambda: (R.counting_case(33, 65, 2), None, {}),
        lambda: (R.counting_case(1, 1, 3), None, dict(QB=128)),
        lambda: (R.counting_case(64, 200, 2), ("pieces", 2), {}),
        lambda: (R.counting_case(300, 2533, 2), ("pieces", 8), dict(groups=[0, 9])),
    ],
    "no_rescale": [
        lambda: (R.spike_case(64, 320, 2, 319), None, {}),
        lambda: (R.spike_case(64, 320, 3, 200), SK, {}),
        lambda: (R.bound_case("late_max", 64, 320, 2), None, {}),
        lambda: (R.bound_case("staircase", 64, 640, 2), None, {}),
    ],
    "piece_last_tile_dropped": [
        lambda: (R.counting_case(64, 320, 2), None, {}),
        lambda: (R.counting_case(64, 320, 2), ("pieces", 2), {}),
        lambda: (R.counting_case(64, 320, 3), SK, {}),
        lambda: (R.spike_case(64, 320, 2, 319), None, dict(static_shift=True)),
        lambda: (R.spike_case(64, 320, 2, 191), ("pieces", 2), {}),
    ],
    "run_boundary_tile_twice": [
        lambda: (R.counting_case(64, 320, 3), SK, {}),
        lambda: (R.counting_case(64, 320, 3), SK, dict(static_shift=True)),
        lambda: (R.bound_case("randn", 64, 320, 3), SK, {}),
    ],
    "stale_accumulator_in_second_segment": [
        lambda: (R.counting_case(64, 320, 3), SK, {}),
        lambda: (R.spike_case(64, 320, 3, 200), SK, {}),
        lambda: (R.spike_case(64, 320, 3, 319), SK, dict(static_shift=True)),
        lambda: (R.bound_case("randn", 64, 320, 3), SK, {}),
    ],
    "merge_ignores_piece_max": [
        lambda: (R.spike_case(64, 320, 2, 319), ("pieces", 2), {}),
        lambda: (R.spike_case(64, 320, 3, 0), SK, {}),
        lambda: (R.bound_case("late_max", 64, 320, 2), ("pieces", 2), {}),
        lambda: (R.bound_case("first_max", 64, 320, 3), SK, {}),
    ],
    "vt_group_permutation_missing": [
        lambda: (R.spike_case(33, 64, 2, 4), None, {}),
        lambda: (R.spike_case(33, 64, 2, 8), None, dict(static_shift=True)),
        lambda: (R.spike_case(33, 64, 2, 20), None, {}),
        lambda: (R.spike_case(64, 320, 3, 260), SK, {}),
        lambda: (R.bound_case("randn", 33, 64, 2), None, {}),
    ],
    "wrong_head": [
        lambda: (R.wrong_head_case(33, 65, 3), None, {}),
        lambda: (R.wrong_head_case(64, 320, 3), SK, {}),
        lambda: (R.counting_case(33, 65, 3), None, {}),
        lambda: (R.spike_case(33, 65, 2, 64), None, {}),
    ],
    "ragged_q_block_reads_row_plus_one": [
        lambda: (R.bound_case("randn", 40, 129, 2), None, {}),
        lambda: (R.bound_case("randn", 130, 65, 2), None, dict(QB=128)),
        lambda: (R.bound_case("randn", 300, 320, 2), ("pieces", 2), dict(groups=[8, 9])),
    ],
}


@pytest.mark.parametrize("defect", R.REGION_DEFECTS)
def test_every_defect_is_rejected(defect):
    assert len(CATCHERS[defect]) >= 2, "fewer than two probes are aimed at this defect"
    for i, make in enumerate(CATCHERS[defect]):
        case, plan, kw = make()
        kw = dict(dict(QB=256), **kw)
        for any_row in (True, False):
            rows, good = R.emulate_region(case.q, case.k, case.v, case.scale, plan, None, any_row=any_row, **kw)
            _, bad = R.emulate_region(case.q, case.k, case.v, case.scale, plan, defect, any_row=any_row, **kw)
            sub = R.sub_case(case, rows=rows)                       # the rows the emulation was asked for (`groups`)
            if case.kind == "bound":
                assert R.bound_ratio(sub, good) <= 1.0 < R.bound_ratio(sub, bad), (defect, i, any_row)
            else:
                assert R.CHECKS[case.kind](sub, good) == 0, (defect, i, "the correct arithmetic must pass the same check")
                assert R.CHECKS[case.kind](sub, bad) > 0, (defect, i, any_row)


@functools.lru_cache(maxsize=None)
def _short_sweep():
    """(name, case, plan, emulation arguments): exact probes and the randn / late_max bound at short shapes, under every kind of plan."""
    out = []
    for Sq, H in ((33, 2), (70, 3)):
        for Skv in (1, 63, 64, 65, 129, 320):
            nt = (Skv + 63) // 64
            plans = [(None, {}), (None, dict(static_shift=True))] + ([(("pieces", 2), {})] if nt >= 2 else [])
            plans += [(("streamk", H, 4), {})] if nt == 5 else []
            for plan, kw in plans:
                if Skv % 64 and kw:
                    continue                                        # the static shift exists on whole tiles only
                cases = [R.counting_case(Sq, Skv, H), R.wrong_head_case(Sq, Skv, H), R.bound_case("randn", Sq, Skv, H),
                         R.bound_case("late_max", Sq, Skv, H)]
                cases += [R.spike_case(Sq, Skv, H, j) for j in sorted({0, Skv - 1, min(4, Skv - 1)})]
                out += [(f"{c.kind} {getattr(c, 'family', '')} Sq={Sq} Skv={Skv} H={H} {plan} {kw}", c, plan, kw) for c in cases]
    return out


def test_the_correct_emulation_passes_the_short_sweep():
    for name, case, plan, kw in _short_sweep():
        assert not _fails(case, plan, None, **kw), name


@pytest.mark.parametrize("defect", R.REGION_DEFECTS)
def test_every_defect_fails_somewhere_in_the_short_sweep(defect):
    n = sum(_fails(case, plan, defect, **kw) for _, case, plan, kw in _short_sweep()
            if R.defect_applies(defect, plan, case.q.shape[1], case.k.shape[1], case.q.shape[0]))
    print(f"{defect}: rejected by {n} probes of the short sweep")
    assert n >= 1


# ---- the gap --------------------------------------------------------------------------------------------------------------------------
def _fp32_reference(case):
    """What the tests before this file compare with: an fp32 softmax."""
    return F.scaled_dot_product_attention(case.q.float()[None], case.k.float()[None], case.v.float()[None], scale=case.scale)[0]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_the_gap_the_last_key_dropped_in_one_item_of_120_passes_the_old_thresholds():
    """N(0, 1) inputs, H = 2, 64 query rows, Skv = 2560.  The last key never counted moves the Frobenius ratio against fp32 from 2.3e-3
    to 1.3e-2 - on every row.  Confined to one item of the 120 of test_attention_stream_k_remainder (every item with the statistics
    of this one) the ratio of the whole output is sqrt((119 good^2 + bad^2) / 120), under `rel_err < 1e-2`, and the ratio between
    the schedules is |bad - good| / |good| / sqrt(120), under `2e-3`.  The counting probe rejects it."""
    case = R.bound_case("randn", 64, 2560, 2)
    ref32 = _fp32_reference(case)
    good, bad = _run(case, None), _run(case, None, "drop_last_key")
    eg, eb = _rel(good, ref32), _rel(bad, ref32)
    whole = ((119 * eg ** 2 + eb ** 2) / 120) ** 0.5
    between = _rel(bad, good) / 120 ** 0.5
    print(f"drop_last_key Skv=2560: Frobenius ratio {eb:.3e} (correct {eg:.3e}); in one item of 120: {whole:.3e} against fp32, "
          f"{between:.3e} between schedules")
    assert eb > 1e-2 > whole and between < 2e-3, "the old thresholds used to pass this defect: the reason for the probes"
    probe = R.counting_case(64, 2560, 2)
    assert R.check_counting(probe, _run(probe, None)) == 0 and R.check_counting(probe, _run(probe, None, "drop_last_key")) > 0


def test_the_gap_a_counted_pad_key_at_2533_passes_the_old_thresholds():
    """N(0, 1) inputs, Skv = 2533: the first pad key (zero K row, zero V) counted with score 0 changes nothing measurable - the
    Frobenius ratio, the element-wise 2^-7 |ref| + 6e-3 of test_attention_random_shapes and even the fp64 bound stay where the correct
    arithmetic has them.  The counting probe rejects it in hundreds of elements (wherever sum / 2534 and sum / 2533 round apart)."""
    case = R.bound_case("randn", 64, 2533, 2)
    ref32, (O_ref, A_ref) = _fp32_reference(case), R.ref64(case.q, case.k, case.v, case.scale)
    good, bad = _run(case, None), _run(case, None, "count_one_padded_key")
    eg, eb = _rel(good, ref32), _rel(bad, ref32)
    tol = float(((bad.double() - O_ref).abs() / (2.0 ** -7 * O_ref.abs() + 6e-3)).max())
    rg, rb = R.bound_ratio(case, good), R.bound_ratio(case, bad)
    print(f"count_one_padded_key Skv=2533: Frobenius ratio {eb:.3e} (correct {eg:.3e}), {tol:.2f} of the random-shapes tolerance, "
          f"err / bound {rb:.2f} (correct {rg:.2f})")
    assert eb < 1e-2 and _rel(bad, good) < 2e-3 and tol <= 1.0, "the old thresholds used to pass this defect: the reason for the probes"
    assert rg <= 1.0
    probe = R.counting_case(64, 2533, 2)
    n = R.check_counting(probe, _run(probe, None, "count_one_padded_key"))
    print(f"counting probe: {n} mismatches")
    assert R.check_counting(probe, _run(probe, None)) == 0 and n > 100


# ---- the plan table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ALL_ROWS))
def test_the_plan_table_is_what_attention_schedule_chooses(name):
    """Kernel class (8-wave bit; hand-scheduled = whole KV tiles), piece count and stream-K bit of every row, through the knobs."""
    row = R.ALL_ROWS[name]
    h = _lib.lib()
    with _lib.plan_override(**row.knobs):
        p = h.rgn_attention_plan_query(row.Sq, row.Skv, row.H, row.ws)
    assert p >= 0
    got = dict(pieces=p & 15, stream_k=bool(p & 16), waves8=bool(p & 32))
    assert got == dict(pieces=1 if row.streamk else row.pieces, stream_k=row.streamk, waves8=row.waves8), (name, got)
    assert p == R.expected_plan_bits(row)
    assert row.asm == (row.waves8 and row.Skv % 64 == 0), "the hand-scheduled kernels take whole KV tiles on 8-wave workgroups"
    if row.pieces > 1:                                              # no empty piece, and the pieces the GPU file names
        nt = (row.Skv + 63) // 64
        assert (row.pieces - 1) * ((nt + row.pieces - 1) // row.pieces) < nt
    if name == "asm-streamk":                                       # runs of two segments
        assert R.streamk_boundary(row.left, row.Skv // 64, row.slots) is not None


def test_the_table_shapes_named_in_the_gpu_file():
    """The facts the GPU file's table states about its rows."""
    assert [s[1] for s in R.item_segments(("pieces", 6), 0, 26)] == [5, 5, 5, 5, 5, 1]          # 1664 keys: the last piece holds 1 tile
    assert [s[1] for s in R.item_segments(("pieces", 7), 0, 41)] == [6, 6, 6, 6, 6, 6, 5]       # 2624 keys
    sk = R.TABLE_BY_NAME["asm-streamk"]
    assert sk.left == 40 and sk.Skv // 64 == 52
    lens = {R.run_bound(w + 1, 40 * 52, 256) - R.run_bound(w, 40 * 52, 256) for w in range(256)}
    assert lens == {8, 9}
    segs = [s for u in range(40) for s in R.item_segments(R.plan_of(sk), u, 52)]
    assert {s[1] for s in segs if s[3] == 0 and not s[4]} == {2, 4, 5, 7}          # the first segments of the runs that cross an item edge
    assert {s[1] for s in segs} == set(range(1, 10))                # and every segment length 1 ... 9: the ring's fill, both loop parities
    r = R.TABLE_BY_NAME["rounds+split4"]
    assert (r.nitems, r.first_item, r.left) == (288, 256, 32)
