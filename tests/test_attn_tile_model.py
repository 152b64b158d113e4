"""CPU: the checks of tests/test_gpu_attn_tile_probes.py separate a correct flash-attention tile arithmetic from a subtly wrong one.

The three sequence front ends of csrc/attn_tile.h were held only to `max |err| <= 2e-2` and `PSNR >= 40 dB` against an fp32 softmax on
N(0, 1) inputs.  tests/attn_tile_model.py emulates the tile arithmetic with named defects; this file shows, at the shapes the GPU tests use:
  * the emulation WITHOUT a defect passes every check the GPU tests apply (exact probes, head map, the element-wise fp64 bound);
  * every defect fails at least one of them, and the particular probes meant to catch it do;
  * the gap: the last key of 1500 never counted, and the T5 bias read wrong at offsets +-(L - 1) of 1000, both stay inside 2e-2 and
    40 dB on N(0, 1) inputs - and both fail the exact probes.
"""
import functools

import pytest
import torch

import attn_tile_model as M


def _probes(long=False):
    """(name, case, check) of every exact probe of the GPU file; `long` adds the L = 1000 / 1500 cases."""
    for L, H in M.text_cases_LH():
        if L > 129 and not long:
            continue
        for causal in (False, True):
            for zero_table in (False, True):
                yield f"text counting L={L} H={H} causal={causal} table={zero_table}", M.counting_case("text", L, H, H, 64, causal, zero_table), M.check_counting
    for L, hq, hkv in M.lm_cases_LH():
        if L > 129 and not long:
            continue
        yield f"lm counting L={L} {hq}/{hkv}", M.counting_case("lm", L, hq, hkv, 128, True), M.check_counting
        yield f"lm head map L={L} {hq}/{hkv}", M.headmap_case(L, hq, hkv), M.check_headmap
    for name, segs in M.VISION_SEGS.items():
        for Dp in M.VISION_WIDTHS:
            for H in M.HEADS:
                yield f"vision counting {name} Dp={Dp} H={H}", M.counting_case("vision", sum(segs), H, H, Dp, segs=segs), M.check_counting
    yield "vision counting items 1/63/64", M.counting_case("vision", 128, 3, 3, 64, segs=[128]), M.check_counting
    yield "vision counting 80 in 96", M.counting_case("vision", 195, 3, 3, 96, segs=[31, 1, 64, 65, 34], width=80), M.check_counting
    if long:
        yield "vision counting long", M.counting_case("vision", M.VISION_LONG, 1, 1, 96, segs=[M.VISION_LONG]), M.check_counting
    for L in M.SPIKE_LENGTHS:
        for Lmax in M.spike_lmaxes(L):
            for delta in M.spike_deltas(L, Lmax):
                for causal in (False, True):
                    yield f"spike L={L} delta={delta} Lmax={Lmax} causal={causal}", M.spike_case(L, 3, delta, Lmax, causal), M.check_spike


def _bounds(long=False):
    """(kernel, family, name, case) of every bound case of the GPU file."""
    for family in M.FAMILIES:
        for L, H in M.text_cases_LH():
            if L > 129 and not long:
                continue
            for causal in (False, True):
                for bias in (False, True):
                    yield "text", family, f"L={L} H={H} causal={causal} bias={bias}", M.bound_case("text", family, L, H, H, 64, causal, bias)
        for L, hq, hkv in M.lm_cases_LH():
            if L > 129 and not long:
                continue
            yield "lm", family, f"L={L} {hq}/{hkv}", M.bound_case("lm", family, L, hq, hkv, 128, True)
        for name, segs in M.VISION_SEGS.items():
            for Dp in M.VISION_WIDTHS:
                yield "vision", family, f"{name} Dp={Dp}", M.bound_case("vision", family, sum(segs), 3, 3, Dp, segs=segs)
        yield "vision", family, "80 in 96", M.bound_case("vision", family, 195, 3, 3, 96, segs=[31, 1, 64, 65, 34], width=80)
        if long:
            yield "vision", family, "long", M.bound_case("vision", family, M.VISION_LONG, 1, 1, 96, segs=[M.VISION_LONG])


@functools.lru_cache(maxsize=None)
def _short_probes():
    return list(_probes())


def test_the_correct_emulation_passes_every_exact_probe():
    for name, case, check in _short_probes() + [p for p in _probes(long=True) if p[1].q.shape[1] > 129]:
        assert check(case, M.run_model(case)) == 0, name


def test_the_correct_emulation_stays_inside_the_fp64_bound():
    worst = {}
    for kernel, family, name, case in _bounds(long=True):
        M.check_stress_shape(case)
        r = M.bound_ratio(case, M.run_model(case))
        assert r <= 1.0, (kernel, family, name, r)
        worst[kernel, family] = max(worst.get((kernel, family), 0.0), r)
    for (kernel, family), r in sorted(worst.items()):
        print(f"emulation {kernel:6s} {family:9s}: worst err / bound {r:.3f}")


# the probes meant to catch each defect: every one of them must fail (a defect with no entry here would be an untested kernel mistake)
CATCHERS = {
    "drop_last_key": [
        lambda: (M.counting_case("text", 33, 1, 1, 64), M.check_counting),
        lambda: (M.counting_case("text", 64, 3, 3, 64, True, True), M.check_counting),
        lambda: (M.counting_case("lm", 65, 4, 2, 128, True), M.check_counting),
        lambda: (M.counting_case("vision", 133, 1, 1, 32, segs=[60, 70, 3]), M.check_counting),
        lambda: (M.bound_case("lm", "late_max", 129, 4, 2, 128, True), None),
        lambda: (M.bound_case("text", "late_max", 97, 3, 3, 64, False, True), None),
    ],
    "count_one_padded_key": [
        lambda: (M.counting_case("text", 33, 1, 1, 64), M.check_counting),
        lambda: (M.counting_case("text", 1, 3, 3, 64, False, True), M.check_counting),
        lambda: (M.counting_case("lm", 63, 1, 1, 128, True), M.check_counting),
        lambda: (M.counting_case("vision", 33, 3, 3, 96, segs=[33]), M.check_counting),
        lambda: (M.bound_case("vision", "randn", 133, 3, 3, 64, segs=[60, 70, 3]), None),
    ],
    "causal_off_by_one": [
        lambda: (M.counting_case("lm", 33, 1, 1, 128, True), M.check_counting),
        lambda: (M.counting_case("lm", 64, 6, 2, 128, True), M.check_counting),
        lambda: (M.counting_case("text", 31, 3, 3, 64, True), M.check_counting),
        lambda: (M.spike_case(65, 3, 1, 65, True), M.check_spike),
        lambda: (M.bound_case("lm", "late_max", 129, 1, 1, 128, True), None),
    ],
    "bias_offset_plus_one": [
        lambda: (M.spike_case(33, 3, 0, 33, False), M.check_spike),
        lambda: (M.spike_case(129, 3, -33, 4096, True), M.check_spike),
        lambda: (M.spike_case(65, 3, 64, 68, False), M.check_spike),
    ],
    "bias_edge_wrong": [
        lambda: (M.spike_case(33, 3, 32, 33, False), M.check_spike),
        lambda: (M.spike_case(65, 3, -64, 68, True), M.check_spike),
        lambda: (M.spike_case(129, 3, 128, 4096, False), M.check_spike),
    ],
    "gqa_head_map_wrong": [
        lambda: (M.headmap_case(1, 4, 2), M.check_headmap),
        lambda: (M.headmap_case(129, 6, 2), M.check_headmap),
        lambda: (M.headmap_case(65, 28, 4), M.check_headmap),
        lambda: (M.counting_case("lm", 33, 4, 2, 128, True), M.check_counting),
    ],
    "no_rescale": [
        lambda: (M.spike_case(65, 3, 32, 65, False), M.check_spike),
        lambda: (M.spike_case(129, 3, 128, 132, False), M.check_spike),
        lambda: (M.bound_case("text", "late_max", 65, 1, 1, 64), None),
        lambda: (M.bound_case("lm", "late_max", 129, 4, 2, 128, True), None),
        lambda: (M.bound_case("vision", "late_max", 133, 3, 3, 96, segs=[60, 70, 3]), None),
    ],
}


def _fails(case, check, defect):
    out = M.run_model(case, defect)
    return M.bound_ratio(case, out) > 1.0 if check is None else check(case, out) > 0


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_defect_is_rejected(defect):
    assert CATCHERS[defect], "no probe is aimed at this defect"
    for i, make in enumerate(CATCHERS[defect]):
        case, check = make()
        assert not _fails(case, check, None), (defect, i, "the correct arithmetic must pass the same check")
        assert _fails(case, check, defect), (defect, i)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_defect_fails_somewhere_in_the_sweep_of_the_gpu_shapes(defect):
    """The whole list of exact probes at the short lengths: how many of them reject the defect (at least one must)."""
    n = sum(check(case, M.run_model(case, defect)) > 0 for _, case, check in _short_probes() if M.defect_applies(case, defect))
    print(f"{defect}: rejected by {n} exact probes")
    assert n >= 1


def _fp32_reference(case):
    """What the tests before this file compare with: an fp32 softmax."""
    hm = M.head_map(case.q.shape[0], case.k.shape[0])
    s = case.scale * case.q.float() @ case.k.float()[hm].transpose(1, 2)
    if case.table is not None:
        s = s + M.dense_bias(case)
    if case.causal:
        s = s.masked_fill(~M.dense_mask(case), float("-inf"))
    return torch.softmax(s, -1) @ case.v.float()[hm]


def test_the_gap_one_dropped_key_of_1500_passes_the_old_thresholds():
    """N(0, 1) inputs, LM shape, L = 1500: the last key never counted stays under 2e-2 and over 40 dB.  On such inputs the key weighs
    about 1 / 1500 in the one row that sees it, so the fp64 bound may or may not notice; the counting probe and the late_max family,
    at the same length, must."""
    case = M.bound_case("lm", "randn", 1500, 2, 1, 128, True)
    ref32, ref = _fp32_reference(case), M.reference(case)
    good, bad = M.run_model(case), M.run_model(case, "drop_last_key")
    err, p = float((bad.float() - ref32).abs().max()), M.psnr(bad, ref32)
    rg, rb = M.bound_ratio(case, good, ref), M.bound_ratio(case, bad, ref)
    print(f"drop_last_key L=1500 D=128: max abs err {err:.3e}, PSNR {p:.2f} dB; err / bound {rb:.2f} (correct arithmetic: {rg:.2f})")
    assert err <= 2e-2 and p >= 40.0, "the old thresholds used to pass this defect: the reason for the probes"
    assert rg <= 1.0
    assert not torch.equal(good[:, -1], bad[:, -1]) and torch.equal(good[:, :-1], bad[:, :-1])     # causal: only the last row sees the key
    probe = M.counting_case("lm", 1500, 2, 1, 128, True)
    assert M.check_counting(probe, M.run_model(probe)) == 0 and M.check_counting(probe, M.run_model(probe, "drop_last_key")) > 0
    late = M.bound_case("lm", "late_max", 1500, 2, 1, 128, True)
    assert M.bound_ratio(late, M.run_model(late)) <= 1.0 < M.bound_ratio(late, M.run_model(late, "drop_last_key"))


def test_the_gap_a_wrong_bias_edge_at_1000_passes_the_old_thresholds():
    """N(0, 1) inputs and a 2 N(0, 1) table, L = 1000, D = 64: the two extreme offsets read wrong leave the old figures where they
    were; the spike probe at delta = +-(L - 1) rejects it."""
    case = M.bound_case("text", "randn", 1000, 1, 1, 64, False, True)
    ref32 = _fp32_reference(case)
    good, bad = M.run_model(case), M.run_model(case, "bias_edge_wrong")
    eg, pg = float((good.float() - ref32).abs().max()), M.psnr(good, ref32)
    eb, pb = float((bad.float() - ref32).abs().max()), M.psnr(bad, ref32)
    print(f"bias_edge_wrong L=1000 D=64: max abs err {eb:.3e} (correct {eg:.3e}), PSNR {pb:.2f} dB (correct {pg:.2f})")
    assert eb <= 2e-2 and pb >= 40.0, "the old thresholds used to pass this defect: the reason for the probes"
    for delta in (-(129 - 1), 129 - 1):
        probe = M.spike_case(129, 3, delta, 4096, False)
        assert M.check_spike(probe, M.run_model(probe)) == 0
        assert M.check_spike(probe, M.run_model(probe, "bias_edge_wrong")) > 0
