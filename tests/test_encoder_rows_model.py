"""The CPU model of the prompt encoders' row kernels (tests/encoder_rows_model.py) is SOUND - the interval holds its own reference
evaluated in fp32 (numpy's expf, torch's erff and torch's eager bf16 ops on the CPU among the evaluations), the bit-exact restatements
equal torch's CPU kernels -, SHARP - every named defect leaves an interval or changes a probe - and HONEST - the share of inputs whose
interval holds more than one bf16 value stays under its cap on the very inputs tests/test_gpu_encoder_rows.py uses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_rows_model as E  # noqa: E402

FINITE = ~E.is_nan(E.ALL16) & ((E.ALL16 & 0x7fff) != 0x7f80)
UNARY = ("quick_gelu", "silu", "gelu_erf")


def _bf(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _np_expf(a):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(a, np.float32))


def _torch_erff(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, np.float32))).numpy()


def _torch_expf(a):
    return torch.exp(torch.from_numpy(np.ascontiguousarray(a, np.float32))).numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# bit patterns
# ------------------------------------------------------------------------------------------------------------------------------------
def test_bit_helpers_agree_with_torch_and_the_key_is_the_order_of_the_values():
    x = E.f2bf_inputs()
    assert x.size == 393216 and np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) < 2.0 ** -126).any()
    got, want = E.f2bf(x), _bits(torch.from_numpy(x.copy()).to(torch.bfloat16))
    ok = ~np.isnan(x)
    assert np.array_equal(got[ok], want[ok]) and E.is_nan(got[~ok]).all() and E.is_nan(want[~ok]).all()
    assert np.array_equal(E.f2bf(E.bf2f(E.ALL16))[FINITE], E.ALL16[FINITE])
    v = E.bf2d(E.ALL16)
    order = np.argsort(E.key(E.ALL16)[~E.is_nan(E.ALL16)], kind="stable")
    vs = v[~E.is_nan(E.ALL16)][order]
    assert (np.diff(vs) >= 0).all() and E.key(np.uint16(0x8000)) == -1 and E.key(np.uint16(0)) == 0
    assert np.array_equal(E.bits_of(v[FINITE]), E.ALL16[FINITE]) and E.bits_of(np.array([2.0 ** 128, -0.0]))[0] == 0x7f80
    assert E.bits_of(E.bf16r(np.array([3.4e38, -3.4e38, -1e-45, 2.0 ** -134])))[:].tolist() == [0x7f80, 0xff80, 0x8000, 0x0000]
    assert E.same_bits(np.uint16(0x7fc1), np.uint16(0xffc0)) and not E.same_bits(np.uint16(0), np.uint16(0x8000))


def test_round32_knows_the_edges_of_fp32():
    lo, hi = E._round32(np.array([1.0, -0.0, np.inf, 2.0 ** -140, -2.0 ** -151, E.FLT_MAX * 1.5]), np.array([1.0, -0.0, np.inf, 2.0 ** -140, -2.0 ** -151, np.inf]))
    assert lo[0] < 1.0 < hi[0] and hi[0] - lo[0] < 2.0 ** -22
    assert np.signbit(lo[1]) and np.signbit(hi[1]) and lo[1] == 0 and hi[1] == 0
    assert lo[2] == np.inf and hi[2] == np.inf
    assert lo[3] == 2.0 ** -140 - 2.0 ** -150 and hi[3] == 2.0 ** -140 + 2.0 ** -150
    assert lo[4] < -2.0 ** -151 and hi[4] == 0 and np.signbit(hi[4])                # a negative result never rounds to +0
    assert lo[5] == np.inf and hi[5] == np.inf
    elo, ehi = E.exp_interval(np.array([0.0, 88.5, 89.0, -np.inf, -104.0, np.nan]))
    assert elo[0] == 1 - 3 * 2.0 ** -23 and ehi[0] == 1 + 3 * 2.0 ** -23 and ehi[1] < E.FLT_MAX and elo[2] == np.inf and elo[3] == 0
    assert elo[4] == 0 and 0 < ehi[4] <= 4 * 2.0 ** -149 and np.isnan(elo[5])
    assert 88.5 < E.LN_FLT_MAX < 89.0
    rlo, rhi = E.erf_interval(np.array([0.5, 4.4, -4.4, 4.2, np.inf, -np.inf]))
    assert rlo[0] < E.erf64(0.5) < rhi[0] and rhi[0] - rlo[0] == 32 * 2.0 ** -24
    assert (rlo[1], rhi[1], rlo[2], rhi[2]) == (1.0, 1.0, -1.0, -1.0) and rlo[3] < 1.0 and (rlo[4], rhi[5]) == (1.0, -1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# activations over all 65 536 inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def _evaluations(name):
    """Conforming fp32 evaluations of one unary kernel over all inputs: the correctly rounded transcendental, numpy's and torch's fp32
    ones, and torch's eager bf16 op sequence on the CPU."""
    x = _bf(E.ALL16)
    if name == "quick_gelu":
        return {"central": E.quick_gelu(E.ALL16), "numpy expf": E.quick_gelu(E.ALL16, expf=_np_expf), "torch expf": E.quick_gelu(E.ALL16, expf=_torch_expf),
                "torch eager bf16": _bits(x * torch.sigmoid(1.702 * x))}
    if name == "silu":
        return {"central": E.silu(E.ALL16), "numpy expf": E.silu(E.ALL16, expf=_np_expf), "torch expf": E.silu(E.ALL16, expf=_torch_expf),
                "torch eager bf16": _bits(torch.nn.functional.silu(x))}
    # the device op sequence (x * 0.5) * (1 + erf(x * 0.70710678)) in torch's fp32 CPU ops, one rounding.  torch's CPU GELU of a bf16 tensor
    # is NOT this sequence: it applies the 0.5 last (inf from 2.55e38 on) and flushes results below 2^-126 - the defect `half_after_sum`
    xf = x.float()
    return {"central": E.gelu_erf(E.ALL16), "torch erff": E.gelu_erf(E.ALL16, erff=_torch_erff),
            "torch fp32 ops": _bits(((xf * 0.5) * (1.0 + torch.erf(xf * float(E.C_RSQRT2)))).to(torch.bfloat16))}


@pytest.mark.parametrize("name", UNARY)
def test_unary_interval_holds_every_fp32_evaluation_on_all_inputs(name):
    t = E.unary_table(name)
    assert (t["lo"] <= t["hi"])[~t["nan"]].all()
    for what, y in _evaluations(name).items():
        bad = E.unary_violations(name, E.ALL16, y)
        off = int((y != t["central"]).sum())
        print(f"{name}: {what}: {off} outputs differ from the central value, {int(bad.sum())} outside the interval")
        assert not bad.any(), (name, what, int(bad.sum()), [hex(int(v)) for v in E.ALL16[bad][:8]], [hex(int(v)) for v in y[bad][:8]])


@pytest.mark.parametrize("name", UNARY)
def test_unary_edges_are_the_ieee_ones(name):
    t = E.unary_table(name)
    at = lambda b: (int(t["lo_bits"][b]), int(t["hi_bits"][b]))
    assert np.array_equal(t["nan"], E.is_nan(E.ALL16) | (E.ALL16 == 0xff80))             # NaN in -> NaN; f(-inf) = NaN
    assert at(0x7f80) == (0x7f80, 0x7f80) and at(0x0000) == (0, 0) and at(0x8000) == (0x8000, 0x8000)
    neg = E.bf2d(E.ALL16)
    big = FINITE & (neg <= {"silu": -89.0, "quick_gelu": -53.0, "gelu_erf": -7.0}[name])
    assert big.any() and (t["lo_bits"][big] == 0x8000).all() and (t["hi_bits"][big] == 0x8000).all()       # x * 0, x / inf: -0, not +0
    assert at(0x7f7f) == (0x7f7f, 0x7f7f)                                               # the largest finite value is its own image
    if name != "gelu_erf":
        edge = E.f2bf(np.array([-88.5 if name == "silu" else -52.0], np.float32))[0]          # expf(88.5) is finite (t = bf16(-52 * 1.702) = -88.5)
        assert at(edge)[0] == at(edge)[1] and 0x8000 < at(edge)[0] < 0x8080 + 0x0400     # below the overflow edge: small, negative, not -0


def test_the_share_of_ambiguous_inputs_stays_under_its_cap():
    for name in UNARY:
        t = E.unary_table(name)
        amb = (t["lo"] != t["hi"]) & ~t["nan"]
        assert not amb[~FINITE].any()
        n = int(amb[FINITE].sum())
        print(f"{name}: {n} of {E.N_FINITE} finite inputs have an interval of more than one bf16 value ({n / E.N_FINITE:.3%})")
        assert FINITE.sum() == E.N_FINITE and n <= E.UNARY_CAP * E.N_FINITE, (name, n)
    x, _ = E.swiglu_all_inputs()
    F = 65536
    lo, hi, nan, split = E.swiglu_interval(x[:, :F], x[:, F:2 * F])
    assert not split.any()
    for r, u in enumerate(E.SWIGLU_UPS):
        n = int(((lo[r] != hi[r]) & ~nan[r])[FINITE].sum())
        print(f"swiglu, up = {u:g}: {n} ambiguous")
        assert n <= E.UNARY_CAP * E.N_FINITE
    # the seeded inputs of the second-pass tests
    n = E.SECOND_PASS["unary_n"]
    xb = E.unary_case(n)[0]
    for name in UNARY:
        t = E.unary_table(name)
        share = float(((t["lo"] != t["hi"]) & ~t["nan"])[xb].mean())
        print(f"{name}, seeded n = {n}: ambiguous share {share:.4%}")
        assert share <= E.UNARY_CAP
        assert all((xb == s).any() for s in E.SPECIALS)
    x, _ = E.glu_case(**E.SECOND_PASS["glu"])
    F = E.SECOND_PASS["glu"]["F"]
    lo, hi, nan, split = E.swiglu_interval(x[:, :F], x[:, F:2 * F])
    assert not split.any() and float(((lo != hi) & ~nan).mean()) <= E.UNARY_CAP


@pytest.mark.parametrize("defect", E.ACT_DEFECTS)
def test_every_named_activation_defect_is_caught(defect):
    if defect in ("c1702_as_1p7", "t_not_rounded", "s_not_rounded"):
        bad = E.unary_violations("quick_gelu", E.ALL16, E.quick_gelu(E.ALL16, defect))
    elif defect in ("tanh_form", "half_after_sum"):
        bad = E.unary_violations("gelu_erf", E.ALL16, E.gelu_erf(E.ALL16, defect))
    elif defect == "silu_sigmoid_rounded":
        bad = E.unary_violations("silu", E.ALL16, E.silu(E.ALL16, defect))
    else:                                                     # addressing: the all-inputs swiglu case and the smallest-but-one glu case
        x, y0 = E.swiglu_all_inputs()
        M, F = len(E.SWIGLU_UPS), 65536
        y = E.swiglu(x, x.shape[1], y0, y0.shape[1], M, F, defect)
        bad = _swiglu_bad(x, y0, y, M, F)
        xg, yg = E.glu_case(5, 24)
        if defect == "ldy_ignored":
            assert not np.array_equal(E.geglu(xg, xg.shape[1], yg, yg.shape[1], 5, 24, defect), E.geglu(xg, xg.shape[1], yg, yg.shape[1], 5, 24))
    print(f"{defect}: {int(bad.sum())} elements outside")
    assert bad.any()
    if defect == "half_after_sum":                            # only the ends of the format see it: the reason to run every input
        v = np.abs(E.bf2d(E.ALL16[bad]))
        assert ((v > 1e38) | (v < 1e-37)).all()


def _swiglu_bad(x, y0, y, M, F):
    """Violations of a swiglu result: the written part outside its interval, anything else changed."""
    bad = np.zeros(y.shape, bool)
    bad[:M, :F] = E.swiglu_violations(x[:M, :F], x[:M, F:2 * F], y[:M, :F])
    keep = np.ones(y.shape, bool)
    keep[:M, :F] = False
    return bad | (keep & (y != y0))


def test_swiglu_and_geglu_restated_lie_in_their_intervals_and_equal_torch():
    x, y0 = E.swiglu_all_inputs()
    M, F = len(E.SWIGLU_UPS), 65536
    for expf in (E.expf_central, _np_expf):
        y = E.swiglu(x, x.shape[1], y0, y0.shape[1], M, F, expf=expf)
        assert not _swiglu_bad(x, y0, y, M, F).any()
    eager = _bits(torch.nn.functional.silu(_bf(x[:, :F])) * _bf(x[:, F:2 * F]))
    assert not E.swiglu_violations(x[:, :F], x[:, F:2 * F], eager).any()
    xg, yg = E.glu_case(67, 40)
    got = E.geglu(xg, xg.shape[1], yg, yg.shape[1], 67, 40)
    want = _bits(_bf(xg[:, 40:80]) * _bf(xg[:, :40]))
    assert E.same_bits(got[:67, :40], want).all() and (got[67:] == E.CANARY).all() and (got[:, 40:] == E.CANARY).all()
    assert E.is_nan(want).any()                               # inf * 0 among the seeded values


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
def test_ln_probes_are_exact_and_every_stage_is_one_operation_on_known_values():
    for p in E.ln_probes():
        d = p.d
        assert np.array_equal(E.bf16_rne(p.X), p.X) and np.array_equal(E.bf16_rne(p.gamma), p.gamma) and np.array_equal(E.bf16_rne(p.beta), p.beta)
        for r in range(p.M):
            assert E.exact_in_any_order(p.X[r]), (p.name, r)
            mean = p.X[r].sum() / d
            assert E.f32(mean) == mean and E.f32(E.f32(p.X[r].sum()) / d) == mean, (p.name, r)        # the fp32 division is exact too
            assert E.exact_in_any_order((p.X[r] - mean) ** 2), (p.name, r)
        got = E._rows_of(p.expected, p.ldo, p.M, d)
        lo, hi = E.ln_interval(p.X, p.gamma, p.beta, p.eps)
        assert ((lo <= got) & (got <= hi)).all(), p.name
        keep = np.ones(len(p.out0), bool)
        for r in range(p.M):
            keep[r * p.ldo:r * p.ldo + d] = False
        assert np.array_equal(p.expected[keep], p.out0[keep]) and (got < 100).all()
        if p.M == 5:                                          # the constant row gives beta, bit for bit
            assert np.array_equal(E.bits_of(got[2]), E.bits_of(p.beta)), p.name
        if d == 1:
            assert np.array_equal(got, np.broadcast_to(p.beta, got.shape))
        # torch's CPU LayerNorm (fp32 statistics of its own order, one rounding) lies in the interval
        ln = torch.nn.functional.layer_norm(torch.from_numpy(p.X).float(), (d,), torch.from_numpy(p.gamma).float(), torch.from_numpy(p.beta).float(), p.eps)
        t = ln.to(torch.bfloat16).double().numpy()
        assert ((lo <= t) & (t <= hi)).all(), (p.name, "torch")


@pytest.mark.parametrize("defect", E.LN_DEFECTS)
def test_every_named_ln_defect_changes_a_probe(defect):
    hit = [p.name for p in E.ln_probes() if not np.array_equal(E.bits_of(p.run(defect)), E.bits_of(p.expected))]
    print(f"{defect}: {len(hit)} probes change: {hit[:6]}")
    assert hit
    if defect == "variance_unbiased":                         # and a random case leaves the interval
        assert not _ln_inside(64, 67, "centred", defect)[0]


def _ln_inside(d, M, fam, defect=None):
    x, gamma, beta = E.ln_random_case(d, M, fam)
    out = E.layer_norm(x.reshape(-1), d, gamma, beta, np.zeros(M * d), d, M, d, E.LN_EPS, defect).reshape(M, d)
    lo, hi = E.ln_interval(x, gamma, beta)
    return bool(((lo <= out) & (out <= hi)).all()), int((lo != hi).sum()), lo.size, lo, hi


def test_ln_interval_holds_the_model_and_torch_and_ambiguity_stays_under_the_trunk_models_caps():
    amb, tot = {}, {}
    for d, M, fam in E.ln_random_grid():
        ok, a, n, lo, hi = _ln_inside(d, M, fam)
        assert ok, (d, M, fam)
        x, gamma, beta = E.ln_random_case(d, M, fam)
        t = torch.nn.functional.layer_norm(torch.from_numpy(x).float(), (d,), torch.from_numpy(gamma).float(), torch.from_numpy(beta).float(), E.LN_EPS)
        t = t.to(torch.bfloat16).double().numpy()
        assert ((lo <= t) & (t <= hi)).all(), (d, M, fam, "torch")
        amb[fam, d], tot[fam, d] = amb.get((fam, d), 0) + a, tot.get((fam, d), 0) + n
    for fam in E.LN_FAMILIES:
        per_d = {d: amb[f, d] / tot[f, d] for (f, d) in amb if f == fam}
        print(f"LayerNorm {fam}: ambiguous share per d: " + ", ".join(f"{d}: {s:.3%}" for d, s in sorted(per_d.items())))
        assert all(s <= E.AMBIGUITY_CAP[fam] for s in per_d.values()), (fam, per_d)


# ------------------------------------------------------------------------------------------------------------------------------------
# the bit-exact kernels: equal to torch's CPU kernels, every defect seen, every second pass reached
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_second_pass_shapes_are_the_smallest_that_pass_the_grid_cap():
    for kind, cap in E.GRID_CAP.items():
        n = E.items(kind, **E.SECOND_PASS[kind])
        assert cap * 256 < n, kind
        s = dict(E.SECOND_PASS[kind])
        first = "M" if "M" in s else "L"
        s[first] -= 1
        assert E.items(kind, **s) <= cap * 256 or kind == "vision_rope", kind          # one row fewer stays inside the first pass
        assert E.items(kind, **E.SMALLEST[kind]) >= 1
    assert E.SECOND_PASS["unary_n"] > E.CAP_2048 * 256


def _rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), -1)


def test_mrope_equals_the_eager_bf16_ops_and_its_defects_are_seen():
    L, Hq, Hkv = 67, 3, 2
    x, cos, sin = E.mrope_case(L, Hq, Hkv)
    got = E.mrope(x[:L], cos, sin, Hq, Hkv)
    n = (Hq + Hkv) * 128
    X = _bf(x[:L, :n]).view(L, Hq + Hkv, 128)
    c, s = _bf(cos)[:, None, :], _bf(sin)[:, None, :]
    want = _bits((X * c + _rot_half(X) * s).reshape(L, n))
    assert E.same_bits(got[:, :n], want).all() and np.array_equal(got[:, n:], x[:L, n:]) and E.is_nan(want).any()
    for defect in ("sin_sign_flipped", "products_not_rounded"):
        assert not E.same_bits(E.mrope(x[:L], cos, sin, Hq, Hkv, defect), got).all(), defect
    s2 = E.SECOND_PASS["mrope"]
    x, cos, sin = E.mrope_case(**s2)
    full, skipped = E.mrope(x[:s2["L"]], cos, sin, s2["Hq"], s2["Hkv"]), E.mrope(x[:s2["L"]], cos, sin, s2["Hq"], s2["Hkv"], "second_pass_skipped")
    diff = ~E.same_bits(full, skipped)
    assert diff.any() and not diff[:s2["L"] - 1].any()       # only the last row lies in the second pass


def test_vision_rope_equals_the_eager_fp32_op_and_its_defects_are_seen():
    L, H, D, Dp = 67, 2, 80, 96
    x, cos, sin = E.vision_rope_case(L, H, D, Dp)
    got = E.vision_rope(x[:L], cos, sin, H, D, Dp)
    X = _bf(x[:L, :2 * H * Dp]).view(L, 2 * H, Dp)[..., :D].float()
    c, s = torch.from_numpy(cos)[:, None, :], torch.from_numpy(sin)[:, None, :]
    want = _bits((X * c + _rot_half(X) * s).to(torch.bfloat16))
    g = got[:, :2 * H * Dp].reshape(L, 2 * H, Dp)
    assert E.same_bits(g[..., :D], want).all() and np.array_equal(g[..., D:], x[:L, :2 * H * Dp].reshape(L, 2 * H, Dp)[..., D:])
    assert np.array_equal(got[:, 2 * H * Dp:], x[:L, 2 * H * Dp:])
    for defect in ("sin_sign_flipped", "products_rounded", "half_taken_from_Dp"):
        assert not E.same_bits(E.vision_rope(x[:L], cos, sin, H, D, Dp, defect), got).all(), defect
    s2 = E.SECOND_PASS["vision_rope"]
    x, cos, sin = E.vision_rope_case(**s2)
    L = s2["L"]
    full = E.vision_rope(x[:L], cos, sin, s2["H"], s2["D"], s2["Dp"])
    skipped = E.vision_rope(x[:L], cos, sin, s2["H"], s2["D"], s2["Dp"], "second_pass_skipped")
    diff = ~E.same_bits(full, skipped)
    assert diff.any() and not diff[:3276].any()              # 4096 * 256 items / 320 per row: rows below 3276 are first-pass rows


def test_the_copies_and_sums_equal_torch_and_a_skipped_second_pass_is_seen():
    # cast_pad_rows: torch's fp32 -> bf16 cast, the copy, the zero columns
    s = E.SECOND_PASS["cast_pad_rows"]
    x32, xb, _ = E.cast_pad_case(**s)
    y = E.cast_pad_rows(x32, s["K"], s["Kp"])
    assert np.array_equal(y[:, :s["K"]], _bits(torch.from_numpy(x32[:, :s["K"]].copy()).to(torch.bfloat16))) and not y[:, s["K"]:].any()
    assert np.array_equal(E.cast_pad_rows(xb, s["K"], s["Kp"])[:, :s["K"]], xb[:, :s["K"]])
    before = np.full(y.shape, E.CANARY, np.uint16)
    assert (E.skip_second_pass(before, y, E.CAP_4096) != y).any() and (x32.view(np.uint32) & 0xffff).any()
    # gate_resid_rows: resid + gate * p in bf16
    s = E.SECOND_PASS["gate_resid_rows"]
    p, gate, resid, y0 = E.gate_resid_case(**s)
    N = s["N"]
    y = E.gate_resid_rows(p, gate, resid, N)
    want = _bits(_bf(resid[:, :N]) + _bf(gate)[None] * _bf(p[:, :N]))
    assert E.same_bits(y, want).all() and E.is_nan(y).any()
    assert (E.skip_second_pass(y0[:s["M"], :N], y, E.CAP_4096) != y).any()
    # kv_append
    s = E.SECOND_PASS["kv_append"]
    qkv, cache0, row0 = E.kv_append_case(**s)
    c = E.kv_append(qkv, cache0, row0, s["Hq"], s["Hkv"])
    assert (c[:row0] == E.CANARY).all() and (c[row0 + s["L"]:] == E.CANARY).all() and np.array_equal(c[row0 + 5], qkv[5, 1024:3072])
    assert (E.skip_second_pass(cache0[row0:row0 + s["L"]], c[row0:row0 + s["L"]], E.CAP_2048) != c[row0:row0 + s["L"]]).any()
    # geglu / swiglu / the unary kernels
    s = E.SECOND_PASS["glu"]
    x, y0 = E.glu_case(**s)
    for fn in (E.geglu, E.swiglu):
        a = fn(x, x.shape[1], y0, y0.shape[1], s["M"], s["F"])
        b = fn(x, x.shape[1], y0, y0.shape[1], s["M"], s["F"], "second_pass_skipped")
        assert (a != b).any() and np.array_equal(a[:s["M"] - 1], b[:s["M"] - 1]) and (a[:, s["F"]:] == E.CANARY).all() and (a[s["M"]:] == E.CANARY).all()
    n = E.SECOND_PASS["unary_n"]
    xb = E.unary_case(n)[0]
    y0 = E.unary_case(n)[1]
    for name in ("quick_gelu", "gelu_erf"):
        full, skipped = E.unary(name, xb, y0), E.unary(name, xb, y0, "second_pass_skipped")
        assert not E.unary_violations(name, xb, full[:n]).any() and E.unary_violations(name, xb, skipped[:n]).any()


def test_text_embed_and_pool_row_equal_torch_and_their_defects_are_seen():
    for d in E.EMBED_D:
        tok, pos = E.embed_case(d)
        ids = np.array(E.embed_ids(), np.int64)
        ok = (ids >= 0) & (ids < E.EMBED_VOCAB)
        assert ok.tolist() == [False, False, True, False, True]
        for P in (None, pos):
            rows = np.concatenate([E.text_embed(ids[i:i + 1], tok, P) for i in range(len(ids))])
            want = _bf(tok)[torch.from_numpy(np.where(ok, ids, 0))]
            if P is not None:
                want = want + _bf(P)
            want = torch.where(torch.from_numpy(ok)[:, None], want, torch.zeros_like(want))
            assert E.same_bits(rows, _bits(want)).all() and not rows[~ok].any()
        twice = E.text_embed(ids[2:3], tok, pos, "pos_added_in_bf16_twice")
        assert not E.same_bits(twice, E.text_embed(ids[2:3], tok, pos)).all()
    for L in E.POOL_L:
        for name, ids, eos in E.pool_cases(L):
            i32 = torch.from_numpy(ids).to(torch.int32)
            want = int(i32.argmax()) if eos == 2 else int((i32 == eos).int().argmax())
            assert E.pooled_index(ids, eos) == want, (L, name)
    seen = [(L, name) for L in E.POOL_L for name, ids, eos in E.pool_cases(L) if E.pooled_index(ids, eos, "tie_to_higher_index") != E.pooled_index(ids, eos)]
    print("tie_to_higher_index changes", seen)
    assert {n for _, n in seen} >= {"all_equal", "first_of_two", "max_at_256"}
    ids = dict((n, i) for n, i, _ in E.pool_cases(600))
    assert E.pooled_index(ids["max_at_256"], 2) == 256 and E.pooled_index(ids["max_last"], 2) == 599 and E.pooled_index(ids["eos_never"], 5000) == 0
    assert E.pooled_index(ids["truncated_to_int32"], 2) != 0


def test_every_named_defect_has_a_test():
    src = open(os.path.abspath(__file__), encoding="utf-8").read()
    for d in E.ACT_DEFECTS + E.LN_DEFECTS + E.ROPE_DEFECTS + E.OTHER_DEFECTS:
        assert d in E.ACT_DEFECTS + E.LN_DEFECTS or f'"{d}"' in src, d
