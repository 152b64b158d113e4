"""-m gpu: the row kernels of the prompt encoders (csrc/text.hip, csrc/vision.hip; rgn_silu_bf16, rgn_gate_resid_rows, rgn_lm_kv_append_bf16)
through their C entries against the CPU model of tests/encoder_rows_model.py - tests/test_encoder_rows_model.py shows that the model holds
its own fp32 evaluations, that every named defect fails one of these checks and that the ambiguity caps hold on these very inputs.

  1  every one of the 65 536 bf16 inputs through quick_gelu, silu, gelu_erf and (against seven up values) swiglu: each output inside its
     interval of bit patterns (expf within 3, erff within 16 ulps of fp32; -0, denormals, +-inf, NaN by IEEE);
  2  the fp32 -> bf16 convert of common.h on the 393 216 fp32 patterns around every rounding decision, and the bf16 copy, via cast_pad_rows;
  3  LayerNorm: exact probes (bits) at d = 1 ... 1280 with strides and canaries, the fp64 interval on seeded random rows;
  4  the second pass of every grid-stride loop at the smallest shape that reaches it, and every kernel at its smallest legal shape, bit-exact
     (the activations: inside the interval) on seeded values with -0, denormals and +-inf;
  5  text_embed and text_pool_row at their edges.
Every output buffer carries canaries behind what may be written; every repeated call is bit-identical."""
import faulthandler
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_rows_model as E  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_p, _stream = ops._p, ops._stream


@pytest.fixture(autouse=True)
def _time_limit(request):
    """Each test here is a handful of launches: one that has not returned after a minute hangs - end the process, with a traceback.
    Prints the test's wall time (-s shows it: profiles/r29_encoder_rows_notes.md quotes these)."""
    faulthandler.dump_traceback_later(60, exit=True)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()
    print(f"  [{request.node.name}: {time.perf_counter() - t0:.2f} s]")


def _dev(bits):
    """uint16 bit patterns -> a bf16 tensor on the device."""
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).to(DEV).view(torch.bfloat16)


def _host(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _vals(v):
    """fp64 holding bf16 values -> a bf16 tensor on the device."""
    return _dev(E.bits_of(v))


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _stream()), name)
    torch.cuda.synchronize()


def _report(bad, *arrays):
    i = np.flatnonzero(np.asarray(bad).reshape(-1))[:6]
    return int(np.asarray(bad).sum()), [[hex(int(np.asarray(a).reshape(-1)[j])) for a in arrays] for j in i]


UNARY_ENTRY = {"quick_gelu": "rgn_quick_gelu_bf16", "silu": "rgn_silu_bf16", "gelu_erf": "rgn_gelu_erf_bf16"}


def _run_unary(name, xb, y0):
    x, y = _dev(xb), _dev(y0)
    _call(UNARY_ENTRY[name], _p(x), _p(y), len(xb))
    assert np.array_equal(_host(x), xb)
    return _host(y)


# ---- 1. all 65 536 inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quick_gelu", "silu", "gelu_erf"])
def test_every_bf16_input_lands_in_its_interval(name):
    y0 = np.full(65536 + 8, E.CANARY, np.uint16)
    y = _run_unary(name, E.ALL16, y0)
    assert (y[65536:] == E.CANARY).all(), "wrote behind the n elements"
    t = E.unary_table(name)
    bad = E.unary_violations(name, E.ALL16, y[:65536])
    off = (y[:65536] != t["central"]) & ~t["nan"]
    print(f"{name}: {int(off.sum())} of 65536 outputs took a non-central value; {int(bad.sum())} outside their interval")
    assert not bad.any(), (name,) + _report(bad, E.ALL16, y[:65536], t["lo_bits"], t["hi_bits"])
    assert np.array_equal(_run_unary(name, E.ALL16, y0), y), "a repeated call must be bit-identical"


def test_every_bf16_gate_against_seven_up_values_through_swiglu():
    x, y0 = E.swiglu_all_inputs()
    M, F = len(E.SWIGLU_UPS), 65536
    xd = _dev(x)
    out = []
    for _ in range(2):
        yd = _dev(y0)
        _call("rgn_swiglu_bf16", _p(xd), x.shape[1], _p(yd), y0.shape[1], M, F)
        out.append(_host(yd))
    y = out[0]
    assert np.array_equal(out[1], y), "a repeated call must be bit-identical"
    assert (y[M:] == E.CANARY).all() and (y[:, F:] == E.CANARY).all(), "wrote outside [M, F]"
    gate, up = x[:, :F], x[:, F:2 * F]
    bad = E.swiglu_violations(gate, up, y[:M, :F])
    central = E.swiglu_central(gate, up)
    for r, u in enumerate(E.SWIGLU_UPS):
        off = (y[r, :F] != central[r]) & ~E.is_nan(central[r])
        print(f"swiglu, up = {u:g}: {int(off.sum())} of 65536 outputs took a non-central value; {int(bad[r].sum())} outside their interval")
    assert not bad.any(), _report(bad, gate, up, y[:M, :F])


# ---- 2. the fp32 -> bf16 convert, exhaustively where it can differ ---------------------------------------------------------------------
def test_f2bf_is_the_add_0x7fff_rounding_on_every_finite_value_and_infinity_and_keeps_a_nan():
    M, K, Kp = 48, 8192, 8200
    x32 = E.f2bf_inputs().reshape(M, K)
    want = E.cast_pad_rows(x32, K, Kp)
    xd = torch.from_numpy(x32.copy()).to(DEV)
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x32.view(np.uint32))               # the patterns reach the device as they are
    out = []
    for _ in range(2):
        yd = _dev(np.full((M + 1, Kp), E.CANARY, np.uint16))
        _call("rgn_cast_pad_rows", _p(xd), ops._dt(xd), K, _p(yd), M, K, Kp)
        out.append(_host(yd))
    y = out[0]
    assert np.array_equal(out[1], y)
    assert (y[M:] == E.CANARY).all() and not y[:M, K:].any()
    nan = np.isnan(x32)
    got = y[:M, :K]
    assert E.is_nan(got[nan]).all(), "a NaN must stay a NaN"
    bad = ~nan & (got != want[:, :K])
    assert not bad.any(), _report(bad, x32.view(np.uint32), got, want[:, :K])
    den = ~nan & (np.abs(x32) < 2.0 ** -126) & (x32 != 0)
    print(f"f2bf: {int((~nan).sum())} non-NaN patterns equal the add-0x7fff rounding, {int(den.sum())} fp32 denormals among them; {int(nan.sum())} NaNs stay NaNs")


def test_cast_pad_rows_copies_every_bf16_pattern():
    M, K, Kp = 16, 4096, 4104
    xb = E.ALL16.reshape(M, K)
    xd = _dev(xb)
    yd = _dev(np.full((M + 1, Kp), E.CANARY, np.uint16))
    _call("rgn_cast_pad_rows", _p(xd), ops._dt(xd), K, _p(yd), M, K, Kp)
    y = _host(yd)
    assert np.array_equal(y[:M, :K], xb) and not y[:M, K:].any() and (y[M:] == E.CANARY).all()         # NaN payloads included: a copy


# ---- 3. LayerNorm ------------------------------------------------------------------------------------------------------------------
def _layer_norm(x, ldx, gamma, beta, out, ldo, M, d, eps):
    _call("rgn_layer_norm_rows", _p(x), ldx, _p(gamma), _p(beta), _p(out), ldo, M, d, eps)


@pytest.mark.parametrize("d", E.LN_PROBE_D)
def test_layer_norm_exact_probes_equal_the_model_bit_for_bit(d):
    for M in E.LN_PROBE_M:
        p = E.LnProbe(d, M)
        x, g, b = _vals(p.x), _vals(p.gamma), _vals(p.beta)
        want = E.bits_of(p.expected)
        out = []
        for _ in range(2):
            o = _vals(p.out0)
            _layer_norm(x, p.ldx, g, b, o, p.ldo, M, d, p.eps)
            out.append(_host(o))
        bad = out[0] != want
        assert not bad.any(), (p.name,) + _report(bad, out[0], want)
        assert np.array_equal(out[0], out[1]) and np.array_equal(_host(x), E.bits_of(p.x)), p.name


@pytest.mark.parametrize("d", E.LN_RANDOM_D)
def test_layer_norm_interval_on_seeded_random_rows(d):
    for dd, M, fam in E.ln_random_grid():
        if dd != d:
            continue
        x, gamma, beta = E.ln_random_case(d, M, fam)
        xw = torch.full((M + 1, d + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
        xw[:M, :d] = _vals(x)
        buf = torch.full((M + 1, d + 16), 77.0, dtype=torch.bfloat16, device=DEV)
        _layer_norm(xw, d + 8, _vals(gamma), _vals(beta), buf, d + 16, M, d, E.LN_EPS)
        out = buf[:M, :d].float().cpu().double().numpy()
        lo, hi = E.ln_interval(x, gamma, beta)
        bad = ~((lo <= out) & (out <= hi))
        print(f"LayerNorm d={d} M={M} {fam}: {int(bad.sum())} outside, {float((lo != hi).mean()):.3%} of the intervals hold more than one value")
        assert not bad.any(), (d, M, fam, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        first = buf.clone()
        buf[:M, :d] = 77.0
        assert bool((buf == 77.0).all()), (d, M, fam, "wrote outside its rows / columns")
        _layer_norm(xw, d + 8, _vals(gamma), _vals(beta), buf, d + 16, M, d, E.LN_EPS)
        assert torch.equal(buf.view(torch.int16), first.view(torch.int16)), "a repeated call must be bit-identical"


# ---- 4. the second pass of every grid-stride loop; the smallest legal shapes --------------------------------------------------------------
SIZES = ("smallest", "second_pass")


def _shape(kind, size):
    return (E.SMALLEST if size == "smallest" else E.SECOND_PASS)[kind]


def _twice(run):
    a, b = run(), run()
    assert np.array_equal(a, b), "a repeated call must be bit-identical"
    return a


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("entry", ["geglu", "swiglu"])
def test_glu_kernels(entry, size):
    s = _shape("glu", size)
    M, F = s["M"], s["F"]
    x, y0 = E.glu_case(M, F)
    assert size == "smallest" or E.items("glu", **s) > E.CAP_2048 * 256
    xd = _dev(x)

    def run():
        yd = _dev(y0)
        _call(f"rgn_{entry}_bf16", _p(xd), x.shape[1], _p(yd), y0.shape[1], M, F)
        return _host(yd)
    y = _twice(run)
    assert (y[M:] == E.CANARY).all() and (y[:, F:] == E.CANARY).all(), "wrote outside [M, F]"
    if entry == "geglu":
        want = E.geglu(x, x.shape[1], y0, y0.shape[1], M, F)
        bad = ~E.same_bits(y, want)
    else:
        bad = E.swiglu_violations(x[:, :F], x[:, F:2 * F], y[:M, :F])
    assert not bad.any(), (entry, size) + _report(bad)
    assert np.array_equal(_host(xd), x)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", ["quick_gelu", "gelu_erf", "silu"])
def test_unary_kernels(name, size):
    n = _shape("unary_n", size)
    xb, y0 = E.unary_case(n)
    y = _twice(lambda: _run_unary(name, xb, y0))
    assert (y[n:] == E.CANARY).all(), "wrote behind the n elements"
    bad = E.unary_violations(name, xb, y[:n])
    assert not bad.any(), (name, size) + _report(bad, xb, y[:n])


@pytest.mark.parametrize("size", SIZES)
def test_mrope(size):
    s = _shape("mrope", size)
    L, Hq, Hkv = s["L"], s["Hq"], s["Hkv"]
    x, cos, sin = E.mrope_case(L, Hq, Hkv)
    assert size == "smallest" or E.items("mrope", **s) > E.CAP_2048 * 256
    want = x.copy()
    want[:L] = E.mrope(x[:L], cos, sin, Hq, Hkv)
    cd, sd = _dev(cos), _dev(sin)

    def run():
        xd = _dev(x)
        _call("rgn_mrope_bf16", _p(xd), x.shape[1], _p(cd), _p(sd), L, Hq, Hkv)
        return _host(xd)
    y = _twice(run)
    bad = ~E.same_bits(y, want)
    assert not bad.any(), (size,) + _report(bad, y, want)
    n = (Hq + Hkv) * 128
    assert np.array_equal(y[:, n:], x[:, n:]) and np.array_equal(y[L:], x[L:]), "V / pad columns and the row behind must be untouched"
    assert not np.array_equal(y[:L, :n], x[:L, :n])


@pytest.mark.parametrize("size", SIZES)
def test_vision_rope(size):
    s = _shape("vision_rope", size)
    L, H, D, Dp = s["L"], s["H"], s["D"], s["Dp"]
    x, cos, sin = E.vision_rope_case(L, H, D, Dp)
    assert size == "smallest" or E.items("vision_rope", **s) > E.CAP_4096 * 256
    want = x.copy()
    want[:L] = E.vision_rope(x[:L], cos, sin, H, D, Dp)
    cd, sd = torch.from_numpy(cos).to(DEV), torch.from_numpy(sin).to(DEV)

    def run():
        xd = _dev(x)
        _call("rgn_vision_rope_bf16", _p(xd), x.shape[1], _p(cd), _p(sd), L, H, D, Dp)
        return _host(xd)
    y = _twice(run)
    bad = ~E.same_bits(y, want)
    assert not bad.any(), (size,) + _report(bad, y, want)
    heads = y[:L, :2 * H * Dp].reshape(L, 2 * H, Dp)
    assert np.array_equal(heads[..., D:], x[:L, :2 * H * Dp].reshape(L, 2 * H, Dp)[..., D:]), "pad columns [D, Dp) must be untouched"
    assert np.array_equal(y[:, 2 * H * Dp:], x[:, 2 * H * Dp:]) and np.array_equal(y[L:], x[L:]), "V columns and the row behind must be untouched"


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_cast_pad_rows(src, size):
    s = _shape("cast_pad_rows", size)
    M, K, Kp = s["M"], s["K"], s["Kp"]
    x32, xb, y0 = E.cast_pad_case(M, K, Kp)
    assert size == "smallest" or E.items("cast_pad_rows", **s) > E.CAP_4096 * 256
    xh = x32 if src == "fp32" else xb
    xd = torch.from_numpy(x32.copy()).to(DEV) if src == "fp32" else _dev(xb)
    want = y0.copy()
    want[:M] = E.cast_pad_rows(xh, K, Kp)

    def run():
        yd = _dev(y0)
        _call("rgn_cast_pad_rows", _p(xd), ops._dt(xd), xh.shape[1], _p(yd), M, K, Kp)
        return _host(yd)
    y = _twice(run)
    bad = y != want
    assert not bad.any(), (src, size) + _report(bad, y, want)


@pytest.mark.parametrize("size", SIZES)
def test_gate_resid_rows(size):
    s = _shape("gate_resid_rows", size)
    M, N = s["M"], s["N"]
    p, gate, resid, y0 = E.gate_resid_case(M, N)
    assert size == "smallest" or E.items("gate_resid_rows", **s) > E.CAP_4096 * 256
    want = y0.copy()
    want[:M, :N] = E.gate_resid_rows(p, gate, resid, N)
    pd, gd, rd = _dev(p), _dev(gate), _dev(resid)

    def run():
        yd = _dev(y0)
        _call("rgn_gate_resid_rows", _p(pd), p.shape[1], _p(gd), _p(rd), resid.shape[1], _p(yd), y0.shape[1], M, N)
        return _host(yd)
    y = _twice(run)
    bad = ~E.same_bits(y, want)
    assert not bad.any(), (size,) + _report(bad, y, want)
    _call("rgn_gate_resid_rows", _p(pd), p.shape[1], _p(gd), _p(rd), resid.shape[1], _p(rd), resid.shape[1], M, N)      # in place on resid
    r = _host(rd)
    assert E.same_bits(r[:, :N], want[:M, :N]).all() and np.array_equal(r[:, N:], resid[:, N:])


@pytest.mark.parametrize("size", SIZES)
def test_kv_append(size):
    s = _shape("kv_append", size)
    L, Hq, Hkv = s["L"], s["Hq"], s["Hkv"]
    qkv, cache0, row0 = E.kv_append_case(L, Hq, Hkv)
    assert size == "smallest" or E.items("kv_append", **s) > E.CAP_2048 * 256
    want = E.kv_append(qkv, cache0, row0, Hq, Hkv)
    qd = _dev(qkv)

    def run():
        cd = _dev(cache0)
        _call("rgn_lm_kv_append_bf16", _p(qd), qkv.shape[1], _p(cd), cache0.shape[0], row0, L, Hq, Hkv)
        return _host(cd)
    y = _twice(run)
    bad = y != want
    assert not bad.any(), (size,) + _report(bad, y, want)


# ---- 5. embedding and pooling edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", E.EMBED_D)
def test_text_embed_edges(d):
    tok, pos = E.embed_case(d)
    td, pd = _dev(tok), _dev(pos)
    for i in E.embed_ids():
        ids = np.array([i], np.int64)
        idd = torch.from_numpy(ids).to(DEV)
        for P, Pd in ((None, None), (pos, pd)):
            out = []
            for _ in range(2):
                yd = _dev(np.full((2, d), E.CANARY, np.uint16))
                _call("rgn_text_embed", _p(idd), 1, _p(td), E.EMBED_VOCAB, _p(Pd), 0 if P is None else 1, _p(yd), d)
                out.append(_host(yd))
            want = E.text_embed(ids, tok, P)
            assert np.array_equal(out[0], out[1]) and (out[0][1] == E.CANARY).all(), (d, i)
            assert E.same_bits(out[0][0], want[0]).all() if P is not None else np.array_equal(out[0][0], want[0]), (d, i, P is not None)
            assert (0 <= i < E.EMBED_VOCAB) or not out[0][0].any(), "an id outside [0, vocab) gives a zero row"


@pytest.mark.parametrize("L", E.POOL_L)
def test_text_pool_row_edges(L):
    d, ldx = 40, 48
    x = E.seeded_bits([15, L], (L, ldx))
    x[:, 0] = E.f2bf(np.arange(L, dtype=np.float32))          # the row index, readable in the result (exact up to 256, distinct rows anyway)
    xd = _dev(x)
    for name, ids, eos in E.pool_cases(L):
        idd = torch.from_numpy(ids).to(DEV)
        out = []
        for _ in range(2):
            yd = _dev(np.full(d + 8, E.CANARY, np.uint16))
            _call("rgn_text_pool_row", _p(idd), L, eos, _p(xd), ldx, d, _p(yd))
            out.append(_host(yd))
        want = E.text_pool_row(ids, eos, x, d)
        assert np.array_equal(out[0], out[1]) and (out[0][d:] == E.CANARY).all(), (L, name)
        assert np.array_equal(out[0][:d], want), (L, name, hex(int(out[0][0])), E.pooled_index(ids, eos))
