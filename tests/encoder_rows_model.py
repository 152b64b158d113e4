"""CPU model of the prompt encoders' row kernels (csrc/text.hip: CLIP-L, T5-XXL, the Qwen2.5-VL language model; csrc/vision.hip: the
Qwen2.5-VL tower; with rgn_silu_bf16 of norm.hip, rgn_gate_resid_rows of connector.hip and rgn_lm_kv_append_bf16 of decode.hip, which
share their grid-stride form): the contracts, an INTERVAL of bf16 bit patterns for the kernels that call expf / erff or sum a row, the
kernels' arithmetic restated in numpy with NAMED DEFECTS, and the probe and case generators of tests/test_gpu_encoder_rows.py.  Test
infrastructure only (numpy, fp64; fp32 numpy arithmetic where one IEEE operation is the contract).

Contracts (the kernels' comments, restated)
-------------------------------------------
Every operation below is ONE fp32 IEEE operation (the files are built with -ffp-contract=off; division and sqrtf are the correctly
rounded forms), bf16(.) rounds to nearest even (common.h: the hardware convert, claimed identical to the add-0x7fff trick for every
finite value and infinity; a NaN stays a NaN).
  quick_gelu  t = bf16(v * 1.702f);  s = bf16(1 / (1 + expf(-t)));  out = bf16(v * s)
  silu        (rgn_silu_bf16, and the gate half of swiglu)  s = bf16(g / (1 + expf(-g)));  swiglu: out = bf16(s * up), gate = x[m, f],
              up = x[m, F + f]
  gelu_erf    out = bf16((v * 0.5f) * (1 + erff(v * 0.70710678f)))
  geglu       out = bf16(x[m, F + f] * x[m, f]): a product of two bf16 values is exact in fp32 - one rounding, bit-exact
  LayerNorm   (rgn_layer_norm_rows)  mean = (sum x) / d;  var = (sum (x - mean)^2) / d (two passes, biased);  rstd = 1 / sqrtf(var + eps);
              out = bf16(gamma * (rstd * (x - mean)) + beta); the two sums in ANY order within CHAIN (tests/trunk_rows_model.py)
  text_embed  out[l] = tok[ids[l]], with a position table bf16(tok[ids[l]] + pos[l]); an id outside [0, vocab) gives a zero row
  text_pool_row  the row of x at the FIRST maximum of int32(ids) when eos == 2, else at the first j with int32(ids[j]) == eos, else row 0
  mrope       per head of 128, a = x[c], b = x[c + 64], c < 64:  out[c] = bf16(bf16(a cos[c]) + bf16(-b sin[c])),
              out[c + 64] = bf16(bf16(b cos[c + 64]) + bf16(a sin[c + 64])); bf16 tables [L, 128]; the V columns are untouched
  vision_rope per head of Dp (D real columns, half = D / 2): out[c] = bf16(a cos[c] + (-b) sin[c]), out[c + half] = bf16(b cos[c + half] +
              a sin[c + half]) - two fp32 products, their fp32 sum, one rounding; fp32 tables [L, D]; pad columns [D, Dp) and V untouched
  cast_pad_rows  y[m, :K] = bf16(x[m, :K]) (fp32 source) or a copy (bf16 source), y[m, K:Kp] = 0
  gate_resid_rows  y = bf16(resid + bf16(gate * p))
  kv_append   cache[row0 + r, :] = QKV[r, Hq 128 : (Hq + 2 Hkv) 128], bit for bit

Interval rule for expf and erff
-------------------------------
Only expf and erff have freedom: their result is the fp64 value +- K ulps of fp32, K_EXP = 3 and K_ERF = 16.  These are the OpenCL
full-profile bounds that the device math library behind HIP's expf / erff is written to.  NOBODY HAS MEASURED THESE FUNCTIONS ON THIS
HARDWARE; the K are taken from that table and are not fitted to any kernel output.  Two exact clauses carry what torch relies on:
  expf(a) is +inf for a above ln(FLT_MAX) = 88.7228; within K_EXP ulps of FLT_MAX either outcome is accepted (for bf16 arguments there is
          none: the neighbours of the threshold are 88.5 and 89);
  erff(a) is exactly +-1 wherever 1 - |erf(a)| < 2^-30.
Every other operation is pushed through as in the trunk model: an exact operation on the end points (monotone: min / max over the
end-point results, _times), then ONE widening by the unit roundoff (_widen) - here made aware of what fp32 does at its edges (_round32: a
result below 2^-126 is off by at most 2^-150 and never crosses zero; a result above FLT_MAX is +-inf; an infinite end point stays) - and
bf16(.) on the end points, which is monotone.  Outputs are compared as BIT PATTERNS in the order -inf < ... < -0 < +0 < ... < +inf
(key()): -0 and +0 are different results.  A NaN input gives a NaN output of any payload; +-inf follow IEEE: quick_gelu(-inf), silu(-inf)
and gelu_erf(-inf) are NaN (-inf * 0, -inf / inf).  Denormals are kept, as IEEE does.  The interval of a unary kernel is a table over all
65 536 inputs (unary_table); swiglu pushes the silu table's end points through the exact product.
The rule stays honest through a CAP: at most 1 % of the 65 280 finite inputs may have an interval that holds more than one bf16 value
(tests/test_encoder_rows_model.py asserts it; with the K above it finds quick_gelu 2, silu 260 - the ties g / 2 of the denormals -,
gelu_erf 366 - the cancelling tail of 1 + erff for v in about [-6.1, -2.7], and denormal ties).  Where both operands of an operation are
known values (v times an end point of s in quick_gelu, s times up in swiglu) the end points are pushed through the one fp32 rounding
exactly, as the trunk model does after y0, instead of being widened: the product of two bf16 values is exact in fp32's normal range.
What torch does: the eager-op tests of the encoders compare these sequences with torch on the device; torch's CPU GELU of a bf16 tensor
is NOT this sequence (it applies the 0.5 last - inf from 2.55e38 on - and flushes results below 2^-126), so the CPU test evaluates
gelu_erf with torch's fp32 ops, one by one.
LayerNorm: ln_y0_interval of the trunk model for rstd * (x - mean), then the product with gamma and the sum with beta widened once each.
Compared as values, as the trunk model does; caps on ambiguity: the trunk model's (1 % centred, 5 % offset rows).

Exact probes (LayerNorm): rows of small integers times a power of two about a mean that is such a number too, so both sums are exact in
fp32 in any order; every later operation is a single correctly rounded operation on known values - the GPU test compares bits.
The bit-exact kernels are restated with numpy's fp32 arithmetic (one IEEE operation per operation) on bit patterns.
"""
import math

import numpy as np

from gemm_mx8_model import f32_to_bf16_bits
from trunk_rows_model import AMBIGUITY_CAP, CHAIN, LN_FAMILIES, U32, _times, _widen, bf16_rne, f32, ln_y0_interval  # noqa: F401

K_EXP, K_ERF = 3, 16
FLT_MAX = float(np.finfo(np.float32).max)
LN_FLT_MAX = math.log(FLT_MAX)                               # 88.7228...
ERF_SATURATED = 2.0 ** -30
C_1702 = np.float32(1.702)
C_RSQRT2 = np.float32(0.70710678118654752440)
UNARY_CAP = 0.01                                             # of the 65 280 finite inputs
N_FINITE = 65280
ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)
SWIGLU_UPS = (1.0, -1.0, 0.0078125, 3.0, -240.0, 2.0 ** -126, 3.39e38)
ACT_DEFECTS = ("c1702_as_1p7", "t_not_rounded", "s_not_rounded", "tanh_form", "half_after_sum", "silu_sigmoid_rounded", "halves_swapped",
               "ldy_ignored")
LN_DEFECTS = ("variance_unbiased", "eps_dropped", "mean_of_squares_minus_square", "beta_dropped", "ldo_ignored")
ROPE_DEFECTS = ("sin_sign_flipped", "products_not_rounded", "products_rounded", "half_taken_from_Dp")
OTHER_DEFECTS = ("second_pass_skipped", "tie_to_higher_index", "pos_added_in_bf16_twice")
CAP_2048, CAP_4096 = 2048, 4096                              # the grid caps (blocks of 256 threads) of the grid-stride kernels
LN_EPS = 1e-5                                                # CLIP's layer_norm_eps


# ------------------------------------------------------------------------------------------------------------------------------------
# bit patterns
# ------------------------------------------------------------------------------------------------------------------------------------
def bf2f(bits):
    """bf16 bits -> fp32."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf2d(bits):
    """bf16 bits -> fp64."""
    with np.errstate(invalid="ignore"):
        return bf2f(bits).astype(np.float64)


def f2bf(x):
    """fp32 -> bf16 bits: the add-0x7fff round-to-nearest-even of gemm_mx8_model; a NaN becomes a quiet NaN (its payload is not part
    of any contract)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    return np.where(np.isnan(x), ((u >> 16) | 0x40).astype(np.uint16), f32_to_bf16_bits(x))


def rbf(x):
    """fp32 -> fp32, rounded through bf16."""
    return bf2f(f2bf(x))


def bits_of(v):
    """fp64 holding bf16 values (2^128 and above: the rounding overflowed) -> bf16 bits."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(v, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def is_nan(bits):
    return (np.asarray(bits, np.uint16) & 0x7fff) > 0x7f80


def key(bits):
    """bf16 bits -> int32 in the order of the values, -0 below +0 (NaN patterns fall outside +-inf: test them with is_nan first)."""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff) - 1, b)


def same_bits(got, want):
    """Equal bit patterns; where the expected value is a NaN, any NaN."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    return (got == want) | (is_nan(got) & is_nan(want))


def bf16r(x):
    """bf16_rne with the overflow of the format: 2^128 (what the largest binade rounds up to) is +-inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = bf16_rne(x)
        return np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)


# ------------------------------------------------------------------------------------------------------------------------------------
# the interval rule
# ------------------------------------------------------------------------------------------------------------------------------------
def _round32(lo, hi):
    """ONE fp32 operation whose exact result lies in [lo, hi] (end points exact, signed zeros included): the interval of its rounded
    result.  _widen, and fp32's edges: an infinite end point stays; a result below 2^-126 is off by at most 2^-150 and does not cross
    zero; beyond FLT_MAX the result is +-inf (at or beyond FLT_MAX + 2^103 it must be)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        wl, wh = _widen(lo, hi)
        wl, wh = np.where(np.isinf(lo) | (lo == 0), lo, wl), np.where(np.isinf(hi) | (hi == 0), hi, wh)      # -0 + 0 would be +0
        tiny = 2.0 ** -150
        dl, dh = lo - tiny, hi + tiny
        wl = np.where((np.abs(lo) < 2.0 ** -126) & (lo != 0), np.where((lo > 0) & (dl <= 0), 0.0, dl), wl)
        wh = np.where((np.abs(hi) < 2.0 ** -126) & (hi != 0), np.where((hi < 0) & (dh >= 0), -0.0, dh), wh)
        top = FLT_MAX + 2.0 ** 103
        wh = np.where(wh > FLT_MAX, np.inf, wh)
        wl = np.where(wl < -FLT_MAX, -np.inf, wl)
        wl = np.where(lo >= top, np.inf, wl)
        wh = np.where(hi <= -top, -np.inf, wh)
    return wl, wh


def _ulp32(x):
    """The fp32 spacing at |x| (fp64, finite): 2^(e - 24) for |x| in [2^(e-1), 2^e), at least 2^-149."""
    x = np.abs(np.asarray(x, np.float64))
    ok = np.isfinite(x) & (x > 0)
    _, e = np.frexp(np.where(ok, x, 1.0))
    return np.where(ok, np.maximum(np.ldexp(1.0, e - 24), 2.0 ** -149), 2.0 ** -149)


def exp_interval(a, k=K_EXP):
    """expf(a) for exactly known a (fp64 holding fp32 values): exp(a) +- k ulps, not below 0, +inf beyond FLT_MAX."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        E = np.exp(np.asarray(a, np.float64))
        w = np.where(np.isfinite(E), k * _ulp32(E), 0.0)
        lo, hi = np.maximum(E - w, 0.0), E + w
        lo, hi = np.where(np.isnan(E), E, lo), np.where(np.isnan(E), E, hi)
        return np.where(lo > FLT_MAX, np.inf, lo), np.where(hi > FLT_MAX, np.inf, hi)


_erf = np.frompyfunc(math.erf, 1, 1)
_erfc = np.frompyfunc(math.erfc, 1, 1)


def erf64(a):
    return np.asarray(_erf(np.asarray(a, np.float64)), np.float64)


def erf_interval(a, k=K_ERF):
    """erff(a) for exactly known a: erf(a) +- k ulps; exactly +-1 where 1 - |erf(a)| < 2^-30."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        R = erf64(a)
        w = k * _ulp32(R)
        sat = np.asarray(_erfc(np.abs(a)), np.float64) < ERF_SATURATED
        one = np.copysign(1.0, a)
        return np.where(sat, one, R - w), np.where(sat, one, R + w)


def _sorted(a, b):
    """min / max of two end-point images (NaN stays NaN; a -0 / +0 pair is ordered -0 first)."""
    with np.errstate(invalid="ignore"):
        swap = (a > b) | ((a == 0) & (b == 0) & np.signbit(b) & ~np.signbit(a))
        return np.where(swap, b, a), np.where(swap, a, b)


def _sigmoid_denominator(a):
    """1 + expf(a): (lo, hi)."""
    elo, ehi = exp_interval(a)
    return _round32(1.0 + elo, 1.0 + ehi)


def silu_interval(g):
    """g (fp64 holding bf16 values) -> (lo, hi) of bf16(g / (1 + expf(-g))), fp64 holding bf16 values."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        qlo, qhi = _sigmoid_denominator(-g)
        lo, hi = _round32(*_sorted(g / qlo, g / qhi))
        return bf16r(lo), bf16r(hi)


def quick_gelu_interval(v):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        t = bf16r(f32(v * float(C_1702)))
        qlo, qhi = _sigmoid_denominator(-t)
        slo, shi = _round32(1.0 / qhi, 1.0 / qlo)
        slo, shi = bf16r(slo), bf16r(shi)
        # v and the end points of s are known bf16 values: their product is pushed through exactly (one fp32 rounding, which acts only
        # outside fp32's normal range), as the trunk model does after y0
        lo, hi = _sorted(f32(v * slo), f32(v * shi))
        return bf16r(lo), bf16r(hi)


def gelu_erf_interval(v):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        h = f32(v * 0.5)
        rlo, rhi = erf_interval(f32(v * float(C_RSQRT2)))
        plo, phi = _round32(1.0 + rlo, 1.0 + rhi)
        lo, hi = _round32(*_times(h, h, plo, phi))
        # _times takes min / max over products: where both are zeros of either sign, order them
        lo, hi = _sorted(lo, hi)
        return bf16r(lo), bf16r(hi)


# ------------------------------------------------------------------------------------------------------------------------------------
# the activation kernels restated (fp32 numpy: one IEEE operation each), with named defects
# ------------------------------------------------------------------------------------------------------------------------------------
def expf_central(a):
    """The correctly rounded expf: fp64 exp, one rounding."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(np.asarray(a, np.float32).astype(np.float64)).astype(np.float32)


def erff_central(a):
    return erf64(np.asarray(a, np.float32)).astype(np.float32)


_ONE = np.float32(1.0)
_ERR = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def quick_gelu(xb, defect=None, expf=expf_central):
    with np.errstate(**_ERR):
        v = bf2f(xb)
        t = v * (np.float32(1.7) if defect == "c1702_as_1p7" else C_1702)
        if defect != "t_not_rounded":
            t = rbf(t)
        s = _ONE / (_ONE + expf(-t))
        if defect != "s_not_rounded":
            s = rbf(s)
        return f2bf(v * s)


def silu(xb, defect=None, expf=expf_central):
    with np.errstate(**_ERR):
        g = bf2f(xb)
        if defect == "silu_sigmoid_rounded":
            return f2bf(g * rbf(_ONE / (_ONE + expf(-g))))
        return f2bf(g / (_ONE + expf(-g)))


def gelu_erf(xb, defect=None, erff=erff_central):
    with np.errstate(**_ERR):
        v = bf2f(xb)
        if defect == "tanh_form":
            u = np.float32(0.7978845608028654) * (v + np.float32(0.044715) * v * v * v)
            return f2bf(v * np.float32(0.5) * (_ONE + np.tanh(u.astype(np.float64)).astype(np.float32)))
        p = _ONE + erff(v * C_RSQRT2)
        if defect == "half_after_sum":
            return f2bf((v * p) * np.float32(0.5))
        return f2bf((v * np.float32(0.5)) * p)


def _first_pass(shape, items_per_row, cap):
    """[rows, cols] mask of what the first pass of a grid-stride loop writes: item i = (row i // items_per_row, 8 columns)."""
    rows, cols = shape
    assert cols == items_per_row * 8
    return (np.arange(rows * cols) < cap * 256 * 8).reshape(rows, cols)


def store_rows(buf, ld, dense, ld_ignored=False, written=None):
    """The strided store of `dense` [M, n] at row stride ld into a copy of the flat buffer `buf`; `written`: a mask of the same shape."""
    out = np.array(buf).reshape(-1)
    M, n = dense.shape
    stride = n if ld_ignored else ld
    for r in range(M):
        seg = out[r * stride:r * stride + n]
        if written is None:
            seg[:] = dense[r]
        else:
            seg[written[r]] = dense[r][written[r]]
    return out.reshape(np.shape(buf))


def _rows_of(flat, ld, M, n, col0=0):
    flat = np.asarray(flat).reshape(-1)
    return np.stack([flat[r * ld + col0:r * ld + col0 + n] for r in range(M)])


def geglu(x, ldx, y0, ldy, M, F, defect=None):
    """x flat [.. M rows of stride ldx ..] bits; returns y0 (flat, bits) after the call."""
    lin, gl = _rows_of(x, ldx, M, F), _rows_of(x, ldx, M, F, F)
    with np.errstate(**_ERR):
        dense = f2bf(bf2f(gl) * bf2f(lin))
    written = _first_pass(dense.shape, F // 8, CAP_2048) if defect == "second_pass_skipped" else None
    return store_rows(y0, ldy, dense, defect == "ldy_ignored", written)


def swiglu(x, ldx, y0, ldy, M, F, defect=None, expf=expf_central):
    gate, up = _rows_of(x, ldx, M, F), _rows_of(x, ldx, M, F, F)
    if defect == "halves_swapped":
        gate, up = up, gate
    with np.errstate(**_ERR):
        dense = f2bf(bf2f(silu(gate, defect, expf)) * bf2f(up))
    written = _first_pass(dense.shape, F // 8, CAP_2048) if defect == "second_pass_skipped" else None
    return store_rows(y0, ldy, dense, defect == "ldy_ignored", written)


def unary(name, xb, y0, defect=None):
    """quick_gelu / gelu_erf / silu on a flat array; y0 after the call (the first two cap the grid at 2048 blocks of one element per thread)."""
    fn = {"quick_gelu": quick_gelu, "gelu_erf": gelu_erf, "silu": silu}[name]
    out = np.array(y0)
    n = len(xb)
    m = min(n, CAP_2048 * 256) if defect == "second_pass_skipped" else n
    out[:m] = fn(xb, None if defect == "second_pass_skipped" else defect)[:m]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# tables over all 65 536 inputs, acceptance
# ------------------------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def unary_table(name):
    """{"lo", "hi": int32 keys of the interval's end points, "nan": the output is a NaN, "central": the bits of the restated kernel with the
    correctly rounded transcendental} over all 65 536 input patterns."""
    if name not in _TABLES:
        v = bf2d(ALL16)
        lo, hi = {"quick_gelu": quick_gelu_interval, "silu": silu_interval, "gelu_erf": gelu_erf_interval}[name](v)
        central = {"quick_gelu": quick_gelu, "silu": silu, "gelu_erf": gelu_erf}[name](ALL16)
        nan = np.isnan(lo) | np.isnan(hi)
        assert np.array_equal(np.isnan(lo), np.isnan(hi)) and np.array_equal(nan, is_nan(central)), name
        _TABLES[name] = dict(lo=key(bits_of(lo)), hi=key(bits_of(hi)), lo_bits=bits_of(lo), hi_bits=bits_of(hi), nan=nan, central=central)
    return _TABLES[name]


def unary_violations(name, xb, yb):
    """Elements of yb = kernel(xb) outside their interval (a NaN where none is due, no NaN where one is)."""
    t = unary_table(name)
    xb, yb = np.asarray(xb, np.uint16), np.asarray(yb, np.uint16)
    k, n = key(yb), is_nan(yb)
    due = t["nan"][xb]
    return (due != n) | (~due & ((k < t["lo"][xb]) | (k > t["hi"][xb])))


def swiglu_interval(gate, up):
    """(lo key, hi key, nan) of bf16(silu(gate) * up) for bit arrays of one shape: the silu table's end points through the exact product
    (a product of two bf16 values: one fp32 rounding where it leaves fp32's range, then the bf16 one)."""
    t = unary_table("silu")
    gate = np.asarray(gate, np.uint16)
    with np.errstate(**_ERR):
        a, b = f2bf(bf2f(t["lo_bits"][gate]) * bf2f(up)), f2bf(bf2f(t["hi_bits"][gate]) * bf2f(up))
    nan = is_nan(a) | is_nan(b)
    ka, kb = key(a), key(b)
    return np.minimum(ka, kb), np.maximum(ka, kb), nan, is_nan(a) != is_nan(b)


def swiglu_violations(gate, up, yb):
    lo, hi, nan, _ = swiglu_interval(gate, up)
    k, n = key(yb), is_nan(yb)
    return (nan != n) | (~nan & ((k < lo) | (k > hi)))


def swiglu_central(gate, up):
    with np.errstate(**_ERR):
        return f2bf(bf2f(unary_table("silu")["central"][np.asarray(gate, np.uint16)]) * bf2f(up))


def up_bits(v):
    return f2bf(np.float32(v).reshape(1))[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------------------------------------------
SPECIALS = (0x8000, 0x0002, 0x8040, 0x7f80, 0xff80)          # -0, a denormal (2^-132: half of it is no tie), a negative one, +inf, -inf


def seeded_bits(seed, shape, scale=3.0, specials=SPECIALS):
    """Normal values times `scale` as bf16 bits, with every pattern of `specials` at about 1 in 256 places each (seeded)."""
    rng = np.random.default_rng(seed)
    b = f2bf((scale * rng.standard_normal(shape)).astype(np.float32))
    flat = b.reshape(-1)
    for s in specials:
        flat[rng.integers(0, flat.size, size=max(1, flat.size // 256))] = s
    return b


def seeded_f32(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def f2bf_inputs():
    """The 393 216 fp32 patterns (b << 16) + {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff}, b over all 16-bit upper halves: exact, just above,
    just below the tie, the tie, just above it, just below the next value - inf, NaN and denormals included."""
    low = np.array([0, 1, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)
    return ((ALL16.astype(np.uint32)[:, None] << 16) + low[None, :]).reshape(-1).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------------
LN_PROBE_D = (1, 8, 63, 64, 255, 256, 257, 768, 1000, 1280)
LN_PROBE_M = (1, 5)
LN_RANDOM_D = (64, 768, 1000, 4096)
LN_RANDOM_M = (1, 67)


def layer_norm(x, ldx, gamma, beta, out0, ldo, M, d, eps, defect=None):
    """The kernel on flat fp64 buffers of bf16 values; the sums are taken in fp64 and rounded once (one conforming order; on the exact
    probes every order gives these bits).  Returns out0 after the call."""
    assert defect is None or defect in LN_DEFECTS
    X = _rows_of(np.asarray(x, np.float64), ldx, M, d)
    eps = float(np.float32(eps))
    with np.errstate(**_ERR):
        mean = f32(f32(X.sum(1)) / d)
        c = f32(X - mean[:, None])
        if defect == "mean_of_squares_minus_square":
            var = f32(f32(f32(f32(X * X).sum(1)) / d) - f32(mean * mean))
        else:
            var = f32(f32(f32(c * c).sum(1)) / (max(d - 1, 1) if defect == "variance_unbiased" else d))
        ve = var if defect == "eps_dropped" else f32(var + eps)
        rstd = f32(1.0 / f32(np.sqrt(ve)))
        y = f32(np.asarray(gamma, np.float64)[None] * f32(rstd[:, None] * c))
        if defect != "beta_dropped":
            y = f32(y + np.asarray(beta, np.float64)[None])
        y = bf16r(y)
    return store_rows(np.asarray(out0, np.float64), ldo, y, defect == "ldo_ignored")


def ln_interval(x, gamma, beta, eps=LN_EPS):
    """(lo, hi) [M, d], bf16 values: rstd * (x - mean) as the trunk model bounds it, times gamma and plus beta widened once each."""
    _, ylo, yhi = ln_y0_interval(x, eps)
    g, b = np.asarray(gamma, np.float64)[None], np.asarray(beta, np.float64)[None]
    plo, phi = _widen(*_times(ylo, yhi, g, g))
    lo, hi = _widen(plo + b, phi + b)
    return bf16_rne(lo), bf16_rne(hi)


def exact_in_any_order(v):
    """Every partial sum of v, in any order, is an integer below 2^24 times one power of two: exact in fp32."""
    v = np.asarray(v, np.float64)
    nz = np.abs(v[v != 0])
    if nz.size == 0:
        return True
    q = None
    for a in np.unique(nz):
        m, e = math.frexp(a)
        i = int(m * 2 ** 53)
        b = e - 53 + ((i & -i).bit_length() - 1)
        q = b if q is None else min(q, b)
    return float(nz.sum() / 2.0 ** q) < 2 ** 24


def _about(rng, d, centre, spread):
    """centre + a seeded arrangement of equally many +s and -s for each s of `spread` (the remainder of d stays at the centre)."""
    n = d // (2 * len(spread))
    v = np.zeros(d)
    k = 0
    for s in spread:
        v[k:k + n], v[k + n:k + 2 * n] = s, -s
        k += 2 * n
    return centre + rng.permutation(v)


LN_PROBE_ROWS = ("pm13", "offset", "constant", "offset192", "tiny")


def ln_probe_rows(rng, d):
    """[5, d].  Sum = d * centre and the sum of squared deviations are exact in any order; mean = centre exactly."""
    return np.stack([
        _about(rng, d, 0.0, (8.0, 24.0)),                      # {+-1, +-3} 2^3: var = 5 * 64 * (d - r) / d, rstd irrational
        _about(rng, d, 0.75, (0.25,)),                         # 1 / 0.5 about 0.75
        np.full(d, -1.5),                                      # constant: x - mean = 0, out = beta (gamma * +-0 + beta)
        _about(rng, d, 192.0, (1.0,)),                         # 191 / 193: the sum of squares would need 16 bits per term, the deviations 1
        _about(rng, d, 0.0, (2.0 ** -9,)),                     # var = 2^-18 (d - r) / d ~ eps / 2.6
    ])


class LnProbe:
    def __init__(self, d, M):
        rng = np.random.default_rng([20261021, d, M])
        rows = ln_probe_rows(rng, d)
        self.d, self.M, self.ldx, self.ldo, self.eps = d, M, d + 24, d + 40, LN_EPS
        self.name = f"d{d}_M{M}"
        self.X = rows if M == 5 else rows[(d % 2) * 3:(d % 2) * 3 + 1]           # M = 1: pm13 at even d, offset192 at odd d
        assert self.X.shape == (M, d)
        self.x = rng.integers(-9, 10, size=M * self.ldx).astype(np.float64)        # the pad columns of x hold values too
        for r in range(M):
            self.x[r * self.ldx:r * self.ldx + d] = self.X[r]
        self.gamma = bf16_rne(1.0 + 0.3 * rng.standard_normal(d))
        self.beta = bf16_rne(0.3 * rng.standard_normal(d))
        self.beta[::7] = 0.0
        self.out0 = rng.integers(100, 121, size=M * self.ldo).astype(np.float64)   # canary: no result reaches 100
        self.expected = self.run()

    def run(self, defect=None):
        return layer_norm(self.x, self.ldx, self.gamma, self.beta, self.out0, self.ldo, self.M, self.d, self.eps, defect)


def ln_probes():
    return [LnProbe(d, M) for d in LN_PROBE_D for M in LN_PROBE_M]


def ln_random_case(d, M, family):
    """Seeded random rows of one of the trunk model's families with fractional gamma / beta: (x [M, d], gamma, beta), bf16 values."""
    mean, std, _ = LN_FAMILIES[family]
    rng = np.random.default_rng([20261021, d, M, sorted(LN_FAMILIES).index(family)])
    x = bf16_rne(mean + std * rng.standard_normal((M, d)))
    # beta about 2: an output near 0 has a bf16 spacing below the width the summation order leaves, whatever the kernel - with beta about
    # 0 the centred rows alone exceed their 1 % cap (1.1 - 1.2 %), so the inputs moved, not the cap
    return x, bf16_rne(1.0 + 0.3 * rng.standard_normal(d)), bf16_rne(2.0 + 0.3 * rng.standard_normal(d))


def ln_random_grid():
    return [(d, M, fam) for fam in LN_FAMILIES for d in LN_RANDOM_D for M in LN_RANDOM_M]


# ------------------------------------------------------------------------------------------------------------------------------------
# the bit-exact kernels (fp32 numpy on bit patterns)
# ------------------------------------------------------------------------------------------------------------------------------------
def text_embed(ids, tok, pos, defect=None):
    """ids [L] int64, tok [vocab, d] bits, pos [>= L, d] bits or None -> [L, d] bits."""
    ids = np.asarray(ids, np.int64)
    vocab = tok.shape[0]
    ok = (ids >= 0) & (ids < vocab)
    out = tok[np.where(ok, ids, 0)]
    if pos is not None:
        with np.errstate(**_ERR):
            p = bf2f(pos[:len(ids)])
            out = f2bf(bf2f(out) + p)
            if defect == "pos_added_in_bf16_twice":
                out = f2bf(bf2f(out) + p)
    return np.where(ok[:, None], out, np.uint16(0))


def pooled_index(ids, eos, defect=None):
    v = np.asarray(ids, np.int64).astype(np.int32)                               # the kernel's (int) truncation
    if eos != 2:
        v = (v == np.int32(eos)).astype(np.int32)
    if defect == "tie_to_higher_index":
        return int(len(v) - 1 - np.argmax(v[::-1]))
    return int(np.argmax(v))                                                     # the first maximum; no hit: all zero -> 0


def text_pool_row(ids, eos, x, d, defect=None):
    """x [L, ldx] bits -> [d] bits."""
    return x[pooled_index(ids, eos, defect), :d].copy()


def mrope(x, cos, sin, Hq, Hkv, defect=None):
    """x [L, ld] bits, cos / sin [L, 128] bits -> x after the call."""
    L, heads = x.shape[0], Hq + Hkv
    out = np.array(x)
    X = bf2f(x[:, :heads * 128]).reshape(L, heads, 128)
    a, b = X[..., :64], X[..., 64:]
    c, s = bf2f(cos)[:, None, :], bf2f(sin)[:, None, :]
    R = (lambda t: t) if defect == "products_not_rounded" else rbf
    with np.errstate(**_ERR):
        if defect == "sin_sign_flipped":
            lo, hi = R(a * c[..., :64]) + R(b * s[..., :64]), R(b * c[..., 64:]) + R(-a * s[..., 64:])
        else:
            lo, hi = R(a * c[..., :64]) + R(-b * s[..., :64]), R(b * c[..., 64:]) + R(a * s[..., 64:])
        new = f2bf(np.concatenate([lo, hi], -1))
    if defect == "second_pass_skipped":                      # item = (row, head, 8 channels c and the 8 at c + 64)
        item = np.arange(L * heads)[:, None] * 8 + (np.arange(128)[None, :] % 64) // 8
        new = np.where((item < CAP_2048 * 256).reshape(L, heads, 128), new, x[:, :heads * 128].reshape(L, heads, 128))
    out[:, :heads * 128] = new.reshape(L, heads * 128)
    return out


def vision_rope(x, cos, sin, H, D, Dp, defect=None):
    """x [L, ld] bits, cos / sin [L, D] fp32 -> x after the call (q and k heads: 2 H heads of Dp columns)."""
    L, heads, half = x.shape[0], 2 * H, D // 2
    out = np.array(x)
    X = x[:, :heads * Dp].reshape(L, heads, Dp)
    hp = Dp // 2 if defect == "half_taken_from_Dp" else half
    A, B = bf2f(X[..., :half]), bf2f(X[..., hp:hp + half])
    c, s = np.asarray(cos, np.float32)[:, None, :], np.asarray(sin, np.float32)[:, None, :]
    R = rbf if defect == "products_rounded" else (lambda t: t)
    sg = np.float32(-1.0 if defect == "sin_sign_flipped" else 1.0)
    with np.errstate(**_ERR):
        lo = R(A * c[..., :half]) + R((-B * sg) * s[..., :half])
        hi = R(B * c[..., half:]) + R((A * sg) * s[..., half:])
    new = np.array(X)
    new[..., :half], new[..., hp:hp + half] = f2bf(lo), f2bf(hi)
    if defect == "second_pass_skipped":                      # item = (row, head, 4 channels c and the 4 at c + half)
        vph = half // 4
        item = np.full((L * heads, Dp), np.iinfo(np.int64).max)
        item[:, :D] = np.arange(L * heads)[:, None] * vph + (np.arange(D)[None, :] % half) // 4
        new = np.where((item < CAP_4096 * 256).reshape(L, heads, Dp), new, X)
    out[:, :heads * Dp] = new.reshape(L, heads * Dp)
    return out


def cast_pad_rows(x, K, Kp, defect=None):
    """x [M, >= K]: fp32 values or bf16 bits (uint16) -> [M, Kp] bits."""
    M = x.shape[0]
    y = np.zeros((M, Kp), np.uint16)
    y[:, :K] = x[:, :K] if x.dtype == np.uint16 else f2bf(x[:, :K])
    return y


def gate_resid_rows(p, gate, resid, N):
    """p [M, ldp], gate [N], resid [M, ldr] bits -> [M, N] bits."""
    with np.errstate(**_ERR):
        return f2bf(bf2f(resid[:, :N]) + rbf(bf2f(gate)[None, :] * bf2f(p[:, :N])))


def kv_append(qkv, cache, row0, Hq, Hkv):
    out = np.array(cache)
    out[row0:row0 + qkv.shape[0]] = qkv[:, Hq * 128:(Hq + 2 * Hkv) * 128]
    return out


def skip_second_pass(before, after, cap):
    """`after` [M, n] with everything past the first pass of a grid of `cap` blocks (one item = 8 columns, row-major) left as `before`."""
    return np.where(_first_pass(after.shape, after.shape[1] // 8, cap), after, before)


# the smallest shapes that pass each grid cap (items > cap * 256), and the smallest legal ones
SECOND_PASS = dict(
    glu=dict(M=513, F=8192), unary_n=CAP_2048 * 256 + 4097, mrope=dict(L=1025, Hq=56, Hkv=8), vision_rope=dict(L=4097, H=16, D=80, Dp=96),
    cast_pad_rows=dict(M=1025, K=8185, Kp=8192), gate_resid_rows=dict(M=1025, N=8192), kv_append=dict(L=2049, Hq=8, Hkv=8))
SMALLEST = dict(glu=dict(M=1, F=8), unary_n=1, mrope=dict(L=1, Hq=1, Hkv=1), vision_rope=dict(L=1, H=1, D=8, Dp=32),
                cast_pad_rows=dict(M=1, K=1, Kp=8), gate_resid_rows=dict(M=1, N=8), kv_append=dict(L=1, Hq=1, Hkv=1))


def items(kind, **s):
    """Work items of the kernel's grid-stride loop at a shape."""
    if kind == "glu":
        return s["M"] * (s["F"] // 8)
    if kind == "mrope":
        return s["L"] * (s["Hq"] + s["Hkv"]) * 8
    if kind == "vision_rope":
        return s["L"] * 2 * s["H"] * (s["D"] // 8)
    if kind == "cast_pad_rows":
        return s["M"] * (s["Kp"] // 8)
    if kind == "gate_resid_rows":
        return s["M"] * (s["N"] // 8)
    if kind == "kv_append":
        return s["L"] * (2 * s["Hkv"] * 128 // 8)
    raise KeyError(kind)


GRID_CAP = dict(glu=CAP_2048, mrope=CAP_2048, kv_append=CAP_2048, vision_rope=CAP_4096, cast_pad_rows=CAP_4096, gate_resid_rows=CAP_4096)
CANARY = 0x4e9a                                              # bf16 1.29e9: no result of a seeded case


# ------------------------------------------------------------------------------------------------------------------------------------
# the seeded cases of the GPU test (bit patterns; one extra row of canary behind every buffer a kernel writes)
# ------------------------------------------------------------------------------------------------------------------------------------
def glu_case(M, F, seed=1):
    """geglu / swiglu: x [M, 2 F + 8] (the pad columns hold values), y0 [M + 1, F + 8] canary."""
    return seeded_bits([seed, M, F], (M, 2 * F + 8)), np.full((M + 1, F + 8), CANARY, np.uint16)


def unary_case(n):
    """quick_gelu / gelu_erf / silu on n elements: x bits, y0 [n + 8] canary.  N(0, 1) values: at 3 N(0, 1) one input in nine would lie in
    the tail of 1 + erff, where the interval of gelu_erf holds several bf16 values, and the second pass would be checked loosely."""
    return seeded_bits([20, n], n, 1.0), np.full(n + 8, CANARY, np.uint16)


def swiglu_all_inputs():
    """One row per up value of SWIGLU_UPS, F = 65 536: every gate pattern against that up.  x [7, 2 F + 8], y0 [8, F + 8]."""
    F = 65536
    x = np.full((len(SWIGLU_UPS), 2 * F + 8), CANARY, np.uint16)
    for r, u in enumerate(SWIGLU_UPS):
        x[r, :F], x[r, F:2 * F] = ALL16, up_bits(u)
    return x, np.full((len(SWIGLU_UPS) + 1, F + 8), CANARY, np.uint16)


def _angle_tables(rng, L, n):
    ang = rng.uniform(0.0, 2 * np.pi, size=(L, n))           # unpaired columns: the kernels are linear in the tables
    return np.cos(ang).astype(np.float32), np.sin(rng.uniform(0.0, 2 * np.pi, size=(L, n))).astype(np.float32)


def mrope_case(L, Hq, Hkv):
    """x [L + 1, (Hq + 2 Hkv) 128 + 8] (row L: behind the rows the kernel is given), cos / sin [L, 128] bits."""
    rng = np.random.default_rng([2, L, Hq, Hkv])
    c, s = _angle_tables(rng, L, 128)
    return seeded_bits([3, L, Hq, Hkv], (L + 1, (Hq + 2 * Hkv) * 128 + 8), 2.0), f2bf(c), f2bf(s)


def vision_rope_case(L, H, D, Dp):
    """x [L + 1, 3 H Dp + 8] bits, cos / sin [L, D] fp32."""
    rng = np.random.default_rng([4, L, H, D])
    c, s = _angle_tables(rng, L, D)
    return seeded_bits([5, L, H, D], (L + 1, 3 * H * Dp + 8), 2.0), c, s


def cast_pad_case(M, K, Kp):
    """x fp32 [M, K + 3] (values with low bits set; the same specials as fp32), its bf16 form [M, K + 3], y0 [M + 1, Kp] canary."""
    xb = seeded_bits([6, M, K], (M, K + 3))
    low = np.random.default_rng([7, M, K]).integers(0, 1 << 16, size=xb.shape, dtype=np.uint32)
    x32 = ((xb.astype(np.uint32) << 16) | np.where(is_nan(xb) | ((xb & 0x7fff) == 0x7f80), 0, low)).view(np.float32)
    return x32, xb, np.full((M + 1, Kp), CANARY, np.uint16)


def gate_resid_case(M, N):
    """p [M, N + 8], gate [N], resid [M, N + 16], y0 [M + 1, N + 24] canary."""
    return (seeded_bits([8, M, N], (M, N + 8)), seeded_bits([9, M, N], (N,), 1.0), seeded_bits([10, M, N], (M, N + 16)),
            np.full((M + 1, N + 24), CANARY, np.uint16))


def kv_append_case(L, Hq, Hkv):
    """qkv [L, (Hq + 2 Hkv) 128 + 8], cache0 [3 + L + 2, 2 Hkv 128] canary, row0 = 3."""
    return seeded_bits([11, L, Hq, Hkv], (L, (Hq + 2 * Hkv) * 128 + 8)), np.full((3 + L + 2, 2 * Hkv * 128), CANARY, np.uint16), 3


EMBED_D = (8, 2048 + 8)                                      # one vector per thread; a second pass of the block's 256 x 8 columns
EMBED_VOCAB = 37


def embed_ids():
    return [-1, EMBED_VOCAB, EMBED_VOCAB - 1, 1 << 40, 0]


def embed_case(d):
    """tok [vocab, d], pos [1, d] bits."""
    return seeded_bits([12, d], (EMBED_VOCAB, d)), seeded_bits([13, d], (1, d))


POOL_L = (1, 256, 257, 600)


def pool_cases(L):
    """(name, ids [L] int64, eos): all-equal ids; the maximum in the last element; the maximum at index 256 (the first element of a
    thread's second pass) with an equal one later; an eos that never occurs; a first hit among several; ids that differ above bit 31."""
    rng = np.random.default_rng([14, L])
    base = rng.integers(3, 290, size=L).astype(np.int64)
    out = [("all_equal", np.full(L, 7, np.int64), 2), ("all_equal_eos", np.full(L, 7, np.int64), 7)]
    last = base.copy()
    last[-1] = 300
    out += [("max_last", last, 2), ("eos_last", last, 300), ("eos_never", base, 5000)]
    if L > 256:
        at = base.copy()
        at[256] = 300
        at[min(L - 1, 300)] = 300 if L > 300 else at[min(L - 1, 300)]
        out += [("max_at_256", at, 2), ("eos_at_256", at, 300)]
    if L > 2:
        two = base.copy()
        two[L // 2], two[L // 3] = 299, 299
        high = base.copy()
        high[0] = (1 << 32) + 1                                 # int32: 1, below every other id
        out += [("first_of_two", two, 2), ("first_hit_of_two", two, 299), ("truncated_to_int32", high, 2)]
    return out
