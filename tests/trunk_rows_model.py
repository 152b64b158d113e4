"""CPU model of the MMDiT trunk's row kernels (csrc/norm.hip; the fused Q/K/V epilogue of csrc/gemm.hip): the contracts, an element-wise
fp64 INTERVAL that every conforming implementation must land in, the kernels' arithmetic restated in numpy with NAMED DEFECTS, the exact
probes and the seeded random cases the GPU test runs.  Test infrastructure only (numpy, fp64).

Contracts (the comments of norm.hip, restated)
----------------------------------------------
AdaLN (rgn_ln_modulate, rgn_ln_modulate_segs), per row of d values, fp32 arithmetic, the two sums in an UNSPECIFIED order:
    mean = (sum x) / d;   var = (sum (x - mean)^2) / d   (two passes, biased);   rstd = 1 / sqrt(var + eps)
    y0 = bf16((x - mean) * rstd);   s1 = bf16(1 + scale);   y1 = bf16(y0 * s1);   out = bf16(y1 + shift)
  Row r uses the modulation vectors of segment #{i : r >= end[i]} (i over all but the last segment).  The `_a8` forms are
  rgn_quantize_rows_a8 of that bf16 row (tests/gemm_a8_model.py: quantize_rows).
Q/K (rgn_qk_norm_rope_store, RGN_EPI_QKV), per row m and head h of 128 values:
    r = 1 / sqrt((sum x^2) / 128 + eps);   n = bf16(bf16(x * r) * w),   w = w0 for m < split_row, else w1
    out[2i]   = bf16(n[2i]   * cos[t, 2i]   - n[2i+1] * sin[t, 2i])
    out[2i+1] = bf16(n[2i+1] * cos[t, 2i+1] + n[2i]   * sin[t, 2i+1])       each product and the sum rounded to fp32 separately (no fma)
  Q: t = m, the Q tables, written in place.  K: t = kr = kv_rows[m] (or m), the K tables, written to k_slab[kr, h * 128 + .].
V:  vt_slab[h * 128 + dd, kvpos(kr)] = V[m, h * 128 + dd], kvpos swapping bits 2 and 3 of the row: a pure copy.  Nothing else in the
  slabs or in the K / V columns of the rows changes.
Summation order: ANY order in which no input passes through more than CHAIN = 80 dependent fp32 additions (a contract of this model, not
  a fit: 80 covers a lane's 64 sequential adds + a 6-step butterfly + 4 partials with room; a sequential sum over 8192 does NOT conform).
Division and sqrtf are the correctly rounded IEEE forms (hipcc's default: common.h, norm.hip).

Acceptance rule: an interval, carried through every rounding
-----------------------------------------------------------
u = 2^-24 is the unit roundoff of fp32.  A sum of values v_i in such an order is S^ = sum v_i (1 + t_i), |t_i| <= (1 + u)^CHAIN - 1 <=
(CHAIN + 1) u  (CHAIN u < 0.01; the `+ 1` pays the second-order terms), hence  |S^ - S| <= (CHAIN + 1) u sum |v_i|.  Every other fp32
operation (a subtraction, a product, a division, sqrtf) returns its exact result times (1 + t), |t| <= u.  The model evaluates the chain
in fp64 on INTERVALS [lo, hi] (fp64's own roundoff, 2^-53, is 2^-29 of u and ignored):
    sum        [S - (CHAIN + 1) u sum|v|, S + (CHAIN + 1) u sum|v|]; for the sum of squares the terms are non-negative intervals
               [qlo_i, qhi_i] themselves rounded once (the product; a fused multiply-add rounds less): [(1 - (CHAIN + 2) u) sum qlo,
               (1 + (CHAIN + 2) u) sum qhi]
    f(lo, hi)  a monotone operation maps end points to end points (x - mean: the mean's end points swapped; 1 / .: swapped; a product
               with a signed factor: min / max over the end-point products), then WIDENS: lo - u |lo|, hi + u |hi|
    bf16(.)    rounding to nearest even is monotone: [bf16(lo), bf16(hi)]
  After y0 (after n for Q/K) the AdaLN chain has no further freedom: 1 + scale, y0 * s1 (16 significant bits) and y1 + shift are single
  IEEE operations on known values, evaluated exactly as fp32 then bf16 - the end points are simply pushed through.  The Q/K rotation
  widens once per product and once for the sum.  Acceptance, element-wise:  lo <= out <= hi.
No tolerance here was tuned on GPU output.  The bound stays honest through a CAP on the share of elements whose interval holds more than
one bf16 value (AMBIGUITY_CAP), asserted by tests/test_trunk_rows_model.py on the very inputs the GPU test uses.

Exact probes: inputs whose sums are exact in fp32 in ANY order (small integers times a power of two), so that every conforming
implementation computes the same fp32 bits; the one inexact stage (x - mean) * rstd, resp. x * r, sits >= 16 interval half-widths from
the nearest bf16 tie (margin checked on the CPU).  The GPU test compares bits.
"""
import numpy as np

U32 = 2.0 ** -24
CHAIN = 80
LN_WAVE_D = (512, 1024, 1536, 2048, 3072, 4096)          # ln_modulate_wave_kernel<1, 2, 3, 4, 6, 8>
LN_BLOCK_D = (8, 256, 520, 2560, 4808, 8192)             # ln_modulate_kernel: 1 partial / 1 / 1 / 2 / 3 (last partial) / 4 passes of 2048
D_ALL = LN_BLOCK_D + LN_WAVE_D
LN_RANDOM_M = (1, 5, 67)
LN_FAMILIES = {"centred": (0.3, 2.0, 8), "offset": (8.0, 1.0, 256)}          # mean, std, smallest d the family is drawn at
AMBIGUITY_CAP = {"centred": 0.01, "offset": 0.05, "qk": 0.02}
MARGIN = 16.0
LN_DEFECTS = ("y0_not_rounded", "one_plus_scale_not_rounded", "y1_not_rounded", "variance_unbiased", "eps_dropped", "segment_end_inclusive",
              "chunk_modulation_offset_dropped", "last_pass_skipped", "ldo_ignored")
QK_DEFECTS = ("rms_over_row", "norm_not_rounded_before_weight", "odd_lane_uses_even_table_entry", "sin_sign_flipped", "k_rotated_with_row_m",
              "k_stored_at_row_m", "split_row_inclusive", "fused_multiply_add", "vt_kvpos_identity", "vt_tail_rows_written")
EPS = float(np.float32(1e-6))                              # the fp32 value the C ABI receives for eps = 1e-6


def bf16_rne(x):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64.  Exact: 8 significant bits, subnormal quantum 2^-133."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    e = np.maximum(e, -125)
    return np.ldexp(np.rint(np.ldexp(x, 8 - e)), e - 8)


def f32(x):
    """fp64 -> the nearest fp32 value, as fp64 (one IEEE rounding)."""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def bf16_tie_distance(x):
    """Distance of x to the nearest point at which bf16 rounding changes its result (the midpoints of neighbouring bf16 values)."""
    x = np.abs(np.asarray(x, np.float64))
    m, e = np.frexp(np.where(x == 0, 1.0, x))
    q = np.ldexp(1.0, e - 8)                                # the bf16 spacing of x's binade [2^(e-1), 2^e)
    t = x / q
    own = np.abs(t - np.floor(t) - 0.5) * q
    below = x - (np.ldexp(1.0, e - 1) - q / 4)             # the last tie of the binade below (half the spacing there)
    return np.where(x == 0, np.inf, np.minimum(own, below))


def kvpos(r):
    r = np.asarray(r, np.int64)
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


def padded(n, m=64):
    return (n + m - 1) // m * m


def _widen(lo, hi, k=1.0):
    return lo - k * U32 * np.abs(lo), hi + k * U32 * np.abs(hi)


def _times(lo, hi, flo, fhi):
    """[lo, hi] * [flo, fhi]: min / max over the end-point products."""
    p = np.stack(np.broadcast_arrays(lo * flo, lo * fhi, hi * flo, hi * fhi))
    return p.min(0), p.max(0)


def _rstd_interval(qlo, qhi, n, eps):
    """1 / sqrt(q / n + eps) for a sum interval: a division, an addition, sqrtf and a division, each widened once."""
    vlo, vhi = _widen(qlo / n, qhi / n)
    vlo, vhi = _widen(vlo + eps, vhi + eps)
    tlo, thi = _widen(np.sqrt(vlo), np.sqrt(vhi))
    return _widen(1.0 / thi, 1.0 / tlo)


# ------------------------------------------------------------------------------------------------------------------------------------
# AdaLN
# ------------------------------------------------------------------------------------------------------------------------------------
def ln_segment_of_rows(M, seg_end, inclusive=False):
    """The segment of every row: #{i : r >= end[i]} over all ends but the last (`inclusive`: the defect that counts r > end[i])."""
    r = np.arange(M)[None, :]
    ends = np.asarray(seg_end[:-1], np.int64).reshape(-1, 1)
    return ((r > ends) if inclusive else (r >= ends)).sum(0)


def _ln_tail(y0, scale, shift, defect=None):
    """Everything after y0, exactly: single IEEE operations on known values."""
    s1 = f32(1.0 + scale)
    if defect != "one_plus_scale_not_rounded":
        s1 = bf16_rne(s1)
    y1 = f32(y0 * s1)
    if defect != "y1_not_rounded":
        y1 = bf16_rne(y1)
    return bf16_rne(f32(y1 + shift))


def ln_y0_interval(x, eps=EPS):
    """x [M, d] (bf16 values) -> (ref, lo, hi) of (x - mean) * rstd BEFORE its rounding to bf16: the fp64 value and the interval."""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    eps = float(np.float32(eps))
    s, sa = x.sum(1), np.abs(x).sum(1)
    k = (CHAIN + 1) * U32
    mlo, mhi = _widen((s - k * sa) / d, (s + k * sa) / d)
    clo, chi = _widen(x - mhi[:, None], x - mlo[:, None])
    sq_lo = np.where((clo <= 0) & (chi >= 0), 0.0, np.minimum(clo * clo, chi * chi))
    sq_hi = np.maximum(clo * clo, chi * chi)
    k2 = (CHAIN + 2) * U32
    rlo, rhi = _rstd_interval(sq_lo.sum(1) * (1 - k2), sq_hi.sum(1) * (1 + k2), d, eps)
    ylo, yhi = _widen(*_times(clo, chi, rlo[:, None], rhi[:, None]))
    mean = s / d
    ref = (x - mean[:, None]) / np.sqrt(((x - mean[:, None]) ** 2).sum(1) / d + eps)[:, None]
    return ref, ylo, yhi


def ln_interval(x, seg_end, shift, scale, eps=EPS):
    """(lo, hi) [M, d] of the bf16 output; shift / scale: one [d] vector per segment."""
    _, ylo, yhi = ln_y0_interval(x, eps)
    seg = ln_segment_of_rows(x.shape[0], seg_end)
    sh, sc = np.stack(shift)[seg], np.stack(scale)[seg]
    a, b = _ln_tail(bf16_rne(ylo), sc, sh), _ln_tail(bf16_rne(yhi), sc, sh)
    return np.minimum(a, b), np.maximum(a, b)


def ln_modulate(x, ldx, out, ldo, M, d, eps, seg_end, shift, scale, defect=None):
    """The kernel on flat buffers (fp64 arrays of bf16 values): `out` is overwritten where the kernel writes and returned.  The sums
    are taken in fp64 and rounded once - one conforming order; on the exact probes every order gives these bits."""
    assert defect is None or defect in LN_DEFECTS
    out = np.array(out, np.float64)
    x = np.asarray(x, np.float64)
    X = np.stack([x[r * ldx:r * ldx + d] for r in range(M)])
    eps = float(np.float32(eps))
    mean = f32(f32(X.sum(1)) / d)
    c = f32(X - mean[:, None])
    var = f32(f32(f32(c * c).sum(1)) / (d - 1 if defect == "variance_unbiased" else d))
    ve = var if defect == "eps_dropped" else f32(var + eps)
    rstd = f32(1.0 / f32(np.sqrt(ve)))
    y0 = f32(c * rstd[:, None])
    if defect != "y0_not_rounded":
        y0 = bf16_rne(y0)
    seg = ln_segment_of_rows(M, seg_end, inclusive=defect == "segment_end_inclusive")
    sh, sc = np.stack(shift)[seg], np.stack(scale)[seg]
    pw = 512 if d in LN_WAVE_D else 2048                      # columns per pass: the wave kernel's, the block kernel's
    npass = (d + pw - 1) // pw
    if defect == "chunk_modulation_offset_dropped":
        col = np.arange(d) % pw
        sh, sc = sh[:, col], sc[:, col]
    y = _ln_tail(y0, sc, sh, defect)
    ncol = (npass - 1) * pw if defect == "last_pass_skipped" and npass > 1 else d
    stride = d if defect == "ldo_ignored" else ldo
    for r in range(M):
        out[r * stride:r * stride + ncol] = y[r, :ncol]
    return out


def _bf_ints(rng, n, lo, hi, q):
    return rng.integers(lo, hi + 1, size=n).astype(np.float64) * q


def ln_modulation(rng, nseg, d):
    """Per segment: shift = multiples of 2^-6 in [-4, 4], scale = ODD multiples of 2^-10 in (-1/4, 1/4): 1 + scale needs more than 8 bits
    and is never a bf16 tie (in units of 2^-10 the ties of [3/4, 1) are = 2 mod 4, those of [1, 5/4) = 4 mod 8: all even).  Independent
    draws: the vectors differ between 8-column groups, passes and segments."""
    shift = [_bf_ints(rng, d, -256, 256, 2.0 ** -6) for _ in range(nseg)]
    scale = [(2 * rng.integers(-127, 127, size=d) + 1).astype(np.float64) * 2.0 ** -10 for _ in range(nseg)]
    return shift, scale


def _balanced(rng, d, values):
    v = np.repeat(np.asarray(values, np.float64), d // len(values))
    return rng.permutation(v)


LN_PROBE_M = 7                                               # not a multiple of the wave kernel's 4 rows per block; two blocks


def ln_probe_rows(rng, d):
    """[7, d]: every sum of these rows and of their squared deviations is exact in fp32 in any order (integers below 2^24 times 2^k)."""
    return np.stack([
        _balanced(rng, d, (-4.0, 4.0)),                                    # +-2^k in equal counts
        3.0 * 2.0 ** -2 + _balanced(rng, d, (-0.25, 0.25)),                # c +- 2^k, d c exact: mean = c
        _balanced(rng, d, (-1.0, 1.0, -3.0, 3.0)) * 2.0 ** 3,              # {+-1, +-3} 2^k: var = 5 4^k, rstd irrational
        _balanced(rng, d, (-2.0 ** -10, 2.0 ** -10)),                      # var = 2^-20 ~ eps
        _balanced(rng, d, (-2.0 ** 5, 2.0 ** 5)),
        -3.0 * 2.0 ** 4 + _balanced(rng, d, (-16.0, 16.0)),
        _balanced(rng, d, (-1.0, 1.0, -3.0, 3.0)) * 2.0 ** -3,
    ])


class LnProbe:
    """One exact case.  `api`: "plain" (ops.ln_modulate), "split" (its split_row form: two segments) or "segs" (ops.ln_modulate_segs)."""

    def __init__(self, name, api, d, ldx, ldo, x, out0, eps, seg_end, shift, scale):
        self.name, self.api, self.M, self.d, self.ldx, self.ldo, self.x, self.out0 = name, api, LN_PROBE_M, d, ldx, ldo, x, out0
        self.eps, self.seg_end, self.shift, self.scale = eps, list(seg_end), shift, scale
        self.expected = self.run()

    def run(self, defect=None):
        return ln_modulate(self.x, self.ldx, self.out0, self.ldo, self.M, self.d, self.eps, self.seg_end, self.shift, self.scale, defect)

    def rows(self):
        return np.stack([self.x[r * self.ldx:r * self.ldx + self.d] for r in range(self.M)])


def ln_probes(d):
    """The probes of width d: plain; split_row at 1 and at M - 1; 1 to 4 segments (ends at rows 1 and M - 1); four segments with
    eps = 0.  Strided (ldx = d + 8, ldo = d + 16) with canaries, except the dense "segs2"."""
    M = LN_PROBE_M
    rng = np.random.default_rng(20261020 + d)
    X = ln_probe_rows(rng, d)
    out = []
    for name, api, seg_end, eps, dense in (("plain", "plain", (M,), EPS, False), ("split_1", "split", (1, M), EPS, False),
                                           ("split_M-1", "split", (M - 1, M), EPS, False), ("segs1", "segs", (M,), EPS, False),
                                           ("segs2", "segs", (M - 1, M), EPS, True), ("segs3", "segs", (1, M - 1, M), EPS, False),
                                           ("segs4", "segs", (1, 3, M - 1, M), EPS, False), ("segs4_eps0", "segs", (1, 3, M - 1, M), 0.0, False)):
        ldx, ldo = (d, d) if dense else (d + 8, d + 16)
        x = _bf_ints(rng, (M - 1) * ldx + d, -9, 9, 1.0)                   # the pad columns of x hold values too
        for r in range(M):
            x[r * ldx:r * ldx + d] = X[r]
        out0 = _bf_ints(rng, (M - 1) * ldo + d, 100, 120, 1.0)             # canary: no result reaches 100 (|y1| < 2, |shift| <= 4)
        shift, scale = ln_modulation(rng, len(seg_end), d)
        out.append(LnProbe(f"{name}_d{d}", api, d, ldx, ldo, x, out0, eps, seg_end, shift, scale))
    return out


def ln_random_segments(M):
    """Four segments over M rows (empty ones at M = 1)."""
    return [M // 5, M // 2, min(M // 2 + 1, M), M]


def ln_random_case(d, M, family):
    """Seeded random rows of one family, four segments with distinct vectors: (x [M, d], seg_end, shift, scale), bf16 values."""
    mean, std, _ = LN_FAMILIES[family]
    rng = np.random.default_rng([d, M, sorted(LN_FAMILIES).index(family)])
    x = bf16_rne(mean + std * rng.standard_normal((M, d)))
    shift = [bf16_rne(0.5 * rng.standard_normal(d)) for _ in range(4)]
    scale = [bf16_rne(0.5 * rng.standard_normal(d)) for _ in range(4)]
    return x, ln_random_segments(M), shift, scale


def ln_random_grid():
    return [(d, M, fam) for fam, (_, _, dmin) in LN_FAMILIES.items() for d in D_ALL if d >= dmin for M in LN_RANDOM_M]


# ------------------------------------------------------------------------------------------------------------------------------------
# Q/K RMSNorm + RoPE + K / V^T store
# ------------------------------------------------------------------------------------------------------------------------------------
def _row_weights(M, split_row, w0, w1, inclusive=False):
    m = np.arange(M)
    first = (m <= split_row) if (inclusive and split_row > 0) else (m < split_row)
    return np.where(first[:, None], np.asarray(w0 if w0 is not None else w1, np.float64)[None], np.asarray(w1, np.float64)[None])


def qk_n_interval(X, eps=EPS):
    """X [M, H, 128] -> (ref, lo, hi) of x * r BEFORE its rounding to bf16."""
    X = np.asarray(X, np.float64)
    eps = float(np.float32(eps))
    ss = (X * X).sum(-1)                                       # a square of a bf16 value is exact in fp32; the pair sums round
    k = (CHAIN + 1) * U32
    rlo, rhi = _rstd_interval(ss * (1 - k), ss * (1 + k), 128.0, eps)
    lo, hi = _widen(*_times(X, X, rlo[..., None], rhi[..., None]))
    return X / np.sqrt(ss / 128.0 + eps)[..., None], lo, hi


def qk_interval(X, w, cos, sin, eps=EPS):
    """(lo, hi) [M, H, 128] of the rotated bf16 output: X [M, H, 128], w [M, 128] the row's weight, cos / sin [M, 128] the row's table rows."""
    _, lo, hi = qk_n_interval(X, eps)
    w = np.asarray(w, np.float64)[:, None, :]
    a, b = bf16_rne(f32(bf16_rne(lo) * w)), bf16_rne(f32(bf16_rne(hi) * w))
    nlo, nhi = np.minimum(a, b), np.maximum(a, b)
    c, s = np.asarray(cos, np.float64)[:, None, :], np.asarray(sin, np.float64)[:, None, :]
    elo, ehi, olo, ohi = nlo[..., 0::2], nhi[..., 0::2], nlo[..., 1::2], nhi[..., 1::2]

    def rot(p, q):                                             # two widened products, a widened sum
        lo_ = _widen(*p)[0] + _widen(*q)[0]
        hi_ = _widen(*p)[1] + _widen(*q)[1]
        return _widen(lo_, hi_)
    l0, h0 = rot(_times(elo, ehi, c[..., 0::2], c[..., 0::2]), _times(olo, ohi, -s[..., 0::2], -s[..., 0::2]))
    l1, h1 = rot(_times(olo, ohi, c[..., 1::2], c[..., 1::2]), _times(elo, ehi, s[..., 1::2], s[..., 1::2]))
    lo, hi = np.empty_like(nlo), np.empty_like(nhi)
    lo[..., 0::2], lo[..., 1::2], hi[..., 0::2], hi[..., 1::2] = bf16_rne(l0), bf16_rne(l1), bf16_rne(h0), bf16_rne(h1)
    return lo, hi


def _norm(X, w, eps, defect=None):
    """n = bf16(bf16(x * r) * w) of X [M, H, 128] with the rows' weights w [M, 128]."""
    M, H, _ = X.shape
    ss = f32((X * X).sum(-1, keepdims=True))
    if defect == "rms_over_row":
        ss = f32((X * X).sum((1, 2), keepdims=True) / H) * np.ones((M, H, 1))
    r = f32(1.0 / f32(np.sqrt(f32(f32(ss / 128.0) + eps))))
    n = f32(X * r)
    if defect != "norm_not_rounded_before_weight":
        n = bf16_rne(n)
    return bf16_rne(f32(n * w[:, None, :]))


def _norm_rope(X, w, cos, sin, eps, defect):
    """X [M, H, 128], w / cos / sin [M, 128] -> rotated bf16 values, the kernel's fp32 operations one by one."""
    n = _norm(X, w, eps, defect)
    a, b = n[..., 0::2], n[..., 1::2]
    c, s = cos[:, None, :], sin[:, None, :]
    ce, se = c[..., 0::2], s[..., 0::2]
    co, so = (ce, se) if defect == "odd_lane_uses_even_table_entry" else (c[..., 1::2], s[..., 1::2])
    sg = -1.0 if defect == "sin_sign_flipped" else 1.0
    if defect == "fused_multiply_add":                         # a * c exact in fp64 (8 + 24 bits), one rounding of the sum
        o0, o1 = f32(a * ce + f32(-sg * b * se)), f32(b * co + f32(sg * a * so))
    else:
        o0, o1 = f32(f32(a * ce) + f32(-sg * b * se)), f32(f32(b * co) + f32(sg * a * so))
    out = np.empty_like(n)
    out[..., 0::2], out[..., 1::2] = bf16_rne(o0), bf16_rne(o1)
    return out


def qk_store(qkv, k_col, v_col, q_col, M, H, split_row, wq0, wk0, wq1, wk1, eps, cos_q, sin_q, cos_k, sin_k, kv_rows, k_slab, vt_slab,
             defect=None):
    """rgn_qk_norm_rope_store on arrays of bf16 values: qkv [M, ld], k_slab [skv_pad, H * 128], vt_slab [H * 128, skv_pad]; returns the
    three after the call (copies)."""
    assert defect is None or defect in QK_DEFECTS
    qkv, k_slab, vt_slab = np.array(qkv, np.float64), np.array(k_slab, np.float64), np.array(vt_slab, np.float64)
    HD, skv_pad = H * 128, k_slab.shape[0]
    eps = float(np.float32(eps))
    kr = np.arange(M) if kv_rows is None else np.asarray(kv_rows, np.int64)[:M]
    incl = defect == "split_row_inclusive"
    wq, wk = _row_weights(M, split_row, wq0, wq1, incl), _row_weights(M, split_row, wk0, wk1, incl)
    cos_q, sin_q, cos_k, sin_k = (np.asarray(t, np.float64) for t in (cos_q, sin_q, cos_k, sin_k))
    Q = qkv[:, q_col:q_col + HD].reshape(M, H, 128)
    K = qkv[:, k_col:k_col + HD].reshape(M, H, 128)
    V = qkv[:, v_col:v_col + HD].copy()
    tk = np.arange(M) if defect == "k_rotated_with_row_m" else kr
    qo = _norm_rope(Q, wq, cos_q[:M], sin_q[:M], eps, defect)
    ko = _norm_rope(K, wk, cos_k[tk], sin_k[tk], eps, defect)
    qkv[:, q_col:q_col + HD] = qo.reshape(M, HD)
    k_slab[np.arange(M) if defect == "k_stored_at_row_m" else kr] = ko.reshape(M, HD)
    vt_slab[:, kr if defect == "vt_kvpos_identity" else kvpos(kr)] = V.T
    if defect == "vt_tail_rows_written":                       # the clamped tail loads of the last 64-row block, stored at their own rows
        for m in range(M, min(padded(M), skv_pad)):
            vt_slab[:, kvpos(m)] = V[M - 1]
    return qkv, k_slab, vt_slab


QK_PROBE_M = (1, 63, 64, 65, 130)
QK_PROBE_H = (1, 3)


class QkProbe:
    def __init__(self, name, M, H, layout, split_row, w, eps, rope_q, rope_k, kv_rows, skv, qkv0, k0, vt0):
        self.name, self.M, self.H, self.split_row, self.eps, self.kv_rows, self.skv = name, M, H, split_row, eps, kv_rows, skv
        self.k_col, self.v_col, self.q_col, self.ld = layout
        self.wq0, self.wk0, self.wq1, self.wk1 = w
        self.rope_q, self.rope_k = rope_q, rope_k                # (cos, sin) each, fp32 values
        self.qkv0, self.k0, self.vt0 = qkv0, k0, vt0
        self.expected = self.run()

    def run(self, defect=None):
        return qk_store(self.qkv0, self.k_col, self.v_col, self.q_col, self.M, self.H, self.split_row, self.wq0, self.wk0, self.wq1,
                        self.wk1, self.eps, self.rope_q[0], self.rope_q[1], self.rope_k[0], self.rope_k[1], self.kv_rows, self.k0, self.vt0,
                        defect)

    def heads(self, col):
        return self.qkv0[:, col:col + self.H * 128].reshape(self.M, self.H, 128)


def _qk_heads(rng, M, H):
    """Heads whose sum of squares is exact in any order: +-2^k with a per-(row, head) k - a whole-row RMS differs from the per-head one
    wherever a row's heads differ in k - alternating with {+-1, +-3} 2^k heads (sum = 640 * 4^k: x * r is irrational)."""
    X = np.empty((M, H, 128))
    for m in range(M):
        for h in range(H):
            k = 2.0 ** int(rng.integers(-3, 4))
            X[m, h] = _balanced(rng, 128, (-1.0, 1.0)) * k if (m + h) % 2 == 0 else _balanced(rng, 128, (-1.0, 1.0, -3.0, 3.0)) * k
    return X


def _dyadic_table(rng, rows):
    """UNPAIRED dyadic cos / sin stand-ins: independent multiples of 1/8 in [-2, 2] per column (not unit-norm: the kernel is linear in them);
    every product with an 8-bit n and the sum of two are exact in fp32."""
    return _bf_ints(rng, (rows, 128), -16, 16, 0.125), _bf_ints(rng, (rows, 128), -16, 16, 0.125)


def _qk_weights(rng):
    """Multiples of 1/16 in [3/4, 5/4], different per stream and per column."""
    return tuple(_bf_ints(rng, 128, 12, 20, 2.0 ** -4) for _ in range(4))


def _qk_buffers(rng, M, H, ld, skv_pad):
    """Prefill patterns, all non-zero: integers in [100, 120] (no result reaches 100)."""
    return (_bf_ints(rng, (M, ld), 100, 120, 1.0), _bf_ints(rng, (skv_pad, H * 128), 100, 120, 1.0), _bf_ints(rng, (H * 128, skv_pad), 100, 120, 1.0))


def qk_layout(H, standard=False):
    """(k_col, v_col, q_col, ld): the trunk's [K | V | Q] packing, or the three blocks moved and separated by pad columns."""
    D = H * 128
    return (0, D, 2 * D, 3 * D) if standard else (D + 16, 8, 2 * D + 32, 3 * D + 48)


def qk_probe(M, H, gathered, split="none", standard=False, seed=0):
    """`split`: "none" (split_row = 0), "1" or "M-1"; `standard`: the column layout and split_row = 0 the fused epilogue supports."""
    rng = np.random.default_rng([20261020, M, H, int(gathered), seed])
    layout = qk_layout(H, standard)
    D = H * 128
    skv = 2 * M + 5 if gathered else M
    kv_rows = rng.permutation(skv)[:M].astype(np.int64) if gathered else None          # non-monotone, entries >= M among them
    skv_pad = padded(skv + 1)                                  # at least one row in [skv, skv_pad)
    split_row = {"none": 0, "1": 1, "M-1": M - 1}[split]
    w = _qk_weights(rng)
    if split_row <= 0:
        split_row, w = 0, (None, None, w[2], w[3])
    qkv0, k0, vt0 = _qk_buffers(rng, M, H, layout[3], skv_pad)
    for col in layout[:3]:
        qkv0[:, col:col + D] = _qk_heads(rng, M, H).reshape(M, D)
    return QkProbe(f"M{M}_H{H}_{'gather' if gathered else 'identity'}_split{split}", M, H, layout, split_row, w, EPS,
                   _dyadic_table(rng, M), _dyadic_table(rng, skv), kv_rows, skv, qkv0, k0, vt0)


def qk_probes(H):
    out = []
    for M in QK_PROBE_M:
        for gathered in (False, True):
            out.append(qk_probe(M, H, gathered, "none"))
            if M > 2:
                out.append(qk_probe(M, H, gathered, "1" if gathered else "M-1"))
    return out


def qk_fma_probe(H=2, M=6, standard=False):
    """Separate roundings versus one fma: every n is 1.25 (x = +2^k, w = 1.25), the tables hold 1 + j 2^-23 (j odd) against +-1, so one
    product is 1.25 + 1.25 j 2^-23 - inexact in fp32 - and the other cancels its leading 1.25.  Two roundings leave round(1.25 j) 2^-23, a
    fused multiply-add 1.25 j 2^-23 (5 j < 256: a bf16 value): different bf16 results in every element.  Even rows put the inexact
    product first, odd rows second (a compiler may fuse either)."""
    rng = np.random.default_rng([20261020, 99, H])
    layout = qk_layout(H, standard)
    D, skv = H * 128, M
    skv_pad = padded(skv + 1)
    qkv0, k0, vt0 = _qk_buffers(rng, M, H, layout[3], skv_pad)
    qkv0[:, layout[1]:layout[1] + D] = _qk_heads(rng, M, H).reshape(M, D)
    for col in (layout[0], layout[2]):
        k = 2.0 ** rng.integers(-2, 3, size=(M, H, 1)).astype(np.float64)
        qkv0[:, col:col + D] = np.broadcast_to(k, (M, H, 128)).reshape(M, D)
    w125 = np.full(128, 1.25)

    def table():
        # out[2i] = n c0 - n s0, out[2i+1] = n c1 + n s1.  Even rows: c = big, s0 = 1, s1 = -1.  Odd rows: c0 = 1, c1 = -1, s = big.
        j = (2 * rng.integers(0, 25, size=(M, 128)) + 1).astype(np.float64)          # odd, 5 j < 256
        big = 1.0 + j * 2.0 ** -23
        alt = np.where(np.arange(128) % 2 == 0, 1.0, -1.0)[None]
        first = (np.arange(M) % 2 == 0)[:, None]
        return np.where(first, big, alt), np.where(first, alt, big)
    rq, rk = table(), table()
    return QkProbe(f"fma_H{H}", M, H, layout, 0, (None, None, w125, w125), EPS, rq, rk, None, skv, qkv0, k0, vt0)


QK_RANDOM = dict(M=130, H=2, seed=7)


def qk_random_ids():
    """Synthetic position ids [rows, 3] for the Q rows and for the cache rows: a text prefix at (0, 0, 0), then a 16-wide image grid;
    the cache's grid starts elsewhere, so the K tables differ from the Q tables."""
    M, skv = QK_RANDOM["M"], 2 * QK_RANDOM["M"] + 5

    def ids(rows, y0, x0):
        r = np.maximum(np.arange(rows) - 47, 0)
        img = (np.arange(rows) >= 47)
        return np.stack([np.zeros(rows), img * (y0 + r // 16), img * (x0 + r % 16)], 1)
    return ids(M, 0, 0), ids(skv, 3, 5)


def qk_random_case(rope_q=None, rope_k=None):
    """Random normal heads, weights 1 +- 0.1, gathered rows, split_row; tables: angles uniform in [0, 2 pi) for Q and - other ones - for
    K, or the caller's ((cos, sin) of M rows, (cos, sin) of 2 M + 5 rows: the oracle's flux_pos_embed of qk_random_ids()).
    Returns a QkProbe-shaped case whose `expected` is one conforming result; the GPU test applies qk_accept."""
    M, H = QK_RANDOM["M"], QK_RANDOM["H"]
    rng = np.random.default_rng(QK_RANDOM["seed"])
    layout = qk_layout(H)
    D, skv = H * 128, 2 * M + 5
    skv_pad = padded(skv + 1)
    kv_rows = rng.permutation(skv)[:M].astype(np.int64)
    qkv0, k0, vt0 = _qk_buffers(rng, M, H, layout[3], skv_pad)
    for col in layout[:3]:
        qkv0[:, col:col + D] = bf16_rne(rng.standard_normal((M, D)) * 2.0 ** rng.integers(-2, 3, size=(M, 1)))
    w = tuple(bf16_rne(1.0 + 0.1 * rng.standard_normal(128)) for _ in range(4))

    def table(rows):
        ang = np.repeat(rng.uniform(0.0, 2 * np.pi, size=(rows, 64)), 2, axis=1)
        return f32(np.cos(ang)), f32(np.sin(ang))
    tq, tk = table(M), table(skv)
    if rope_q is not None:
        tq, tk = tuple(f32(t) for t in rope_q), tuple(f32(t) for t in rope_k)
        assert tq[0].shape == (M, 128) and tk[0].shape == (skv, 128)
    return QkProbe("random", M, H, layout, 47, w, EPS, tq, tk, kv_rows, skv, qkv0, k0, vt0)


def qk_case_intervals(p):
    """(qlo, qhi, klo, khi) [M, H * 128] of a case: Q in place, K as stored at rows kv_rows."""
    M, D = p.M, p.H * 128
    kr = np.arange(M) if p.kv_rows is None else p.kv_rows[:M]
    wq, wk = _row_weights(M, p.split_row, p.wq0, p.wq1), _row_weights(M, p.split_row, p.wk0, p.wk1)
    qlo, qhi = qk_interval(p.heads(p.q_col), wq, p.rope_q[0][:M], p.rope_q[1][:M], p.eps)
    klo, khi = qk_interval(p.heads(p.k_col), wk, p.rope_k[0][kr], p.rope_k[1][kr], p.eps)
    return qlo.reshape(M, D), qhi.reshape(M, D), klo.reshape(M, D), khi.reshape(M, D)


def qk_accept(p, qkv, k_slab, vt_slab):
    """Everything the call may change lies in its interval, everything else - V^T included: a copy - equals the restated kernel's result
    (= the prefill outside the written places).  Returns the number of violations."""
    M, D = p.M, p.H * 128
    kr = np.arange(M) if p.kv_rows is None else p.kv_rows[:M]
    qlo, qhi, klo, khi = qk_case_intervals(p)
    eq, ek, ev = p.expected
    bad = 0
    q, k = qkv[:, p.q_col:p.q_col + D], k_slab[kr]
    bad += int(((q < qlo) | (q > qhi)).sum()) + int(((k < klo) | (k > khi)).sum())
    qkv, k_slab, eq, ek = qkv.copy(), k_slab.copy(), eq.copy(), ek.copy()
    qkv[:, p.q_col:p.q_col + D] = eq[:, p.q_col:p.q_col + D] = 0
    k_slab[kr] = ek[kr] = 0
    return bad + int((qkv != eq).sum()) + int((k_slab != ek).sum()) + int((vt_slab != ev).sum())
