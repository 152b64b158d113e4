"""CPU model of rgn_lora_merge_bf16 (include/regione_hip.h, csrc/lora.hip): the fp64 reference, the derived element-wise bound, the kernel's
arithmetic contract restated in numpy with NAMED DEFECTS, and the exact probes the GPU test runs.  Test infrastructure only.

Contract, per element (n, k):   t = f32(W[n, k]);  for each term in order: acc = 0; for r ascending: acc = fmaf(B[n, r], A[r, k], acc);
                                t = fmaf(scale, acc, t);   dst[n, k] = bf16_rne(t).

Bound.  Every fmaf rounds once to fp32 (unit roundoff u32 = 2^-24).  A term's chain makes r roundings on partial sums bounded by
sum_r |B||A|, its `t = fmaf(scale, acc, t)` one more on a value bounded by |W| + sum over the terms so far: to first order the fp32 value t
differs from the exact W + sum_t s_t (B_t A_t) by at most
        e[n, k] = u32 * (r_total + n_terms + 1) * (|W| + sum_t |s_t| * sum_r |B_t||A_t|)
(r_total = sum of the ranks; the `+ 1` pays for the second-order terms: (1 + u)^(r + n) - 1 <= (r + n + 1) u for (r + n) u < 0.01, and
r_total <= 8 * 1024 keeps it below 5e-4).  The one rounding to bf16 is monotone, hence the acceptance rule
        bf16_rne(ref - e) <= out <= bf16_rne(ref + e).

The model evaluates each fmaf as fp32(fp64(b) * fp64(a) + fp64(acc)): the product is exact in fp64, the sum is rounded to fp64 and then to
fp32 - a double rounding that can differ from a true fma in the last fp32 bit in rare ties-after-rounding cases, far inside e; on the exact
probes (every product and partial sum exact in fp32) there is no rounding at all before the final bf16 one, which is exact too.
"""
import numpy as np

U32 = 2.0 ** -24
DEFECTS = ("delta_rounded_to_bf16", "scale_applied_to_w", "terms_beyond_first_dropped", "b_read_transposed", "ldd_ignored",
           "last_partial_row_tile_skipped")
ROW_TILE = 64                # the kernel's row tile (csrc/lora.hip LM_TN): what "last partial row tile" means


def bf16_rne(x):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64.  Exact: 8 significant bits, subnormal quantum 2^-133."""
    x = np.asarray(x, dtype=np.float64)
    m, e = np.frexp(x)
    e = np.maximum(e, -125)
    return np.ldexp(np.rint(np.ldexp(x, 8 - e)), e - 8)


def reference(W, terms):
    """fp64: W + sum_t s_t * B_t @ A_t."""
    ref = np.asarray(W, dtype=np.float64).copy()
    for A, B, s in terms:
        ref += float(s) * (np.asarray(B, np.float64) @ np.asarray(A, np.float64))
    return ref


def bound(W, terms):
    mag = np.abs(np.asarray(W, np.float64))
    for A, B, s in terms:
        mag = mag + abs(float(s)) * (np.abs(np.asarray(B, np.float64)) @ np.abs(np.asarray(A, np.float64)))
    r_total = sum(A.shape[0] for A, _, _ in terms)
    return U32 * (r_total + len(terms) + 1) * mag


def accepted(out, W, terms):
    """Element-wise acceptance of `out` (bf16 values as floats) - the boolean array."""
    ref, e = reference(W, terms), bound(W, terms)
    out = np.asarray(out, np.float64)
    return (bf16_rne(ref - e) <= out) & (out <= bf16_rne(ref + e))


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def merge(dst, ldd, W, ldw, N, K, terms, defect=None):
    """The kernel on flat buffers: `dst` (fp64 array holding bf16 values, len >= (N - 1) * ldd + K) is overwritten where the kernel writes
    and returned; W flat with row stride ldw; terms = [(A [r, K], B [N, r], scale)].  `defect`: None or one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    dst = np.array(dst, dtype=np.float64)
    Wf = np.asarray(W, np.float64)
    rows = np.arange(N)
    t = np.stack([Wf[n * ldw:n * ldw + K] for n in rows]).astype(np.float32) if N else np.zeros((0, K), np.float32)
    use = terms[:1] if defect == "terms_beyond_first_dropped" else terms
    for A, B, s in use:
        A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
        R = A.shape[0]
        if defect == "b_read_transposed":
            B = B.reshape(-1)[(np.arange(R)[None, :] * N + rows[:, None])]                # B[n, r] read at r * N + n
        acc = np.zeros((N, K), np.float32)
        for r in range(R):
            acc = _f32(B[:, r:r + 1].astype(np.float64) * A[r:r + 1, :].astype(np.float64) + acc.astype(np.float64))
        s32 = np.float32(s).astype(np.float64)
        if defect == "delta_rounded_to_bf16":
            t = _f32(bf16_rne(_f32(s32 * acc.astype(np.float64)).astype(np.float64)) + t.astype(np.float64))
        elif defect == "scale_applied_to_w":
            t = _f32(s32 * (acc.astype(np.float64) + t.astype(np.float64)))
        else:
            t = _f32(s32 * acc.astype(np.float64) + t.astype(np.float64))
    out = bf16_rne(t.astype(np.float64))
    stride = K if defect == "ldd_ignored" else ldd
    n_written = N // ROW_TILE * ROW_TILE if defect == "last_partial_row_tile_skipped" else N
    for n in range(n_written):
        dst[n * stride:n * stride + K] = out[n]
    return dst


class Probe:
    """One exact case: flat buffers and the expectation.  `expected` is the whole destination buffer (canaries included)."""

    def __init__(self, name, N, K, ldw, ldd, W, dst, terms):
        self.name, self.N, self.K, self.ldw, self.ldd, self.W, self.dst, self.terms = name, N, K, ldw, ldd, W, dst, terms
        self.expected = merge(dst, ldd, W, ldw, N, K, terms)

    def w_rows(self):
        return np.stack([self.W[n * self.ldw:n * self.ldw + self.K] for n in range(self.N)])


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def _probe(name, rng, N, K, ldw, ldd, ranks, scales):
    """Small integers times powers of two: every product, partial sum and the result is exact, and the result is a bf16 value.  The result Y
    is drawn first (|Y| <= 60) and W = Y - delta (|delta| <= 50, a multiple of 1/2, so |W| < 128 has at most 8 significant bits)."""
    terms = [(_ints(rng, (r, K), -2, 2), _ints(rng, (N, r), -2, 2), s) for r, s in zip(ranks, scales)]
    assert sum(abs(s) * 4 * r for r, s in zip(ranks, scales)) <= 50
    Y = _ints(rng, (N, K), -60, 60)
    Wm = Y - (reference(np.zeros((N, K)), terms))
    W = _ints(rng, ((N - 1) * ldw + K,), -9, 9)                 # the pad columns of W hold values too (never read into the result)
    dst = _ints(rng, ((N - 1) * ldd + K,), 100, 120)           # canary: no result is in [100, 120]
    for n in range(N):
        W[n * ldw:n * ldw + K] = Wm[n]
    return Probe(name, N, K, ldw, ldd, W, dst, terms)


def probes():
    rng = np.random.default_rng(20261019)
    out = [
        # two terms of different rank, a partial row tile (67 = 64 + 3), a partial column tile (72), strides > K on both sides
        _probe("two_terms_strided", rng, 67, 72, 80, 88, (3, 5), (0.5, -2.0)),
        # more than one column tile (520 = 2 * 256 + 8), more than one rank chunk (r = 20 > 16), dense
        _probe("wide_deep", rng, 5, 520, 520, 520, (20,), (0.5,)),
        _probe("single_row", rng, 1, 8, 8, 8, (1,), (-2.0,)),
    ]
    # the delta alone is NOT a bf16 value (257 = 16 * 16 + 1 * 1 needs 9 bits) while W + delta is: rounding the delta first gives 1, not 2
    N, K = 5, 16
    A = np.stack([np.full(K, 16.0), np.ones(K)])
    B = np.tile(np.array([[16.0, 1.0]]), (N, 1))
    out.append(Probe("delta_needs_nine_bits", N, K, K, K, np.full(N * K, -255.0), np.full(N * K, 100.0), [(A, B, 1.0)]))
    return out
