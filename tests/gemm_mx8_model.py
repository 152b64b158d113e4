"""The specification of "mx8 rows" (include/regione_hip.h) in numpy: OCP e4m3fn bytes with one E8M0 scale byte per 32 consecutive values,
and the quantiser that writes them (regione_amd/csrc/norm.hip: rgn_quantize_rows_mx8).  No torch, no GPU import: bf16 values travel as
their uint16 bit patterns, every value is handled in float64, where all of this arithmetic is exact.

  E4M3                the 256 e4m3fn codes as float64 (NaN at 0x7f / 0xff);
  e4m3fn_rne          float64 (|y| <= 448) -> code, round to nearest even, subnormals kept, the sign of zero kept;
  scale_byte          amax (as float32 bits) -> E8M0 byte b: 2^(b - 127) is the smallest power of two X with amax / X <= 448, from the bits
                      of amax; b clamped to [0, 254]; a block of zeros gets 127;
  quantize_rows       bf16 bits [M, K] -> (codes uint8 [M, K], scales uint8 [M, K / 32]), with the named defects of MUTANTS;
  dequantize          the values an mx8 consumer multiplies with, float64 [M, K];
  linear              what a GEMM on mx8 rows computes before its epilogue, in float64: dequantize(q, s) @ (W8 * wscale)^T + bias;
  pool / rows         the blocks of 32 the quantiser is probed with, and [M, K] inputs cut from them.
tests/test_gemm_mx8_model.py pins the model to the definition (and to torch's e4m3fn conversion) and shows that every mutant changes a
probe output; tests/test_gpu_quantize_rows_mx8.py compares the kernel with it bit for bit.
"""
import numpy as np

BLK = 32                                        # values per scale byte
KT = 128                                        # K tile: four blocks, one aligned dword of scales per row
MUTANTS = ("e8m0_bias_minus_1", "e8m0_bias_plus_1", "floor_exponent", "zero_block_0", "zero_block_255", "amax_16", "amax_64")


def _e4m3_table():
    c = np.arange(256)
    e, m = (c >> 3) & 15, (c & 7).astype(np.float64)
    v = np.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e.astype(np.float64) - 7))
    v = np.where(c & 0x80, -v, v)
    v[(c & 0x7f) == 0x7f] = np.nan
    return v


E4M3 = _e4m3_table()
_POS = E4M3[:0x7f]                              # the 127 finite non-negative values, ascending: the code IS the index


def bf16_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f32_to_bf16_bits(x):
    """float32 -> bf16 bits, round to nearest even (finite input)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def e4m3fn_rne(y):
    """float64, |y| <= 448 -> e4m3fn code.  The grid step at |y| in [2^e, 2^(e+1)) is 2^(e-3), below 2^-6 it is 2^-9; np.rint rounds
    halves to even, and a value that rounds up to the next binade lands on that binade's first value."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert np.all(a <= 448.0), "the quantiser never hands a value above 448 to the convert"
    _, ex = np.frexp(a)                                          # a = f 2^ex, f in [0.5, 1): a in [2^(ex-1), 2^ex)
    step = np.exp2(np.maximum(ex - 1, -6).astype(np.float64) - 3)
    r = np.rint(a / step) * step
    code = np.searchsorted(_POS, r)
    assert np.array_equal(_POS[code], r)
    return (code | (np.signbit(y).astype(np.int64) << 7)).astype(np.uint8)


def scale_byte(amax_bits, mutant=None):
    """float32 bits of a non-negative amax -> E8M0 byte.  amax = m 2^(E-127), m in [1, 2): amax / 2^t <= 448 = 1.75 * 2^8 first holds at
    t = E - 135 if m <= 1.75, at t = E - 134 if not; b = t + 127."""
    u = np.asarray(amax_bits, dtype=np.int64)
    E, man = u >> 23, u & 0x7fffff
    b = E - 8 + (0 if mutant == "floor_exponent" else (man > 0x600000))
    b += {"e8m0_bias_minus_1": -1, "e8m0_bias_plus_1": 1}.get(mutant, 0)
    b = np.clip(b, 0, 254)
    return np.where(u == 0, {"zero_block_0": 0, "zero_block_255": 255}.get(mutant, 127), b).astype(np.uint8)


def quantize_rows(x_bits, mutant=None):
    """bf16 bits [M, K], K % 128 == 0, finite -> (codes uint8 [M, K], scales uint8 [M, K / 32])."""
    x_bits = np.asarray(x_bits, dtype=np.uint16)
    M, K = x_bits.shape
    assert K % KT == 0
    x = bf16_to_f64(x_bits)
    span = {"amax_16": 16, "amax_64": 64}.get(mutant, BLK)
    amax = np.abs(x).reshape(M, K // span, span).max(axis=2)
    amax = np.repeat(amax, span // BLK, axis=1) if span >= BLK else amax[:, ::BLK // span]      # amax_16: the block's first half only
    s = scale_byte(amax.astype(np.float32).view(np.uint32), mutant)
    y = x * np.exp2(127.0 - np.repeat(s, BLK, axis=1).astype(np.float64))
    if mutant is not None:
        y = np.clip(y, -448.0, 448.0)           # a defective scale can leave values above 448: what a saturating convert makes of them
    return e4m3fn_rne(y), s


def dequantize(q, s):
    """float64 [M, K]: value(q[m, k]) 2^(s[m, k / 32] - 127)."""
    return E4M3[np.asarray(q, dtype=np.uint8)] * np.exp2(np.repeat(np.asarray(s, dtype=np.uint8), BLK, axis=1).astype(np.float64) - 127.0)


def linear(q, s, w_codes, wscale, bias=None):
    """float64 [M, N]: the pre-epilogue result of a GEMM that reads mx8 rows and fp8 weights with per-channel scales - no row scale."""
    out = dequantize(q, s) @ (E4M3[np.asarray(w_codes, dtype=np.uint8)] * np.asarray(wscale, dtype=np.float64)[:, None]).T
    return out if bias is None else out + np.asarray(bias, dtype=np.float64)[None, :]


# ---- probe inputs ---------------------------------------------------------------------------------------------------------------------
SLOTS = (0, BLK - 1, 13)                        # where a block's amax sits: first, last, a middle slot


def _block(amax_bits, slot, rng, negative=False):
    """A block whose amax is the bf16 `amax_bits` at `slot`; the other values are random fractions of it (bf16, so some equal it in
    magnitude, many are subnormal results), with random signs."""
    a = bf16_to_f64(amax_bits)
    v = a * rng.uniform(0, 1, BLK) * np.exp2(-rng.integers(0, 12, BLK).astype(np.float64))
    b = f32_to_bf16_bits(v.astype(np.float32))
    b = np.minimum(b, np.uint16(amax_bits))                      # rounding to bf16 must not pass the amax
    b = b | (rng.integers(0, 2, BLK).astype(np.uint16) << 15)
    b[slot] = np.uint16(amax_bits) | (0x8000 if negative else 0)
    return b


def pool():
    """name -> list of blocks (uint16 [32]) the quantiser must get right bit for bit."""
    rng = np.random.default_rng(2025)
    fam = {}
    # every finite bf16 exponent field as block amax, subnormals (E = 0) included, at the mantissas around the 1.75 threshold
    # (0x60 = 1.75 exactly, 0x61 the first above it) and at both ends
    ex, i = [], 0
    for E in range(255):
        for man in (0x00, 0x60, 0x61, 0x7f):
            bits = (E << 7) | man
            if bits == 0:
                bits = 0x0001                                    # the smallest subnormal instead of zero
            ex.append(_block(bits, SLOTS[i % 3], rng, negative=bool((i // 3) & 1)))
            i += 1
    fam["exponents"] = ex
    z, nz = np.zeros(BLK, np.uint16), np.full(BLK, 0x8000, np.uint16)
    mixed = np.where(np.arange(BLK) % 3 == 0, 0x8000, 0).astype(np.uint16)
    fam["zeros"] = [z, nz, mixed]
    # values that round UP to 448, the largest e4m3fn value: 432 is the tie between 416 and 448 (448 is the even one), 440 and 446 lie
    # above it; amax 446 (m < 1.75) keeps X = 1, amax 450 (m > 1.75) takes X = 2 and lands on 224 (225 rounds down)
    up = []
    for amax, others in ((448.0, (432.0, 440.0, -432.0, -446.0, 430.0)), (446.0, (432.0, -440.0, 446.0)), (450.0, (-450.0, 448.0, 432.0)),
                         (446.0 * 2.0 ** -40, (432.0 * 2.0 ** -40, -440.0 * 2.0 ** -40)), (448.0 * 2.0 ** 90, (-432.0 * 2.0 ** 90, 440.0 * 2.0 ** 90))):
        for slot in SLOTS:
            v = np.zeros(BLK)
            free = [k for k in range(BLK) if k != slot]
            for j, o in enumerate(others):
                v[free[(7 * j + 3) % len(free)]] = o
            v[slot] = amax
            b = f32_to_bf16_bits(v.astype(np.float32))
            assert np.array_equal(bf16_to_f64(b), v), "the probe values are bf16 values"
            up.append(b)
    fam["round_up_to_448"] = up
    # amax = 448 (X = 1): every midpoint between neighbouring e4m3fn values, both signs, and the bf16 neighbours of each midpoint
    mids = (_POS[:-1] + _POS[1:]) / 2
    ties = np.concatenate([mids, -mids, mids * (1 + 2.0 ** -7), -mids * (1 - 2.0 ** -7)])
    tb = f32_to_bf16_bits(ties.astype(np.float32))
    tie_blocks = []
    for j in range(0, len(tb), BLK - 1):
        part = tb[j:j + BLK - 1]
        b = np.zeros(BLK, np.uint16)
        slot = SLOTS[(j // (BLK - 1)) % 3]
        b[[k for k in range(BLK) if k != slot][:len(part)]] = part
        b[slot] = f32_to_bf16_bits(np.float32(448.0))
        tie_blocks.append(b)
    fam["ties"] = tie_blocks
    # ordinary data at three magnitudes, and an outlier channel: one value 2^10 above its neighbours
    rnd = []
    for mag in (2.0 ** -20, 1.0, 2.0 ** 20):
        for _ in range(8):
            rnd.append(f32_to_bf16_bits((rng.standard_normal(BLK) * mag).astype(np.float32)))
    out = rng.standard_normal(BLK)
    out[21] = 1024.0
    rnd.append(f32_to_bf16_bits(out.astype(np.float32)))
    fam["randn"] = rnd
    return fam


def rows(M, K, offset=0):
    """bf16 bits [M, K] cut from the pool's blocks, in order from block `offset`, cyclically: neighbouring blocks of a row (and the same
    block column of neighbouring rows) differ in magnitude by orders, so a scale taken from a neighbour shows."""
    blocks = np.stack([b for f in pool().values() for b in f])
    n = M * (K // BLK)
    idx = (offset + np.arange(n)) % len(blocks)
    return blocks[idx].reshape(M, K)


def pool_size():
    return sum(len(f) for f in pool().values())


# the launches of tests/test_gpu_quantize_rows_mx8.py: (M, K, first pool block).  [130, 1024] holds the whole pool (two passes of 512
# columns per row, 33 workgroups); [63, 384] a ragged last pass (384 = 3 K tiles: the last group of 16 lanes idle) and a ragged last
# workgroup; [1, 128] one row, one K tile - cut from the pool where the zero blocks sit
SHAPES = ((130, 1024, 0), (63, 384, 1000), (1, 128, 1017))
