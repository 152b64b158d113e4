"""The numpy specification of mx8 rows (tests/gemm_mx8_model.py) against the definition it restates, against torch's e4m3fn conversion, and
against its own named defects: each mutant of the quantiser changes at least one byte of what the probe inputs produce, so a kernel with
that defect cannot pass tests/test_gpu_quantize_rows_mx8.py."""
import numpy as np
import pytest
import torch

import gemm_mx8_model as X


def test_the_code_table_is_torchs():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.isnan(X.E4M3), np.isnan(want)) and np.array_equal(X.E4M3[~np.isnan(want)], want[~np.isnan(want)])
    assert int(np.isnan(X.E4M3).sum()) == 2 and np.nanmax(X.E4M3) == 448.0


def test_the_rounding_is_torchs_on_every_probe_value_and_every_tie():
    fin = np.sort(np.unique(X.E4M3[~np.isnan(X.E4M3)]))
    mids = (fin[:-1] + fin[1:]) / 2
    rng = np.random.default_rng(1)
    y = np.concatenate([fin, mids, mids * (1 + 2.0 ** -20), mids * (1 - 2.0 ** -20), rng.uniform(-448, 448, 4096),
                        rng.uniform(-1, 1, 4096) * 2.0 ** -7, [0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 2.0 ** -11, 448.0, -448.0]])
    y = y.astype(np.float32).astype(np.float64)                  # torch converts from fp32: hand both the same values
    want = torch.from_numpy(y).float().to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(X.e4m3fn_rne(y), want)
    assert X.e4m3fn_rne(np.array([-0.0]))[0] == 0x80 and X.e4m3fn_rne(np.array([432.0]))[0] == 0x7e      # the tie below 448 goes UP (even)


def test_the_scale_is_the_smallest_power_of_two_that_does_not_clip_for_every_bf16_amax():
    bits = np.arange(1, 0x7f80, dtype=np.uint16)                 # every finite positive bf16
    a = X.bf16_to_f64(bits)
    b = X.scale_byte(bits.astype(np.uint32) << 16).astype(np.int64)
    assert b.min() == 0 and b.max() == 247                       # 255 never, and the upper clamp of the format is out of reach
    scale = np.exp2(b - 127.0)
    assert np.all(a / scale <= 448.0)
    assert np.all((a / (scale / 2) > 448.0) | (b == 0))          # one step smaller would clip, except at the clamp
    assert np.all(a[b == 0] <= 448.0 * 2.0 ** -127)
    assert X.scale_byte(np.array([0], dtype=np.uint32))[0] == 127


@pytest.fixture(scope="module")
def probe():
    x = X.rows(130, 1024)
    return x, X.quantize_rows(x)


def test_the_probe_rows_hold_the_whole_pool_and_every_family_is_what_its_name_says(probe):
    x, (q, s) = probe
    fam = X.pool()
    assert X.pool_size() <= 130 * 1024 // X.BLK
    amax = np.abs(X.bf16_to_f64(np.stack(fam["exponents"]))).max(axis=1)
    seen = set((amax.astype(np.float32).view(np.uint32) >> 23).tolist())
    assert seen == set(range(255))                               # every finite exponent field, 0 (subnormals) included
    held = [[k for k in X.SLOTS if abs(X.bf16_to_f64(b)[k]) == np.abs(X.bf16_to_f64(b)).max()] for b in fam["round_up_to_448"]]
    assert all(len(h) == 1 for h in held) and {h[0] for h in held} == set(X.SLOTS)
    up = X.quantize_rows(np.concatenate(fam["round_up_to_448"][:4]).reshape(1, 128))[0]
    assert (up & 0x7f).max() == 0x7e                             # 448, reached by rounding - and nothing beyond it
    assert np.all((q & 0x7f) != 0x7f) and np.all(s != 255)       # no NaN code, no NaN scale, for finite input


def test_zero_blocks_and_the_sign_of_zero():
    z = np.zeros((1, 128), np.uint16)
    z[0, 32:64] = 0x8000
    z[0, 64:96] = np.where(np.arange(32) % 3 == 0, 0x8000, 0)
    z[0, 96:128] = X.pool()["randn"][9]
    q, s = X.quantize_rows(z)
    assert s[0, :3].tolist() == [127, 127, 127] and np.all(q[0, :32] == 0) and np.all(q[0, 32:64] == 0x80)
    assert np.array_equal(q[0, 64:96], z[0, 64:96] >> 8)


def test_the_reconstruction_error_is_that_of_three_mantissa_bits(probe):
    x, (q, s) = probe
    v, d = X.bf16_to_f64(x), X.dequantize(q, s)
    scale = np.exp2(np.repeat(s, X.BLK, axis=1).astype(np.float64) - 127.0)
    # normal results: half a step of 2^-3 relative; subnormal results: half of 2^-9 X absolute
    assert np.all(np.abs(d - v) <= np.maximum(2.0 ** -4 * np.abs(v), 2.0 ** -10 * scale))
    assert np.all(np.abs(d) <= 448.0 * scale)
    # the block's amax lands in [224, 448] X (amax / X > 224, or X / 2 would have done) wherever the lower clamp is not active
    top = np.abs(d / scale).reshape(130, -1, X.BLK).max(axis=2)
    nonzero = np.abs(v).reshape(130, -1, X.BLK).max(axis=2) > 0
    assert np.all(top[nonzero & (s > 0)] >= 224.0)


def test_linear_is_the_product_of_the_dequantised_operands():
    rng = np.random.default_rng(3)
    q, s = X.quantize_rows(X.rows(5, 256, offset=7))
    w = rng.integers(0, 0x7e, (6, 256)).astype(np.uint8)
    ws, bias = np.exp2(rng.integers(-3, 3, 6).astype(np.float64)), rng.integers(-4, 4, 6).astype(np.float64)
    want = np.array([[sum(X.E4M3[q[m, k]] * 2.0 ** (int(s[m, k // 32]) - 127) * X.E4M3[w[n, k]] for k in range(256)) * ws[n] + bias[n]
                      for n in range(6)] for m in range(5)])
    got = X.linear(q, s, w, ws, bias)
    S = np.abs(X.dequantize(q, s)) @ (np.abs(X.E4M3[w]) * ws[:, None]).T + np.abs(bias)[None, :]      # fp64 sums in another order
    assert np.all(np.abs(got - want) <= 1e-12 * S)


@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_every_named_defect_of_the_quantiser_changes_a_probe_output(probe, mutant):
    x, (q, s) = probe
    qm, sm = X.quantize_rows(x, mutant)
    assert not (np.array_equal(q, qm) and np.array_equal(s, sm)), mutant
    # ... and each of the three shapes the GPU test runs notices it too
    for M, K, off in X.SHAPES:
        xi = X.rows(M, K, off)
        a, b = X.quantize_rows(xi), X.quantize_rows(xi, mutant)
        assert not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), (mutant, M, K)


def test_the_small_shapes_still_hold_zero_blocks_and_round_up_blocks():
    fam = X.pool()
    n_exp = len(fam["exponents"])
    assert n_exp == 1020
    for M, K, off in X.SHAPES:
        blocks = (off + np.arange(M * K // X.BLK)) % X.pool_size()
        assert np.any((blocks >= n_exp) & (blocks < n_exp + 3)), (M, K)          # a zero block
