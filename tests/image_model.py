"""CPU model of the rgn_image_* entries (include/regione_hip.h section a12, csrc/image.hip) and of regione_amd/image_ops.py: the host's
image arithmetic restated in numpy, with NAMED DEFECTS.  Test infrastructure only.  The contract is equality of bits, so there is no bound.

Resampler (Pillow, src/libImaging/Resample.c, 8 bits per channel).  Per output index xx of a pass over `in_size` -> `out_size`:
    scale = in_size / out_size;  fscale = max(scale, 1);  support = filter_support * fscale;  ksize = ceil(support) * 2 + 1
    center = (xx + 0.5) * scale;  first = max(int(center - support + 0.5), 0);  last = min(int(center + support + 0.5), in_size)
    w[k] = filter((k + first - center + 0.5) / fscale), k < count = last - first;  w /= sum(w)            (all in float64)
    W[k] = int(w[k] * 2^22 + 0.5) for w >= 0, int(w[k] * 2^22 - 0.5) for w < 0                          (truncation: half away from zero)
    out = clip((2^21 + sum_k in[first + k] * W[k]) >> 22, 0, 255)                                          (int32)
The x pass runs first into a uint8 intermediate, the y pass second; a pass whose size does not change is skipped.

Preprocess table: (2.0 * (arange(256, fp32) / 255.0) - 1.0) rounded to bf16 (a true fp32 division).
Patch rows: the Qwen2-VL processor's float32(float64(byte) * (1 / 255)), then (x - mean) / std in fp32; rows in the order
(gh / 2, gw / 2, 2, 2), columns (C, temporal 2 with the frame duplicated, 14, 14).
bf16 -> u8: t = bf16(x * 0.5); t = bf16(t + 0.5); clamp to [0, 1]; rint_half_even(fp32(t) * 255).
"""
import math

import numpy as np

PRECISION_BITS = 22
RESAMPLE_DEFECTS = ("y_pass_first", "accumulator_starts_at_zero", "float_accumulation", "first_not_clamped", "count_not_clamped",
                    "weights_truncated", "single_2d_pass")
OTHER_DEFECTS = ("reciprocal_multiply", "temporal_channel_swapped", "round_half_up")
DEFECTS = RESAMPLE_DEFECTS + OTHER_DEFECTS

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PATCH, MERGE, TEMPORAL = 14, 2, 2


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}


def coeffs(in_size, out_size, filt, defect=None):
    """(bounds int32 [out, 2] = (first, count), weights [out, ksize], ksize).  The weights are int32 fixed point, or the normalised float64
    ones under the defects that need them (float_accumulation, single_2d_pass)."""
    f, fsupport = FILTERS[filt]
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = fsupport * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    lo_pad = ksize if defect == "first_not_clamped" else 0        # the unclamped taps address a zero-extended input
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize + (2 if defect in ("first_not_clamped", "count_not_clamped") else 0)), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        first = int(center - support + 0.5)
        last = int(center + support + 0.5)
        if defect == "first_not_clamped":
            first = int(math.floor(center - support + 0.5))
        elif first < 0:
            first = 0
        if last > in_size and defect != "count_not_clamped":
            last = in_size
        n = last - first
        w = [f((k + first - center + 0.5) / fscale) for k in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        kk[xx, :n] = w
        bounds[xx] = (first, n)
    if defect in ("float_accumulation", "single_2d_pass"):
        return bounds, kk, kk.shape[1]
    scaled = kk * float(1 << PRECISION_BITS)
    if defect == "weights_truncated":
        W = np.trunc(scaled)
    else:
        W = np.where(kk < 0, np.trunc(scaled - 0.5), np.trunc(scaled + 0.5))
    return bounds, W.astype(np.int32), kk.shape[1]


def _pass(img, out_size, filt, axis, defect=None):
    """One pass over axis 1 (x) or 0 (y) of a uint8 [H, W, C] image."""
    a = np.moveaxis(np.asarray(img), axis, 0)                       # the resampled dimension first
    n = a.shape[0]
    bounds, W, _ = coeffs(n, out_size, filt, defect)
    if defect in ("first_not_clamped", "count_not_clamped"):        # what an unclamped window reads: zeros outside the image
        pad = W.shape[1]
        a = np.concatenate([np.zeros((pad,) + a.shape[1:], a.dtype), a, np.zeros((pad,) + a.shape[1:], a.dtype)], 0)
        off = pad
    else:
        off = 0
    out = np.empty((out_size,) + a.shape[1:], np.uint8)
    for i in range(out_size):
        first, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        win = a[off + first:off + first + cnt]
        if defect == "float_accumulation":
            acc = np.tensordot(W[i, :cnt], win.astype(np.float64), axes=(0, 0))
            out[i] = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
            continue
        acc = np.tensordot(W[i, :cnt].astype(np.int64), win.astype(np.int64), axes=(0, 0))
        acc = acc + (0 if defect == "accumulator_starts_at_zero" else (1 << (PRECISION_BITS - 1)))
        acc = acc.astype(np.int32)                                  # the accumulator IS int32 (no input makes it wrap: |sum| < 2^31)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, out_h, out_w, filt, defect=None):
    """uint8 [H, W, 3] -> uint8 [out_h, out_w, 3], as PIL.Image.resize((out_w, out_h), filt) on an RGB image."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, Wd = img.shape[:2]
    if defect == "single_2d_pass":                                  # both passes in float64, one rounding: no uint8 intermediate
        bx, kx, _ = coeffs(Wd, out_w, filt, defect)
        by, ky, _ = coeffs(H, out_h, filt, defect)
        t = np.zeros((H, out_w, img.shape[2]), np.float64)
        for x in range(out_w):
            f, c = int(bx[x, 0]), int(bx[x, 1])
            t[:, x] = np.tensordot(img[:, f:f + c].astype(np.float64), kx[x, :c], axes=(1, 0))
        o = np.zeros((out_h, out_w, img.shape[2]), np.float64)
        for y in range(out_h):
            f, c = int(by[y, 0]), int(by[y, 1])
            o[y] = np.tensordot(ky[y, :c], t[f:f + c], axes=(0, 0))
        return np.clip(np.rint(o), 0, 255).astype(np.uint8)
    order = ((0, out_h, H), (1, out_w, Wd)) if defect == "y_pass_first" else ((1, out_w, Wd), (0, out_h, H))
    for axis, out_size, in_size in order:
        if out_size != in_size:
            img = _pass(img, out_size, filt, axis, defect)
    return np.ascontiguousarray(img)


# ---- bf16 helpers -----------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """fp32 array -> the uint16 patterns of the nearest bf16 values (ties to even; no NaN handling: NaN is out of contract)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _rbf(x):
    return bf16_to_f32(bf16_bits(x))


# ---- the tables and maps -----------------------------------------------------------------------------------------------------------------
def vae_table(defect=None):
    """uint16 [256]: bf16 patterns of 2 * (v / 255) - 1 evaluated in fp32."""
    v = np.arange(256, dtype=np.float32)
    if defect == "reciprocal_multiply":
        q = v * np.float32(1.0 / 255.0)
    else:
        q = v / np.float32(255.0)
    return bf16_bits(np.float32(2.0) * q - np.float32(1.0))


def to_vae_input(img, defect=None):
    """uint8 [H, W, 3] -> uint16 [1, 3, H, W] (bf16 patterns)."""
    return vae_table(defect)[np.asarray(img, np.uint8)].transpose(2, 0, 1)[None].copy()


def patch_table(mean=CLIP_MEAN, std=CLIP_STD, rescale=1 / 255):
    """fp32 [3, 256]: the processor's rescale (float64 product, cast to fp32), then its fp32 (x - mean) / std."""
    x = (np.arange(256, dtype=np.uint8).astype(np.float64) * rescale).astype(np.float32)
    m, s = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32)
    return ((x[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


def patch_rows(img, defect=None):
    """uint8 [H, W, 3] (H, W multiples of 28) -> fp32 [N, 1176]."""
    img = np.asarray(img, np.uint8)
    H, Wd = img.shape[:2]
    assert H % (PATCH * MERGE) == 0 and Wd % (PATCH * MERGE) == 0
    tab = patch_table()
    chw = np.stack([tab[c][img[:, :, c]] for c in range(3)])                              # [3, H, W]
    gh, gw = H // PATCH, Wd // PATCH
    p = chw.reshape(3, gh // MERGE, MERGE, PATCH, gw // MERGE, MERGE, PATCH).transpose(1, 4, 2, 5, 0, 3, 6)
    p = np.broadcast_to(p[:, :, :, :, :, None], p.shape[:5] + (TEMPORAL,) + p.shape[5:])    # (gh/2, gw/2, 2, 2, C, T, 14, 14)
    if defect == "temporal_channel_swapped":
        p = p.transpose(0, 1, 2, 3, 5, 4, 6, 7)
    return np.ascontiguousarray(p).reshape(gh * gw, 3 * TEMPORAL * PATCH * PATCH)


def pad_rows_bf16(rows, Kp):
    """fp32 [N, K] -> uint16 [N, Kp]: bf16 patterns, the columns [K, Kp) zero (rgn_cast_pad_rows)."""
    out = np.zeros((rows.shape[0], Kp), np.uint16)
    out[:, :rows.shape[1]] = bf16_bits(rows)
    return out


def _rbf_half_up(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return bf16_to_f32(((u + 0x8000) >> 16).astype(np.uint16))


def unit_u8(bits, defect=None):
    """bf16 patterns (any shape) -> uint8: torch's bf16 `(x * 0.5 + 0.5).clamp(0, 1)`, numpy's fp32 `(a * 255).round().astype(uint8)`.

    round_half_up: every rounding of the map breaks ties upwards (in magnitude) instead of to even - the two bf16 roundings and the last
    one to an integer.  The last one ALONE cannot be seen: t is a bf16 value in [0, 1] (8 significant bits) and 255 has 8, so t * 255 is
    exact in fp32, and t * 255 = k + 1/2 needs 255 m = (2 k + 1) 2^(e - 1) for t = m / 2^e, m odd, i.e. e = 1, t = 1/2 (x = 0): the one
    tie is 127.5, which both rules send to 128.  The ties of bf16(t + 0.5) are many (any t in [0.5, 1) with 8 significant bits has 9
    after the sum), and there the two rules differ."""
    x = bf16_to_f32(bits)
    rb = _rbf_half_up if defect == "round_half_up" else _rbf
    with np.errstate(over="ignore", invalid="ignore"):
        t = rb(x * np.float32(0.5))
        t = rb(t + np.float32(0.5))
        t = np.minimum(np.maximum(t, np.float32(0.0)), np.float32(1.0))
        v = t * np.float32(255.0)
    if defect == "round_half_up":
        return np.floor(v.astype(np.float64) + 0.5).astype(np.uint8)
    return np.rint(v).astype(np.uint8)


def all_bf16_image():
    """Every bf16 pattern whose exponent field is not all ones (the 65280 = 3 * 160 * 136 finite ones: the 254 NaNs are out of contract,
    the two infinities are probed apart) once, as uint16 [3, 160, 136]."""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80].astype(np.uint16)
    assert bits.size == 65280
    return bits.reshape(3, 160, 136)


def smart_resize(height, width, factor=28, min_pixels=56 * 56, max_pixels=28 * 28 * 1280):
    if max(height, width) / min(height, width) > 200:
        raise ValueError("aspect ratio above 200")
    h_bar = round(height / factor) * factor
    w_bar = round(width / factor) * factor
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = max(factor, math.floor(height / beta / factor) * factor)
        w_bar = max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar
