"""Image pre- and post-processing on the device, bit-exact with the host (include/regione_hip.h section a12, csrc/image.hip): what a
hosted edit does with `image_processor.resize / preprocess / postprocess` and the Qwen2-VL image processor - PIL's 8-bit Lanczos /
bicubic resampling, `x / 255 -> NCHW -> 2 x - 1`, the VLM's rescale / normalise / patchify, and `(x * 0.5 + 0.5).clamp(0, 1) -> uint8`.

The tables are built HERE, on the host, with the host's own arithmetic (float64 coefficients as Pillow's precompute_coeffs /
normalize_coeffs_8bpc, the torch / numpy expressions of the processors); the kernels only apply them in integer arithmetic, so every
output equals the host path's bit for bit.  No CPU fallback: inputs the kernels do not cover are refused by name (RegionEHipError).
"""
from __future__ import annotations

import collections
import functools
import math
from typing import Tuple

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream, padded

PRECISION_BITS = 22                       # Pillow: 32 - 8 - 2
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PATCH, MERGE, TEMPORAL = 14, 2, 2
PATCH_K = 3 * TEMPORAL * PATCH * PATCH    # 1176
IMAGE_PADDED, IMAGE_NCHW = 0, 1           # RGN_IMAGE_*
TABLE_CACHE = 64                          # resample tables kept, on the host and per HipImageOps on the device


def _refuse(what: str, why: str):
    raise _lib.RegionEHipError(f"{what}: {why}")


def _sin(x: np.ndarray) -> np.ndarray:
    """libm's sin of every element (math.sin, as Pillow's C code calls it): numpy's own float64 sin may differ from libm in the last bit,
    and the last bit of a coefficient can move its 22-bit rounding."""
    return np.array(list(map(math.sin, x.ravel().tolist())), dtype=np.float64).reshape(x.shape)


def _sinc(x: np.ndarray) -> np.ndarray:
    zero = x == 0.0
    t = np.where(zero, 1.0, x) * math.pi
    return np.where(zero, 1.0, _sin(t) / t)


def _lanczos(x: np.ndarray) -> np.ndarray:
    inside = (-3.0 <= x) & (x < 3.0)
    x = np.where(inside, x, 0.0)
    return np.where(inside, _sinc(x) * _sinc(x / 3), 0.0)


def _bicubic(x: np.ndarray) -> np.ndarray:
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


_FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}


@functools.lru_cache(maxsize=TABLE_CACHE)
def resample_table(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray, int]:
    """(bounds int32 [out_size, 2] = (first, count), weights int32 [out_size, ksize], ksize) of one pass of Pillow's 8-bit resampler
    over box (0, 0, W, H) with reducing_gap None: precompute_coeffs in float64, then normalize_coeffs_8bpc (22-bit fixed point, rounded
    half away from zero by truncation).  Every float64 operation is Pillow's, element by element, in Pillow's order - numpy only runs
    them over all taps at once: libm's sin, the weight sum accumulated tap by tap (not numpy's pairwise sum), a true division.  A first
    call for a size pair costs a few milliseconds of host time (2048 -> 1248 Lanczos: about 27 k sines); cached per (in, out, filter);
    the arrays are read-only."""
    if filter not in _FILTERS:
        _refuse("resample_table", f"filter {filter!r} (\"lanczos\" and \"bicubic\" are covered)")
    if in_size < 1 or out_size < 1:
        _refuse("resample_table", f"sizes {in_size} -> {out_size} (both must be >= 1)")
    f, fsupport = _FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)                      # (int) truncates towards zero
    xmax = np.minimum(np.trunc(center + support + 0.5), float(in_size)) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    valid = x < xmax[:, None]
    k = np.where(valid, f(((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                                        # ww += w, tap by tap (taps past the count add 0.0)
        ww = ww + k[:, j]
    k = np.where((ww != 0.0)[:, None], k / np.where(ww != 0.0, ww, 1.0)[:, None], k)
    scaled = k * float(1 << PRECISION_BITS)
    weights = np.where(k < 0, np.trunc(-0.5 + scaled), np.trunc(0.5 + scaled)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    weights.setflags(write=False)
    return bounds, weights, ksize


def smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = 56 * 56, max_pixels: int = 28 * 28 * 1280) -> Tuple[int, int]:
    """The Qwen2-VL processor's target size: both sides multiples of `factor`, the area inside [min_pixels, max_pixels]."""
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"absolute aspect ratio must be smaller than 200, got {max(height, width) / min(height, width)}")
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


def vae_table() -> torch.Tensor:
    """bf16 [256]: the host's `2 * (uint8 / 255) - 1` (numpy fp32 division, torch fp32 `2.0 * x - 1.0`), rounded to bf16."""
    return (2.0 * (torch.arange(256, dtype=torch.float32) / 255.0) - 1.0).to(torch.bfloat16)


def patch_table(mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD, rescale_factor: float = 1 / 255) -> torch.Tensor:
    """fp32 [3, 256]: the processor's numpy arithmetic on every byte - rescale `float32(float64(v) * rescale_factor)`, then normalise
    `(x - float32(mean)) / float32(std)` in fp32."""
    x = (np.arange(256, dtype=np.uint8).astype(np.float64) * rescale_factor).astype(np.float32)
    m, s = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(((x[None, :].T - m) / s).T.astype(np.float32)))


class HipImageOps:
    """The device side of a hosted edit's image work.  Images are uint8 [H, W, 3] tensors on `device`."""
    what = "HipImageOps"
    smart_resize = staticmethod(smart_resize)

    def __init__(self, device, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, rescale_factor: float = 1 / 255):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            _refuse(self.what, f"device {self.device} (the kernels need the GPU: there is no CPU fallback)")
        self._vae_tab = vae_table().to(self.device)
        self._patch_tab = patch_table(image_mean, image_std, rescale_factor).to(self.device)
        self._tabs = collections.OrderedDict()     # (in, out, filter) -> (bounds, weights, ksize) on the device: the last 64 used

    # ---- host <-> device ---------------------------------------------------------------------------------------------------------------
    def upload(self, image) -> torch.Tensor:
        """A mode "RGB" PIL image or a uint8 [H, W, 3] array (numpy or torch) -> uint8 [H, W, 3] on the device."""
        if hasattr(image, "mode") and hasattr(image, "size") and not isinstance(image, (np.ndarray, torch.Tensor)):
            if image.mode != "RGB":
                _refuse(self.what + ".upload", f"PIL mode {image.mode!r} (mode \"RGB\" is covered)")
            image = np.array(image)                    # a writable copy: torch.from_numpy does not take PIL's read-only view
        if isinstance(image, np.ndarray):
            if image.dtype != np.uint8:
                _refuse(self.what + ".upload", f"array of dtype {image.dtype} (uint8 is covered)")
            if image.ndim != 3 or image.shape[2] != 3:
                _refuse(self.what + ".upload", f"array of shape {tuple(image.shape)} (one [H, W, 3] image is covered, no batches)")
            image = torch.from_numpy(np.ascontiguousarray(image))
        if not isinstance(image, torch.Tensor):
            _refuse(self.what + ".upload", f"{type(image).__name__} (an RGB PIL image or a uint8 [H, W, 3] array is covered)")
        return self._check(image.to(self.device), "upload")

    def _check(self, u8, who: str) -> torch.Tensor:
        if not isinstance(u8, torch.Tensor):
            _refuse(f"{self.what}.{who}", f"{type(u8).__name__} (a uint8 [H, W, 3] tensor on the device: see upload())")
        if u8.dtype != torch.uint8:
            _refuse(f"{self.what}.{who}", f"tensor of dtype {u8.dtype} (uint8 is covered)")
        if u8.dim() != 3 or u8.shape[2] != 3 or u8.shape[0] < 1 or u8.shape[1] < 1:
            _refuse(f"{self.what}.{who}", f"tensor of shape {tuple(u8.shape)} (one [H, W, 3] image is covered, no batches)")
        if not u8.is_cuda:
            _refuse(f"{self.what}.{who}", "a CPU tensor (upload() it first: there is no CPU fallback)")
        return u8.contiguous()

    def to_pil(self, u8):
        """uint8 [H, W, 3] on the device -> a PIL RGB image (the one download of the output path)."""
        import PIL.Image
        return PIL.Image.fromarray(self._check(u8, "to_pil").cpu().numpy())

    # ---- kernels -----------------------------------------------------------------------------------------------------------------------
    def _table(self, in_size: int, out_size: int, filt: str):
        key = (in_size, out_size, filt)
        if key not in self._tabs:
            b, w, k = resample_table(in_size, out_size, filt)
            self._tabs[key] = (torch.from_numpy(b.copy()).to(self.device), torch.from_numpy(w.copy()).to(self.device), k)
            if len(self._tabs) > TABLE_CACHE:                # launches already enqueued keep their tables alive (stream-ordered free)
                self._tabs.popitem(last=False)
        self._tabs.move_to_end(key)
        return self._tabs[key]

    def resize(self, u8, H: int, W: int, filter: str = "lanczos", box=None, reducing_gap=None) -> torch.Tensor:
        """`PIL.Image.resize((W, H), filter)` of an RGB image: the x pass into a uint8 intermediate, then the y pass; a pass whose size does
        not change is skipped (both: a copy)."""
        if box is not None or reducing_gap is not None:
            _refuse(self.what + ".resize", "box / reducing_gap (the whole image, reducing_gap None is covered)")
        if filter not in _FILTERS:
            _refuse(self.what + ".resize", f"filter {filter!r} (\"lanczos\" and \"bicubic\" are covered)")
        x = self._check(u8, "resize")
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            _refuse(self.what + ".resize", f"target size {H} x {W}")
        lib = _lib.lib()
        ih, iw = x.shape[0], x.shape[1]
        if iw != W:
            b, w, k = self._table(iw, W, filter)
            y = torch.empty((ih, W, 3), dtype=torch.uint8, device=self.device)
            _lib.check(lib.rgn_image_resample_u8(_p(x), ih, iw, _p(y), ih, W, _p(b), _p(w), k, 0, _stream()), "rgn_image_resample_u8")
            x = y
        if ih != H:
            b, w, k = self._table(ih, H, filter)
            y = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            _lib.check(lib.rgn_image_resample_u8(_p(x), ih, W, _p(y), H, W, _p(b), _p(w), k, 1, _stream()), "rgn_image_resample_u8")
            x = y
        return x.clone() if x is u8 else x

    def to_vae_input(self, u8) -> torch.Tensor:
        """`preprocess` of the VAE image processor: bf16 [1, 3, H, W] = bf16(2 * (byte / 255) - 1)."""
        x = self._check(u8, "to_vae_input")
        H, W = x.shape[0], x.shape[1]
        out = torch.empty((1, 3, H, W), dtype=torch.bfloat16, device=self.device)
        _lib.check(_lib.lib().rgn_image_u8_to_nchw_bf16(_p(x), _p(out), H, W, _p(self._vae_tab), _stream()), "rgn_image_u8_to_nchw_bf16")
        return out

    def to_patch_rows(self, u8, out: str = "fp32", Kp: int = padded(PATCH_K, 64)) -> torch.Tensor:
        """The Qwen2-VL processor's rescale, normalise and patchify of an image whose sides are multiples of 28.  out = "fp32": fp32
        [N, 1176], the processor's `pixel_values`; "padded_bf16": bf16 [N, Kp] with the columns [1176, Kp) zero, the vision tower's GEMM
        operand (what rgn_cast_pad_rows makes of the fp32 rows)."""
        if out not in ("fp32", "padded_bf16"):
            _refuse(self.what + ".to_patch_rows", f"out = {out!r} (\"fp32\" and \"padded_bf16\" are covered)")
        x = self._check(u8, "to_patch_rows")
        H, W = x.shape[0], x.shape[1]
        if H % (PATCH * MERGE) or W % (PATCH * MERGE):
            _refuse(self.what + ".to_patch_rows", f"image {H} x {W} (both sides must be multiples of {PATCH * MERGE})")
        N = (H // PATCH) * (W // PATCH)
        bf = out == "padded_bf16"
        if bf and (Kp < PATCH_K or Kp % 8):
            _refuse(self.what + ".to_patch_rows", f"Kp = {Kp} (a multiple of 8, at least {PATCH_K})")
        ldo = int(Kp) if bf else PATCH_K
        rows = torch.empty((N, ldo), dtype=torch.bfloat16 if bf else torch.float32, device=self.device)
        _lib.check(_lib.lib().rgn_image_patchify_u8(_p(x), H, W, _p(self._patch_tab), _p(rows), int(bf), ldo, _stream()), "rgn_image_patchify_u8")
        return rows

    def to_uint8(self, decoded) -> torch.Tensor:
        """`postprocess` up to the bytes: a decoded bf16 image - [1, 3, H, W] / [3, H, W] on the device, or a decoder's padded pixel-major
        image - through `(x * 0.5 + 0.5).clamp(0, 1)` in bf16 and `(a * 255).round()` in fp32 to uint8 [H, W, 3]."""
        from .vae import PaddedImage
        lib = _lib.lib()
        if isinstance(decoded, PaddedImage):
            if decoded.C < 4 or decoded.C % 4:
                _refuse(self.what + ".to_uint8", f"padded image of {decoded.C} channels (a multiple of 4 is covered)")
            H, W = decoded.H, decoded.W
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            _lib.check(lib.rgn_image_bf16_to_u8(decoded.ptr(), IMAGE_PADDED, decoded.C, _p(out), H, W, _stream()), "rgn_image_bf16_to_u8")
            return out
        if not isinstance(decoded, torch.Tensor):
            _refuse(self.what + ".to_uint8", f"{type(decoded).__name__} (a bf16 [1, 3, H, W] tensor is covered)")
        if decoded.dtype != torch.bfloat16:
            _refuse(self.what + ".to_uint8", f"tensor of dtype {decoded.dtype} (bf16 is covered)")
        x = decoded[0] if decoded.dim() == 4 and decoded.shape[0] == 1 else decoded
        if x.dim() != 3 or x.shape[0] != 3:
            _refuse(self.what + ".to_uint8", f"tensor of shape {tuple(decoded.shape)} (one [1, 3, H, W] image is covered, no batches)")
        if not x.is_cuda:
            _refuse(self.what + ".to_uint8", "a CPU tensor (there is no CPU fallback)")
        x = x.contiguous()
        H, W = x.shape[1], x.shape[2]
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
        _lib.check(lib.rgn_image_bf16_to_u8(_p(x), IMAGE_NCHW, 0, _p(out), H, W, _stream()), "rgn_image_bf16_to_u8")
        return out
