"""VAE decode on the HIP kernels.

The reference ends every edit with `image = self.vae.decode(latents, return_dict=False)[0]` (FluxKontext/inplace.py:396-402; the
Step1X-Edit pipelines make the same call) and its latency protocol times the whole `pipe(...)` call (src/FluxKontext/main.py:62-73),
so the decode is part of the reference's end-to-end edit time.  The module is the [EXT] `AutoencoderKL` decoder of the public
FLUX.1 / Step1X-Edit checkpoints (diffusers layout: conv_in -> mid block (ResNet, one attention head of width 512, ResNet) ->
four up levels of three ResNet blocks (512, 512, 256, 128 channels; nearest 2 x upsample + 3 x 3 conv after the first three) ->
GroupNorm + SiLU + conv_out); nothing of it lives in /root/reference: [EXT], unpinned, checked against an fp32 PyTorch module of the
same architecture (tests/host_vae.py) instead of the oracle.

`HipVaeDecoder(state_dict, device)` adopts a decoder's parameters (diffusers names, with or without the `decoder.` prefix) once:
3 x 3 kernels re-laid [Cout, Cin, 3, 3] -> [Cout, 3, 3, Cin] bf16.  `decode(z)` runs ~95 launches, all `rgn::` kernels:

  * every convolution = rgn_conv_bf16: an implicit GEMM on the hand-scheduled 256 x 256 MFMA loop over a zero-bordered, pixel-major
    activation image (csrc/vae.hip header), bias / ResNet skip / border zeroing in its epilogue;
  * GroupNorm(32) + SiLU = rgn_groupnorm_silu (statistics pass + apply pass, bit-reproducible);
  * the mid-block attention = three GEMMs + rgn_softmax_rows while its score matrix fits that pass (attention_path), else the fused
    flash-style rgn_vae_attention_bf16 (no score matrix in memory);
  * nearest upsample, NCHW <-> padded pixel-major conversions = row kernels.

No CPU / eager fallback: a missing library raises RegionEHipError like every other op of the package.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, ops

_p, _stream = ops._p, ops._stream

SOFTMAX_MAX_ROWS = 24576              # rgn_softmax_rows: (h + 2) (w + 2) of the mid-block image, the materialised attention's limit
# the largest image either VAE family (this module and qwen_vae.py) decodes or encodes: H * W <= 2048^2 and each side <= 4096 (the
# biggest activation, 256 channels at full resolution, then stays below the 2^32-byte reach of the convolution's buffer offsets)
MAX_IMAGE_PIXELS = 2048 * 2048
MAX_IMAGE_SIDE = 4096
ATTENTION_MODES = ("auto", "fused", "materialized")


def check_image_size(H: int, W: int, what: str):
    """Raise RegionEHipError, before anything is allocated or launched, for an image (pixels, not latents) past the documented maximum."""
    if H * W > MAX_IMAGE_PIXELS or H > MAX_IMAGE_SIDE or W > MAX_IMAGE_SIDE:
        raise _lib.RegionEHipError(f"{what}: image {H} x {W} is past the HIP VAE's maximum (H * W <= {MAX_IMAGE_PIXELS} = 2048^2, "
                                   f"each side <= {MAX_IMAGE_SIDE})")


def attention_path(mode: str, rows: int) -> str:
    """Which mid-block attention runs on a padded image of `rows` rows: "materialized" (three GEMMs + rgn_softmax_rows over a score
    matrix S [rows, rows]) or "fused" (rgn_vae_attention_bf16, no S).  "auto" keeps the materialised path wherever it runs."""
    if mode not in ATTENTION_MODES:
        raise _lib.RegionEHipError(f"attention = {mode!r}: one of {ATTENTION_MODES}")
    if mode == "auto":
        return "materialized" if rows <= SOFTMAX_MAX_ROWS else "fused"
    if mode == "materialized" and rows > SOFTMAX_MAX_ROWS:
        raise _lib.RegionEHipError(f"attention = 'materialized': {rows} rows, rgn_softmax_rows covers at most {SOFTMAX_MAX_ROWS}")
    return mode


class PaddedImage:
    """A zero-bordered pixel-major activation image [Hp * Wp, C] bf16 inside a storage tensor with guard rows on both sides.
    `border_zero`: the border rows are known to be zero - true from creation, then whatever the last writer left (`_wrote`).
    Guard rows (include/regione_hip.h; tests/test_gpu_conv_probes.py probe f): most launches read them only for outputs they then mask,
    but a 3 x 3 pixel-group convolution adds the up to group - 1 rows next to the image, on either side, into interior outputs through the
    zero entries of its Toeplitz matrix - those rows must stay FINITE.  They are zero from creation; the writers that touch them keep them
    finite: a pixel-group launch writes zeros to the group - 1 rows behind its output, conv_up2 a zeroed scratch row, conv_s2 a scratch row
    of real (finite, but undefined: racing stores) convolution values - no pipeline here feeds a conv_s2 output to a pixel-group launch."""

    def __init__(self, H: int, W: int, C: int, device):
        self.H, self.W, self.C = H, W, C
        self.Hp, self.Wp = H + 2, W + 2
        self.rows = self.Hp * self.Wp
        g = self.Wp + 72                     # guard rows: a window reads up to Wp + 1 + group rows outside the image (group <= 64), pixel groups write group - 1
        self.storage = torch.zeros((self.rows + 2 * g, C), dtype=torch.bfloat16, device=device)
        self.t = self.storage[g:g + self.rows]
        self.border_zero = True

    def ptr(self) -> int:
        return self.t.data_ptr()


class _Pool:
    """Per-decoder activation buffers, reused across layers and calls (everything runs stream-ordered on one stream)."""

    def __init__(self, device):
        self.device = device
        self.free: Dict[Tuple[int, int, int], List[PaddedImage]] = {}

    def get(self, H, W, C) -> PaddedImage:
        lst = self.free.setdefault((H, W, C), [])
        return lst.pop() if lst else PaddedImage(H, W, C, self.device)

    def put(self, img: PaddedImage):
        self.free.setdefault((img.H, img.W, img.C), []).append(img)


class ConvWeights:
    """One convolution's parameters as rgn_conv_bf16 wants them.  `w4`: [Cout, kh, kw, Cin] fp32 (kh = kw = 3 or 1).  group = 1: the matrix
    [Cout, taps * Cin].  group > 1 (narrow outputs): the block-Toeplitz matrix over a window of group + 2 pixels per kernel row - output row =
    `group` pixels x `ldy` columns, row p * ldy + c holds w4[c, ky, kx] at window pixel p + kx of kernel row ky (include/regione_hip.h)."""

    def __init__(self, w4: torch.Tensor, bias: torch.Tensor, group: int = 1, ldy: Optional[int] = None):
        co, kh, kw, ci = w4.shape
        assert kh == kw and kh in (1, 3)
        self.taps, self.cout, self.cin, self.group = kh * kw, co, ci, group
        self.ldy = co if ldy is None else ldy
        dev = w4.device
        if group == 1:
            self.w = w4.reshape(co, -1).to(torch.bfloat16).contiguous()
            self.b = bias.to(dev, torch.bfloat16).contiguous()
        else:
            win = group + 2 if kh == 3 else group
            t = torch.zeros((group, self.ldy, kh, win, ci), dtype=torch.float32, device=dev)
            for p in range(group):
                for kx in range(kw):
                    t[p, :co, :, p + kx, :] = w4[:, :, kx, :]
            self.w = t.reshape(group * self.ldy, -1).to(torch.bfloat16).contiguous()
            b = torch.zeros((group, self.ldy), dtype=torch.float32, device=dev)
            b[:, :co] = bias.to(dev, torch.float32)
            self.b = b.reshape(-1).to(torch.bfloat16).contiguous()


class GnHandoff:
    """One stream's GroupNorm hand-off: the workspace of per-tile partial sums every image on the stream shares, and whose statistics it
    holds right now (`owner`, in `nblk` tiles; None: nobody's).  A convolution with gn = True is the producer, the next groupnorm_silu of
    that image the consumer; any other write to the owner in between makes the sums stale and drops them."""

    def __init__(self):
        self.ws, self.owner, self.nblk = None, None, 0

    def workspace(self, device) -> torch.Tensor:
        if self.ws is None:
            self.ws = torch.empty(_lib.lib().rgn_groupnorm_workspace_bytes() // 4, dtype=torch.float32, device=device)
        return self.ws

    def set(self, img: Optional[PaddedImage], nblk: int = 0):
        self.owner, self.nblk = img, nblk

    def wrote(self, img: PaddedImage):
        if self.owner is img:
            self.set(None)

    def take(self, img: PaddedImage) -> int:
        """The tile count of `img`'s sums (0: the workspace does not hold them); consumed either way."""
        nblk = self.nblk if self.owner is img else 0
        self.set(None)
        return nblk


_gn_lanes: Dict[Tuple[str, int], GnHandoff] = {}


def _handoff(device) -> GnHandoff:
    return ops._ws_lane(_gn_lanes, device, GnHandoff)        # per (device, stream), bounded like the GEMM and attention scratch


def gn_handoff(device) -> Tuple[Optional[PaddedImage], int]:
    """(owner, tile count) of the current stream's GroupNorm hand-off."""
    lane = _handoff(device)
    return lane.owner, lane.nblk


def _wrote(img: PaddedImage, border_zero: bool):
    """Every writer of a PaddedImage reports here: what it leaves on the border, and that statistics handed off for `img` - on whichever
    stream: the few lanes are walked, no stream is looked up - are stale."""
    img.border_zero = border_zero
    for lane in _gn_lanes.values():
        lane.wrote(img)


def _need_zero_border(img: PaddedImage, what: str):
    if not img.border_zero:
        raise _lib.RegionEHipError(f"{what}: the border of the {img.H} x {img.W} x {img.C} image is not known to be zero (its last writer - the "
                                   "attention's P V GEMM - wrote it; a convolution or a norm has to rewrite the image first)")


def conv(x: PaddedImage, cw: ConvWeights, out: PaddedImage, resid: Optional[PaddedImage] = None, gn: bool = False):
    """out = conv(x) + bias (+ resid), border rows zero (rgn_conv_bf16).  gn = True: the epilogue also leaves the GroupNorm statistics of `out`
    in the stream's groupnorm workspace (the next `groupnorm_silu(out, ...)` then skips its statistics pass)."""
    if cw.cin != x.C or out.C != cw.ldy or (resid is not None and (resid.C != out.C or resid.rows != out.rows)) or out.rows != x.rows:
        raise _lib.RegionEHipError(f"conv: weights for {cw.cin} -> {cw.cout} (row stride {cw.ldy}) on images with {x.C} -> {out.C} channels")
    nblk, ws = ctypes.c_int(0), None
    _wrote(out, True)
    if gn:
        lane = _handoff(x.t.device)
        lane.set(None)                                   # whatever the workspace held is about to be overwritten
        ws = lane.workspace(x.t.device)
    rc = _lib.lib().rgn_conv_bf16(x.ptr(), x.C, _p(cw.w), _p(cw.b), None if resid is None else resid.ptr(), out.ptr(), out.C, x.Hp, x.Wp,
                                  x.C, cw.cout, cw.taps, cw.group, _p(ws), ctypes.byref(nblk) if gn else None, _stream())
    _lib.check(rc, "rgn_conv_bf16")
    if gn:
        lane.set(out, nblk.value)
    return out


def groupnorm_silu(x: PaddedImage, gamma: torch.Tensor, beta: torch.Tensor, out: PaddedImage, silu: bool = True, eps: float = 1e-6):
    lane = _handoff(x.t.device)
    pre = lane.take(x)                                   # > 0: the convolution that wrote x left its tiles' sums in the workspace
    if pre == 0:
        _need_zero_border(x, "groupnorm_silu")           # the statistics pass sums the border rows too
    ws = lane.workspace(x.t.device)
    _wrote(out, True)
    rc = _lib.lib().rgn_groupnorm_silu(x.ptr(), out.ptr(), x.Hp, x.Wp, x.C, _p(gamma), _p(beta), float(eps), int(silu), _p(ws), pre, _stream())
    _lib.check(rc, "rgn_groupnorm_silu")
    return out


def upsample2x(x: PaddedImage, out: PaddedImage):
    assert out.H == 2 * x.H and out.W == 2 * x.W and out.C == x.C
    _wrote(out, True)
    _lib.check(_lib.lib().rgn_upsample2x(x.ptr(), out.ptr(), x.Hp, x.Wp, x.C, _stream()), "rgn_upsample2x")
    return out


def gemm_into(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], out: PaddedImage) -> PaddedImage:
    """out = A W^T + bias over every row of the image, border rows included (ops.gemm): they are not zero afterwards."""
    _wrote(out, False)
    ops.gemm(A, W, bias, out.t)
    return out


def _conv_shapes(s, n, co, ci, k):
    s[n + ".weight"], s[n + ".bias"] = (co, ci, k, k), (co,)


def _norm_shapes(s, n, c):
    s[n + ".weight"], s[n + ".bias"] = (c,), (c,)


def _res_shapes(s, n, ci, co):
    _norm_shapes(s, n + ".norm1", ci); _conv_shapes(s, n + ".conv1", co, ci, 3)
    _norm_shapes(s, n + ".norm2", co); _conv_shapes(s, n + ".conv2", co, co, 3)
    if ci != co:
        _conv_shapes(s, n + ".conv_shortcut", co, ci, 1)


def _mid_shapes(s, c):
    _res_shapes(s, "mid_block.resnets.0", c, c); _res_shapes(s, "mid_block.resnets.1", c, c)
    a = "mid_block.attentions.0."
    _norm_shapes(s, a + "group_norm", c)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        s[a + n + ".weight"], s[a + n + ".bias"] = (c, c), (c,)


def decoder_param_shapes(block_out_channels=(128, 256, 512, 512), latent_channels: int = 16, layers_per_block: int = 2):
    """Parameter names and shapes of the [EXT] AutoencoderKL decoder (diffusers state-dict layout) - for synthetic weights (bench.py,
    tools): a real checkpoint's `vae.decoder.state_dict()` has exactly these entries."""
    ch = list(reversed(block_out_channels))
    s: Dict[str, Tuple[int, ...]] = {}
    _conv_shapes(s, "conv_in", ch[0], latent_channels, 3)
    _mid_shapes(s, ch[0])
    cin = ch[0]
    for i, co in enumerate(ch):
        for j in range(layers_per_block + 1):
            _res_shapes(s, f"up_blocks.{i}.resnets.{j}", cin if j == 0 else co, co)
        if i < len(ch) - 1:
            _conv_shapes(s, f"up_blocks.{i}.upsamplers.0.conv", co, co, 3)
        cin = co
    _norm_shapes(s, "conv_norm_out", cin)
    _conv_shapes(s, "conv_out", 3, cin, 3)
    return s


def encoder_param_shapes(block_out_channels=(128, 256, 512, 512), latent_channels: int = 16, layers_per_block: int = 2):
    """The same for the encoder (`vae.encoder.state_dict()`)."""
    ch = list(block_out_channels)
    s: Dict[str, Tuple[int, ...]] = {}
    _conv_shapes(s, "conv_in", ch[0], 3, 3)
    cin = ch[0]
    for i, co in enumerate(ch):
        for j in range(layers_per_block):
            _res_shapes(s, f"down_blocks.{i}.resnets.{j}", cin if j == 0 else co, co)
        if i < len(ch) - 1:
            _conv_shapes(s, f"down_blocks.{i}.downsamplers.0.conv", co, co, 3)
        cin = co
    _mid_shapes(s, cin)
    _norm_shapes(s, "conv_norm_out", cin)
    _conv_shapes(s, "conv_out", 2 * latent_channels, cin, 3)
    return s


def synthetic_decoder_state_dict(seed: int = 0, device="cpu", shapes=None, **kw):
    """Seeded weights of that layout: convolutions / linears U(-1, 1) / sqrt(fan_in) (PyTorch's default scale), norm weights 1 + 0.2 N(0, 1).
    `shapes=encoder_param_shapes()` draws an encoder."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, shape in (decoder_param_shapes(**kw) if shapes is None else shapes).items():
        if name.endswith(".bias"):
            sd[name] = 0.1 * torch.randn(shape, generator=g, device=device)
        elif len(shape) == 1:
            sd[name] = 1.0 + 0.2 * torch.randn(shape, generator=g, device=device)
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            sd[name] = (torch.rand(shape, generator=g, device=device) * 2 - 1) / math.sqrt(fan_in)
    return sd


def conv_s2(x: PaddedImage, cw: "ConvWeights", out: PaddedImage, rows_table: torch.Tensor):
    """The encoder's downsampler: 3 x 3, stride 2, F.pad (0, 1, 0, 1) (rgn_conv_s2_bf16); `rows_table` = downsample_rows(x, out)."""
    if cw.cin != x.C or out.C != cw.ldy or cw.group != 1 or cw.taps != 9 or out.H * 2 != x.H or out.W * 2 != x.W:
        raise _lib.RegionEHipError(f"conv_s2: weights for {cw.cin} -> {cw.cout} on {x.H} x {x.W} x {x.C} -> {out.H} x {out.W} x {out.C}")
    _need_zero_border(out, "conv_s2")                    # the launch does not write its output's border rows
    _wrote(out, True)
    rc = _lib.lib().rgn_conv_s2_bf16(x.ptr(), _p(cw.w), _p(cw.b), out.ptr(), out.C, x.Hp, x.Wp, x.C, cw.cout, _p(rows_table), _stream())
    _lib.check(rc, "rgn_conv_s2_bf16")
    return out


class UpConvWeights:
    """`upsamplers.0.conv` for rgn_conv_up2_bf16: the four phase matrices [4][Cout, 2, 2, Cin] with the taps a low-resolution pixel is seen
    through summed (in fp32, then rounded to bf16 once).  `w4`: [Cout, 3, 3, Cin] fp32."""

    def __init__(self, w4: torch.Tensor, bias: torch.Tensor):
        co, kh, kw, ci = w4.shape
        assert kh == 3 and kw == 3
        self.cout, self.cin = co, ci
        fold = ([[0], [1, 2]], [[0, 1], [2]])                    # phase 0: window rows (y - 1, y) <- taps (0), (1, 2); phase 1: (y, y + 1) <- (0, 1), (2)
        mats = []
        for a in range(2):
            for b in range(2):
                t = torch.zeros((co, 2, 2, ci), dtype=torch.float32, device=w4.device)
                for r in range(2):
                    for c in range(2):
                        for ky in fold[a][r]:
                            for kx in fold[b][c]:
                                t[:, r, c, :] += w4[:, ky, kx, :]
                mats.append(t.reshape(co, -1))
        self.w = torch.stack(mats).to(torch.bfloat16).contiguous()
        self.b = bias.to(w4.device, torch.bfloat16).contiguous()


def upsample_rows(H: int, W: int, device) -> torch.Tensor:
    """rgn_conv_up2_bf16's row tables [4][(H + 2) * (W + 2)] for an H x W low-resolution image: low-resolution padded pixel (py, px), phase
    (a, b) -> padded row of pixel (2 (py - 1) + a, 2 (px - 1) + b) of the (2H + 2) x (2W + 2) image; border pixels -> the first guard row
    behind that image.  Built once per size (setup)."""
    Hp, Wp, Wq = H + 2, W + 2, 2 * W + 2
    m = torch.arange(Hp * Wp, dtype=torch.int64, device=device)
    py, px = m // Wp, m % Wp
    ok = (py >= 1) & (py <= H) & (px >= 1) & (px <= W)
    scratch = (2 * H + 2) * Wq
    out = []
    for a in range(2):
        for b in range(2):
            row = (2 * (py - 1) + a + 1) * Wq + 2 * (px - 1) + b + 1
            out.append(torch.where(ok, row, torch.full_like(row, scratch)))
    return torch.stack(out).contiguous()


def conv_up2(x: PaddedImage, uw: UpConvWeights, out: PaddedImage, rows_table: torch.Tensor, gn: bool = False):
    """out = conv3x3(upsample2x(x)) + bias without the upsampled image (rgn_conv_up2_bf16); `rows_table` = upsample_rows(x.H, x.W)."""
    if uw.cin != x.C or out.C != uw.cout or out.H != 2 * x.H or out.W != 2 * x.W:
        raise _lib.RegionEHipError(f"conv_up2: weights for {uw.cin} -> {uw.cout} on {x.H} x {x.W} x {x.C} -> {out.H} x {out.W} x {out.C}")
    _need_zero_border(out, "conv_up2")                   # the launch does not write its output's border rows
    nblk, ws = ctypes.c_int(0), None
    _wrote(out, True)
    if gn:
        lane = _handoff(x.t.device)
        lane.set(None)
        ws = lane.workspace(x.t.device)
    rc = _lib.lib().rgn_conv_up2_bf16(x.ptr(), _p(uw.w), _p(uw.b), out.ptr(), out.C, x.Hp, x.Wp, x.C, uw.cout, _p(rows_table), _p(ws),
                                      ctypes.byref(nblk) if gn else None, _stream())
    _lib.check(rc, "rgn_conv_up2_bf16")
    if gn:
        lane.set(out, nblk.value)
    return out


def downsample_rows(H: int, W: int, device) -> torch.Tensor:
    """rgn_conv_s2_bf16's row table for an H x W input (padded pitch W + 2): GEMM row m = yo * (W + 2) + xo -> padded row of output pixel
    (yo, xo) in the (H / 2 + 2) x (W / 2 + 2) image, or - for the unused columns xo >= W / 2 of the wide grid - the first guard row behind
    the output image: the scratch row.  It receives real convolution values from many GEMM rows (the last store wins) and is never read by
    a group = 1, 1 x 1, stride-2 or upsampling launch; a 3 x 3 PIXEL-GROUP launch on that image would add it, times zero, into the last
    image row (PaddedImage), which is harmless while it is finite and the reason not to chain the two without clearing it.  Built once per
    size (setup, not on the decode / encode path)."""
    Wp, Ho, Wo = W + 2, H // 2, W // 2
    m = torch.arange(Ho * Wp, dtype=torch.int64, device=device)
    yo, xo = m // Wp, m % Wp
    row = (yo + 1) * (Wo + 2) + xo + 1
    return torch.where(xo < Wo, row, torch.full_like(row, (Ho + 2) * (Wo + 2))).contiguous()


def _res_flops(p, ci, co):
    """Algorithmic FLOPs of one ResNet block over p pixels: 2 * pixels * Cout * taps * Cin per convolution (the shortcut where ci != co)."""
    return 2.0 * p * (9 * ci * co + 9 * co * co + (ci * co if ci != co else 0))


def _mid_flops(p, c):
    """The mid block: two ResNets, the four attention projections, Q K^T and P V."""
    return 2 * _res_flops(p, c, c) + 2.0 * p * c * c * 4 + 4.0 * p * p * c


def _levels_flops(p, levels, nres, scale, up_flops):
    """(FLOPs, pixels behind the last level) of levels [(cin, cout, resample)] of nres ResNets each from p pixels; a resampling level
    multiplies the pixels by `scale` and adds up_flops(pixels behind it, cout)."""
    f = 0.0
    for cin, co, resample in levels:
        f += _res_flops(p, cin, co) + (nres - 1) * _res_flops(p, co, co)
        if resample:
            p = int(p * scale)
            f += up_flops(p, co)
    return f, p


class _KLBase:
    """Parameter adoption and the forward steps shared by the decoders and the encoders of both VAE families (qwen_vae.py derives from it)."""

    def _init_params(self, state_dict, device, prefix, pixel_groups):
        self.device = torch.device(device)
        self._sd = {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in state_dict.items()}
        self.p: Dict[str, torch.Tensor] = {}
        self.c: Dict[str, ConvWeights] = {}
        self.u: Dict[str, UpConvWeights] = {}
        self.pixel_groups = pixel_groups
        self.fuse_gn = True              # GroupNorm statistics in the producing convolution's epilogue (False: the standalone statistics pass)
        self.fuse_upsample = True        # nearest 2 x upsample folded into its convolution (rgn_conv_up2_bf16); False: upsample pass + 3 x 3
        self.attention = "auto"          # mid-block attention: "auto" | "fused" | "materialized" (attention_path)
        self._v_conv = None              # to_v as a 1 x 1 convolution (bias-free: b_v is added by the fused kernel), built at first use
        self.pool = _Pool(self.device)
        self._attn_buf = {}
        self._rows = {}                  # (kind, H, W) -> row table of the resampling convolutions, built at first use

    def _done(self, what, ignore=()):
        unused = [k for k in self._sd if not k.startswith(tuple(ignore))]
        if unused:
            raise _lib.RegionEHipError(f"{what}: state dict entries it does not know: {unused[:6]}")
        del self._sd

    def _attention(self, a, top):
        self._vec(a + "group_norm.weight"); self._vec(a + "group_norm.bias")
        for n in ("to_q", "to_k", "to_out.0"):
            self._conv(a + n)
        self.p[a + "to_v.weight"] = self._take(a + "to_v.weight").reshape(top, top).to(self.device, torch.bfloat16).contiguous()
        self._vec(a + "to_v.bias")

    # -- parameter adoption -------------------------------------------------------------------------------------------------------
    def _take(self, name):
        if name not in self._sd:
            raise _lib.RegionEHipError(f"{type(self).__name__}: parameter {name} missing from the state dict")
        return self._sd.pop(name)

    def _vec(self, name):
        self.p[name] = self._take(name).to(self.device, torch.bfloat16).contiguous()

    def _conv(self, prefix, pad_in: Optional[int] = None, ldy: Optional[int] = None, groups: bool = True):
        """groups = False: a convolution that stores through a row table (the stride-2 launch) takes no pixel groups."""
        w = self._take(prefix + ".weight").to(self.device, torch.float32)          # [Cout, Cin, kh, kw] (or [Cout, Cin]: a Linear)
        if w.dim() == 2:
            w = w[:, :, None, None]
        co, ci, kh, kw = w.shape
        w = w.permute(0, 2, 3, 1)                                                  # [Cout, kh, kw, Cin]
        if pad_in is not None and ci < pad_in:
            w = torch.nn.functional.pad(w, (0, pad_in - ci))
        # narrow outputs fill the 256-wide MFMA tile through pixel groups: 128 channels -> 2 pixels per GEMM row, the RGB head -> 8
        group = 2 if co == 128 else (8 if co <= 8 else 1)
        self.c[prefix] = ConvWeights(w, self._take(prefix + ".bias"), group=group if self.pixel_groups and groups else 1, ldy=ldy)

    def _resnet(self, prefix):
        for n in ("norm1", "norm2"):
            self._vec(f"{prefix}.{n}.weight"); self._vec(f"{prefix}.{n}.bias")
        self._conv(prefix + ".conv1"); self._conv(prefix + ".conv2")
        if prefix + ".conv_shortcut.weight" in self._sd:
            self._conv(prefix + ".conv_shortcut")

    def _kl_widths(self, block_out_channels):
        self.ch = tuple(block_out_channels)
        for c in self.ch:
            if c not in (128, 256, 512):
                raise _lib.RegionEHipError(f"{type(self).__name__}: block width {c} (the kernels cover 128 / 256 / 512 channels)")

    def _kl_mid(self):
        for r in (0, 1):
            self._resnet(f"mid_block.resnets.{r}")
        self._attention("mid_block.attentions.0.", self.ch[-1])

    # -- forward steps ------------------------------------------------------------------------------------------------------------
    _attn_norm = "group_norm"

    def _load(self, x: torch.Tensor, C: int, H: int, W: int) -> PaddedImage:
        """NCHW bf16 [1, C, H, W] -> a pooled 64-channel padded image (channels past C and the border zero)."""
        img = self.pool.get(H, W, 64)
        _wrote(img, True)
        _lib.check(_lib.lib().rgn_nchw_to_padded(_p(x), img.ptr(), C, H, W, 64, _stream()), "rgn_nchw_to_padded")
        return img

    def _conv_to(self, x: PaddedImage, name: str, cout: int, gn: bool = False) -> PaddedImage:
        """conv `name` of x into a pooled image of cout channels; x goes back to the pool."""
        y = conv(x, self.c[name], self.pool.get(x.H, x.W, cout), gn=gn)
        self.pool.put(x)
        return y

    def _norm(self, x: PaddedImage, name: str, out: PaddedImage, silu: bool = True) -> PaddedImage:
        return groupnorm_silu(x, self.p[name + ".weight"], self.p[name + ".bias"], out, silu=silu, eps=self.eps)

    def _run_resnet(self, x: PaddedImage, prefix: str, cout: int) -> PaddedImage:
        Cv, pool = self.c, self.pool
        n = self._norm(x, prefix + ".norm1", pool.get(x.H, x.W, x.C))
        h = conv(n, Cv[prefix + ".conv1"], pool.get(x.H, x.W, cout), gn=self.fuse_gn)
        pool.put(n)
        n2 = self._norm(h, prefix + ".norm2", pool.get(x.H, x.W, cout))
        skip = x
        if prefix + ".conv_shortcut" in Cv:
            skip = conv(x, Cv[prefix + ".conv_shortcut"], pool.get(x.H, x.W, cout))
        conv(n2, Cv[prefix + ".conv2"], h, resid=skip, gn=self.fuse_gn)      # h is not an input of this launch; every ResNet output feeds a GroupNorm
        pool.put(n2)
        if skip is not x:
            pool.put(skip)
        pool.put(x)
        return h

    def _run_attention(self, x: PaddedImage) -> PaddedImage:
        """One head of width C over every pixel (diffusers `Attention`, residual_connection=True): three GEMMs + a row softmax, or - with Q, K,
        V as 1 x 1 convolutions - one rgn_vae_attention_bf16 launch and no score matrix in memory (attention_path).  The border pixels of the
        padded image are masked out as keys; as outputs the P V GEMM writes them (`o.border_zero` turns false: o must be rewritten before
        anything relies on its border) and the last projection's epilogue zeroes them in `out`."""
        P, Cv, pool, a = self.p, self.c, self.pool, "mid_block.attentions.0."
        C, rows = x.C, x.rows
        fused = attention_path(self.attention, rows) == "fused"
        if fused and self._v_conv is None:
            self._v_conv = ConvWeights(P[a + "to_v.weight"].float().reshape(C, 1, 1, C), torch.zeros(C, device=self.device))
        if not fused:
            ldp = ops.padded(rows, 64)
            if (rows, C) not in self._attn_buf:
                self._attn_buf[(rows, C)] = (torch.zeros((rows, ldp), dtype=torch.bfloat16, device=self.device),       # S / P
                                             torch.zeros((C, ldp), dtype=torch.bfloat16, device=self.device))          # V^T (padding columns stay 0)
            S, vt = self._attn_buf[(rows, C)]
        n = self._norm(x, a + self._attn_norm, pool.get(x.H, x.W, C), silu=False)
        q = conv(n, Cv[a + "to_q"], pool.get(x.H, x.W, C))
        k = conv(n, Cv[a + "to_k"], pool.get(x.H, x.W, C))
        o, v = q, None                                                            # q is dead once read: O = P V + b_v overwrites it
        if fused:
            v = conv(n, self._v_conv, pool.get(x.H, x.W, C))
            _wrote(o, o.border_zero)                                              # the launch does not write O's border rows: q's stay
            _lib.check(_lib.lib().rgn_vae_attention_bf16(q.ptr(), k.ptr(), v.ptr(), _p(P[a + "to_v.bias"]), o.ptr(), x.Hp, x.Wp, C,
                                                         1.0 / math.sqrt(C), _stream()), "rgn_vae_attention_bf16")
        else:
            ops.gemm(P[a + "to_v.weight"], n.t, None, vt[:, :rows])              # V^T = W_v X^T; b_v is added behind P V (rows of P sum to 1)
            ops.gemm(q.t, k.t, None, S[:, :rows])                                 # S = Q K^T
            _lib.check(_lib.lib().rgn_softmax_rows(_p(S), ldp, x.Hp, x.Wp, 1.0 / math.sqrt(C), _stream()), "rgn_softmax_rows")
            gemm_into(S, vt, P[a + "to_v.bias"], o)
        out = conv(o, Cv[a + "to_out.0"], k, resid=x, gn=self.fuse_gn)           # k is dead; a 1 x 1 convolution: o's border rows meet nobody
        pool.put(n); pool.put(o)
        if v is not None:
            pool.put(v)
        pool.put(x)
        return out

    def _run_mid(self, x: PaddedImage, c: int) -> PaddedImage:
        x = self._run_resnet(x, "mid_block.resnets.0", c)
        x = self._run_attention(x)
        return self._run_resnet(x, "mid_block.resnets.1", c)

    def _row_table(self, kind: str, H: int, W: int) -> torch.Tensor:
        key = (kind, H, W)
        if key not in self._rows:
            self._rows[key] = (upsample_rows if kind == "up" else downsample_rows)(H, W, self.device)
        return self._rows[key]

    def _up(self, x: PaddedImage, name: str, cout: int) -> PaddedImage:
        """Nearest 2 x upsample + the 3 x 3 convolution `name`: one launch (weights self.u), or the two passes (weights self.c)."""
        if self.fuse_upsample:
            y = conv_up2(x, self.u[name], self.pool.get(2 * x.H, 2 * x.W, cout), self._row_table("up", x.H, x.W), gn=self.fuse_gn)
            self.pool.put(x)
            return y
        u = upsample2x(x, self.pool.get(2 * x.H, 2 * x.W, x.C))
        self.pool.put(x)
        return self._conv_to(u, name, cout, gn=self.fuse_gn)

    def _down(self, x: PaddedImage, name: str) -> PaddedImage:
        d = conv_s2(x, self.c[name], self.pool.get(x.H // 2, x.W // 2, x.C), self._row_table("down", x.H, x.W))
        self.pool.put(x)
        return d

    def _head(self, x: PaddedImage, norm: str, cout: int) -> PaddedImage:
        n = self._norm(x, norm, self.pool.get(x.H, x.W, x.C))
        self.pool.put(x)
        return self._conv_to(n, "conv_out", cout)

    def _to_host(self, y: PaddedImage, c: int) -> torch.Tensor:
        out = torch.empty((1, c, y.H, y.W), dtype=torch.bfloat16, device=self.device)
        _lib.check(_lib.lib().rgn_padded_to_nchw(y.ptr(), y.C, _p(out), c, y.H, y.W, _stream()), "rgn_padded_to_nchw")
        self.pool.put(y)
        return out

    def _to_u8(self, y: PaddedImage) -> torch.Tensor:
        """The decoded image's channels 0..2 as uint8 [H, W, 3]: the host's `postprocess` arithmetic (rgn_image_bf16_to_u8)."""
        out = torch.empty((y.H, y.W, 3), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().rgn_image_bf16_to_u8(y.ptr(), 0, y.C, _p(out), y.H, y.W, _stream()), "rgn_image_bf16_to_u8")
        self.pool.put(y)
        return out


class HipVaeDecoder(_KLBase):
    """AutoencoderKL decoder ([EXT] diffusers layout) on libregione_hip.so.  `decode(z)`: z [1, Cz, h, w] -> image [1, 3, 8h, 8w] bf16."""

    def __init__(self, state_dict, device, block_out_channels=(128, 256, 512, 512), latent_channels: int = 16, layers_per_block: int = 2,
                 norm_eps: float = 1e-6, pixel_groups: bool = True):
        self._kl_widths(block_out_channels)
        self.zc, self.nres, self.eps = latent_channels, layers_per_block + 1, norm_eps
        self._init_params(state_dict, device, "decoder.", pixel_groups)
        self._conv("conv_in", pad_in=64)
        self._kl_mid()
        cin = self.ch[-1]
        self.levels = []
        for i, co in enumerate(reversed(self.ch)):
            for j in range(self.nres):
                self._resnet(f"up_blocks.{i}.resnets.{j}")
            up = i < len(self.ch) - 1
            if up:
                n = f"up_blocks.{i}.upsamplers.0.conv"
                w = self._sd[n + ".weight"].to(self.device, torch.float32).permute(0, 2, 3, 1)
                self.u[n] = UpConvWeights(w, self._sd[n + ".bias"])          # the fused upsample + convolution (four 2 x 2 phases)
                self._conv(n)                                               # and the plain form (fuse_upsample = False)
            self.levels.append((cin, co, up))
            cin = co
        self._vec("conv_norm_out.weight"); self._vec("conv_norm_out.bias")
        self._conv("conv_out", ldy=8)
        if any(k.startswith("post_quant_conv") for k in self._sd):
            raise _lib.RegionEHipError("HipVaeDecoder: post_quant_conv is not part of the FLUX.1 / Step1X-Edit VAE (use_post_quant_conv = False)")
        self._done("HipVaeDecoder", ignore=("encoder.", "quant_conv"))

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return self._to_host(self._forward(z, "decode"), 3)

    @torch.no_grad()
    def decode_u8(self, z: torch.Tensor) -> torch.Tensor:
        """The same forward, ending in the bytes of the host's `postprocess(decode(z), "pil")`: uint8 [8h, 8w, 3] on the device."""
        return self._to_u8(self._forward(z, "decode_u8"))

    def _forward(self, z: torch.Tensor, who: str) -> PaddedImage:
        if not z.is_cuda or z.dim() != 4 or z.shape[0] != 1 or z.shape[1] != self.zc:
            raise _lib.RegionEHipError(f"HipVaeDecoder.{who}: one latent image [1, {self.zc}, h, w] on the GPU, got {tuple(z.shape)} on {z.device}")
        h, w = z.shape[2], z.shape[3]
        check_image_size(8 * h, 8 * w, f"HipVaeDecoder.{who}")
        top = self.ch[-1]
        x = self._conv_to(self._load(z.to(torch.bfloat16).contiguous(), self.zc, h, w), "conv_in", top, gn=self.fuse_gn)
        x = self._run_mid(x, top)
        for i, (cin, co, up) in enumerate(self.levels):
            for j in range(self.nres):
                x = self._run_resnet(x, f"up_blocks.{i}.resnets.{j}", co)
            if up:
                x = self._up(x, f"up_blocks.{i}.upsamplers.0.conv", co)
        return self._head(x, "conv_norm_out", 8)

    def flops(self, h: int, w: int) -> float:
        """Algorithmic FLOPs of one decode of an h x w latent (2 * valid pixels * Cout * taps * Cin per convolution + the attention GEMMs)."""
        top, px = self.ch[-1], h * w
        f, full = _levels_flops(px, self.levels, self.nres, 4, lambda p, co: 2.0 * p * 9 * co * co)
        return 2.0 * px * top * 9 * self.zc + _mid_flops(px, top) + f + 2.0 * full * 9 * self.ch[0] * 3


class LatentDist:
    """`vae.encode(x).latent_dist` of diffusers' AutoencoderKL (DiagonalGaussianDistribution) over the HIP encoder's moments: what the host's
    `retrieve_latents(encoder_output, generator, sample_mode)` reads - `.mode()` (FLUX.1-Kontext: sample_mode = "argmax") and `.sample()`."""

    def __init__(self, moments: torch.Tensor):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar.float(), -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar).to(moments.dtype)

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device if generator is None else generator.device,
                            dtype=torch.float32).to(self.mean.device, self.mean.dtype)
        return self.mean + self.std * noise


class EncoderOutput:
    def __init__(self, moments):
        self.latent_dist = LatentDist(moments)


class HipVaeEncoder(_KLBase):
    """AutoencoderKL encoder ([EXT] diffusers layout: conv_in, four down levels of two ResNet blocks (128, 256, 512, 512; a stride-2 3 x 3
    convolution with F.pad (0, 1, 0, 1) after the first three), the mid block, GroupNorm + SiLU + conv_out to 2 x latent channels; no
    quant_conv in the FLUX.1 / Step1X-Edit VAE) on libregione_hip.so - the VAE encode of the condition image the host's `prepare_latents`
    runs before the loop (reference call site FluxKontext/inplace.py:210-226).  `encode(x)`: image [1, 3, H, W] (H, W multiples of 8) ->
    moments [1, 2 Cz, H / 8, W / 8] bf16; `encode_dist(x)` wraps them as `vae.encode(x)` does (`.latent_dist.mode() / .sample()`)."""

    def __init__(self, state_dict, device, block_out_channels=(128, 256, 512, 512), latent_channels: int = 16, layers_per_block: int = 2,
                 norm_eps: float = 1e-6, pixel_groups: bool = True):
        self._kl_widths(block_out_channels)
        self.zc, self.nres, self.eps = latent_channels, layers_per_block, norm_eps
        self._init_params(state_dict, device, "encoder.", pixel_groups)
        self._conv("conv_in", pad_in=64)
        cin = self.ch[0]
        self.levels = []
        for i, co in enumerate(self.ch):
            for j in range(self.nres):
                self._resnet(f"down_blocks.{i}.resnets.{j}")
            down = i < len(self.ch) - 1
            if down:
                self._conv(f"down_blocks.{i}.downsamplers.0.conv", groups=False)
            self.levels.append((cin, co, down))
            cin = co
        self._kl_mid()
        self._vec("conv_norm_out.weight"); self._vec("conv_norm_out.bias")
        self._conv("conv_out")
        if any(k.startswith("quant_conv") for k in self._sd):
            raise _lib.RegionEHipError("HipVaeEncoder: quant_conv is not part of the FLUX.1 / Step1X-Edit VAE (use_quant_conv = False)")
        self._done("HipVaeEncoder", ignore=("decoder.", "post_quant_conv"))

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 3 or x.shape[2] % 8 or x.shape[3] % 8:
            raise _lib.RegionEHipError(f"HipVaeEncoder.encode: one image [1, 3, H, W] on the GPU, H and W multiples of 8; got {tuple(x.shape)} on {x.device}")
        H, W = x.shape[2], x.shape[3]
        check_image_size(H, W, "HipVaeEncoder.encode")
        h = self._conv_to(self._load(x.to(torch.bfloat16).contiguous(), 3, H, W), "conv_in", self.ch[0], gn=self.fuse_gn)
        for i, (cin, co, down) in enumerate(self.levels):
            for j in range(self.nres):
                h = self._run_resnet(h, f"down_blocks.{i}.resnets.{j}", co)
            if down:
                h = self._down(h, f"down_blocks.{i}.downsamplers.0.conv")
        h = self._run_mid(h, self.ch[-1])
        return self._to_host(self._head(h, "conv_norm_out", 2 * self.zc), 2 * self.zc)

    def encode_dist(self, x: torch.Tensor) -> EncoderOutput:
        return EncoderOutput(self.encode(x))

    def flops(self, H: int, W: int) -> float:
        top, px = self.ch[-1], H * W
        f, low = _levels_flops(px, self.levels, self.nres, 0.25, lambda p, co: 2.0 * p * 9 * co * co)
        return 2.0 * px * self.ch[0] * 9 * 3 + f + _mid_flops(low, top) + 2.0 * low * 9 * top * 2 * self.zc
