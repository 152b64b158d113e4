"""The Qwen-Image VAE (decode and condition-image encode) on the HIP kernels (Qwen-Image-Edit / -Edit-Plus).

The module is the [EXT] `AutoencoderKLQwenImage` of diffusers (the Wan-2.1 3-D causal VAE; config base_dim 96, z_dim 16, dim_mult
(1, 2, 4, 4), num_res_blocks 2, no attention outside the mid block, temperal_downsample (False, True, True)).  The reference only calls
`self.vae.decode` (QwenImageEdit/inplace.py:437-451, QwenImageEditPlus/inplace.py:460-474) and `self.vae.encode` inside the host's
`prepare_latents`; nothing of the VAE lives in /root/reference: [EXT], unpinned, checked against an fp32 PyTorch restatement with the
diffusers parameter names and genuine 3-D causal convolutions (tests/host_qwen_vae.py).

For one image (T = 1, the first and only causal chunk) the module reduces to a 2-D network:
  * a 3 x 3 x 3 `CausalConv3d` pads two zero frames in front, so only its last temporal slice `weight[:, :, -1]` meets the frame: a 3 x 3
    convolution with zero padding 1 (and 1 x 1 x 1 = `weight[:, :, 0]`); the 5-D weights are sliced once at load;
  * the `time_conv` of `upsample3d` / `downsample3d` is skipped on the first chunk: its weights are accepted and unused;
  * `RMS_norm` (gamma, no bias) = x / max(||x||_2, 1e-12) * sqrt(C) * gamma per pixel over the channels: rgn_rms_norm_silu (+ SiLU in every
    ResNet half and in norm_out, without it in the attention block);
  * upsample = nearest 2 x + Conv2d(C, C / 2, 3, pad 1): rgn_conv_up2_bf16; downsample = ZeroPad2d(0, 1, 0, 1) + Conv2d(C, C, 3, stride 2):
    rgn_conv_s2_bf16; the mid-block attention (one head of width C) = the scheme of regione_amd/vae.py with `to_qkv` split into three weights;
  * decode: post_quant_conv (1 x 1, a launch of its own: conv_in's zero padding would see its bias) ... conv_out, clamp(-1, 1) in the
    conversion to the host layout; encode: ... conv_out with quant_conv folded into it (a 1 x 1 behind a convolution: exact).

The 96-channel level is stored at 128 channels (zero weights, bias and gamma in channels 96..127: rgn_conv_bf16 walks K in steps of 64, and
the 128-channel pixel-group path fills the 256-wide MFMA tile); 192 channels fill 3/4 of a 256-wide tile.  Activations are bf16 (fp32
accumulation, one bf16 rounding per launch); the output is converted to the host VAE's dtype (bf16 or fp32) by the last launch.
No CPU / eager fallback inside: a missing library raises RegionEHipError; the adapter (regione_amd.adapters, components.py) decides, before calling,
whether the kernels cover a call and otherwise keeps the host module.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from . import _lib, ops
from .vae import EncoderOutput, PaddedImage, UpConvWeights, _KLBase, _levels_flops, _mid_flops, _wrote, check_image_size

_p, _stream = ops._p, ops._stream

# the configuration the kernels are built for (AutoencoderKLQwenImage of Qwen-Image / -Edit / -Edit-Plus)
QWEN_VAE_CONFIG = dict(base_dim=96, z_dim=16, dim_mult=(1, 2, 4, 4), num_res_blocks=2, attn_scales=(), temperal_downsample=(False, True, True))
SOFTMAX_MAX_ROWS = 24576              # rgn_softmax_rows: (h + 2) (w + 2) of the mid-block image (the adapter's hosted-path threshold)


def cs(c: int) -> int:
    """Stored channels of a level: the row stride rgn_conv_bf16 can walk (a multiple of 64): 96 -> 128."""
    return ops.padded(c, 64)


def qwen_vae_param_shapes(base_dim=96, z_dim=16, dim_mult=(1, 2, 4, 4), num_res_blocks=2, temperal_downsample=(False, True, True)):
    """Parameter names and shapes of the whole [EXT] AutoencoderKLQwenImage (`vae.state_dict()`, diffusers layout)."""
    s: Dict[str, Tuple[int, ...]] = {}

    def conv_(n, co, ci, k):
        s[n + ".weight"], s[n + ".bias"] = (co, ci, k, k, k), (co,)

    def rms_(n, c, images=False):
        s[n + ".gamma"] = (c, 1, 1) if images else (c, 1, 1, 1)

    def res_(n, ci, co):
        rms_(n + ".norm1", ci); conv_(n + ".conv1", co, ci, 3); rms_(n + ".norm2", co); conv_(n + ".conv2", co, co, 3)
        if ci != co:
            conv_(n + ".conv_shortcut", co, ci, 1)

    def mid_(n, c):
        res_(n + ".resnets.0", c, c)
        a = n + ".attentions.0."
        rms_(a + "norm", c, images=True)
        s[a + "to_qkv.weight"], s[a + "to_qkv.bias"] = (3 * c, c, 1, 1), (3 * c,)
        s[a + "proj.weight"], s[a + "proj.bias"] = (c, c, 1, 1), (c,)
        res_(n + ".resnets.1", c, c)
    nlev = len(dim_mult)
    # encoder
    dims = [base_dim * u for u in (1,) + tuple(dim_mult)]
    conv_("encoder.conv_in", dims[0], 3, 3)
    k = 0
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(num_res_blocks):
            res_(f"encoder.down_blocks.{k}", ci, co)
            ci, k = co, k + 1
        if i != nlev - 1:
            n = f"encoder.down_blocks.{k}."
            s[n + "resample.1.weight"], s[n + "resample.1.bias"] = (co, co, 3, 3), (co,)
            if temperal_downsample[i]:
                s[n + "time_conv.weight"], s[n + "time_conv.bias"] = (co, co, 3, 1, 1), (co,)
            k += 1
    mid_("encoder.mid_block", dims[-1])
    rms_("encoder.norm_out", dims[-1])
    conv_("encoder.conv_out", 2 * z_dim, dims[-1], 3)
    conv_("quant_conv", 2 * z_dim, 2 * z_dim, 1)
    conv_("post_quant_conv", z_dim, z_dim, 1)
    # decoder
    dims = [base_dim * u for u in (dim_mult[-1],) + tuple(dim_mult[::-1])]
    up3d = tuple(temperal_downsample[::-1])
    conv_("decoder.conv_in", dims[0], z_dim, 3)
    mid_("decoder.mid_block", dims[0])
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        if i > 0:
            ci //= 2
        for j in range(num_res_blocks + 1):
            res_(f"decoder.up_blocks.{i}.resnets.{j}", ci if j == 0 else co, co)
        if i != nlev - 1:
            n = f"decoder.up_blocks.{i}.upsamplers.0."
            s[n + "resample.1.weight"], s[n + "resample.1.bias"] = (co // 2, co, 3, 3), (co // 2,)
            if up3d[i]:
                s[n + "time_conv.weight"], s[n + "time_conv.bias"] = (2 * co, co, 3, 1, 1), (2 * co,)
    rms_("decoder.norm_out", dims[-1])
    conv_("decoder.conv_out", 3, dims[-1], 3)
    return s


def rms_norm_silu(x: PaddedImage, gamma: torch.Tensor, c_valid: int, out: PaddedImage, silu: bool = True) -> PaddedImage:
    """out = [silu](RMS_norm(x)) over the first c_valid channels (rgn_rms_norm_silu); gamma [x.C] bf16, zero past c_valid."""
    if gamma.numel() != x.C or out.C != x.C or out.rows != x.rows:
        raise _lib.RegionEHipError(f"rms_norm_silu: gamma of {gamma.numel()} channels on images of {x.C} -> {out.C} channels")
    _wrote(out, True)
    _lib.check(_lib.lib().rgn_rms_norm_silu(x.ptr(), out.ptr(), x.Hp, x.Wp, int(c_valid), x.C, _p(gamma), int(silu), _stream()),
               "rgn_rms_norm_silu")
    return out


class _QwenBase(_KLBase):
    """Adoption shared by the decoder and the encoder: strict name / shape check against qwen_vae_param_shapes(), 5-D weights sliced to
    their last temporal slice, channels padded to cs(c); then the KL VAE's blocks (ResNet, mid-block attention) with RMS_norm as the norm."""
    _attn_norm = "norm"
    _part, _top, _other = "", "", ()

    def _adopt(self, state_dict, device, pixel_groups, out_dtype):
        if out_dtype not in (torch.bfloat16, torch.float32):
            raise _lib.RegionEHipError(f"{type(self).__name__}: output dtype {out_dtype} (the kernels store bf16 or fp32)")
        self.out_dtype = out_dtype
        self._init_params({}, device, "", pixel_groups)
        self.fuse_gn = False             # RMS_norm: no GroupNorm statistics in the convolution epilogues
        self.nc: Dict[str, int] = {}     # valid channels of each norm
        own = {}
        for k, v in qwen_vae_param_shapes().items():
            if k.startswith(self._part + "."):
                own[k[len(self._part) + 1:]] = v
            elif k.startswith(self._top + "."):
                own[k] = v
        raw = {}
        for k, v in state_dict.items():
            if k.startswith(self._other):
                continue
            n = k[len(self._part) + 1:] if k.startswith(self._part + ".") else k
            if n not in own:
                raise _lib.RegionEHipError(f"{type(self).__name__}: state dict entry it does not know: {k}")
            if tuple(v.shape) != own[n]:
                raise _lib.RegionEHipError(f"{type(self).__name__}: {k} has shape {tuple(v.shape)}, the kernels' config needs {own[n]}")
            raw[n] = v
        missing = [n for n in own if n not in raw]
        if missing:
            raise _lib.RegionEHipError(f"{type(self).__name__}: parameters missing from the state dict: {missing[:6]}")
        for n in [n for n in raw if ".time_conv." in n]:                 # the first causal chunk skips time_conv
            del raw[n]
        self._raw = raw

    def _w(self, name, ci_p, co_p):
        """Sliced (5-D -> last temporal slice), channel-padded fp32 weight [co_p, ci_p, kh, kw] and bias [co_p] of a raw convolution."""
        w = self._raw.pop(name + ".weight").to(self.device, torch.float32)
        if w.dim() == 5:
            w = w[:, :, -1]
        co, ci = w.shape[:2]
        w = F.pad(w, (0, 0, 0, 0, 0, ci_p - ci, 0, co_p - co))
        b = F.pad(self._raw.pop(name + ".bias").to(self.device, torch.float32), (0, co_p - co))
        return w, b

    def _conv_q(self, name, ci_p, co_p, ldy=None, weights=None, groups=True):
        self._sd[name + ".weight"], self._sd[name + ".bias"] = self._w(name, ci_p, co_p) if weights is None else weights
        self._conv(name, ldy=ldy, groups=groups)

    def _gamma(self, name):
        g = self._raw.pop(name + ".gamma").reshape(-1).to(self.device, torch.float32)
        self.nc[name] = g.numel()
        self.p[name + ".gamma"] = F.pad(g, (0, cs(g.numel()) - g.numel())).to(torch.bfloat16).contiguous()

    def _resnet_q(self, prefix, ci, co):
        self._gamma(prefix + ".norm1"); self._gamma(prefix + ".norm2")
        self._conv_q(prefix + ".conv1", cs(ci), cs(co)); self._conv_q(prefix + ".conv2", cs(co), cs(co))
        if ci != co:
            self._conv_q(prefix + ".conv_shortcut", cs(ci), cs(co))

    def _mid_q(self, c):
        self._resnet_q("mid_block.resnets.0", c, c)
        a = "mid_block.attentions.0."
        self._gamma(a + "norm")
        w, b = self._w(a + "to_qkv", c, 3 * c)
        for i, n in enumerate(("to_q", "to_k", "to_v")):
            self._sd[a + n + ".weight"], self._sd[a + n + ".bias"] = w[i * c:(i + 1) * c], b[i * c:(i + 1) * c]
        self._conv(a + "to_q"); self._conv(a + "to_k")
        self.p[a + "to_v.weight"] = self._sd.pop(a + "to_v.weight").reshape(c, c).to(torch.bfloat16).contiguous()
        self.p[a + "to_v.bias"] = self._sd.pop(a + "to_v.bias").to(torch.bfloat16).contiguous()
        w, b = self._w(a + "proj", c, c)
        self._conv_q(a + "to_out.0", c, c, weights=(w, b))
        self._resnet_q("mid_block.resnets.1", c, c)

    def _finish(self):
        if self._raw:
            raise _lib.RegionEHipError(f"{type(self).__name__}: parameters left unused: {list(self._raw)[:6]}")
        del self._raw
        self._done(type(self).__name__)

    def _norm(self, x, name, out, silu=True):
        return rms_norm_silu(x, self.p[name + ".gamma"], self.nc[name], out, silu)

    def _to_host(self, y: PaddedImage, c: int, clamp: bool = False) -> torch.Tensor:
        out = torch.empty((1, c, 1, y.H, y.W), dtype=self.out_dtype, device=self.device)
        _lib.check(_lib.lib().rgn_padded_to_nchw_cvt(y.ptr(), y.C, _p(out), c, y.H, y.W, int(clamp), int(self.out_dtype == torch.float32),
                                                     _stream()), "rgn_padded_to_nchw_cvt")
        self.pool.put(y)
        return out


class HipQwenVaeDecoder(_QwenBase):
    """AutoencoderKLQwenImage decode of one frame on libregione_hip.so.  `decode(z)`: z [1, 16, 1, h, w] -> image [1, 3, 1, 8h, 8w] in
    `out_dtype`, clamped to [-1, 1] (`vae.decode(z).sample` of the module)."""
    _part, _top, _other = "decoder", "post_quant_conv", ("encoder.", "quant_conv.")

    def __init__(self, state_dict, device, out_dtype=torch.bfloat16, pixel_groups: bool = True):
        self._adopt(state_dict, device, pixel_groups, out_dtype)
        c = QWEN_VAE_CONFIG
        self.zc, self.nres = c["z_dim"], c["num_res_blocks"] + 1
        dm = c["dim_mult"]
        dims = [c["base_dim"] * u for u in (dm[-1],) + tuple(dm[::-1])]
        self.top = dims[0]
        self._conv_q("post_quant_conv", 64, 64)
        self._conv_q("conv_in", 64, cs(self.top))
        self._mid_q(self.top)
        self.levels = []
        for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
            ci = ci // 2 if i > 0 else ci
            for j in range(self.nres):
                self._resnet_q(f"up_blocks.{i}.resnets.{j}", ci if j == 0 else co, co)
            up = i != len(dm) - 1
            if up:
                n = f"up_blocks.{i}.upsamplers.0.resample.1"
                w, b = self._w(n, cs(co), cs(co // 2))
                self.u[n] = UpConvWeights(w.permute(0, 2, 3, 1), b)
            self.levels.append((ci, co, up))
        self._gamma("norm_out")
        self._conv_q("conv_out", cs(dims[-1]), 3, ldy=8)
        self._finish()

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return self._to_host(self._forward(z, "decode"), 3, clamp=True)

    @torch.no_grad()
    def decode_u8(self, z: torch.Tensor) -> torch.Tensor:
        """The same forward, ending in the bytes of the host's `postprocess(decode(z)[:, :, 0], "pil")`: uint8 [8h, 8w, 3] on the device.
        decode()'s clamp to [-1, 1] needs no launch here: `x * 0.5 + 0.5` is monotone through its bf16 roundings and sends -1 to 0 and 1 to
        1, so the byte map's own clamp to [0, 1] gives every value beyond +-1 the byte the clamped value gets."""
        if self.out_dtype != torch.bfloat16:
            raise _lib.RegionEHipError(f"HipQwenVaeDecoder.decode_u8: out_dtype {self.out_dtype} (the host's bf16 postprocess arithmetic is covered)")
        return self._to_u8(self._forward(z, "decode_u8"))

    def _forward(self, z: torch.Tensor, who: str):
        if not z.is_cuda or z.dim() != 5 or z.shape[0] != 1 or z.shape[1] != self.zc or z.shape[2] != 1:
            raise _lib.RegionEHipError(f"HipQwenVaeDecoder.{who}: one latent frame [1, {self.zc}, 1, h, w] on the GPU, got {tuple(z.shape)} on {z.device}")
        h, w = z.shape[3], z.shape[4]
        check_image_size(8 * h, 8 * w, f"HipQwenVaeDecoder.{who}")
        top = cs(self.top)
        zq = self._conv_to(self._load(z[:, :, 0].to(torch.bfloat16).contiguous(), self.zc, h, w), "post_quant_conv", 64)
        x = self._run_mid(self._conv_to(zq, "conv_in", top), top)
        for i, (ci, co, up) in enumerate(self.levels):
            for j in range(self.nres):
                x = self._run_resnet(x, f"up_blocks.{i}.resnets.{j}", cs(co))
            if up:
                x = self._up(x, f"up_blocks.{i}.upsamplers.0.resample.1", cs(co // 2))
        return self._head(x, "norm_out", 8)

    def flops(self, h: int, w: int) -> float:
        """Algorithmic FLOPs of one decode of an h x w latent frame as the 2-D network (valid channels; no padding, no time taps)."""
        px = h * w
        f, full = _levels_flops(px, self.levels, self.nres, 4, lambda p, co: 2.0 * p * 9 * co * (co // 2))
        return 2.0 * px * self.zc * self.zc + 2.0 * px * 9 * self.zc * self.top + _mid_flops(px, self.top) + f + 2.0 * full * 9 * self.levels[-1][1] * 3


class HipQwenVaeEncoder(_QwenBase):
    """AutoencoderKLQwenImage encode of one frame on libregione_hip.so (the condition images of Qwen-Image-Edit / -Edit-Plus, inside the host's
    `prepare_latents`).  `encode(x)`: image [1, 3, 1, H, W] (H, W multiples of 8) -> moments [1, 32, 1, H / 8, W / 8] (quant_conv applied)
    in `out_dtype`; `encode_dist(x)` wraps them as `vae.encode(x)` does (`.latent_dist.mode()` = channels [0, 16))."""
    _part, _top, _other = "encoder", "quant_conv", ("decoder.", "post_quant_conv.")

    def __init__(self, state_dict, device, out_dtype=torch.bfloat16, pixel_groups: bool = True):
        self._adopt(state_dict, device, pixel_groups, out_dtype)
        c = QWEN_VAE_CONFIG
        self.zc = c["z_dim"]
        dims = [c["base_dim"] * u for u in (1,) + tuple(c["dim_mult"])]
        self.c0, self.top = dims[0], dims[-1]
        self._conv_q("conv_in", 64, cs(dims[0]))
        self.levels = []                 # (list of ResNet prefixes, downsampler name or None, stored output channels)
        k = 0
        for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
            res = []
            for _ in range(c["num_res_blocks"]):
                self._resnet_q(f"down_blocks.{k}", ci, co)
                res.append(f"down_blocks.{k}")
                ci, k = co, k + 1
            down = None
            if i != len(c["dim_mult"]) - 1:
                down = f"down_blocks.{k}.resample.1"
                self._conv_q(down, cs(co), cs(co), groups=False)
                k += 1
            self.levels.append((res, down, cs(co), ci))
        self._mid_q(self.top)
        self._gamma("norm_out")
        wo, bo = self._w("conv_out", cs(self.top), 2 * self.zc)              # quant_conv (1 x 1) folded into conv_out, in fp32
        wq, bq = self._w("quant_conv", 2 * self.zc, 2 * self.zc)
        wq = wq[:, :, 0, 0]
        self._conv_q("conv_out", cs(self.top), 2 * self.zc, weights=(torch.einsum("oc,cikl->oikl", wq, wo), wq @ bo + bq))
        self._finish()

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda or x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 3 or x.shape[2] != 1 or x.shape[3] % 8 or x.shape[4] % 8:
            raise _lib.RegionEHipError(f"HipQwenVaeEncoder.encode: one frame [1, 3, 1, H, W] on the GPU, H and W multiples of 8; got {tuple(x.shape)} on {x.device}")
        H, W = x.shape[3], x.shape[4]
        check_image_size(H, W, "HipQwenVaeEncoder.encode")
        h = self._conv_to(self._load(x[:, :, 0].to(torch.bfloat16).contiguous(), 3, H, W), "conv_in", cs(self.c0))
        for res, down, co, _ in self.levels:
            for r in res:
                h = self._run_resnet(h, r, co)
            if down is not None:
                h = self._down(h, down)
        h = self._run_mid(h, self.top)
        return self._to_host(self._head(h, "norm_out", 2 * self.zc), 2 * self.zc)

    def encode_dist(self, x: torch.Tensor) -> EncoderOutput:
        return EncoderOutput(self.encode(x))

    def flops(self, H: int, W: int) -> float:
        px, c, z2 = H * W, QWEN_VAE_CONFIG, 2 * self.zc
        dims = [c["base_dim"] * u for u in (1,) + tuple(c["dim_mult"])]
        levels = [(ci, co, i != len(dims) - 2) for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:]))]
        f, low = _levels_flops(px, levels, c["num_res_blocks"], 0.25, lambda p, co: 2.0 * p * 9 * co * co)
        return 2.0 * px * 9 * 3 * dims[0] + f + _mid_flops(low, self.top) + 2.0 * low * 9 * self.top * z2 + 2.0 * low * z2 * z2
