"""A PyTorch restatement of the [EXT] `AutoencoderKLQwenImage` of the public Qwen-Image / -Edit / -Edit-Plus checkpoints (the Wan-2.1 3-D
causal VAE; diffusers layout and parameter names) - the checker of regione_amd/qwen_vae.py (test infrastructure; `diffusers` is not
installable in this image, and nothing of the VAE lives in /root/reference: the reference only CALLS `self.vae.decode` / `self.vae.encode`).

Semantics restated from the public diffusers sources, for the first causal chunk of a clip (an image: T = 1):
  * CausalConv3d: a Conv3d whose time padding (2 p_t frames) sits in front of the clip; with no cached frames (the first chunk) those are
    zero frames.  The convolutions here ARE 3-D, so the tests pin the single-frame reduction (only weight[:, :, -1] meets the frame)
    instead of assuming it;
  * RMS_norm (channel-first, bias=False): F.normalize(x, dim=1) * sqrt(C) * gamma;
  * ResidualBlock: shortcut(x) + conv2(silu(norm2(conv1(silu(norm1(x)))))) (1 x 1 x 1 conv_shortcut when the width changes);
  * AttentionBlock (mid block only): per frame, RMS_norm (images=True), to_qkv (Conv2d C -> 3C), one head of width C, proj, + identity;
  * Resample: upsample2d / upsample3d = nearest 2 x + Conv2d(C, C / 2, 3, pad 1); downsample2d / downsample3d = ZeroPad2d(0, 1, 0, 1) +
    Conv2d(C, C, 3, stride 2); the `time_conv` of the *3d modes is skipped on the first chunk (its weights exist, unused for an image);
  * the VAE: encode = encoder(x[:, :, :1]) -> quant_conv -> DiagonalGaussian; decode = post_quant_conv -> decoder -> clamp(-1, 1).
Clips of more than one frame (the cached-chunk path) are not restated: the stand-in raises for them.

`decode2d` / `encode2d`: the same network as plain 2-D fp32 convolutions of the sliced weights (a CPU test shows they equal the 3-D module) -
the 1024 x 1024 references on the host cores."""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F


class CausalConv3d(nn.Conv3d):
    def __init__(self, cin, cout, kernel, stride=1, padding=0):
        super().__init__(cin, cout, kernel, stride=stride, padding=padding)
        self._padding = (self.padding[2], self.padding[2], self.padding[1], self.padding[1], 2 * self.padding[0], 0)
        self.padding = (0, 0, 0)

    def forward(self, x, cache_x=None):
        padding = list(self._padding)
        if cache_x is not None and self._padding[4] > 0:
            x = torch.cat([cache_x, x], dim=2)
            padding[4] -= cache_x.shape[2]
        return super().forward(F.pad(x, padding))


class RMS_norm(nn.Module):
    def __init__(self, dim, images=True):
        super().__init__()
        self.scale = dim ** 0.5
        self.gamma = nn.Parameter(torch.ones((dim, 1, 1) if images else (dim, 1, 1, 1)))

    def forward(self, x):
        return F.normalize(x, dim=1) * self.scale * self.gamma


class ResidualBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm1, self.conv1 = RMS_norm(cin, images=False), CausalConv3d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = RMS_norm(cout, images=False), CausalConv3d(cout, cout, 3, padding=1)
        self.conv_shortcut = CausalConv3d(cin, cout, 1) if cin != cout else nn.Identity()

    def forward(self, x):
        h = self.conv_shortcut(x)
        x = self.conv1(F.silu(self.norm1(x)))             # first chunk: no cached frames -> two zero frames in front
        x = self.conv2(F.silu(self.norm2(x)))
        return x + h


class AttentionBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = RMS_norm(dim)
        self.to_qkv, self.proj = nn.Conv2d(dim, dim * 3, 1), nn.Conv2d(dim, dim, 1)

    def forward(self, x):
        identity = x
        b, c, t, h, w = x.shape
        x = self.norm(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w))
        q, k, v = self.to_qkv(x).reshape(b * t, 1, c * 3, -1).permute(0, 1, 3, 2).contiguous().chunk(3, dim=-1)
        x = F.scaled_dot_product_attention(q, k, v)
        x = self.proj(x.squeeze(1).permute(0, 2, 1).reshape(b * t, c, h, w))
        return x.view(b, t, c, h, w).permute(0, 2, 1, 3, 4) + identity


class Resample(nn.Module):
    def __init__(self, dim, mode):
        super().__init__()
        self.mode = mode
        if mode in ("upsample2d", "upsample3d"):
            self.resample = nn.Sequential(nn.Upsample(scale_factor=(2.0, 2.0), mode="nearest-exact"), nn.Conv2d(dim, dim // 2, 3, padding=1))
            if mode == "upsample3d":
                self.time_conv = CausalConv3d(dim, dim * 2, (3, 1, 1), padding=(1, 0, 0))
        else:
            self.resample = nn.Sequential(nn.ZeroPad2d((0, 1, 0, 1)), nn.Conv2d(dim, dim, 3, stride=(2, 2)))
            if mode == "downsample3d":
                self.time_conv = CausalConv3d(dim, dim, (3, 1, 1), stride=(2, 1, 1), padding=(0, 0, 0))

    def forward(self, x, first_chunk=True):
        if not first_chunk:
            raise NotImplementedError("the stand-in restates the first causal chunk only")
        b, c, t, h, w = x.shape                                # first chunk: time_conv skipped (the feature cache is empty)
        x = self.resample(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w))
        return x.view(b, t, x.shape[1], x.shape[2], x.shape[3]).permute(0, 2, 1, 3, 4)


class MidBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.resnets = nn.ModuleList([ResidualBlock(dim, dim), ResidualBlock(dim, dim)])
        self.attentions = nn.ModuleList([AttentionBlock(dim)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class UpBlock(nn.Module):
    def __init__(self, cin, cout, nres, mode):
        super().__init__()
        self.resnets = nn.ModuleList([ResidualBlock(cin if j == 0 else cout, cout) for j in range(nres + 1)])
        self.upsamplers = nn.ModuleList([Resample(cout, mode)]) if mode is not None else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if self.upsamplers is not None else x


class Encoder3d(nn.Module):
    def __init__(self, dim, z_dim, dim_mult, nres, temperal_downsample):
        super().__init__()
        dims = [dim * u for u in [1] + list(dim_mult)]
        self.conv_in = CausalConv3d(3, dims[0], 3, padding=1)
        blocks = []
        for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
            for _ in range(nres):
                blocks.append(ResidualBlock(ci, co))
                ci = co
            if i != len(dim_mult) - 1:
                blocks.append(Resample(co, "downsample3d" if temperal_downsample[i] else "downsample2d"))
        self.down_blocks = nn.ModuleList(blocks)
        self.mid_block = MidBlock(dims[-1])
        self.norm_out = RMS_norm(dims[-1], images=False)
        self.conv_out = CausalConv3d(dims[-1], z_dim, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.norm_out(self.mid_block(x))))


class Decoder3d(nn.Module):
    def __init__(self, dim, z_dim, dim_mult, nres, temperal_upsample):
        super().__init__()
        dims = [dim * u for u in [dim_mult[-1]] + list(dim_mult[::-1])]
        self.conv_in = CausalConv3d(z_dim, dims[0], 3, padding=1)
        self.mid_block = MidBlock(dims[0])
        ups = []
        for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
            if i > 0:
                ci //= 2
            up = i != len(dim_mult) - 1
            ups.append(UpBlock(ci, co, nres, ("upsample3d" if temperal_upsample[i] else "upsample2d") if up else None))
        self.up_blocks = nn.ModuleList(ups)
        self.norm_out = RMS_norm(dims[-1], images=False)
        self.conv_out = CausalConv3d(dims[-1], 3, 3, padding=1)

    def forward(self, x):
        x = self.mid_block(self.conv_in(x))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.norm_out(x)))


class DiagonalGaussian:
    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))

    def mode(self):
        return self.mean

    def sample(self, generator=None):
        return self.mean + self.std * torch.randn(self.mean.shape, generator=generator, dtype=self.mean.dtype).to(self.mean.device)


class AutoencoderKLQwenImage(nn.Module):
    """`vae` of the Qwen-Image pipelines: encode(x [B, 3, T, H, W]).latent_dist, decode(z [B, 16, T, h, w]).sample (clamped).  Counts the calls
    that reach it (`calls`) so that tests can tell the host module's work from the HIP kernels'."""

    def __init__(self, base_dim=96, z_dim=16, dim_mult=(1, 2, 4, 4), num_res_blocks=2, attn_scales=(), temperal_downsample=(False, True, True)):
        super().__init__()
        self.config = SimpleNamespace(base_dim=base_dim, z_dim=z_dim, dim_mult=list(dim_mult), num_res_blocks=num_res_blocks,
                                      attn_scales=list(attn_scales), temperal_downsample=list(temperal_downsample),
                                      latents_mean=[0.02 * i - 0.1 for i in range(z_dim)], latents_std=[1.5 + 0.1 * i for i in range(z_dim)])
        self.encoder = Encoder3d(base_dim, z_dim * 2, dim_mult, num_res_blocks, temperal_downsample)
        self.quant_conv = CausalConv3d(z_dim * 2, z_dim * 2, 1)
        self.post_quant_conv = CausalConv3d(z_dim, z_dim, 1)
        self.decoder = Decoder3d(base_dim, z_dim, dim_mult, num_res_blocks, list(temperal_downsample)[::-1])
        self.use_tiling = self.use_slicing = False
        self.calls = []

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def _one_frame(self, x):
        if x.dim() != 5 or x.shape[2] != 1:
            raise NotImplementedError("the stand-in restates single-frame clips (the first causal chunk) only")

    def encode(self, x, return_dict=True):
        self.calls.append(("encode", tuple(x.shape)))
        self._one_frame(x)
        d = DiagonalGaussian(self.quant_conv(self.encoder(x)))
        return SimpleNamespace(latent_dist=d) if return_dict else (d,)

    def decode(self, z, return_dict=True):
        self.calls.append(("decode", tuple(z.shape)))
        self._one_frame(z)
        out = torch.clamp(self.decoder(self.post_quant_conv(z)), min=-1.0, max=1.0)
        return SimpleNamespace(sample=out) if return_dict else (out,)


def seeded(seed=0, **kw):
    """Checkpoint-like statistics without a checkpoint: convolutions U(-1, 1) / sqrt(fan_in of the frame's taps) (the 2-D scale of the slice
    that meets an image), gamma near 1 with spread, biases 0.05 N(0, 1), a non-zero `proj` (Wan initialises it to zero)."""
    m = AutoencoderKLQwenImage(**kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith(".gamma"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p.shape[1] * p.shape[-1] * p.shape[-2]
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / math.sqrt(fan_in))
    return m.eval()


# ---- the 2-D form (one frame) ---------------------------------------------------------------------------------------------------------
def _c2(sd, n, x, **kw):
    w = sd[n + ".weight"]
    return F.conv2d(x, w[:, :, -1] if w.dim() == 5 else w, sd[n + ".bias"], **kw)


def _rms(sd, n, x, silu=True):
    y = F.normalize(x, dim=1) * math.sqrt(x.shape[1]) * sd[n + ".gamma"].reshape(1, -1, 1, 1)
    return F.silu(y) if silu else y


def _res2(sd, n, x):
    h = _c2(sd, n + ".conv_shortcut", x) if n + ".conv_shortcut.weight" in sd else x
    y = _c2(sd, n + ".conv1", _rms(sd, n + ".norm1", x), padding=1)
    return _c2(sd, n + ".conv2", _rms(sd, n + ".norm2", y), padding=1) + h


def _mid2(sd, n, x):
    x = _res2(sd, n + ".resnets.0", x)
    a = n + ".attentions.0."
    b, c, h, w = x.shape
    q, k, v = _c2(sd, a + "to_qkv", _rms(sd, a + "norm", x, silu=False)).reshape(b, 3 * c, h * w).transpose(1, 2).chunk(3, dim=-1)
    o = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(c), dim=-1) @ v
    x = _c2(sd, a + "proj", o.transpose(1, 2).reshape(b, c, h, w)) + x
    return _res2(sd, n + ".resnets.1", x)


def decode2d(m, z):
    """decode of one frame as 2-D convolutions: z [1, 16, h, w] -> image [1, 3, 8h, 8w] (clamped)."""
    sd = {k: v.float() for k, v in m.state_dict().items()}
    x = _c2(sd, "decoder.conv_in", _c2(sd, "post_quant_conv", z), padding=1)
    x = _mid2(sd, "decoder.mid_block", x)
    for i, b in enumerate(m.decoder.up_blocks):
        for j in range(len(b.resnets)):
            x = _res2(sd, f"decoder.up_blocks.{i}.resnets.{j}", x)
        if b.upsamplers is not None:
            x = _c2(sd, f"decoder.up_blocks.{i}.upsamplers.0.resample.1", F.interpolate(x, scale_factor=2.0, mode="nearest"), padding=1)
    x = _c2(sd, "decoder.conv_out", _rms(sd, "decoder.norm_out", x), padding=1)
    return x.clamp(-1.0, 1.0)


def encode2d(m, x):
    """encode of one frame as 2-D convolutions: x [1, 3, H, W] -> moments [1, 32, H / 8, W / 8] (quant_conv applied)."""
    sd = {k: v.float() for k, v in m.state_dict().items()}
    x = _c2(sd, "encoder.conv_in", x, padding=1)
    for k, b in enumerate(m.encoder.down_blocks):
        n = f"encoder.down_blocks.{k}"
        x = _res2(sd, n, x) if isinstance(b, ResidualBlock) else _c2(sd, n + ".resample.1", F.pad(x, (0, 1, 0, 1)), stride=2)
    x = _mid2(sd, "encoder.mid_block", x)
    x = _c2(sd, "encoder.conv_out", _rms(sd, "encoder.norm_out", x), padding=1)
    return _c2(sd, "quant_conv", x)
