"""CPU: the host logic of the Qwen-Image VAE on the HIP kernels (regione_amd/qwen_vae.py, the adapter's adoption / fallback) - no GPU.

The stand-in (tests/host_qwen_vae.py) is a genuine 3-D causal module; these tests show that one frame of it IS the 2-D network the kernels
run, and emulate that network with plain torch over the ADOPTED weights (sliced, channel-padded, re-laid, bf16) against the module."""
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from regione_amd import _lib, adapters as A, ops, qwen_vae as Q
from tests import host_qwen_vae as HQ


def _psnr(a, b):
    a, b = a.float(), b.float()
    return 10 * math.log10(float(b.max() - b.min()) ** 2 / max(float(((a - b) ** 2).mean()), 1e-30))


@pytest.fixture(scope="module")
def m():
    return HQ.seeded(3)


def test_state_dict_names_and_shapes_are_the_adopted_layout(m):
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == Q.qwen_vae_param_shapes()


def test_one_frame_of_the_3d_module_equals_the_2d_form(m):
    g = torch.Generator().manual_seed(0)
    z = torch.randn(1, 16, 1, 5, 7, generator=g)
    x = torch.rand(1, 3, 1, 40, 56, generator=g) * 2 - 1
    with torch.no_grad():
        img3 = m.decode(z, return_dict=False)[0]
        mom3 = m.quant_conv(m.encoder(x))
        assert img3.shape == (1, 3, 1, 40, 56) and mom3.shape == (1, 32, 1, 5, 7)
        assert torch.allclose(img3[:, :, 0], HQ.decode2d(m, z[:, :, 0]), atol=1e-4)
        assert torch.allclose(mom3[:, :, 0], HQ.encode2d(m, x[:, :, 0]), atol=1e-4)
        assert torch.equal(m.encode(x).latent_dist.mode(), mom3[:, :16])
        # the reduction is not vacuous: the earlier temporal slices of the 3 x 3 x 3 kernels are non-zero, and the time_conv weights exist
        assert m.decoder.conv_in.weight[:, :, :2].abs().sum() > 0 and m.decoder.up_blocks[0].upsamplers[0].time_conv.weight.abs().sum() > 0


def test_adoption_slices_pads_and_splits(m):
    sd = m.state_dict()
    dec = Q.HipQwenVaeDecoder(sd, "cpu", pixel_groups=False)
    enc = Q.HipQwenVaeEncoder({k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in sd.items()}, "cpu")
    # a 96-channel ResNet of the last up level: [128, 3, 3, 128] re-laid, the last temporal slice, zeros in channels 96..127
    n = "up_blocks.3.resnets.1.conv1"
    w = dec.c[n].w.float().view(128, 3, 3, 128)
    ref = sd["decoder." + n + ".weight"][:, :, -1].permute(0, 2, 3, 1)
    assert torch.equal(w[:96, :, :, :96], ref.bfloat16().float())
    assert w[96:].abs().sum() == 0 and w[:, :, :, 96:].abs().sum() == 0 and dec.c[n].b[96:].abs().sum() == 0
    g = dec.p["up_blocks.3.resnets.1.norm1.gamma"]
    assert g.numel() == 128 and g[96:].abs().sum() == 0 and dec.nc["up_blocks.3.resnets.1.norm1"] == 96
    # with pixel groups the 128-channel (96-valid) convolutions take the 2-pixel block-Toeplitz path
    assert Q.HipQwenVaeDecoder(sd, "cpu").c[n].group == 2
    # to_qkv split into q / k / v
    a = "mid_block.attentions.0."
    qkv = sd["decoder." + a + "to_qkv.weight"][:, :, 0, 0]
    assert torch.equal(dec.c[a + "to_q"].w.float(), qkv[:384].bfloat16().float())
    assert torch.equal(dec.c[a + "to_k"].w.float(), qkv[384:768].bfloat16().float())
    assert torch.equal(dec.p[a + "to_v.weight"].float(), qkv[768:].bfloat16().float())
    assert torch.equal(dec.c[a + "to_out.0"].w.float(), sd["decoder." + a + "proj.weight"][:, :, 0, 0].bfloat16().float())
    # the 1 x 1 x 1 post_quant_conv on the 64-channel latent image; the encoder's conv_out carries quant_conv
    assert dec.c["post_quant_conv"].w.shape == (64, 64) and enc.c["conv_out"].w.shape == (32, 9 * 384)
    assert dec.c["conv_in"].w.shape == (384, 9 * 64) and enc.c["conv_in"].w.shape[0] == 2 * 128


# ---- the adopted weights as plain torch (fp32 math over the bf16 weights) ----------------------------------------------------------
def _cv(cw, x, stride=1):
    co_p = cw.w.shape[0]
    k = 3 if cw.taps == 9 else 1
    w = cw.w.float().view(co_p, k, k, -1).permute(0, 3, 1, 2)[:cw.cout]
    if stride == 2:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, cw.b.float(), stride=2)
    return F.conv2d(x, w, cw.b.float(), padding=k // 2)


def _up(uw, x):
    """rgn_conv_up2_bf16's four 2 x 2 phase convolutions of the low-resolution image."""
    _, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(1, uw.cout, 2 * H, 2 * W)
    for a in range(2):
        for b in range(2):
            w = uw.w[a * 2 + b].float().view(uw.cout, 2, 2, -1).permute(0, 3, 1, 2)
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], w, uw.b.float())
    return out


def _norm(mod, name, x, silu=True):
    c = mod.nc[name]
    y = x.clone()
    y[:, :c] = F.normalize(x[:, :c], dim=1) * math.sqrt(c)
    y = y * mod.p[name + ".gamma"].float().view(1, -1, 1, 1)
    return F.silu(y) if silu else y


def _res(mod, p, x):
    h = _cv(mod.c[p + ".conv1"], _norm(mod, p + ".norm1", x))
    skip = _cv(mod.c[p + ".conv_shortcut"], x) if p + ".conv_shortcut" in mod.c else x
    return _cv(mod.c[p + ".conv2"], _norm(mod, p + ".norm2", h)) + skip


def _mid(mod, x):
    a = "mid_block.attentions.0."
    x = _res(mod, "mid_block.resnets.0", x)
    n = _norm(mod, a + "norm", x, silu=False)
    c = x.shape[1]
    q, k = _cv(mod.c[a + "to_q"], n).flatten(2)[0].T, _cv(mod.c[a + "to_k"], n).flatten(2)[0].T
    v = n.flatten(2)[0].T @ mod.p[a + "to_v.weight"].float().T + mod.p[a + "to_v.bias"].float()
    o = (torch.softmax(q @ k.T / math.sqrt(c), -1) @ v).T.reshape(x.shape)
    return _res(mod, "mid_block.resnets.1", _cv(mod.c[a + "to_out.0"], o) + x)


def test_cpu_emulation_of_the_adopted_decoder_and_encoder_matches_the_module(m):
    sd = m.state_dict()
    dec, enc = Q.HipQwenVaeDecoder(sd, "cpu", pixel_groups=False), Q.HipQwenVaeEncoder(sd, "cpu", pixel_groups=False)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, 16, 1, 4, 6, generator=g)
    x = torch.rand(1, 3, 1, 32, 48, generator=g) * 2 - 1
    with torch.no_grad():
        y = _cv(dec.c["conv_in"], _cv(dec.c["post_quant_conv"], F.pad(z[:, :, 0], (0, 0, 0, 0, 0, 48))))
        y = _mid(dec, y)
        for i, (ci, co, up) in enumerate(dec.levels):
            for j in range(dec.nres):
                y = _res(dec, f"up_blocks.{i}.resnets.{j}", y)
            if up:
                y = _up(dec.u[f"up_blocks.{i}.upsamplers.0.resample.1"], y)
        img = _cv(dec.c["conv_out"], _norm(dec, "norm_out", y)).clamp(-1, 1)
        ref = m.decode(z, return_dict=False)[0][:, :, 0]
        assert img.shape == ref.shape and _psnr(img, ref) >= 40.0, _psnr(img, ref)
        h = _cv(enc.c["conv_in"], F.pad(x[:, :, 0], (0, 0, 0, 0, 0, 61)))
        for res, down, _, _ in enc.levels:
            for r in res:
                h = _res(enc, r, h)
            if down is not None:
                h = _cv(enc.c[down], h, stride=2)
        mom = _cv(enc.c["conv_out"], _norm(enc, "norm_out", _mid(enc, h)))
        ref = m.quant_conv(m.encoder(x))[:, :, 0]
        assert mom.shape == ref.shape and _psnr(mom, ref) >= 40.0, _psnr(mom, ref)


def test_flops_of_the_1024_image():
    sd = HQ.seeded(0).state_dict()
    assert abs(Q.HipQwenVaeDecoder(sd, "cpu").flops(128, 128) / 1e12 - 4.71) < 0.01
    assert abs(Q.HipQwenVaeEncoder(sd, "cpu").flops(1024, 1024) / 1e12 - 2.85) < 0.01


# ---- refusal: the adapter keeps the host module ----------------------------------------------------------------------------------------
class _Host:
    def __init__(self, vae):
        self.vae = vae


def test_unknown_missing_and_rms_bias_parameters_are_refused(m):
    sd = dict(m.state_dict())
    bad = [dict(sd, **{"decoder.up_blocks.0.resnets.0.norm1.bias": torch.zeros(384, 1, 1, 1)}),      # RMS_norm(bias=True)
           {k: v for k, v in sd.items() if k != "decoder.mid_block.attentions.0.proj.weight"},
           dict(sd, **{"decoder.up_blocks.9.resnets.0.conv1.weight": torch.zeros(1)})]
    for d in bad:
        with pytest.raises(_lib.RegionEHipError):
            Q.HipQwenVaeDecoder(d, "cpu")
    with pytest.raises(_lib.RegionEHipError):
        Q.HipQwenVaeEncoder(dict(sd, **{"encoder.norm_out.bias": torch.zeros(384, 1, 1, 1)}), "cpu")
    with pytest.raises(_lib.RegionEHipError):
        Q.HipQwenVaeEncoder({k: v for k, v in sd.items() if k != "quant_conv.weight"}, "cpu")
    # through the adapter: one warning naming the reason, the host module stays
    m2 = HQ.seeded(3)
    m2.decoder.up_blocks[0].resnets[0].norm1.register_parameter("bias", torch.nn.Parameter(torch.zeros(384, 1, 1, 1)))
    host = _Host(m2)
    with pytest.warns(RuntimeWarning, match="kept on the host module.*norm1.bias"):
        assert A.hip_vae_for(host, torch.device("cpu")) is None
    assert A.hip_vae_encoder_for(host, torch.device("cpu")) is None
    host = _Host(HQ.seeded(0, base_dim=64))
    with pytest.warns(RuntimeWarning, match="config"):
        assert A.hip_vae_for(host, torch.device("cpu")) is None


def test_the_adapter_adopts_the_qwen_layout_and_the_opt_out_keeps_the_host_module(m):
    host = _Host(m)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert isinstance(A.hip_vae_for(host, torch.device("cpu")), Q.HipQwenVaeDecoder)
        assert isinstance(A.hip_vae_encoder_for(host, torch.device("cpu")), Q.HipQwenVaeEncoder)
    host = _Host(m)
    host._regione_hip_vae = False
    assert A.hip_vae_for(host, torch.device("cpu")) is None and A.hip_vae_encoder_for(host, torch.device("cpu")) is None


def test_calls_the_kernels_do_not_cover_are_named():
    vae = HQ.AutoencoderKLQwenImage.__new__(HQ.AutoencoderKLQwenImage)
    torch.nn.Module.__init__(vae)
    vae.use_tiling = vae.use_slicing = False
    R = A._qwen_vae_refusal
    assert R(vae, torch.zeros(1, 16, 1, 128, 128), "decode") is None
    assert R(vae, torch.zeros(1, 3, 1, 1024, 1024), "encode") is None
    assert "T = 2" in R(vae, torch.zeros(1, 16, 2, 8, 8), "decode")
    assert "batch 2" in R(vae, torch.zeros(2, 16, 1, 8, 8), "decode")
    assert "softmax" in R(vae, torch.zeros(1, 16, 1, 160, 160), "decode")
    assert "softmax" in R(vae, torch.zeros(1, 3, 1, 1280, 1280), "encode")
    assert "multiples of 8" in R(vae, torch.zeros(1, 3, 1, 100, 64), "encode")
    assert "4-D" in R(vae, torch.zeros(1, 16, 8, 8), "decode")
    assert "arguments" in R(vae, torch.zeros(1, 3, 1, 64, 64), "encode", {"generator": None})
    vae.use_tiling = True
    assert "use_tiling" in R(vae, torch.zeros(1, 16, 1, 8, 8), "decode")


def test_new_entry_points_validate_their_arguments():
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()
    assert h.rgn_rms_norm_silu(P, P, 10, 10, 200, 192, P, 1, None) < 0 and "C_valid > C_pad" in msg()
    assert h.rgn_rms_norm_silu(P, P, 10, 10, 96, 96, P, 1, None) < 0 and "multiple of 64" in msg()
    assert h.rgn_rms_norm_silu(P, P, 10, 10, 96, 128, P + 2, 1, None) < 0 and "aligned" in msg()
    assert h.rgn_rms_norm_silu(None, P, 10, 10, 96, 128, P, 1, None) < 0
    assert h.rgn_padded_to_nchw_cvt(P, 2, P, 3, 8, 8, 1, 0, None) < 0 and "bad argument" in msg()
    assert ops.padded(96, 64) == Q.cs(96) == 128 and Q.cs(192) == 192
