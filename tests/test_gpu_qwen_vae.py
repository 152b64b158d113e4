"""-m gpu: the Qwen-Image VAE on the HIP kernels (regione_amd/qwen_vae.py: rgn_rms_norm_silu + the f4 convolutions) against the fp32
stand-in of the [EXT] AutoencoderKLQwenImage (tests/host_qwen_vae.py: genuine 3-D causal convolutions; its 2-D form, shown equal on the
CPU by tests/test_qwen_vae_host_logic.py, for the 1024 x 1024 references on the host cores), and the hosted Qwen-Image-Edit / -Edit-Plus
pipelines decoding and encoding through it.  Tolerance: PSNR >= 40 dB (peak = the reference's value range), 48 dB for the norm pass."""
import math
import time
import warnings

import pytest
import torch

from regione_amd import RegionEHelper, _lib, adapters as A, ops, qwen_vae as Q
from regione_amd.vae import PaddedImage
from tests import host_qwen_vae as HQ
from tests import host_standins as HS

pytestmark = pytest.mark.gpu


def _psnr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    peak = float(b.max() - b.min())
    return 10 * math.log10(peak * peak / max(float(((a - b) ** 2).mean()), 1e-30))


def _fp32_on_cpu(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 64))
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.set_num_threads(n)


@pytest.fixture(scope="module")
def m():
    return HQ.seeded(4)


@pytest.fixture(scope="module")
def pair(m):
    sd = m.state_dict()
    return Q.HipQwenVaeDecoder(sd, "cuda"), Q.HipQwenVaeEncoder(sd, "cuda")


def _median_ms(fn, n=20):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[n // 2]


@pytest.mark.parametrize("H,W,c", [(13, 17, 96), (9, 31, 192), (21, 11, 384)])
@pytest.mark.parametrize("silu", [True, False])
def test_rms_norm_kernel_vs_torch(H, W, c, silu):
    g = torch.Generator().manual_seed(c + H)
    cp = Q.cs(c)
    x = PaddedImage(H, W, cp, "cuda")
    v = torch.randn(H, W, c, generator=g) * 3 + 0.5
    x.t.view(H + 2, W + 2, cp)[1:-1, 1:-1, :c] = v.to("cuda", torch.bfloat16)
    gamma = torch.zeros(cp)
    gamma[:c] = 1.0 + 0.3 * torch.randn(c, generator=g)
    gb = gamma.to("cuda", torch.bfloat16)
    outs = []
    for _ in range(2):
        out = PaddedImage(H, W, cp, "cuda")
        out.storage.fill_(7.0)                                  # every row of the image is written
        Q.rms_norm_silu(x, gb, c, out, silu=silu)
        torch.cuda.synchronize()
        outs.append(out.t.view(H + 2, W + 2, cp).float().cpu())
    assert torch.equal(outs[0], outs[1])                        # bit-reproducible
    o = outs[0]
    xv = v.bfloat16().float()
    ref = torch.nn.functional.normalize(xv, dim=-1) * math.sqrt(c) * gb.float().cpu()[:c]
    ref = torch.nn.functional.silu(ref) if silu else ref
    assert o[0].abs().sum() == 0 and o[-1].abs().sum() == 0 and o[:, 0].abs().sum() == 0 and o[:, -1].abs().sum() == 0
    assert o[..., c:].abs().sum() == 0
    p = _psnr(o[1:-1, 1:-1, :c], ref)
    assert p >= 48.0, p


def test_rms_norm_pass_bandwidth_at_1024():
    """The 96-channel level's norm pass at 1024 x 1024 (stored at 128 channels): HBM-bound, one read + one write of the image."""
    x, out = PaddedImage(1024, 1024, 128, "cuda"), PaddedImage(1024, 1024, 128, "cuda")
    x.t.normal_()
    gb = torch.ones(128, device="cuda", dtype=torch.bfloat16)
    ms = _median_ms(lambda: Q.rms_norm_silu(x, gb, 96, out))
    gbs = 2 * x.rows * 128 * 2 / (ms * 1e-3) / 1e9
    print(f"[qwen vae] rms_norm_silu 1024 x 1024 x 128: {ms * 1e3:.0f} us, {gbs:.0f} GB/s")
    assert gbs >= 1000.0, gbs


@pytest.mark.parametrize("h,w", [(8, 8), (12, 20), (16, 16)])
def test_decoder_vs_3d_module(m, pair, h, w):
    dec, _ = pair
    z = torch.randn(1, 16, 1, h, w, generator=torch.Generator().manual_seed(h * w))
    with torch.no_grad():
        ref = m.decode(z.bfloat16().float(), return_dict=False)[0]
    img = dec.decode(z.cuda())
    torch.cuda.synchronize()
    assert img.shape == (1, 3, 1, 8 * h, 8 * w) and img.dtype == torch.bfloat16
    assert float(img.float().abs().max()) <= 1.0
    p = _psnr(img, ref)
    print(f"[qwen vae] decode {h} x {w}: {p:.1f} dB")
    assert p >= 40.0, p


@pytest.mark.parametrize("H,W", [(64, 64), (96, 160), (128, 128)])
def test_encoder_vs_3d_module(m, pair, H, W):
    _, enc = pair
    x = torch.rand(1, 3, 1, H, W, generator=torch.Generator().manual_seed(H + W)) * 2 - 1
    with torch.no_grad():
        ref = m.encode(x.bfloat16().float()).latent_dist.mode()
    mom = enc.encode(x.cuda())
    torch.cuda.synchronize()
    assert mom.shape == (1, 32, 1, H // 8, W // 8) and torch.isfinite(mom.float()).all()
    assert torch.equal(enc.encode_dist(x.cuda()).latent_dist.mode(), mom[:, :16])
    p = _psnr(mom[:, :16], ref)
    print(f"[qwen vae] encode {H} x {W}: mean {p:.1f} dB")
    assert p >= 40.0, p


def test_1024_decode_and_encode_vs_2d_reference_and_timing(m, pair):
    """The headline size against the 2-D fp32 form on the host cores.  Time bounds: the medians measured on an MI355X
    (profiles/r07_qwen_vae_bench.json) with the slack tests/test_gpu_vae.py allows a slow box."""
    dec, enc = pair
    g = torch.Generator().manual_seed(9)
    z = torch.randn(1, 16, 1, 128, 128, generator=g)
    x = torch.rand(1, 3, 1, 1024, 1024, generator=g) * 2 - 1
    zc, xc = z.cuda(), x.cuda()
    img, mom = dec.decode(zc), enc.encode(xc)
    torch.cuda.synchronize()
    t_dec, t_enc = _median_ms(lambda: dec.decode(zc)), _median_ms(lambda: enc.encode(xc))
    ref_img = _fp32_on_cpu(lambda: HQ.decode2d(m, z[:, :, 0].bfloat16().float()))
    ref_mom = _fp32_on_cpu(lambda: HQ.encode2d(m, x[:, :, 0].bfloat16().float()))
    pd, pe = _psnr(img[:, :, 0], ref_img), _psnr(mom[:, :16, 0], ref_mom[:, :16])
    print(f"[qwen vae] 1024 x 1024: decode {pd:.1f} dB {t_dec:.2f} ms ({dec.flops(128, 128) / t_dec / 1e9:.0f} TFLOP/s); "
          f"encode {pe:.1f} dB {t_enc:.2f} ms ({enc.flops(1024, 1024) / t_enc / 1e9:.0f} TFLOP/s)")
    assert pd >= 40.0 and pe >= 40.0, (pd, pe)
    assert t_dec <= DECODE_MS_BOUND and t_enc <= ENCODE_MS_BOUND, (t_dec, t_enc)


DECODE_MS_BOUND, ENCODE_MS_BOUND = 16.0, 12.0            # measured medians 9.8 / 7.2 ms


def test_warm_decode_and_encode_dispatch_only_libregione_hip_kernels(m):
    from tests.test_gpu_no_eager_kernels import _foreign, _gpu_activity_names
    sd = m.state_dict()
    for dt in (torch.bfloat16, torch.float32):
        dec, enc = Q.HipQwenVaeDecoder(sd, "cuda", out_dtype=dt), Q.HipQwenVaeEncoder(sd, "cuda", out_dtype=dt)
        z = torch.randn(1, 16, 1, 24, 32).to("cuda", torch.bfloat16)
        x = torch.randn(1, 3, 1, 192, 256).clamp(-1, 1).to("cuda", torch.bfloat16)
        dec.decode(z), enc.encode(x)
        torch.cuda.synchronize()
        img, names = _gpu_activity_names(lambda: dec.decode(z))
        assert any("rms_norm_kernel" in n for n in names) and any("padded_to_nchw_cvt_kernel" in n for n in names), names[:5]
        assert _foreign(names) == [], _foreign(names)
        mom, names = _gpu_activity_names(lambda: enc.encode(x))
        assert len(names) > 40 and _foreign(names) == [], _foreign(names)
        assert img.shape == (1, 3, 1, 192, 256) and img.dtype == dt and mom.shape == (1, 32, 1, 24, 32) and mom.dtype == dt


# ---- the hosted pipelines ------------------------------------------------------------------------------------------------------------
def _picture(h=256, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(1, 3, h, w, generator=g)
    p[:, :, h // 4: h // 4 + h // 3, w // 3: w // 3 + w // 3] = 0.0
    return p


def _norm_lat(vae, z):
    c = vae.config
    mean = torch.tensor(c.latents_mean).view(1, c.z_dim, 1, 1)
    std = torch.tensor(c.latents_std).view(1, c.z_dim, 1, 1)
    return (z.float().cpu() - mean) / std


class _QwenVaeHost:
    """diffusers' Qwen pipelines around the VAE: `_encode_vae_image` = retrieve_latents(vae.encode(image), "argmax"), normalised by
    latents_mean / latents_std; `_unpack_latents` -> [B, 16, 1, h, w]."""

    def _unpack_latents(self, latents, height, width, vae_scale_factor):
        return super()._unpack_latents(latents, height, width, vae_scale_factor).unsqueeze(2)

    def prepare_latents(self, image, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        images = image if isinstance(image, list) else [image]
        self.seen_images = [im for im in images]
        cond = torch.cat([self._pack_latents(_norm_lat(self.vae, self.vae.encode(im).latent_dist.mode()[:, :, 0])).to(dtype)
                          for im in images], dim=1)
        self.seen_cond = cond
        if latents is None:
            latents = torch.randn(1, (height // 16) * (width // 16), 64, generator=generator).to(dtype)
        return latents, cond


class QwenImageEditPipeline(_QwenVaeHost, HS.QwenImageEditPipeline):            # RegionEHelper dispatches on the class NAME
    pass


class QwenImageEditPlusPipeline(_QwenVaeHost, HS.QwenImageEditPlusPipeline):
    pass


@pytest.mark.parametrize("plus", [False, True])
def test_hosted_qwen_edit_decodes_and_encodes_on_the_hip_vae(plus):
    cls = QwenImageEditPlusPipeline if plus else QwenImageEditPipeline
    torch.manual_seed(13)
    pipe = cls(HS.stub_trunk("qwen"))
    vae = pipe.vae = HQ.seeded(6)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        helper.enable()
    assert isinstance(pipe._regione_hip_vae, Q.HipQwenVaeDecoder) and isinstance(pipe._regione_hip_vae_encoder, Q.HipQwenVaeEncoder)
    images = [_picture(192, 384, seed=2), _picture(256, 256, seed=3)] if plus else _picture()
    kw = dict(image=images, prompt="add a hat", negative_prompt=" ", true_cfg_scale=4.0)
    out = pipe(generator=torch.Generator().manual_seed(1), output_type="pt", **kw)
    assert vae.calls == [] and "encode" not in vae.__dict__          # the host module neither decoded nor encoded; the binding is undone
    assert tuple(out.images.shape) == (1, 3, 1024, 1024)
    # the condition latents the loop saw = the host module's encode (2-D fp32 form) of the same images
    assert len(pipe.seen_images) == (2 if plus else 1)
    ref = torch.cat([pipe._pack_latents(_norm_lat(vae, _fp32_on_cpu(lambda: HQ.encode2d(vae, im[:, :, 0].float()))[:, :16]))
                     for im in pipe.seen_images], dim=1)
    p = _psnr(pipe.seen_cond, ref)
    assert p >= 40.0, p
    # the image = the host module's decode of the same latents
    lat = pipe(generator=torch.Generator().manual_seed(1), output_type="latent", **kw).images
    zl = pipe._unpack_latents(lat.float().cpu(), 1024, 1024, 8)[:, :, 0]
    c = vae.config
    z = zl * torch.tensor(c.latents_std).view(1, 16, 1, 1) + torch.tensor(c.latents_mean).view(1, 16, 1, 1)
    ref = pipe.image_processor.postprocess(_fp32_on_cpu(lambda: HQ.decode2d(vae, z.bfloat16().float())))
    mse = float(((out.images.float().cpu() - ref) ** 2).mean())
    assert 10 * math.log10(1.0 / max(mse, 1e-30)) >= 40.0
    helper.disable()


def test_hosted_qwen_fallbacks_keep_the_host_module():
    """Opt-out, `use_tiling`, an oversized latent: the host module runs (with one warning naming the reason); the toy VAE is untouched."""
    dev = torch.device("cuda", 0)
    pipe = QwenImageEditPipeline(HS.stub_trunk("qwen"))
    vae = pipe.vae = HQ.seeded(6)
    assert isinstance(A.hip_vae_for(pipe, dev), Q.HipQwenVaeDecoder)
    z = torch.randn(1, 16, 1, 6, 6)
    x = torch.rand(1, 3, 1, 48, 48) * 2 - 1
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        img = A._decode_qwen_image(pipe, vae, z, dev)
    assert vae.calls == [] and img.is_cuda and img.shape == (1, 3, 48, 48)
    vae.use_tiling = True
    with pytest.warns(RuntimeWarning, match="decode on the host module: vae.use_tiling"):
        img2 = A._decode_qwen_image(pipe, vae, z, dev)
    with pytest.warns(RuntimeWarning, match="encode on the host module: vae.use_tiling"):
        with A._hip_vae_encode(pipe, dev):
            vae.encode(x)
    assert [c[0] for c in vae.calls] == ["decode", "encode"] and not img2.is_cuda
    assert _psnr(img.cpu(), img2) >= 40.0
    vae.use_tiling = False
    vae.calls.clear()
    big = torch.zeros(1, 16, 1, 160, 160)
    own = vae.decode
    vae.decode = lambda zz, return_dict=True: (vae.calls.append(("decode", tuple(zz.shape))), (torch.zeros(1, 3, 1, 8, 8),))[1]
    with pytest.warns(RuntimeWarning, match="softmax"):
        A._decode_qwen_image(pipe, vae, big, dev)
    assert vae.calls == [("decode", (1, 16, 1, 160, 160))]
    vae.decode = own
    vae.calls.clear()
    pipe2 = QwenImageEditPipeline(HS.stub_trunk("qwen"))
    pipe2.vae = vae
    pipe2._regione_hip_vae = False
    assert A.hip_vae_for(pipe2, dev) is None and A.hip_vae_encoder_for(pipe2, dev) is None
    A._decode_qwen_image(pipe2, vae, z, dev)
    assert [c[0] for c in vae.calls] == ["decode"]
    # the toy stand-in VAE of the other tests is not touched
    pipe3 = HS.QwenImageEditPipeline(HS.stub_trunk("qwen"))
    assert A.hip_vae_for(pipe3, dev) is None and A.hip_vae_encoder_for(pipe3, dev) is None
