"""Hosted FLUX / Qwen edits with their image pre- and post-processing on the device (`pipe._regione_hip_image = True`) against the same
call on the host's own methods (`= False`): the output PIL image, the condition latents and the vision tower's input rows are the SAME
BYTES, and on the device path the host's `resize`, `preprocess`, `postprocess` and VLM image processor are never entered (call counters
on the stand-ins of tests/host_image_processor.py).  Inputs the device path does not cover take the host path unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_image_processor as HI  # noqa: E402
import host_qwen_text_pipeline as HQT  # noqa: E402
import host_qwen_vae  # noqa: E402
import host_standins as HS  # noqa: E402
import host_vae  # noqa: E402
import image_model as M  # noqa: E402
from regione_amd import RegionEHelper, adapters as A, image_ops  # noqa: E402

pytestmark = pytest.mark.gpu
PIL_Image = pytest.importorskip("PIL.Image")


def _pil(h=72, w=96, seed=4, mode="RGB"):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[h // 4:h // 2, w // 3:2 * w // 3] = (255, 0, 32)
    return PIL_Image.fromarray(a).convert(mode)


def _gen():
    return torch.Generator().manual_seed(1)


# ---- FLUX ---------------------------------------------------------------------------------------------------------------------------------
class KL(host_vae.AutoencoderKLStandIn):
    dtype = torch.float32
    config = HS.Vae.config


class FluxKontextPipeline(HS.FluxKontextPipeline):              # RegionEHelper dispatches on the class NAME
    def _latents(self, image, dtype, generator, latents):       # diffusers' _encode_vae_image: retrieve_latents(vae.encode(image), "argmax")
        z = self.vae.encode(image).latent_dist.mode()
        z = (z - self.vae.config.shift_factor) * self.vae.config.scaling_factor
        self.seen_image, self.seen_cond = image, z.float().cpu()
        image_latents = self._pack_latents(z.float().cpu()).to(dtype)
        if latents is None:
            latents = torch.randn(image_latents.shape, generator=generator).to(dtype)
        return latents, image_latents


@pytest.fixture(scope="module")
def flux():
    torch.manual_seed(11)
    pipe = FluxKontextPipeline(HS.stub_trunk("flux"))
    pipe.vae = KL().eval()
    pipe.image_processor = HI.VaeImageProcessor()
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    yield pipe
    helper.disable()


def _flux_call(pipe, flag, image=None, output_type="pil"):
    pipe._regione_hip_image = flag
    pipe.image_processor.calls.clear()
    out = pipe(image=_pil() if image is None else image, prompt="make the square red", guidance_scale=2.5, preferred_resolutions=[(256, 256)],
               generator=_gen(), output_type=output_type).images
    return out, dict(pipe.image_processor.calls), pipe.seen_cond.clone(), pipe.seen_image


def test_flux_edit_is_byte_identical_on_the_device_path(flux):
    dev_out, dev_calls, dev_cond, dev_img = _flux_call(flux, True)
    host_out, host_calls, host_cond, host_img = _flux_call(flux, False)
    assert dev_calls == {} and host_calls == {"resize": 1, "preprocess": 1, "postprocess": 1}
    assert dev_img.is_cuda and dev_img.dtype == torch.bfloat16 and not host_img.is_cuda
    assert torch.equal(dev_img.cpu(), host_img.to(torch.bfloat16))                     # the VAE's input: the same bf16 values
    assert torch.equal(dev_cond, host_cond)                                            # the condition latents
    assert len(dev_out) == 1 and dev_out[0].mode == "RGB" and dev_out[0].size == host_out[0].size == (256, 256)
    assert dev_out[0].tobytes() == host_out[0].tobytes()
    assert isinstance(flux._regione_hip_image_ops, image_ops.HipImageOps)


def test_flux_uncovered_inputs_take_the_host_path(flux):
    tensor = torch.rand(1, 3, 72, 96, generator=torch.Generator().manual_seed(3))
    out, calls, _, img = _flux_call(flux, True, image=tensor, output_type="np")        # a tensor image, output_type "np": the host's methods
    assert calls == {"resize": 2, "preprocess": 1, "postprocess": 1} and isinstance(out, np.ndarray) and not img.is_cuda
    _, calls, _, _ = _flux_call(flux, True, output_type="np")                           # a PIL image in, "np" out: only the output stays
    assert calls == {"postprocess": 1}
    # an "RGBA" image: the host's own resize and preprocess run, as with the device path switched off, and what they make of it - four
    # channels, which the VAE's first convolution does not take (diffusers' processor does the same without do_convert_rgb) - is the
    # host's own error on both settings: the hosted call adds and removes nothing
    errors = []
    for flag in (True, False):
        flux._regione_hip_image = flag
        flux.image_processor.calls.clear()
        with pytest.raises(RuntimeError) as e:
            flux(image=_pil(mode="RGBA"), prompt="make the square red", guidance_scale=2.5, preferred_resolutions=[(256, 256)],
                 generator=_gen(), output_type="pil")
        assert dict(flux.image_processor.calls) == {"resize": 1, "preprocess": 1}, flag
        assert "encode" not in flux.vae.__dict__                                        # the VAE binding is undone after the exception
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "channels" in errors[0]
    flux._regione_hip_image = True
    dev = flux._regione_engine.transformer.device
    assert A._image_inputs_on_device(flux, dev, [_pil(mode="RGBA")]) is None
    assert A._image_inputs_on_device(flux, dev, [_pil()]) is not None
    for name, value in (("resample", "bicubic"), ("do_convert_rgb", True), ("do_binarize", True), ("do_normalize", False)):
        old = flux.image_processor.config[name]
        flux.image_processor.config[name] = value
        try:
            assert A.hip_image_ops_for(flux, dev, "resize") is None, name
        finally:
            flux.image_processor.config[name] = old
    del flux.__dict__["_regione_hip_image"]                                             # unset: the stages of IMAGE_STAGES_DEFAULT
    for stage in A.IMAGE_STAGES:
        assert (A.hip_image_ops_for(flux, dev, stage) is not None) == (stage in A.IMAGE_STAGES_DEFAULT)


# ---- Qwen ---------------------------------------------------------------------------------------------------------------------------------
def _norm_lat(vae, z):
    c = vae.config
    return (z.float().cpu() - torch.tensor(c.latents_mean).view(1, c.z_dim, 1, 1)) / torch.tensor(c.latents_std).view(1, c.z_dim, 1, 1)


class _QwenHost:
    """diffusers' Qwen pipelines around the VAE (`_encode_vae_image`, `_unpack_latents` -> [B, 16, 1, h, w]); the pipeline lives on the GPU."""
    _execution_device = torch.device("cuda")

    def _unpack_latents(self, latents, height, width, vae_scale_factor):
        return super()._unpack_latents(latents, height, width, vae_scale_factor).unsqueeze(2)

    def prepare_latents(self, image, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        images = image if isinstance(image, list) else [image]
        self.seen_images = list(images)
        self.seen_cond = torch.cat([self._pack_latents(_norm_lat(self.vae, self.vae.encode(im).latent_dist.mode()[:, :, 0])).to(dtype)
                                    for im in images], dim=1)
        if latents is None:
            latents = torch.randn(1, (height // 16) * (width // 16), 64, generator=generator).to(dtype)
        return latents, self.seen_cond


class QwenImageEditPipeline(_QwenHost, HQT.QwenImageEditPipeline):
    pass


class QwenImageEditPlusPipeline(_QwenHost, HQT.QwenImageEditPlusPipeline):
    pass


def _qwen(plus):
    torch.manual_seed(13)
    pipe = (QwenImageEditPlusPipeline if plus else QwenImageEditPipeline)(HS.stub_trunk("qwen"), HQT.tiny_qwen25vl())
    pipe.vae = host_qwen_vae.seeded(6).to(torch.bfloat16)    # bf16, as the pipelines load it (an fp32 VAE's postprocess is fp32 arithmetic: the host's)
    pipe.image_processor = HI.VaeImageProcessor()
    pipe.processor = HI.QwenProcessor(min_pixels=3136, max_pixels=12845056)      # the limits of Qwen2.5-VL's preprocessor_config.json
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    return pipe, helper


def _qwen_call(pipe, flag, plus, output_type="pil"):
    pipe._regione_hip_image = flag
    pipe.image_processor.calls.clear()
    pipe.processor.image_processor.calls.clear()
    pipe.processor.seen.clear()
    pipe.encoded.clear()
    image = [_pil(), _pil(64, 64, seed=9)] if plus else _pil()
    out = pipe(image=image, prompt="add a red hat", generator=_gen(), output_type=output_type).images      # no CFG branch: half the work
    return dict(out=out, calls=dict(pipe.image_processor.calls), vlm_calls=dict(pipe.processor.image_processor.calls),
                rows=list(pipe.processor.seen), cond=pipe.seen_cond.clone(), images=list(pipe.seen_images),
                embeds=[e.clone() for e, _ in pipe.encoded])


def _tower_rows(pv, Kp):
    """The rows the vision tower's patch GEMM reads: the padded bf16 rows as they stand, or rgn_cast_pad_rows of the processor's fp32 rows."""
    if pv.dtype == torch.bfloat16:
        return pv.cpu().view(torch.int16).numpy().view(np.uint16)
    return M.pad_rows_bf16(pv.cpu().numpy(), Kp)


@pytest.mark.parametrize("plus", [False, True], ids=["edit", "plus"])
def test_qwen_edit_is_byte_identical_on_the_device_path(plus):
    pipe, helper = _qwen(plus)
    Kp = pipe._regione_hip_qwen_text.vision.Kp
    d = _qwen_call(pipe, True, plus)
    h = _qwen_call(pipe, False, plus)
    n = 2 if plus else 1
    assert d["calls"] == {} and d["vlm_calls"] == {}
    assert h["calls"] == {"resize": n, "preprocess": n, "postprocess": 1} and h["vlm_calls"] == {"preprocess": 1}
    assert "image_processor" in pipe.processor.__dict__ and pipe.processor.image_processor.calls is not None           # the binding is undone
    assert type(pipe.processor.image_processor).__name__ == "Counting"
    # the VAE's inputs and the condition latents
    assert len(d["images"]) == len(h["images"]) == n
    for a, b in zip(d["images"], h["images"]):
        assert a.is_cuda and a.dtype == torch.bfloat16 and torch.equal(a.cpu(), b.to(torch.bfloat16).cpu())
    assert torch.equal(d["cond"], h["cond"])
    # the vision tower's input rows: on the device as padded bf16 (rgn_cast_pad_rows is skipped), the same bits as the host's fp32 rows cast
    assert len(d["rows"]) == len(h["rows"]) == 1 and len(d["embeds"]) == len(h["embeds"]) == 1
    for (dp, dg), (hp, hg) in zip(d["rows"], h["rows"]):
        assert dp.is_cuda and dp.dtype == torch.bfloat16 and dp.shape[1] == Kp and hp.dtype == torch.float32 and hp.shape[1] == 1176
        assert torch.equal(torch.as_tensor(dg), torch.as_tensor(hg))
        assert np.array_equal(_tower_rows(dp, Kp), _tower_rows(hp, Kp))
    for a, b in zip(d["embeds"], h["embeds"]):
        assert torch.equal(a, b)
    # the output image
    assert len(d["out"]) == 1 and d["out"][0].size == h["out"][0].size and d["out"][0].mode == "RGB"
    assert d["out"][0].tobytes() == h["out"][0].tobytes()
    helper.disable()


def test_qwen_bound_processor_hands_the_rest_to_the_host_and_is_restored_after_an_exception():
    pipe, helper = _qwen(False)
    pipe._regione_hip_image = True
    dev = pipe._regione_engine.transformer.device
    own = pipe.processor.image_processor
    with A._hip_qwen_image_processor(pipe, dev):
        bound = pipe.processor.image_processor
        assert bound is not own and bound.merge_size == 2
        got = bound(images=[_pil(56, 84)], return_tensors="pt")                            # covered: on the device
        assert own.calls == {} and got["pixel_values"].is_cuda and got["image_grid_thw"].tolist() == [[1, 4, 6]]
        want = own(images=[_pil(56, 84)], return_tensors="pt")
        assert np.array_equal(_tower_rows(got["pixel_values"], got["pixel_values"].shape[1]),
                              _tower_rows(want["pixel_values"], got["pixel_values"].shape[1]))
        own.calls.clear()
        for kw in (dict(images=[_pil(mode="RGBA")], return_tensors="pt"),                  # another PIL mode
                   dict(images=[_pil(28, 28)], return_tensors="pt"),                       # below the processor's pixel limits
                   dict(images=[_pil()], return_tensors="np"),                             # other arguments
                   dict(images=[_pil()], return_tensors="pt", do_normalize=False)):
            before = own.calls["preprocess"]
            res = bound(**kw)
            pv = res["pixel_values"]
            assert own.calls["preprocess"] == before + 1 and not (torch.is_tensor(pv) and pv.is_cuda), sorted(kw)
    assert pipe.processor.image_processor is own

    class Boom(RuntimeError):
        pass
    enc = pipe.text_encoder

    def fail(*a, **k):
        raise Boom("inside encode_prompt")
    pipe._get_qwen_prompt_embeds = fail
    with pytest.raises(Boom):
        pipe(image=_pil(), prompt="add a red hat", generator=_gen(), output_type="latent")
    assert pipe.processor.image_processor is own and pipe.text_encoder is enc and "text_encoder" in pipe.__dict__
    helper.disable()


class Qwen2VLImageProcessor:
    """A look-alike of transformers' OTHER backend of the same processor (torchvision: what AutoProcessor picks when torchvision is
    installed): every setting the PIL backend has, another class, another `backend`, other arithmetic behind the same settings."""
    backend = "torchvision"

    def __init__(self, pil):
        self.pil, self.calls = pil, 0
        for name in ("do_resize", "do_rescale", "do_normalize", "do_convert_rgb", "resample", "rescale_factor", "image_mean", "image_std",
                     "patch_size", "merge_size", "temporal_patch_size", "size"):
            setattr(self, name, getattr(pil, name))

    def __call__(self, images=None, **kw):
        self.calls += 1
        return self.pil(images=images, **kw)


def test_another_backend_of_the_vlm_processor_stays_on_the_host():
    pipe, helper = _qwen(False)
    pipe._regione_hip_image = True
    dev = pipe._regione_engine.transformer.device
    pil = pipe.processor.image_processor
    assert A._qwen2vl_processor_refusal(pil) is None
    look = pipe.processor.image_processor = Qwen2VLImageProcessor(pil)
    why = A._qwen2vl_processor_refusal(look)
    assert why is not None and "Qwen2VLImageProcessor " in why and "torchvision" in why and "PIL backend" in why
    with A._hip_qwen_image_processor(pipe, dev):
        assert pipe.processor.image_processor is look                                   # not bound
    try:                                                                                 # the genuine torchvision backend, where it can be built
        from transformers.models.qwen2_vl.image_processing_qwen2_vl import Qwen2VLImageProcessor as Genuine
        genuine = Genuine()
    except Exception:                                                                    # noqa: BLE001 - torchvision is not installed
        genuine = None
    if genuine is not None:
        assert A._qwen2vl_processor_refusal(genuine) is not None
    out = pipe(image=_pil(), prompt="add a red hat", generator=_gen(), output_type="latent").images
    assert torch.isfinite(out.float()).all()
    assert look.calls == 1 and pil.calls == {"preprocess": 1}                           # the host's processor did the work ...
    (pv, _), = pipe.processor.seen
    assert pv.dtype == torch.float32 and not pv.is_cuda and pv.shape[1] == 1176          # ... and handed its own fp32 rows on
    assert pipe.image_processor.calls == {}                                              # the VAE-side stages still moved
    helper.disable()


# ---- Step1X: only the "pil" postprocess moves ---------------------------------------------------------------------------------------------
class Step1XEditPipeline(HS.Step1XEditPipeline):                 # RegionEHelper dispatches on the class NAME
    def _latents(self, image, dtype, generator, latents):
        z = self.vae.encode(image).latent_dist.mode()
        image_latents = self._pack_latents(z.float().cpu()).to(dtype)
        if latents is None:
            latents = torch.randn(image_latents.shape, generator=generator).to(dtype)
        return latents, image_latents


def test_step1x_pil_output_is_byte_identical_on_the_device_path():
    torch.manual_seed(12)
    trunk = HS.stub_trunk("step1x")
    pipe = Step1XEditPipeline(trunk)
    object.__setattr__(trunk, "connector", HS.ToyConnector().to(torch.bfloat16))
    pipe.vae = KL().eval()
    pipe.image_processor = HI.VaeImageProcessor()
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    picture = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(5))     # Step1X's input processing is the fork's own code
    res = {}
    for flag in (True, False):
        pipe._regione_hip_image = flag
        pipe.image_processor.calls.clear()
        pipe.calls.clear()
        out = pipe(image=picture, prompt="turn the sky green", generator=_gen(), output_type="pil", latents=None).images
        res[flag] = (out, dict(pipe.image_processor.calls), [c for c in pipe.calls if c[0] == "output_process"])
    (d_out, d_calls, d_post), (h_out, h_calls, h_post) = res[True], res[False]
    assert d_calls.get("postprocess", 0) == 0 and h_calls["postprocess"] == 1
    assert {k: v for k, v in h_calls.items() if k != "postprocess"} == d_calls             # the input side is the host's on both
    assert len(d_post) == len(h_post) == 1                                                # _output_process_image got the images either way
    assert len(d_out) == 1 and d_out[0].mode == "RGB" and d_out[0].size == h_out[0].size == (256, 256)
    assert d_out[0].tobytes() == h_out[0].tobytes()
    helper.disable()
