"""The hosted `__call__`s (one per family, each following its reference `__call__` line by line) and the ways onto them: `adopt`,
`attach`, `swap_host_class`."""
from __future__ import annotations

import warnings

import torch

from .components import (_QWEN_TEXT_HOSTS, _STEP1X_TEXT_HOSTS, _bf, _bound, _host_name, _step1x_text_sampling_default, _hip_qwen_image_processor, _hip_qwen_text_encoder, _hip_text_encoders, _hip_vae_encode,
                         _image_inputs_on_device, _postprocess_image, _postprocess_qwen_image, hip_qwen_text_encoder_for,
                         hip_text_encoders_for, hip_vae_encoder_for, hip_vae_for)
from .connector import _HipConnector, _HostConnector, hip_step1x_connector_for
from .trunk import adopt_engine, lora_sync

# ---------------------------------------------------------------------------------------------------------------------
# hosted calls: everything OUTSIDE the denoise loop on the host pipeline's own methods, the loop on the engine
# ---------------------------------------------------------------------------------------------------------------------
# Kontext's training resolutions (diffusers FluxKontextPipeline; reference copy RegionE/FluxKontext/utils.py:18-36):
# the default target of `_auto_resize`
PREFERRED_KONTEXT_RESOLUTIONS = [(672, 1568), (688, 1504), (720, 1456), (752, 1392), (800, 1328), (832, 1248), (880, 1184),
                                 (944, 1104), (1024, 1024), (1104, 944), (1184, 880), (1248, 832), (1328, 800), (1392, 752),
                                 (1456, 720), (1504, 688), (1568, 672)]
STEP1X_DEFAULT_NEGATIVE = ("worst quality, wrong limbs, unreasonable limbs, normal quality, low quality, low res, blurry, text, "
                           "watermark, logo, banner, extra digits, cropped, jpeg artifacts, signature, username, error, sketch ,"
                           "duplicate, ugly, monochrome, horror, geometry, mutation, disgusting")    # Step1XEdit/inplace.py:231
QWEN_CONDITION_IMAGE_SIZE, QWEN_VAE_IMAGE_SIZE = 384 * 384, 1024 * 1024                                # QwenImageEditPlus/inplace.py:53-54


# Step1X-Edit v1p2's thinking / reflection retry loop is the module AFTER this one (adapters/thinking.py; a module of this package imports
# only from the ones before it): importing the package puts its `Retry` here, `_hosted_step1x` calls it when a v1p2 switch is on
_STEP1X_RETRY = []


class HostedOutput(dict):
    def __init__(self, images, timing=None, **extra):
        super().__init__(images=images, **extra)      # extra: what a family's output carries besides (Step1X v1p2: final_images, ...)
        self.images = images
        self.__dict__.update(extra)
        self.timing = timing or {}           # wall-clock seconds of the three stages: encode / loop / decode


def _one_image_only(prompt, num_images_per_prompt):
    if num_images_per_prompt != 1 or (isinstance(prompt, list) and len(prompt) != 1):
        raise ValueError("the region-aware loop is batch-1 (token_selector squeezes the batch, utils.py:337-343): "
                         "one image per call, shard images across GPUs")


# stock-pipeline arguments the hosted calls take no action on, with the value at which ignoring them changes nothing
_IGNORABLE_DEFAULTS = {"max_sequence_length": 512, "num_images_per_prompt": 1, "guidance_scale": None, "ip_adapter_image": None,
                       "ip_adapter_image_embeds": None, "negative_ip_adapter_image": None, "negative_ip_adapter_image_embeds": None,
                       "joint_attention_kwargs": None, "attention_kwargs": None, "prompt_2": None, "negative_prompt_2": None}


def _refuse_unused(fn_name: str, unused: dict):
    """A stock-pipeline argument the hosted loop does not implement must not be dropped silently (advisor finding, round 2:
    the reference honours `joint_attention_kwargs`, IP-adapter inputs ... - FluxKontext/inplace.py:76-110): None or the
    documented default passes, anything else raises."""
    for k, v in unused.items():
        if v is None or (k in _IGNORABLE_DEFAULTS and v == _IGNORABLE_DEFAULTS[k]):
            continue
        known = k in _IGNORABLE_DEFAULTS
        raise (NotImplementedError if known else TypeError)(
            f"{fn_name}: argument {k}={v!r} is {'not implemented by' if known else 'unknown to'} the hosted HIP loop")


def _lora_call(host, eng, unused: dict, key: str) -> dict:
    """The start of every hosted call: `{key: {"scale": s}}` (the stock pipelines' call-time LoRA scale) multiplies every term's scale
    for THIS call - honoured by a re-merge, and the weights are restored by the next call that differs; then the engine's weights are
    brought to the host's current adapter state (lora_sync: a no-op while the fingerprint is unchanged).  Any other content of `key`
    stays in `unused` and is refused as before."""
    kw, scale = unused.get(key), 1.0
    if isinstance(kw, dict) and set(kw) == {"scale"} and isinstance(kw["scale"], (int, float)) and not isinstance(kw["scale"], bool):
        scale = float(kw["scale"])
        unused = {k: v for k, v in unused.items() if k != key}
    lora_sync(host, eng, scale)
    return unused


class _Clock:
    """Wall-clock of the stages of an edit (end-to-end = encode + loop + decode)."""

    def __init__(self, dev):
        import time
        self.dev, self.t, self.time, self.out = dev, None, time, {}
        self.mark(None)

    def mark(self, name):
        if torch.cuda.is_available():
            torch.cuda.synchronize(self.dev)
        now = self.time.perf_counter()
        if name is not None:
            self.out[name] = now - self.t
        self.t = now


def _run_loop(eng, clk, kw: dict, trace, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs):
    """The denoise loop on the engine: its latents, `loop_s` marked.  `trace`, `sigmas` (inplace.py:229-242) and `callback_on_step_end`
    (:376-383) travel to the engine's loop when given."""
    if trace is not None:
        kw["trace"] = trace
    if sigmas is not None:
        kw["sigmas"] = sigmas
    if callback_on_step_end is not None:
        kw["callback_on_step_end"] = callback_on_step_end
        kw["callback_on_step_end_tensor_inputs"] = tuple(callback_on_step_end_tensor_inputs)
    latents = eng(**kw)[0]
    clk.mark("loop_s")
    return latents


def _finish(host, clk, out, return_dict):
    """The end of every hosted call: the host's offload hooks, `decode_s` marked, the stock pipelines' return shape."""
    if hasattr(host, "maybe_free_model_hooks"):
        host.maybe_free_model_hooks()
    clk.mark("decode_s")
    return HostedOutput(out, clk.out) if return_dict else (out,)


def _wh(img):
    """(width, height) of a PIL image or of a [..., H, W] tensor."""
    return img.size if hasattr(img, "size") and not isinstance(img, torch.Tensor) else (img.shape[-1], img.shape[-2])


def _keyword_only_call(fn):
    """`__call__(self, **kw)` of a hosted pipeline object or class: `fn(self, **kw)` without autograd; positional arguments are refused."""
    @torch.no_grad()
    def __call__(self, *a, **kw):
        if a:
            raise TypeError("pass the pipeline arguments by keyword (image=..., prompt=...)")
        return fn(self, **kw)
    return __call__


def _hosted_flux(host, eng, image=None, prompt=None, prompt_2=None, negative_prompt=None, negative_prompt_2=None,
                 true_cfg_scale: float = 1.0, height=None, width=None, num_inference_steps: int = 28, guidance_scale: float = 3.5,
                 num_images_per_prompt: int = 1, generator=None, latents=None, prompt_embeds=None, pooled_prompt_embeds=None,
                 negative_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type: str = "pil",
                 return_dict: bool = True, max_sequence_length: int = 512, max_area: int = 1024 ** 2, _auto_resize: bool = True,
                 preferred_resolutions=None, trace=None, sigmas=None, callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs=("latents",), **unused):
    """FluxKontextPipeline.__call__ around the engine loop (RegionE/FluxKontext/inplace.py:112-240, :396-410)."""
    unused = _lora_call(host, eng, unused, "joint_attention_kwargs")
    _refuse_unused("FluxKontextPipeline.__call__", unused)
    dev = eng.transformer.device
    clk = _Clock(dev)
    multiple_of = host.vae_scale_factor * 2
    preferred = PREFERRED_KONTEXT_RESOLUTIONS if preferred_resolutions is None else preferred_resolutions
    # 1. image preprocessing (inplace.py:115-140)
    if image is not None and not (isinstance(image, torch.Tensor) and image.size(1) == host.latent_channels):
        img = image[0] if isinstance(image, list) else image
        image_height, image_width = host.image_processor.get_default_height_width(img)
        if _auto_resize and preferred:
            ar = image_width / image_height
            _, image_width, image_height = min((abs(ar - w / h), w, h) for w, h in preferred)
        image_width, image_height = image_width // multiple_of * multiple_of, image_height // multiple_of * multiple_of
        io = _image_inputs_on_device(host, dev, image if isinstance(image, list) else [image])
        if io is not None and not (isinstance(image, list) and len(image) != 1):
            image = io.to_vae_input(io.resize(io.upload(img), image_height, image_width, "lanczos"))     # the same bits, on the device
        else:
            image = host.image_processor.resize(image, image_height, image_width)
            image = host.image_processor.preprocess(image, image_height, image_width)
        height, width = image.shape[-2], image.shape[-1]
    else:
        height = height or host.default_sample_size * host.vae_scale_factor
        width = width or host.default_sample_size * host.vae_scale_factor
        ar = width / height
        width = round((max_area * ar) ** 0.5) // multiple_of * multiple_of
        height = round((max_area / ar) ** 0.5) // multiple_of * multiple_of
    # 2./3. prompts (inplace.py:142-208)
    _one_image_only(prompt, num_images_per_prompt)
    exec_dev = getattr(host, "_execution_device", dev)
    has_neg = negative_prompt is not None or (negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None)
    do_true_cfg = true_cfg_scale > 1 and has_neg
    with _hip_text_encoders(host, dev):
        prompt_embeds, pooled_prompt_embeds, _ = host.encode_prompt(
            prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
            device=exec_dev, num_images_per_prompt=1, max_sequence_length=max_sequence_length, lora_scale=None)
        if do_true_cfg:
            negative_prompt_embeds, negative_pooled_prompt_embeds, _ = host.encode_prompt(
                prompt=negative_prompt, prompt_2=negative_prompt_2, prompt_embeds=negative_prompt_embeds,
                pooled_prompt_embeds=negative_pooled_prompt_embeds, device=exec_dev, num_images_per_prompt=1,
                max_sequence_length=max_sequence_length, lora_scale=None)
    # 4. latents: the host packs noise and the VAE-encoded condition image (inplace.py:210-226)
    with _hip_vae_encode(host, dev):
        latents, image_latents, _, _ = host.prepare_latents(image, 1, eng.transformer.cfg_model.in_channels // 4, height, width,
                                                            prompt_embeds.dtype, exec_dev, generator, latents)
    if image_latents is None:
        raise ValueError("FluxKontext editing needs a condition image")
    clk.mark("encode_s")
    # 5.-6. the denoise loop on the engine (inplace.py:228-394)
    kw = dict(image=_bf(image_latents, dev), prompt_embeds=_bf(prompt_embeds, dev), pooled_prompt_embeds=_bf(pooled_prompt_embeds, dev),
              height=height, width=width, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
              latents=_bf(latents, dev), return_dict=False, true_cfg_scale=true_cfg_scale,
              negative_prompt_embeds=_bf(negative_prompt_embeds, dev) if do_true_cfg else None,
              negative_pooled_prompt_embeds=_bf(negative_pooled_prompt_embeds, dev) if do_true_cfg else None)
    latents = _run_loop(eng, clk, kw, trace, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs)
    # 7. decode (inplace.py:396-410)
    if output_type == "latent":
        out = latents
    else:
        vae = host.vae
        lat = host._unpack_latents(latents.to(vae.dtype if hasattr(vae, "dtype") else latents.dtype), height, width,
                                   host.vae_scale_factor)
        lat = lat / vae.config.scaling_factor + vae.config.shift_factor
        out = _postprocess_image(host, vae, lat, dev, output_type)
    return _finish(host, clk, out, return_dict)


def _hosted_step1x(host, eng, image=None, prompt=None, negative_prompt=None, true_cfg_scale: float = 6.0, height=None, width=None,
                   num_inference_steps: int = 28, guidance_scale: float = 6.0, num_images_per_prompt: int = 1, generator=None,
                   latents=None, prompt_embeds=None, prompt_embeds_mask=None, negative_prompt_embeds=None,
                   negative_prompt_embeds_mask=None, output_type: str = "pil", return_dict: bool = True,
                   timesteps_truncate: float = 0.93, process_norm_power: float = 0.4, size_level=None, trace=None, sigmas=None,
                   callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), enable_thinking_mode=None,
                   enable_reflection_mode=None, max_try_cnt=None, **unused):
    """Step1XEditPipeline / Step1XEditPipelineV1P2 `__call__` around the engine loop (Step1XEdit/inplace.py:185-330,:437-455;
    Step1XEditV1P2/inplace.py:192-300, :470-543).  One edit - `encode_image` to `_output_process_image` - is `edit_once`; the host's own
    `encode_prompt` runs with `text_encoder` bound to the adopted HIP Qwen2.5-VL encoder and the VLM image processor on the device.
    v1p2's switches `enable_thinking_mode` / `enable_reflection_mode` / `max_try_cnt` (:107-109) run `reflection_loop` (adapters/thinking.py)
    around `edit_once` with the host's thinker (`thinker_for`; a host without one raises NotImplementedError) and return a HostedOutput
    with `images`, `final_images`, `think_info`, `best_info` (and `reformat_prompt` with thinking on) whatever `return_dict` says, as the
    reference does.  `enable_reflection_mode` left unspecified runs ONE attempt without reflection, with a warning (the reference's
    signature default is reflection on: stated deviation).  `timing`: encode_s / loop_s / decode_s summed over the tries,
    `think_s`, `reflect_s`, and `tries` (one dict per try)."""
    unused = _lora_call(host, eng, unused, "joint_attention_kwargs")
    v1p2 = _host_name(host).endswith("V1P2")
    think = dict(enable_thinking_mode=enable_thinking_mode, enable_reflection_mode=enable_reflection_mode, max_try_cnt=max_try_cnt)
    dev = eng.transformer.device
    retry = None
    if v1p2:
        for k in ("enable_thinking_mode", "enable_reflection_mode"):
            if think[k] and retry is None:
                retry = _STEP1X_RETRY[0](host, dev, k)        # finds the host's thinker, or raises the NotImplementedError naming `k`
        if enable_reflection_mode and output_type == "latent":
            raise ValueError(f"{_host_name(host)}.__call__: enable_reflection_mode=True with output_type=\"latent\": reflection shows the "
                             "edited IMAGE to the VLM, latents cannot be reflected on")
        if enable_reflection_mode is None:
            # the reference's signature default is reflection ON (Step1XEditV1P2/inplace.py:108): a caller that leaves it unspecified
            # gets ONE attempt here - say so instead of deviating silently (advisor finding, round 4)
            warnings.warn(f"{_host_name(host)}.__call__: enable_reflection_mode left unspecified - the reference defaults to True (a VLM "
                          "reflection retry loop), the HIP-hosted call runs ONE attempt without reflection; pass "
                          "enable_reflection_mode=False to acknowledge", stacklevel=3)
    else:                                   # v1p1 has no such arguments: a caller passing them gets the usual refusal
        unused = dict(unused, **{k: v for k, v in think.items() if v is not None})
    _refuse_unused(_host_name(host) + ".__call__", unused)
    exec_dev = getattr(host, "_execution_device", dev)
    _one_image_only(prompt, num_images_per_prompt)
    # the prompt encoder of this host (adopted at attach(); here for a caller that came another way), before anything binds it
    hip_qwen_text_encoder_for(host, dev, sampling_default=_step1x_text_sampling_default(host))
    embeds_in = (prompt_embeds, prompt_embeds_mask, negative_prompt_embeds, negative_prompt_embeds_mask)
    tries = []

    def edit_once(image, prompt):
        nonlocal width, height                                # carried from try to try (Step1XEditV1P2/inplace.py:214 reassigns them)
        clk = _Clock(dev)
        prompt_embeds, prompt_embeds_mask, negative_prompt_embeds, negative_prompt_embeds_mask = embeds_in
        neg_prompt = negative_prompt
        # 1. image (host.encode_image resizes, keeps the reference image for the VLM, remembers how to undo the resize)
        args = (image, width, height, size_level, exec_dev, 1) if v1p2 else (image, width, height, exec_dev, 1)
        image, ref_image, img_info, width, height = host.encode_image(*args)
        # 2./3. prompts through the host's VLM encoder: its language model and vision tower on the HIP kernels, its image processor on
        # the device
        has_neg = neg_prompt is not None or (negative_prompt_embeds is not None and negative_prompt_embeds_mask is not None)
        if not has_neg:
            neg_prompt = "" if image is not None else STEP1X_DEFAULT_NEGATIVE
        with _hip_qwen_text_encoder(host, dev), _hip_qwen_image_processor(host, dev):
            if v1p2:      # encode_prompt returns a record: embedding / mask / txt_ids / text_embeds / text_masks (:241-254)
                pos = host.encode_prompt(ref_image=ref_image, prompt=prompt, device=exec_dev, num_images_per_prompt=1)
                neg = host.encode_prompt(ref_image=ref_image, prompt=neg_prompt, device=exec_dev, num_images_per_prompt=1)
                prompt_embeds, prompt_embeds_mask = pos.embedding, pos.mask
                negative_prompt_embeds, negative_prompt_embeds_mask = neg.embedding, neg.mask
                text = [(pos.text_embeds, pos.text_masks), (neg.text_embeds, neg.text_masks)]
                dtype = pos.embedding.dtype
            else:
                prompt_embeds, prompt_embeds_mask, _ = host.encode_prompt(
                    ref_image=ref_image, prompt=prompt, prompt_embeds=prompt_embeds, prompt_embeds_mask=prompt_embeds_mask,
                    device=exec_dev, num_images_per_prompt=1)
                negative_prompt_embeds, negative_prompt_embeds_mask, _ = host.encode_prompt(
                    ref_image=ref_image, prompt=neg_prompt, prompt_embeds=negative_prompt_embeds,
                    prompt_embeds_mask=negative_prompt_embeds_mask, device=exec_dev, num_images_per_prompt=1)
                text, dtype = None, prompt_embeds.dtype
        # 4. latents
        pl = (image, 1, eng.transformer.cfg_model.in_channels // 4, height, width, dtype, exec_dev, generator)
        with _hip_vae_encode(host, dev):
            lat, image_latents, _, _ = host.prepare_latents(*pl) if v1p2 else host.prepare_latents(*pl, latents)
        # the connector: the adopted HIP one (prepared once per edit, advanced per computed step), or the host module per branch per step
        masks, embeds = [prompt_embeds_mask, negative_prompt_embeds_mask], [prompt_embeds, negative_prompt_embeds]
        hip = hip_step1x_connector_for(host, dev)
        if hip is not None:
            why, n_valid = _HipConnector.parse(masks, embeds)
            if why is not None:
                warnings.warn(f"connector kept on the host module for this call: {why}", RuntimeWarning, stacklevel=5)
                hip = None
        if hip is not None:
            connector = _HipConnector(hip, host.transformer, dev, n_valid, embeds, text)
            connector.bind_text()
        else:
            connector = _HostConnector(host.transformer, dev, masks, text)
        clk.mark("encode_s")
        # 5.-6. loop on the engine; the connector feeds it per computed step
        kw = dict(image=_bf(image_latents, dev), prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                  pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, height=height, width=width,
                  num_inference_steps=num_inference_steps, true_cfg_scale=true_cfg_scale, guidance_scale=guidance_scale,
                  latents=_bf(lat, dev), return_dict=False, timesteps_truncate=timesteps_truncate,
                  process_norm_power=process_norm_power)
        with _bound(eng.transformer, "connector", connector):
            lat = _run_loop(eng, clk, kw, trace, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs)
        # 7. decode (:437-446)
        if output_type == "latent":
            out = lat
        else:
            vae = host.vae
            lat = host._unpack_latents(lat.to(getattr(vae, "dtype", lat.dtype)), height, width, host.vae_scale_factor)
            lat = lat / vae.config.scaling_factor + vae.config.shift_factor
            out = _postprocess_image(host, vae, lat, dev, output_type)
            out = host._output_process_image(out, img_info)
        clk.mark("decode_s")
        tries.append(clk.out)
        return out

    if retry is None:                                         # one attempt, no VLM prompting: the call as it always was
        out = edit_once(image, prompt)
    else:
        res = retry(edit_once, image, prompt, enable_thinking_mode, enable_reflection_mode, 3 if max_try_cnt is None else max_try_cnt)
        out = res.images
    if hasattr(host, "maybe_free_model_hooks"):               # once, after the last try (:488-489)
        host.maybe_free_model_hooks()
    timing = {k: sum(t[k] for t in tries) for k in ("encode_s", "loop_s", "decode_s")}
    if retry is None:
        return HostedOutput(out, timing) if return_dict else (out,)
    timing.update(retry.thinker.seconds, tries=tries)
    extra = dict(final_images=res.final_images, think_info=res.think_info, best_info=res.best_info)
    if enable_thinking_mode:
        extra["reformat_prompt"] = res.reformat_prompt
    return HostedOutput(out, timing, **extra)


def _qwen_dims(target_area, ratio):
    """calculate_dimensions (QwenImageEdit/utils.py:96-103)."""
    import math
    width = math.sqrt(target_area * ratio)
    height = width / ratio
    return round(width / 32) * 32, round(height / 32) * 32


def _hosted_qwen(host, eng, image=None, prompt=None, negative_prompt=None, true_cfg_scale: float = 4.0, height=None, width=None,
                 num_inference_steps: int = 28, guidance_scale=None, num_images_per_prompt: int = 1, generator=None, latents=None,
                 prompt_embeds=None, prompt_embeds_mask=None, negative_prompt_embeds=None, negative_prompt_embeds_mask=None,
                 output_type: str = "pil", return_dict: bool = True, max_sequence_length: int = 512, trace=None, sigmas=None,
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), **unused):
    """QwenImageEditPipeline / QwenImageEditPlusPipeline `__call__` around the engine loop (QwenImageEdit/inplace.py:180-330,
    :434-455; QwenImageEditPlus/inplace.py:189-300: a LIST of condition images, each resized twice - 384^2 area for the VLM,
    1024^2 area for the VAE - the last one fixing the output size)."""
    unused = _lora_call(host, eng, unused, "attention_kwargs")
    _refuse_unused(_host_name(host) + ".__call__", unused)
    plus = "Plus" in _host_name(host)
    dev = eng.transformer.device
    clk = _Clock(dev)
    exec_dev = getattr(host, "_execution_device", dev)
    _one_image_only(prompt, num_images_per_prompt)
    imgs = image if isinstance(image, list) else [image]
    ref = imgs[-1] if plus else imgs[0]
    ref_w, ref_h = _wh(ref)
    calc_w, calc_h = _qwen_dims(1024 * 1024, ref_w / ref_h)
    height, width = height or calc_h, width or calc_w
    multiple_of = host.vae_scale_factor * 2
    width, height = width // multiple_of * multiple_of, height // multiple_of * multiple_of
    tok = lambda px: px // host.vae_scale_factor // 2
    is_latent = isinstance(image, torch.Tensor) and image.size(1) == getattr(host, "latent_channels", -1)
    io = None if is_latent or (not plus and isinstance(image, list)) else _image_inputs_on_device(host, dev, imgs)
    twins = {}                                             # id(prompt image) -> its uint8 twin on the device (the VLM stage reads it there)

    def prompt_twin(u8):
        pil = io.to_pil(u8)                                # the host's encode_prompt wants a PIL image: one download
        twins[id(pil)] = u8
        return pil
    if plus and not is_latent:
        prompt_image, vae_images, cond_shapes = [], [], []
        for img in imgs:
            iw, ih = _wh(img)
            cw, ch = _qwen_dims(QWEN_CONDITION_IMAGE_SIZE, iw / ih)
            vw, vh = _qwen_dims(QWEN_VAE_IMAGE_SIZE, iw / ih)
            if io is not None:
                u8 = io.upload(img)
                prompt_image.append(prompt_twin(io.resize(u8, ch, cw, "lanczos")))
                vae_images.append(io.to_vae_input(io.resize(u8, vh, vw, "lanczos")).unsqueeze(2))
            else:
                prompt_image.append(host.image_processor.resize(img, ch, cw))
                vae_images.append(host.image_processor.preprocess(img, vh, vw).unsqueeze(2))
            cond_shapes.append((tok(vh), tok(vw)))
        image = vae_images
    elif not is_latent and io is not None:
        u8 = io.resize(io.upload(image), calc_h, calc_w, "lanczos")
        prompt_image = prompt_twin(u8)
        image = io.to_vae_input(u8).unsqueeze(2)
        cond_shapes = [(tok(calc_h), tok(calc_w))]
    elif not is_latent:
        image = host.image_processor.resize(image, calc_h, calc_w)
        prompt_image = image
        image = host.image_processor.preprocess(image, calc_h, calc_w).unsqueeze(2)
        cond_shapes = [(tok(calc_h), tok(calc_w))]
    else:
        prompt_image, cond_shapes = None, None
    has_neg = negative_prompt is not None or (negative_prompt_embeds is not None and negative_prompt_embeds_mask is not None)
    do_true_cfg = true_cfg_scale > 1 and has_neg
    enc = lambda p, e, m: host.encode_prompt(image=prompt_image, prompt=p, prompt_embeds=e, prompt_embeds_mask=m, device=exec_dev,
                                             num_images_per_prompt=1, max_sequence_length=max_sequence_length)
    # the Qwen2.5-VL language model of encode_prompt on the HIP kernels; its image processor on the device
    with _hip_qwen_text_encoder(host, dev), _hip_qwen_image_processor(host, dev, twins):
        prompt_embeds, prompt_embeds_mask = enc(prompt, prompt_embeds, prompt_embeds_mask)
        if do_true_cfg:
            negative_prompt_embeds, negative_prompt_embeds_mask = enc(negative_prompt, negative_prompt_embeds, negative_prompt_embeds_mask)
    with _hip_vae_encode(host, dev):                       # vae.encode of the condition images on the HIP encoder (Qwen VAE: one frame each)
        latents, image_latents = host.prepare_latents(image, 1, eng.transformer.cfg_model.in_channels // 4, height, width,
                                                      prompt_embeds.dtype, exec_dev, generator, latents)
    clk.mark("encode_s")
    kw = dict(image=_bf(image_latents, dev), prompt_embeds=_bf(prompt_embeds, dev),
              negative_prompt_embeds=_bf(negative_prompt_embeds, dev) if do_true_cfg else None, height=height, width=width,
              num_inference_steps=num_inference_steps, true_cfg_scale=true_cfg_scale, latents=_bf(latents, dev),
              return_dict=False, cond_shapes=cond_shapes)
    latents = _run_loop(eng, clk, kw, trace, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs)
    if output_type == "latent":
        out = latents
    else:                                                                                  # QwenImageEdit/inplace.py:437-451
        vae = host.vae
        lat = host._unpack_latents(latents, height, width, host.vae_scale_factor).to(vae.dtype)
        mean = torch.tensor(vae.config.latents_mean).view(1, vae.config.z_dim, 1, 1, 1).to(lat.device, lat.dtype)
        inv_std = 1.0 / torch.tensor(vae.config.latents_std).view(1, vae.config.z_dim, 1, 1, 1).to(lat.device, lat.dtype)
        out = _postprocess_qwen_image(host, vae, lat / inv_std + mean, dev, output_type)
    return _finish(host, clk, out, return_dict)


_HOSTED = {"FluxKontextPipeline": _hosted_flux, "Step1XEditPipeline": _hosted_step1x, "Step1XEditPipelineV1P2": _hosted_step1x,
           "QwenImageEditPipeline": _hosted_qwen, "QwenImageEditPlusPipeline": _hosted_qwen}


def is_engine_pipeline(pipe) -> bool:
    """True for a regione_amd.harness pipeline (latent-level, HIP transformer); False for a stock host pipeline."""
    from ..harness import flux as HF
    return isinstance(pipe, HF.FluxKontextPipeline) or isinstance(getattr(pipe, "transformer", None), HF.FluxTransformer2DModel)


class HostedPipeline:
    """Wrapper object: `hosted(image=..., prompt=...)` = host pre / post-processing + engine loop.  `RegionEHelper(hosted)`
    patches the engine.  (RegionEHelper(pipe) on the stock pipeline itself is the reference's call shape - see attach.)"""

    def __init__(self, host, engine):
        self.host, self._regione_engine = host, engine
        self._call = _HOSTED[_host_name(host)]

    @property
    def engine(self):
        return self._regione_engine

    __call__ = _keyword_only_call(lambda self, **kw: self._call(self.host, self._regione_engine, **kw))


HostedFluxKontextPipeline = HostedPipeline          # round-1 name


def adopt(pipe, device="cuda"):
    """Hosted wrapper (image + prompt in, image out) for any of the five pipeline classes."""
    if _host_name(pipe) not in _HOSTED:
        raise NotImplementedError(f"no hosted call for {pipe.__class__.__name__}")
    return HostedPipeline(pipe, attach(pipe, device))


def attach(pipe, device="cuda"):
    """Adopt the host pipeline's transformer once and keep the engine ON the host object (`pipe._regione_engine`)."""
    eng = pipe.__dict__.get("_regione_engine") if hasattr(pipe, "__dict__") else None
    if eng is not None:
        lora_sync(pipe, eng)                                  # adapters loaded, switched or removed since the adoption
    if eng is None:
        eng = adopt_engine(pipe, device)
        pipe._regione_engine = eng
        # the VAE too, HERE rather than inside the first edit (weights are re-laid once: ~0.5 s that would otherwise sit in that edit's
        # decode_s / encode_s); a VAE of another layout returns None and keeps running on the host module
        if getattr(pipe, "vae", None) is not None:
            dev = eng.transformer.device
            hip_vae_for(pipe, dev)
            hip_vae_encoder_for(pipe, dev)
        if _host_name(pipe) == "FluxKontextPipeline":         # the text encoders of encode_prompt likewise (CLIP-L, T5-XXL)
            hip_text_encoders_for(pipe, eng.transformer.device)
        if _host_name(pipe) in _QWEN_TEXT_HOSTS:              # Qwen-Image-Edit's prompt encoder: the Qwen2.5-VL language model
            hip_qwen_text_encoder_for(pipe, eng.transformer.device)
        if _host_name(pipe) in _STEP1X_TEXT_HOSTS:            # Step1X-Edit's prompt encoder and v1p2's thinker: the same module
            hip_qwen_text_encoder_for(pipe, eng.transformer.device, sampling_default=_step1x_text_sampling_default(pipe))
    return eng


def swap_host_class(pipe):
    """Hook (1) of the reference (`pipeline.__class__ = RegionE<...>Pipeline`, inplace.py:53-62) on the HOST object: a
    subclass of the host's own class whose `__call__` is the hosted call.  The user keeps calling `pipe(...)`."""
    if getattr(pipe, "_regione_host_class", None) is not None:
        return pipe
    base = pipe.__class__
    call = _HOSTED[base.__name__]
    pipe._regione_host_class = base
    pipe.__class__ = type("RegionE" + base.__name__, (base,), {
        "__call__": _keyword_only_call(lambda self, **kw: call(self, self._regione_engine, **kw))})
    return pipe


def restore_host_class(pipe):
    base = getattr(pipe, "_regione_host_class", None)
    if base is not None:
        pipe.__class__ = base
        pipe._regione_host_class = None
    return pipe
