"""The host pipeline's components outside the trunk on the HIP kernels: both VAEs, CLIP / T5, the Qwen2.5-VL prompt encoder with its vision
tower, the image processors.  Each `hip_*_for` adopts once per host pipeline and keeps the result on it as `_regione_hip_*` (the switches
its docstring documents); each `_hip_*` binder puts the adopted object in front of the host's own method for the length of a `with`."""
from __future__ import annotations

import contextlib
import warnings
from typing import Optional

import torch

from .. import _lib

_UNSET = object()


def _memo(host, attr):
    """What an earlier call kept on the host pipeline as `attr` (its instance dict only), or _UNSET."""
    return host.__dict__.get(attr, _UNSET)


def _adopt_or_keep(label: str, why: Optional[str], make, stacklevel: int):
    """`make()` when no refusal `why` stands; a RegionEHipError it raises is a refusal as well.  A refusal keeps the host module: one
    RuntimeWarning naming the reason, seen `stacklevel` frames up from the caller (what the caller would hand warnings.warn), and None."""
    if why is None:
        try:
            return make()
        except _lib.RegionEHipError as e:
            why = str(e)
    warnings.warn(f"{label} kept on the host module: {why}", RuntimeWarning, stacklevel=stacklevel + 1)
    return None


@contextlib.contextmanager
def _bound(obj, attr, value):
    """`obj.attr` is `value` inside the `with` - written to the instance dict: no __setattr__ (a diffusers pipeline would re-register the
    component).  On exit, an exception included, the previous instance-dict entry is back, or the key is gone if there was none."""
    d = obj.__dict__
    prev = d.get(attr, _UNSET)
    d[attr] = value
    try:
        yield value
    finally:
        if prev is _UNSET:
            del d[attr]
        else:
            d[attr] = prev


def _host_name(pipe) -> str:
    cls = getattr(pipe, "_regione_host_class", None) or pipe.__class__
    return cls.__name__


def _bf(t, dev):
    return t.to(device=dev, dtype=torch.bfloat16) if t is not None else None


def _is_qwen_vae(vae) -> bool:
    """The [EXT] AutoencoderKLQwenImage layout (3-D causal VAE of the Qwen-Image pipelines): RMS_norm `norm_out`, a Wan-style config."""
    cfg = getattr(vae, "config", None)
    return all(getattr(getattr(vae, p, None), "norm_out", None) is not None for p in ("decoder", "encoder")) and \
        getattr(cfg, "base_dim", None) is not None and getattr(cfg, "z_dim", None) is not None and hasattr(vae, "state_dict")


def _adopt_qwen_vae(host, dev):
    """Both halves of a Qwen-Image VAE onto the HIP kernels (regione_amd/qwen_vae.py), once per host pipeline.  Whatever the kernels do not
    cover (another config, unknown or missing parameters, a dtype other than bf16 / fp32) keeps the host module, with one warning naming
    the reason: (None, None)."""
    from .. import qwen_vae as Q
    vae = host.vae
    cfg, want = vae.config, Q.QWEN_VAE_CONFIG
    got = {k: (tuple(getattr(cfg, k)) if isinstance(want[k], tuple) else getattr(cfg, k)) if hasattr(cfg, k) else None for k in want}

    def make():
        sd = vae.state_dict()
        return Q.HipQwenVaeDecoder(sd, dev, out_dtype=vae.dtype), Q.HipQwenVaeEncoder(sd, dev, out_dtype=vae.dtype)
    why = f"config {got} (the kernels cover {want})" if got != want else None
    return _adopt_or_keep("Qwen-Image VAE", why, make, stacklevel=3) or (None, None)


def _qwen_vae_refusal(vae, x, kind: str, kw=None) -> Optional[str]:
    """Why the HIP Qwen-Image VAE does not serve this `vae.decode(z)` / `vae.encode(x)` call (None: it does)."""
    from .. import qwen_vae as Q
    if kw:
        return f"{kind} arguments {sorted(kw)}"
    if getattr(vae, "use_tiling", False) or getattr(vae, "use_slicing", False):
        return "vae.use_tiling / use_slicing is set"
    if not isinstance(x, torch.Tensor) or x.dim() != 5:
        return f"{kind} of a {getattr(x, 'dim', lambda: '?')()}-D input (one [1, C, 1, H, W] frame is covered)"
    if x.shape[0] != 1:
        return f"batch {x.shape[0]} > 1"
    if x.shape[2] != 1:
        return f"T = {x.shape[2]} frames (single images are covered)"
    if kind == "encode" and (x.shape[1] != 3 or x.shape[3] % 8 or x.shape[4] % 8):
        return f"image {tuple(x.shape)} (3 channels, H and W multiples of 8 are covered)"
    h, w = (x.shape[3], x.shape[4]) if kind == "decode" else (x.shape[3] // 8, x.shape[4] // 8)
    if (h + 2) * (w + 2) > Q.SOFTMAX_MAX_ROWS:
        return f"latent {h} x {w}: (h + 2) (w + 2) > {Q.SOFTMAX_MAX_ROWS}, the mid-block softmax's limit"
    return None


def _kl_kwargs(cfg) -> dict:
    """The widths an AutoencoderKL config states, as HipVaeDecoder / HipVaeEncoder keyword arguments (what it leaves out keeps their default)."""
    kw = {}
    for name in ("block_out_channels", "latent_channels", "layers_per_block"):
        v = getattr(cfg, name, None) if cfg is not None else None
        if v is not None:
            kw[name] = tuple(v) if name == "block_out_channels" else int(v)
    return kw


def hip_vae_for(host, dev):
    """The host's AutoencoderKL decoder adopted onto the HIP kernels (regione_amd/vae.py) - once per host pipeline,
    kept on it as `_regione_hip_vae`; Qwen-Image's 3-D causal VAE goes to regione_amd/qwen_vae.py (`_adopt_qwen_vae`, both halves at once).
    None when the host's VAE is of neither layout (e.g. a module with a post_quant_conv): the host module then decodes, exactly as in the reference (`self.vae.decode`, FluxKontext/inplace.py:396-402).  A VAE
    that HAS the layout but cannot be adopted (unknown parameters, other widths) raises instead of silently running the slower module;
    `pipe._regione_hip_vae = False` before the first call keeps the host module on purpose."""
    cached = _memo(host, "_regione_hip_vae")
    if cached is False or cached is None:
        return None
    if cached is not _UNSET:
        return cached
    vae = getattr(host, "vae", None)
    if _is_qwen_vae(vae):
        host._regione_hip_vae, host._regione_hip_vae_encoder = _adopt_qwen_vae(host, dev)
        return host._regione_hip_vae
    dec = getattr(vae, "decoder", None)
    ok = dec is not None and all(hasattr(dec, n) for n in ("conv_in", "mid_block", "up_blocks", "conv_norm_out", "conv_out")) and \
        getattr(vae, "post_quant_conv", None) is None and hasattr(dec, "state_dict")
    if not ok:
        host._regione_hip_vae = None
        return None
    from .. import vae as V
    host._regione_hip_vae = V.HipVaeDecoder(dec.state_dict(), dev, **_kl_kwargs(getattr(vae, "config", None)))
    return host._regione_hip_vae


def hip_vae_encoder_for(host, dev):
    """The host's AutoencoderKL ENCODER on the HIP kernels (regione_amd/vae.py HipVaeEncoder), adopted once per host pipeline
    (`_regione_hip_vae_encoder`); None when the VAE has no such encoder, carries a quant_conv, or `pipe._regione_hip_vae = False`."""
    if _memo(host, "_regione_hip_vae") is False:
        return None
    cached = _memo(host, "_regione_hip_vae_encoder")
    if cached is not _UNSET:
        return cached
    vae = getattr(host, "vae", None)
    if _is_qwen_vae(vae):
        if "_regione_hip_vae" not in host.__dict__:
            hip_vae_for(host, dev)
        return host._regione_hip_vae_encoder
    enc = getattr(vae, "encoder", None)
    ok = enc is not None and all(hasattr(enc, n) for n in ("conv_in", "down_blocks", "mid_block", "conv_norm_out", "conv_out")) and \
        getattr(vae, "quant_conv", None) is None and hasattr(enc, "state_dict")
    if not ok:
        host._regione_hip_vae_encoder = None
        return None
    from .. import vae as V
    host._regione_hip_vae_encoder = V.HipVaeEncoder(enc.state_dict(), dev, **_kl_kwargs(getattr(vae, "config", None)))
    return host._regione_hip_vae_encoder


_TEXT_ENCODERS = (("text_encoder", "clip"), ("text_encoder_2", "t5"))


def _adopt_text_encoder(attr: str, mod, kind: str, dev):
    """The HIP encoder of the host's `attr`, or None with the warning naming the reason the host module keeps running."""
    from .. import text_encoders as TE
    cfg = getattr(mod, "config", None)
    if cfg is None or not hasattr(mod, "state_dict"):
        why = f"{type(mod).__name__} is not a transformers module"
    else:
        why = TE.clip_refusal(cfg) if kind == "clip" else TE.t5_refusal(cfg)
        if why is None and type(mod).__name__ != ("CLIPTextModel" if kind == "clip" else "T5EncoderModel"):
            why = f"{type(mod).__name__} (another layout: the kernels restate CLIPTextModel / T5EncoderModel)"
        if why is None and any("lora" in n.lower() for n, _ in mod.named_modules()):
            why = "PEFT / LoRA layers in the module"
    return _adopt_or_keep(attr, why, lambda: TE.HipClipTextModel(mod, dev) if kind == "clip" else TE.HipT5EncoderModel(mod, dev), stacklevel=4)


def hip_text_encoders_for(host, dev):
    """(CLIP, T5) of a FLUX.1 Kontext host adopted onto the HIP kernels (regione_amd/text_encoders.py), once
    per host pipeline and kept on it as `_regione_hip_text`.  A module the kernels do not cover (another layout, head dim != 64, non-bf16
    weights, PEFT / LoRA layers) stays the host's, with one warning naming the reason: None in its place.  A host without the modules
    gets (None, None) silently; `pipe._regione_hip_text = False` before the first call keeps the host modules on purpose."""
    cached = _memo(host, "_regione_hip_text")
    if cached is False or cached is None:
        return None, None
    if cached is not _UNSET:
        return cached
    got = []
    for attr, kind in _TEXT_ENCODERS:
        mod = getattr(host, attr, None)
        got.append(None if mod is None else _adopt_text_encoder(attr, mod, kind, dev))
    host._regione_hip_text = tuple(got)
    return host._regione_hip_text


def _hip_text_encoders(host, dev):
    """`with _hip_text_encoders(host, dev): host.encode_prompt(...)` - the host's own `encode_prompt` (tokenizers, `_get_clip_prompt_embeds`,
    `_get_t5_prompt_embeds`: its code, untouched) runs with `text_encoder` / `text_encoder_2` bound to the adopted HIP encoders; the
    bindings are undone on exit, an exception included."""
    stack = contextlib.ExitStack()
    for (attr, _), enc in zip(_TEXT_ENCODERS, hip_text_encoders_for(host, dev)):
        if enc is not None:
            stack.enter_context(_bound(host, attr, enc))
    return stack


_QWEN_TEXT_HOSTS = ("QwenImageEditPipeline", "QwenImageEditPlusPipeline")
# Step1X-Edit's prompt encoder is the same module; v1p2's thinker also calls its `generate`, under the module's own generation_config
_STEP1X_TEXT_HOSTS = ("Step1XEditPipeline", "Step1XEditPipelineV1P2")


def _step1x_text_sampling_default(host) -> bool:
    """What an absent `_regione_hip_text_sampling` means for this host: True for Step1XEditPipelineV1P2 (Qwen2.5-VL's generation_config
    samples with a repetition penalty, and the thinker passes no decoding argument), False for every other host."""
    return _host_name(host) == "Step1XEditPipelineV1P2"


def hip_qwen_text_encoder_for(host, dev, sampling_default: bool = False):
    """The host's Qwen2.5-VL prompt encoder with its language model adopted onto the HIP kernels (regione_amd/qwen_text_encoder.py;
    SURVEY.md section 8 row f4), once per host pipeline and kept on it as `_regione_hip_qwen_text`.  A module the kernels do not cover
    (`qwen25vl_refusal`: sliding-window layers, another head dim, ...; non-bf16 weights; PEFT / LoRA layers) stays the host's, with one
    warning naming the reason.  With the language model the vision tower is adopted (regione_amd/qwen_vision.py) and handed to the encoder
    as `vision=`; a tower `vision_refusal` names (or one with non-bf16 weights) stays the host's eager module under the adopted language
    model, with one "vision tower kept on the host module: ..." warning; `pipe._regione_hip_vision = False` keeps it there on purpose,
    silently.  A `text_encoder` that is not a `Qwen2_5_VLForConditionalGeneration` is left alone silently;
    `pipe._regione_hip_text = False` before the first call keeps the whole host module on purpose.
    `pipe._regione_hip_text_weights = "fp8"` before the first call adopts the layers' projection matrices as fp8 e4m3fn with per-channel
    scales (HipQwen25VLTextEncoder(weights="fp8")); absent, the adoption is "bf16"; another value raises ValueError naming the two.
    `pipe._regione_hip_text_sampling = True` before the first call adopts with `sampling=True` (generate honours do_sample, temperature,
    top_k, top_p and repetition_penalty); absent, it is False; a value that is not a bool raises ValueError.
    (`sampling_default=True`, what the hosted Step1X-Edit v1p2 call passes, makes an ABSENT switch mean True; an explicit False is honoured.)
    `pipe._regione_hip_text_batch = N` before the first call adopts with `max_batch=N` (generate takes up to N left-padded rows and
    decodes them from one weight stream); absent, it is 1; a value that is not an int in 1..8 raises ValueError naming the range.
    `pipe._regione_hip_text_batch_sampling = True` before the first call adopts with `batch_sampling=True` (such a batch takes the decoding
    configuration of `sampling=True`); absent, it is False; a value that is not a bool, or True without the two switches above, raises
    ValueError naming the attribute that is wrong or missing, with nothing adopted or cached.
    `pipe._regione_hip_text_batch_kernels = "mfma"` before the first call adopts with `batch_kernels="mfma"` (every decode step on the MFMA
    row GEMM); with it `_regione_hip_text_batch` is accepted in 1..32.  Absent, it is "fma" and every message is as above; another value
    raises ValueError naming the two, with nothing adopted or cached.
    `pipe._regione_hip_text_lookup = True` before the first call adopts with `lookup=True` (generate takes prompt_lookup_num_tokens,
    max_matching_ngram_size and draft_tokens and verifies the drafts in one step); absent, it is False; a value that is not a bool raises
    ValueError, with nothing adopted or cached.
    `pipe._regione_hip_text_lookup_sampling = True` before the first call, beside `_regione_hip_text_lookup` and the sampling switch (on by
    default for Step1X-Edit v1p2), adopts with `lookup_sampling=True` (the drafted steps run under the sampled pick, and generate takes
    the module's generation_config.prompt_lookup_num_tokens); absent, it is False; a value that is not a bool, or True without the two
    switches it needs, raises ValueError, with nothing adopted or cached."""
    if _memo(host, "_regione_hip_text") is False:
        return None
    cached = _memo(host, "_regione_hip_qwen_text")
    if cached is not _UNSET:
        return cached
    fmt = host.__dict__.get("_regione_hip_text_weights", "bf16")
    if fmt not in ("bf16", "fp8"):
        raise ValueError(f"pipe._regione_hip_text_weights = {fmt!r}: \"bf16\" and \"fp8\" are accepted")
    sampling = host.__dict__.get("_regione_hip_text_sampling", sampling_default)
    if not isinstance(sampling, bool):
        raise ValueError(f"pipe._regione_hip_text_sampling = {sampling!r}: True and False are accepted")
    kernels = host.__dict__.get("_regione_hip_text_batch_kernels", "fma")
    if not isinstance(kernels, str) or kernels not in ("fma", "mfma"):
        raise ValueError(f"pipe._regione_hip_text_batch_kernels = {kernels!r}: \"fma\" and \"mfma\" are accepted")
    batch = host.__dict__.get("_regione_hip_text_batch", 1)
    top = 32 if kernels == "mfma" else 8
    if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= top:
        raise ValueError(f"pipe._regione_hip_text_batch = {batch!r}: an int in 1..{top} is accepted")
    rows_pick = host.__dict__.get("_regione_hip_text_batch_sampling", False)
    if not isinstance(rows_pick, bool):
        raise ValueError(f"pipe._regione_hip_text_batch_sampling = {rows_pick!r}: True and False are accepted")
    if rows_pick and not sampling:
        raise ValueError("pipe._regione_hip_text_batch_sampling = True needs pipe._regione_hip_text_sampling = True")
    if rows_pick and batch < 2:
        raise ValueError(f"pipe._regione_hip_text_batch_sampling = True needs pipe._regione_hip_text_batch = N with N in 2..{top}")
    lookup = host.__dict__.get("_regione_hip_text_lookup", False)
    if not isinstance(lookup, bool):
        raise ValueError(f"pipe._regione_hip_text_lookup = {lookup!r}: True and False are accepted")
    look_pick = host.__dict__.get("_regione_hip_text_lookup_sampling", False)
    if not isinstance(look_pick, bool):
        raise ValueError(f"pipe._regione_hip_text_lookup_sampling = {look_pick!r}: True and False are accepted")
    if look_pick and not lookup:
        raise ValueError("pipe._regione_hip_text_lookup_sampling = True needs pipe._regione_hip_text_lookup = True")
    if look_pick and not sampling:
        raise ValueError("pipe._regione_hip_text_lookup_sampling = True needs pipe._regione_hip_text_sampling = True")
    mod = getattr(host, "text_encoder", None)
    enc = None
    if type(mod).__name__ == "Qwen2_5_VLForConditionalGeneration" and getattr(mod, "config", None) is not None:
        from .. import qwen_text_encoder as QT
        why = QT.qwen25vl_refusal(mod.config)
        if why is None and any("lora" in n.lower() for n, _ in mod.named_modules()):
            why = "PEFT / LoRA layers in the module"
        enc = _adopt_or_keep("text_encoder", why, stacklevel=3,
                             make=lambda: QT.HipQwen25VLTextEncoder(mod, dev, weights=fmt, **({"sampling": True} if sampling else {}),
                                                                    **({"max_batch": batch} if batch > 1 else {}),
                                                                    **({"batch_sampling": True} if rows_pick else {}),
                                                                    **({"batch_kernels": "mfma"} if kernels == "mfma" else {}),
                                                                    **({"lookup": True} if lookup else {}),
                                                                    **({"lookup_sampling": True} if look_pick else {})))
        if enc is not None and _memo(host, "_regione_hip_vision") is not False:
            from .. import qwen_vision as QV
            tower = _adopt_or_keep("vision tower", QV.vision_refusal(mod.config), lambda: QV.HipQwen25VLVisionTower(mod, dev), stacklevel=3)
            if tower is not None:
                enc.vision = tower
    host._regione_hip_qwen_text = enc
    return enc


def _hip_qwen_text_encoder(host, dev):
    """`with _hip_qwen_text_encoder(host, dev): host.encode_prompt(...)` - the host's own `encode_prompt` (the template, the processor,
    `_get_qwen_prompt_embeds`, `_extract_masked_hidden`: its code, untouched) runs with `text_encoder` bound to the adopted HIP encoder,
    which answers what that code touches (the call, `.dtype`, `.device`, `.config`); the binding is undone on exit, an exception included."""
    enc = hip_qwen_text_encoder_for(host, dev)
    return _bound(host, "text_encoder", enc) if enc is not None else contextlib.nullcontext()


def _hip_vae_encode(host, dev):
    """`with _hip_vae_encode(host, dev): host.prepare_latents(...)` - the host's own `prepare_latents` (resize, `_encode_vae_image`,
    `retrieve_latents`, shift / scale, packing: its code, untouched) runs with `vae.encode` answered by the HIP encoder for single 4-D
    images; anything else (batches, 5-D video-style inputs) falls through to the module's own method.  The binding is undone on exit."""
    enc = hip_vae_encoder_for(host, dev)
    if enc is None:
        return contextlib.nullcontext()
    vae = host.vae
    own = vae.encode
    qwen = _is_qwen_vae(vae)

    def encode(x, return_dict=True, **kw):
        if qwen:
            why = _qwen_vae_refusal(vae, x, "encode", kw)
            if why is None:
                out = enc.encode_dist(x.to(dev))
                return out if return_dict else (out.latent_dist,)
            warnings.warn(f"Qwen-Image VAE encode on the host module: {why}", RuntimeWarning, stacklevel=2)
            return own(x, return_dict=return_dict, **kw)
        if isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[0] == 1 and x.shape[1] == 3 and not kw:
            out = enc.encode_dist(x.to(dev))
            return out if return_dict else (out.latent_dist,)
        return own(x, return_dict=return_dict, **kw)
    return _bound(vae, "encode", encode)


def _decode_image(host, vae, lat, dev):
    """`vae.decode(lat, return_dict=False)[0]` - on the HIP decoder when the host's VAE is an AutoencoderKL (one image per call)."""
    hv = hip_vae_for(host, dev)
    if hv is not None and lat.dim() == 4 and lat.shape[0] == 1:
        return hv.decode(lat.to(dev))
    return vae.decode(lat, return_dict=False)[0]


def _decode_qwen_image(host, vae, z, dev):
    """`vae.decode(z, return_dict=False)[0][:, :, 0]` of the Qwen pipelines (QwenImageEdit/inplace.py:437-451) - on the HIP decoder when the
    host's VAE was adopted and the call is one it covers, else on the host module (with a warning naming the reason)."""
    from .. import qwen_vae as Q
    hv = hip_vae_for(host, dev)
    if isinstance(hv, Q.HipQwenVaeDecoder):
        why = _qwen_vae_refusal(vae, z, "decode")
        if why is None:
            return hv.decode(z.to(dev))[:, :, 0]
        warnings.warn(f"Qwen-Image VAE decode on the host module: {why}", RuntimeWarning, stacklevel=3)
    return vae.decode(z, return_dict=False)[0][:, :, 0]


# ---- image pre- and post-processing on the device (regione_amd/image_ops.py) ------------------------------------------------------------
# The stages a hosted call may run on the device, and the ones that do so without being asked (`pipe._regione_hip_image` unset): a stage
# is on by default when its device path, upload and download included, beat the host leg of tools/image_processing_bench.py on the GPU
# host - all four did (profiles/r24_image_processing_bench.json), and the outputs are the same bits.
IMAGE_STAGES = ("resize", "preprocess", "postprocess", "vlm")
IMAGE_STAGES_DEFAULT = frozenset(IMAGE_STAGES)


def _cfg_get(cfg, name):
    return cfg.get(name) if isinstance(cfg, dict) else getattr(cfg, name, None)


def _is_rgb_pil(img) -> bool:
    return getattr(img, "mode", None) == "RGB" and hasattr(img, "size") and hasattr(img, "resize") and not isinstance(img, torch.Tensor)


def hip_image_ops_for(host, dev, stage: str):
    """The HipImageOps of this host (made once, kept on it as `_regione_hip_image_ops`) when `stage` of its image work runs on the device,
    else None: `pipe._regione_hip_image = False` keeps every stage on the host's own methods, `= True` moves every stage a call qualifies
    for, unset moves the stages of IMAGE_STAGES_DEFAULT.  A call qualifies when the host's `image_processor.config` says do_resize,
    do_normalize and resample == "lanczos" and sets none of do_binarize, do_convert_grayscale, do_convert_rgb: the arithmetic the kernels
    restate.  Every other host keeps its own methods, silently."""
    flag = host.__dict__.get("_regione_hip_image", None)
    if flag is False or (flag is not True and stage not in IMAGE_STAGES_DEFAULT):
        return None
    cfg = getattr(getattr(host, "image_processor", None), "config", None)
    if cfg is None or not (_cfg_get(cfg, "do_resize") and _cfg_get(cfg, "do_normalize") and _cfg_get(cfg, "resample") == "lanczos"):
        return None
    if _cfg_get(cfg, "do_binarize") or _cfg_get(cfg, "do_convert_grayscale") or _cfg_get(cfg, "do_convert_rgb"):
        return None
    io = host.__dict__.get("_regione_hip_image_ops")
    if io is None:
        from ..image_ops import HipImageOps
        io = host._regione_hip_image_ops = HipImageOps(dev)
    return io


def _image_inputs_on_device(host, dev, images):
    """HipImageOps when the condition images' resize + preprocess run on the device: every image one RGB PIL image, both stages on, and
    the VAE encoder adopted (it reads bf16, the rounding the device preprocess ends in; a host encoder keeps the host's fp32 tensor)."""
    if not images or not all(_is_rgb_pil(i) for i in images):
        return None
    io = hip_image_ops_for(host, dev, "resize")
    if io is None or hip_image_ops_for(host, dev, "preprocess") is None or hip_vae_encoder_for(host, dev) is None:
        return None
    return io


def _postprocess_image(host, vae, lat, dev, output_type):
    """`image_processor.postprocess(vae.decode(lat))` of the FLUX / Step1X calls; output_type "pil" with the adopted decoder ends in the
    byte kernel (decode_u8) and one download."""
    io = hip_image_ops_for(host, dev, "postprocess") if output_type == "pil" else None
    hv = hip_vae_for(host, dev) if io is not None else None
    if hv is not None and hasattr(hv, "decode_u8") and lat.dim() == 4 and lat.shape[0] == 1:
        return [io.to_pil(hv.decode_u8(lat.to(dev)))]
    return host.image_processor.postprocess(_decode_image(host, vae, lat, dev), output_type=output_type)


def _postprocess_qwen_image(host, vae, z, dev, output_type):
    """The same for the Qwen pipelines (`vae.decode(z)[0][:, :, 0]`)."""
    from .. import qwen_vae as Q
    io = hip_image_ops_for(host, dev, "postprocess") if output_type == "pil" else None
    hv = hip_vae_for(host, dev) if io is not None else None
    if isinstance(hv, Q.HipQwenVaeDecoder) and hv.out_dtype == torch.bfloat16 and _qwen_vae_refusal(vae, z, "decode") is None:
        return [io.to_pil(hv.decode_u8(z.to(dev)))]
    return host.image_processor.postprocess(_decode_qwen_image(host, vae, z, dev), output_type=output_type)


def _qwen2vl_processor_refusal(own) -> Optional[str]:
    """Why the device does not restate this VLM image processor (None: it is transformers' PIL backend with the Qwen2-VL defaults, the
    arithmetic the kernels restate)."""
    from ..image_ops import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    if not callable(own):
        return "not callable"
    # the PIL / numpy backend ONLY: transformers' torchvision backend (`Qwen2VLImageProcessor`, what AutoProcessor picks when torchvision
    # is installed) carries the same attribute values and other arithmetic - torchvision's antialiased bicubic, rescale and normalise
    # fused as (v - 255 mean) / (255 std) in torch fp32 - so it is told apart by class and `backend`, never by its settings
    if not any(c.__name__ == "Qwen2VLImageProcessorPil" for c in type(own).__mro__) or getattr(own, "backend", None) != "pil":
        return f"{type(own).__name__} (backend {getattr(own, 'backend', None)!r}): Qwen2VLImageProcessorPil, the PIL backend, is covered"
    for name, want in (("do_resize", True), ("do_rescale", True), ("do_normalize", True), ("patch_size", 14), ("merge_size", 2),
                       ("temporal_patch_size", 2)):
        if getattr(own, name, None) != want:
            return f"{name} = {getattr(own, name, None)!r}"
    if int(getattr(own, "resample", -1) or -1) != 3:                      # PILImageResampling.BICUBIC
        return f"resample = {getattr(own, 'resample', None)!r}"
    if getattr(own, "rescale_factor", None) != 1 / 255:
        return f"rescale_factor = {getattr(own, 'rescale_factor', None)!r}"
    for name, want in (("image_mean", OPENAI_CLIP_MEAN), ("image_std", OPENAI_CLIP_STD)):
        got = getattr(own, name, None)
        if got is None or tuple(float(v) for v in got) != want:
            return f"{name} = {got!r}"
    size = getattr(own, "size", None)
    if _cfg_get(size, "shortest_edge") is None or _cfg_get(size, "longest_edge") is None:
        return f"size = {size!r}"
    if getattr(own, "do_pad", None) or getattr(own, "do_center_crop", None):
        return "do_pad / do_center_crop"
    return None


class _HipQwen2VLImageProcessor:
    """What `processor.image_processor` is bound to during a hosted Qwen `encode_prompt`: `(images=[...], return_tensors="pt")` of RGB PIL
    images is answered on the device - smart_resize, bicubic resize, rescale / normalise / patchify - with `pixel_values` ON the device
    (fp32 [N, 1176], or the vision tower's padded bf16 rows when the HIP tower reads them) and `image_grid_thw`.  Anything else - videos,
    other keyword arguments, other image types, a size outside the processor's pixel limits - goes to the host's own image processor, as
    does every attribute (`merge_size`, `get_number_of_image_patches`, ...)."""

    def __init__(self, own, io, twins, Kp=None):
        self.__dict__.update(_own=own, _io=io, _twins=twins, _Kp=Kp)

    def __getattr__(self, name):
        return getattr(self.__dict__["_own"], name)

    def __call__(self, images=None, *args, **kw):
        own, io = self._own, self._io
        imgs = list(images) if isinstance(images, (list, tuple)) else [images]
        if args or set(kw) - {"return_tensors"} or kw.get("return_tensors") != "pt" or not imgs or \
                not all(id(i) in self._twins or _is_rgb_pil(i) for i in imgs):
            return own(images, *args, **kw)
        lo, hi = _cfg_get(own.size, "shortest_edge"), _cfg_get(own.size, "longest_edge")
        plan = []
        for i in imgs:
            w, h = i.size
            if min(h, w) < 1 or max(h, w) / min(h, w) > 200:
                return own(images, **kw)
            rh, rw = round(h / 28) * 28, round(w / 28) * 28
            if rh < 28 or rw < 28 or not lo <= rh * rw <= hi:             # the processor's rescaling branches: its own code
                return own(images, **kw)
            plan.append((i, rh, rw))
        rows, grids = [], []
        for i, rh, rw in plan:
            u8 = self._twins.get(id(i))
            u8 = io.upload(i) if u8 is None else u8
            u8 = io.resize(u8, rh, rw, "bicubic")
            rows.append(io.to_patch_rows(u8, out="padded_bf16", Kp=self._Kp) if self._Kp else io.to_patch_rows(u8))
            grids.append([1, rh // 14, rw // 14])
        data = {"pixel_values": rows[0] if len(rows) == 1 else torch.cat(rows, 0), "image_grid_thw": torch.tensor(grids, dtype=torch.int64)}
        try:
            from transformers.feature_extraction_utils import BatchFeature
            return BatchFeature(data=data)
        except ImportError:
            return data


def _hip_qwen_image_processor(host, dev, twins=None):
    """`with _hip_qwen_image_processor(host, dev, twins): host.encode_prompt(...)` - the host's own code runs with
    `processor.image_processor` bound (in the processor's instance dict) to a _HipQwen2VLImageProcessor; undone on exit, an exception
    included.  `twins`: id(PIL image) -> its uint8 twin on the device, so an image this call made on the device is not uploaded again."""
    proc = getattr(host, "processor", None)
    own = getattr(proc, "image_processor", None)
    io = hip_image_ops_for(host, dev, "vlm") if own is not None and hasattr(proc, "__dict__") else None
    if io is None or _qwen2vl_processor_refusal(own) is not None:
        return contextlib.nullcontext()
    tower = getattr(hip_qwen_text_encoder_for(host, dev), "vision", None)
    if type(tower).__name__ != "HipQwen25VLVisionTower":     # the rows stay on the device: only the HIP tower is known to read them there
        return contextlib.nullcontext()
    Kp = tower.Kp if tower.Kp != tower.K else None
    return _bound(proc, "image_processor", _HipQwen2VLImageProcessor(own, io, {} if twins is None else twins, Kp))

