"""Host-pipeline adapter: a STOCK diffusers editing pipeline on the HIP engine, with the
reference's call shape (RegionE/README.md:85-113):

    helper = RegionEHelper(pipe)                # FluxKontext / Step1XEdit(V1P2) / QwenImageEdit(Plus)Pipeline object
    helper.set_params(...); helper.enable()     # adopts the transformer weights once, patches the engine, swaps pipe.__class__
    image = pipe(image=pil_image, prompt="...").images[0]        # the user keeps calling the pipeline itself
    helper.disable()                            # pipe is the stock pipeline again

Lower levels, for callers that want them:
    engine = adopt_engine(pipe)                 # latent-level HIP pipeline of the host's family (weights adopted)
    hosted = adopt(pipe)                        # wrapper object: hosted(image=..., prompt=...) without touching pipe.__class__

`adopt_engine` reads the host transformer's `state_dict()` (tensor by tensor, straight to the GPU in bf16), infers the
trunk dimensions from the tensor shapes, maps the family's parameter names onto the engine's FLUX-layout names and
returns the matching `regione_amd.harness` pipeline (latent-level API).  `adopt` additionally keeps the host pipeline for
everything OUTSIDE the denoise loop - image preprocessing, prompt encoders, VAE encode / decode, post-processing - calling
the host's own methods in the order the reference's patched `__call__` does (RegionE/FluxKontext/inplace.py:112-240 and
:396-410), and runs the loop itself (:240-394) on the engine.

diffusers is not installed in the build image: the call sequence follows the reference's copy of the diffusers
`__call__`, and is exercised in tests/test_adapters.py against host-pipeline stand-ins with the same method surface
(tests/host_trunks.py module trees, whose own vanilla forward the adopted engine is compared with).  Treat the first run against a real checkpoint as the remaining validation step.

LoRA adapters loaded into the host transformer (PEFT layers: `load_lora_weights` without `fuse_lora`) are merged into the engine's weights
on the device at adoption and re-merged when the adapter state changes (`lora_sync`, the LoRA section below): no per-step side path.
"""
from __future__ import annotations

import re
import warnings
from typing import Dict, Iterable, Iterator, Optional, Tuple

import torch

from . import _lib, ops
from .synth import FluxConfig, flux_param_shapes

# host parameter name -> engine (FLUX-layout) parameter name, per family; applied as ordered regex substitutions
_KEYMAPS: Dict[str, Tuple[Tuple[str, str], ...]] = {
    "flux": (),
    "step1x": ((r"^time_embed\.", "time_text_embed.timestep_embedder."),           # Step1XEditV1P2/inplace.py:590-600
               (r"^vec_embed\.", "time_text_embed.text_embedder.")),
    "qwen": ((r"^img_in\.", "x_embedder."), (r"^txt_in\.", "context_embedder."),    # QwenImageEdit/inplace.py:497-507
             (r"\.img_mod\.1\.", ".norm1.linear."), (r"\.txt_mod\.1\.", ".norm1_context.linear."),
             (r"\.img_mlp\.", ".ff."), (r"\.txt_mlp\.", ".ff_context.")),
}

_FAMILY_OF = {
    "FluxKontextPipeline": "flux",
    "Step1XEditPipeline": "step1x",
    "Step1XEditPipelineV1P2": "step1x",
    "QwenImageEditPipeline": "qwen",
    "QwenImageEditPlusPipeline": "qwen",
}


def map_key(name: str, family: str) -> str:
    for pat, rep in _KEYMAPS[family]:
        name = re.sub(pat, rep, name)
    return name


def infer_config(shapes: Dict[str, Tuple[int, ...]], axes_dim: Optional[Iterable[int]] = None) -> FluxConfig:
    """Trunk dimensions from (engine-named) parameter shapes; raises KeyError / ValueError on a foreign layout."""
    d, in_channels = shapes["x_embedder.weight"]
    joint_dim = shapes["context_embedder.weight"][1]
    n_double = 1 + max((int(m.group(1)) for k in shapes if (m := re.match(r"transformer_blocks\.(\d+)\.attn\.to_q\.weight$", k))),
                       default=-1)
    n_single = 1 + max((int(m.group(1)) for k in shapes if (m := re.match(r"single_transformer_blocks\.(\d+)\.proj_mlp\.weight$", k))),
                       default=-1)
    if n_double == 0:
        raise ValueError("no transformer_blocks.*.attn.to_q.weight in the host state dict: not an MMDiT trunk this engine knows")
    head_dim = shapes["transformer_blocks.0.attn.norm_q.weight"][0]
    if d % head_dim:
        raise ValueError(f"inner dim {d} is not a multiple of head_dim {head_dim}")
    pooled = shapes.get("time_text_embed.text_embedder.linear_1.weight")
    cfg = FluxConfig(in_channels=in_channels, n_double=n_double, n_single=n_single, heads=d // head_dim, head_dim=head_dim,
                     joint_dim=joint_dim, pooled_dim=pooled[1] if pooled else 768,
                     axes_dim=tuple(axes_dim) if axes_dim is not None else (16, 56, 56),
                     mlp_ratio=shapes["transformer_blocks.0.ff.net.0.proj.weight"][0] // d,
                     guidance_embeds="time_text_embed.guidance_embedder.linear_1.weight" in shapes,
                     pooled_embeds=pooled is not None, txt_norm="txt_norm.weight" in shapes)
    if sum(cfg.axes_dim) != head_dim:
        raise ValueError(f"rotary axes {cfg.axes_dim} do not sum to head_dim {head_dim}")
    return cfg


def _axes_dim(transformer):
    c = getattr(transformer, "config", None)
    for key in ("axes_dims_rope", "axes_dim"):
        v = (c.get(key) if hasattr(c, "get") else getattr(c, key, None)) if c is not None else None
        if v is not None:
            return tuple(v)
    pe = getattr(transformer, "pos_embed", None)
    return tuple(pe.axes_dim) if pe is not None and hasattr(pe, "axes_dim") else None


# ---------------------------------------------------------------------------------------------------------------------
# LoRA on the trunk (PEFT layout): merged on the device at adoption, re-merged when the adapter state changes
# ---------------------------------------------------------------------------------------------------------------------
# `pipe.load_lora_weights(...)` without `fuse_lora()` leaves PEFT layers in pipe.transformer: a wrapped Linear X holds `X.base_layer`,
# `X.lora_A[adapter]` ([r, in]) and `X.lora_B[adapter]` ([out, r]) Linears, `X.scaling[adapter]` (alpha / r times the set_adapters weight),
# `X.active_adapters`, `X.disable_adapters`, `X.merged_adapters`.  The engine has no per-step side path: it holds
# W_eff = W_base + sum over the active, not disabled adapters of scaling[a] * B_a A_a, built by rgn_lora_merge_bf16 (ops.lora_merge: fp32
# fma in adapter order, ONE rounding to bf16) in the engine's packed layouts.  `lora_dropout` is training-only and ignored.
_PEFT_OTHER_TUNERS = ("lokr_", "hada_", "ia3_")


def _lora_decline(what: str):
    raise NotImplementedError(f"host transformer carries {what}: the HIP engine merges plain LoRA on the trunk's Linear layers only "
                              "(fuse or unload it on the host first)")


def lora_layers(transformer) -> Dict[str, object]:
    """{module path: PEFT LoRA wrapper} of a host transformer ({} for a module tree without any, or an object without named_modules)."""
    if not hasattr(transformer, "named_modules"):
        return {}
    return {n: m for n, m in transformer.named_modules() if hasattr(m, "base_layer") and hasattr(m, "lora_A")}


def _lora_active(m):
    """The adapters a wrapped module applies in its forward, in `active_adapters` order: none when the adapters are disabled or when the
    module is merged (PEFT merge_adapter / fuse_lora already added them to base_layer.weight: they are not applied a second time)."""
    if getattr(m, "disable_adapters", False) or list(getattr(m, "merged_adapters", None) or ()):
        return []
    act = getattr(m, "active_adapters", None)
    if act is None:
        act = getattr(m, "active_adapter", ())
    if isinstance(act, str):
        act = [act]
    return [a for a in act if a in m.lora_A]


def _lora_checked(transformer, sd, ignore_prefixes) -> Dict[str, object]:
    """lora_layers() of the trunk (layers under an ignored prefix stay the host's business) after every by-name refusal - host-side
    attribute and shape reads only, nothing allocated, nothing launched."""
    for k in sd:
        for t in _PEFT_OTHER_TUNERS:
            if t in k:
                _lora_decline(f"a non-LoRA PEFT tuner ({t}* in {k!r})")
        if "lora_embedding_" in k:
            _lora_decline(f"a LoRA embedding layer (lora_embedding_* in {k!r})")
        if "lora_magnitude_vector" in k:
            _lora_decline(f"DoRA (lora_magnitude_vector in {k!r})")
    layers = {n: m for n, m in lora_layers(transformer).items() if not n.startswith(tuple(ignore_prefixes))}
    for n, m in layers.items():
        if any(dict(getattr(m, "use_dora", None) or {}).values()) or len(getattr(m, "lora_magnitude_vector", None) or ()):
            _lora_decline(f"DoRA (use_dora / lora_magnitude_vector on {n})")
        if len(getattr(m, "lora_embedding_A", None) or ()) or len(getattr(m, "lora_embedding_B", None) or ()):
            _lora_decline(f"a LoRA embedding layer (lora_embedding_* on {n})")
        if any(dict(getattr(m, "lora_bias", None) or {}).values()) or any(getattr(b, "bias", None) is not None for b in m.lora_B.values()):
            _lora_decline(f"lora_bias=True on {n}")
        base = m.base_layer
        if hasattr(base, "lora_A") or not isinstance(base, torch.nn.Linear):
            _lora_decline(f"LoRA on {n}, a {type(base).__name__}, not a Linear the trunk layout knows")
        act = _lora_active(m)
        if len(act) > ops.LORA_MAX_TERMS:
            _lora_decline(f"{len(act)} active adapters on {n} (at most {ops.LORA_MAX_TERMS} are merged)")
        out_f, in_f = base.weight.shape
        for a in act:
            A, B = m.lora_A[a].weight, m.lora_B[a].weight
            if A.dim() != 2 or B.dim() != 2 or A.shape[1] != in_f or B.shape[0] != out_f or A.shape[0] != B.shape[1]:
                _lora_decline(f"adapter {a!r} on {n} with A {tuple(A.shape)} / B {tuple(B.shape)} that do not fit the base weight {(out_f, in_f)}")
            if A.shape[0] > ops.LORA_MAX_RANK:
                _lora_decline(f"adapter {a!r} on {n} of rank {A.shape[0]} > {ops.LORA_MAX_RANK}")
    return layers


def _peft_names(sd, layers) -> Dict[str, str]:
    """host state-dict key -> the name it has without the PEFT wrapper levels (`X.base_layer.weight` -> `X.weight`); the adapters' own
    tensors (`X.lora_A.<adapter>.weight`, `X.lora_B.<adapter>.weight`) are left out.  The identity for a host without LoRA layers."""
    if not layers:
        return {k: k for k in sd}
    own = tuple(n + s for n in layers for s in (".lora_A.", ".lora_B."))
    return {k: k.replace(".base_layer.", ".") for k in sd if not k.startswith(own)}


def _ver(t):
    return None if t.is_inference() else t._version


def _lora_fingerprint(layers, scale: float) -> Dict[str, tuple]:
    """Per wrapped module, everything its effective weight depends on - host-side reads only (no device reads): the active adapters, their
    `scaling` times the call-time scale, disable_adapters, merged_adapters, (data_ptr, _version) of the base weight and of each A / B."""
    fp = {}
    for n, m in layers.items():
        act = _lora_active(m)
        w = m.base_layer.weight
        fp[n] = (tuple(act), tuple(float(m.scaling[a]) * scale for a in act), bool(getattr(m, "disable_adapters", False)),
                 tuple(getattr(m, "merged_adapters", None) or ()), (w.data_ptr(), _ver(w)),
                 tuple((t.data_ptr(), _ver(t)) for a in act for t in (m.lora_A[a].weight, m.lora_B[a].weight)))
    return fp


def _lora_terms(m, device, scale: float):
    """[(A [r, in] fp32, B [out, r] fp32, scaling * scale)] on the device for the module's active adapters (real LoRA files are bf16, fp16
    or fp32 and tiny: converted once per merge)."""
    return [(m.lora_A[a].weight.detach().to(device, torch.float32).contiguous(),
             m.lora_B[a].weight.detach().to(device, torch.float32).contiguous(), float(m.scaling[a]) * scale) for a in _lora_active(m)]


def _staged(host_w, device):
    return host_w.detach().to(device=device, dtype=torch.bfloat16).contiguous()


def _stream(sd, names, family: str, device, lora=None, scale: float = 1.0) -> Iterator[Tuple[str, torch.Tensor]]:
    """(engine name, bf16 device tensor) of every host tensor; a LoRA-carrying weight is merged here, in place on its staged copy, before
    load_state_dict_stream packs it (the engine never writes to a host tensor: a host already on the device in bf16 gets a new one)."""
    for k, stripped in names.items():
        name, v = map_key(stripped, family), sd[k]
        m = lora.get(name) if lora else None
        terms = _lora_terms(m, device, scale) if m is not None else None
        if not terms:
            yield name, v.detach().to(device=device, dtype=torch.bfloat16)
            continue
        w = _staged(v, device)
        yield name, ops.lora_merge(w if w.data_ptr() != v.data_ptr() else torch.empty_like(w), w, terms)


def _lora_plan(pipe, family, ignore_prefixes):
    """(state dict, key -> stripped name, {engine weight name: wrapped module}) of the host transformer, refusals raised."""
    sd = pipe.transformer.state_dict()
    layers = _lora_checked(pipe.transformer, sd, ignore_prefixes)
    return sd, _peft_names(sd, layers), {map_key(n + ".weight", family): m for n, m in layers.items()}


def lora_sync(pipe, engine, scale: float = 1.0, ignore_prefixes: Tuple[str, ...] = ("connector.",)) -> bool:
    """Bring the engine's weights to the host transformer's CURRENT adapter state (set_adapters, disable_lora, unload_lora_weights, a
    second load_lora_weights, fuse_lora, a call-time scale): compare the host-side fingerprint with the one the weights were built
    from and, when it differs, re-stage the base rows of every engine weight whose module changed and re-apply its terms into the
    recorded slot (FluxTransformer2DModel.weight_slots); an fp8 trunk rebuilds and re-quantises the touched packed tensors.  False: the
    fingerprint is unchanged, nothing was launched."""
    tr = engine.transformer
    rec = tr.__dict__.get("_lora")
    if rec is None:
        return False                                             # an engine that was not adopted from a host pipeline
    layers = {n: m for n, m in lora_layers(pipe.transformer).items() if not n.startswith(tuple(ignore_prefixes))}
    if not layers and not rec["fp"]:
        return False                                             # a pipeline that never saw a LoRA
    family = rec["family"]
    scale = float(scale) if layers else 1.0
    fp = {map_key(n + ".weight", family): v for n, v in _lora_fingerprint(layers, scale).items()}
    if fp == rec["fp"]:
        return False
    sd, names, lora = _lora_plan(pipe, family, ignore_prefixes)
    slots, dev = tr.weight_slots(), tr.device
    bad = [k for k in lora if k not in slots]
    if bad:
        _lora_decline(f"LoRA on {bad[0][:-len('.weight')]}, not a Linear the trunk layout knows")
    host_key = {map_key(s, family): k for k, s in names.items()}
    touched = sorted(k for k in set(fp) | set(rec["fp"]) if fp.get(k) != rec["fp"].get(k))

    def fill(rows, name):
        """rows <- the host's base weight with the module's current terms."""
        w = _staged(sd[host_key[name]], dev)
        m = lora.get(name)
        terms = _lora_terms(m, dev, scale) if m is not None else []
        if terms:
            ops.lora_merge(rows, w, terms)
        elif rows.data_ptr() != w.data_ptr():
            rows.copy_(w)

    done = set()
    for name in touched:
        obj, attr, lo, hi = slots[name]
        tgt = getattr(obj, attr)
        if tgt.dtype == ops.FP8:                                 # rebuild the whole packed tensor in bf16, then quantise it as quantize_fp8_ does
            if (id(obj), attr) in done:
                continue
            done.add((id(obj), attr))
            full = torch.empty(tgt.shape, dtype=torch.bfloat16, device=dev)
            for n, s in slots.items():
                if s[0] is obj and s[1] == attr:
                    fill(full[s[2]:s[3]] if s[3] is not None else full, n)
            setattr(obj, attr, ops.quantize_w8(full))
        elif hi is None and tgt.data_ptr() == sd[host_key[name]].data_ptr():
            # adopted without a copy from a host that is already on the device in bf16: the engine never writes to a host tensor
            full = torch.empty_like(tgt)
            fill(full, name)
            setattr(obj, attr, full)
        else:
            fill(tgt[lo:hi] if hi is not None else tgt, name)
    if any(re.search(r"\.(to_[qkv]|add_[qkv]_proj)\.weight$", n) for n in touched):
        tr.refresh_score_bounds()
    tr.clear_modulations()                                       # AdaLN tables of earlier edits were built from the old mod_w / embedders
    rec["fp"] = fp
    return True


def adopt_engine(pipe, device="cuda", family: Optional[str] = None, ignore_prefixes: Tuple[str, ...] = ("connector.",)):
    """The harness pipeline of the host pipeline's family, its transformer loaded from `pipe.transformer`.
    `ignore_prefixes`: host sub-modules that run in front of the hot path and stay on the host (Step1X-Edit's text
    connector, Step1XEditV1P2/inplace.py:606-609); any other name the trunk layout does not know is an error."""
    from .harness import flux as HF, qwen as HQ, step1x as HS
    name = pipe.__class__.__name__
    family = family or _FAMILY_OF.get(name)
    if family is None:
        raise NotImplementedError(f"no RegionE patch set for pipeline class {name}")
    sd, names, lora = _lora_plan(pipe, family, ignore_prefixes)       # PEFT wrapper levels stripped; what is not plain LoRA is refused by name
    shapes = {map_key(s, family): tuple(sd[k].shape) for k, s in names.items()}
    cfg = infer_config(shapes, _axes_dim(pipe.transformer))
    want = flux_param_shapes(cfg)
    for k in lora:
        if k not in want or len(want[k]) != 2:
            _lora_decline(f"LoRA on {k[:-len('.weight')]}, not a Linear the trunk layout knows")
    extra =[k for k in shapes if k not in want and not k.startswith(tuple(ignore_prefixes))]
    missing = [k for k in want if k not in shapes]
    wrong = [k for k in want if k in shapes and tuple(shapes[k]) != tuple(want[k])]
    if extra or missing or wrong:
        raise KeyError(f"host transformer does not match the {family} trunk layout: missing {missing[:4]}, unexpected {extra[:4]}, "
                       f"shape mismatch {[(k, shapes[k], want[k]) for k in wrong[:4]]}")
    device = torch.device(device)
    if family == "flux":
        tr = HF.FluxTransformer2DModel(cfg, device)
        engine_cls = HF.FluxKontextPipeline
    elif family == "step1x":
        if cfg.guidance_embeds:
            raise ValueError("Step1X-Edit trunk with a guidance embedder: unexpected layout")
        tr = HS.Step1XEditTransformer2DModel(cfg, device)
        engine_cls = HS.Step1XEditPipelineV1P2 if name.endswith("V1P2") else HS.Step1XEditPipeline
    else:
        if cfg.n_single or cfg.pooled_embeds or cfg.guidance_embeds or not cfg.txt_norm:
            raise ValueError("Qwen-Image trunk expected: double-stream blocks only, timestep-only conditioning, txt_norm")
        tr = HQ.QwenImageTransformer2DModel(cfg, device)
        engine_cls = HQ.QwenImageEditPlusPipeline if "Plus" in name else HQ.QwenImageEditPipeline
    fp = _lora_fingerprint(lora, 1.0)
    tr.load_state_dict_stream((k, v) for k, v in _stream(sd, names, family, device, lora) if k in want)
    tr._lora = {"family": family, "fp": fp}          # the adapter state the weights were built from: lora_sync re-merges when it changes
    sched_cfg = dict(getattr(pipe.scheduler, "config", {}) or {}) if getattr(pipe, "scheduler", None) is not None else {}
    # every key travels: the engine's scheduler implements shift_terminal / time_shift_type / invert_sigmas and REFUSES
    # what it does not implement (karras / exponential / beta sigmas, stochastic sampling, unknown keys)
    engine = engine_cls(tr, HF.FlowMatchEulerDiscreteScheduler(**sched_cfg))
    if hasattr(pipe, "vae_scale_factor"):
        engine.vae_scale_factor = pipe.vae_scale_factor
    return engine


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


class HostedOutput(dict):
    def __init__(self, images, timing=None):
        super().__init__(images=images)
        self.images = images
        self.timing = timing or {}           # wall-clock seconds of the three stages: encode / loop / decode


def _bf(t, dev):
    return t.to(device=dev, dtype=torch.bfloat16) if t is not None else None


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


def _loop_extras(kw: dict, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs):
    """`sigmas` (inplace.py:229-242) and `callback_on_step_end` (:376-383) travel to the engine's loop."""
    if sigmas is not None:
        kw["sigmas"] = sigmas
    if callback_on_step_end is not None:
        kw["callback_on_step_end"] = callback_on_step_end
        kw["callback_on_step_end_tensor_inputs"] = tuple(callback_on_step_end_tensor_inputs)
    return kw


_NO_HIP_VAE = object()


def _is_qwen_vae(vae) -> bool:
    """The [EXT] AutoencoderKLQwenImage layout (3-D causal VAE of the Qwen-Image pipelines): RMS_norm `norm_out`, a Wan-style config."""
    cfg = getattr(vae, "config", None)
    return all(getattr(getattr(vae, p, None), "norm_out", None) is not None for p in ("decoder", "encoder")) and \
        getattr(cfg, "base_dim", None) is not None and getattr(cfg, "z_dim", None) is not None and hasattr(vae, "state_dict")


def _adopt_qwen_vae(host, dev):
    """Both halves of a Qwen-Image VAE onto the HIP kernels (regione_amd/qwen_vae.py), once per host pipeline.  Whatever the kernels do not
    cover (another config, unknown or missing parameters, a dtype other than bf16 / fp32) keeps the host module, with one warning naming
    the reason: (None, None)."""
    from . import qwen_vae as Q
    vae = host.vae
    cfg, want = vae.config, Q.QWEN_VAE_CONFIG
    got = {k: (tuple(getattr(cfg, k)) if isinstance(want[k], tuple) else getattr(cfg, k)) if hasattr(cfg, k) else None for k in want}
    why = None
    if got != want:
        why = f"config {got} (the kernels cover {want})"
    else:
        try:
            sd = vae.state_dict()
            return Q.HipQwenVaeDecoder(sd, dev, out_dtype=vae.dtype), Q.HipQwenVaeEncoder(sd, dev, out_dtype=vae.dtype)
        except _lib.RegionEHipError as e:
            why = str(e)
    warnings.warn(f"Qwen-Image VAE kept on the host module: {why}", RuntimeWarning, stacklevel=3)
    return None, None


def _qwen_vae_refusal(vae, x, kind: str, kw=None) -> Optional[str]:
    """Why the HIP Qwen-Image VAE does not serve this `vae.decode(z)` / `vae.encode(x)` call (None: it does)."""
    from . import qwen_vae as Q
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


def hip_vae_for(host, dev):
    """The host's AutoencoderKL decoder adopted onto the HIP kernels (regione_amd/vae.py) - once per host pipeline,
    kept on it as `_regione_hip_vae`; Qwen-Image's 3-D causal VAE goes to regione_amd/qwen_vae.py (`_adopt_qwen_vae`, both halves at once).
    None when the host's VAE is of neither layout (e.g. a module with a post_quant_conv): the host module then decodes, exactly as in the reference (`self.vae.decode`, FluxKontext/inplace.py:396-402).  A VAE
    that HAS the layout but cannot be adopted (unknown parameters, other widths) raises instead of silently running the slower module;
    `pipe._regione_hip_vae = False` before the first call keeps the host module on purpose."""
    cached = host.__dict__.get("_regione_hip_vae", _NO_HIP_VAE)
    if cached is False or cached is None:
        return None
    if cached is not _NO_HIP_VAE:
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
    from . import vae as V
    cfg = getattr(vae, "config", None)
    kw = {}
    for name in ("block_out_channels", "latent_channels", "layers_per_block"):
        v = getattr(cfg, name, None) if cfg is not None else None
        if v is not None:
            kw[name] = tuple(v) if name == "block_out_channels" else int(v)
    host._regione_hip_vae = V.HipVaeDecoder(dec.state_dict(), dev, **kw)
    return host._regione_hip_vae


def hip_vae_encoder_for(host, dev):
    """The host's AutoencoderKL ENCODER on the HIP kernels (regione_amd/vae.py HipVaeEncoder), adopted once per host pipeline
    (`_regione_hip_vae_encoder`); None when the VAE has no such encoder, carries a quant_conv, or `pipe._regione_hip_vae = False`."""
    if host.__dict__.get("_regione_hip_vae", _NO_HIP_VAE) is False:
        return None
    cached = host.__dict__.get("_regione_hip_vae_encoder", _NO_HIP_VAE)
    if cached is not _NO_HIP_VAE:
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
    from . import vae as V
    cfg = getattr(vae, "config", None)
    kw = {}
    for name in ("block_out_channels", "latent_channels", "layers_per_block"):
        v = getattr(cfg, name, None) if cfg is not None else None
        if v is not None:
            kw[name] = tuple(v) if name == "block_out_channels" else int(v)
    host._regione_hip_vae_encoder = V.HipVaeEncoder(enc.state_dict(), dev, **kw)
    return host._regione_hip_vae_encoder


_TEXT_ENCODERS = (("text_encoder", "clip"), ("text_encoder_2", "t5"))


def _adopt_text_encoder(mod, kind: str, dev):
    """(HIP encoder, None) or (None, the reason the host module keeps running)."""
    from . import text_encoders as TE
    cfg = getattr(mod, "config", None)
    if cfg is None or not hasattr(mod, "state_dict"):
        return None, f"{type(mod).__name__} is not a transformers module"
    why = TE.clip_refusal(cfg) if kind == "clip" else TE.t5_refusal(cfg)
    if why is None and type(mod).__name__ != ("CLIPTextModel" if kind == "clip" else "T5EncoderModel"):
        why = f"{type(mod).__name__} (another layout: the kernels restate CLIPTextModel / T5EncoderModel)"
    if why is None and any("lora" in n.lower() for n, _ in mod.named_modules()):
        why = "PEFT / LoRA layers in the module"
    if why is not None:
        return None, why
    try:
        return (TE.HipClipTextModel(mod, dev) if kind == "clip" else TE.HipT5EncoderModel(mod, dev)), None
    except _lib.RegionEHipError as e:
        return None, str(e)


def hip_text_encoders_for(host, dev):
    """(CLIP, T5) of a FLUX.1 Kontext host adopted onto the HIP kernels (regione_amd/text_encoders.py), once
    per host pipeline and kept on it as `_regione_hip_text`.  A module the kernels do not cover (another layout, head dim != 64, non-bf16
    weights, PEFT / LoRA layers) stays the host's, with one warning naming the reason: None in its place.  A host without the modules
    gets (None, None) silently; `pipe._regione_hip_text = False` before the first call keeps the host modules on purpose."""
    cached = host.__dict__.get("_regione_hip_text", _NO_HIP_VAE)
    if cached is False or cached is None:
        return None, None
    if cached is not _NO_HIP_VAE:
        return cached
    got = []
    for attr, kind in _TEXT_ENCODERS:
        mod = getattr(host, attr, None)
        enc, why = (None, None) if mod is None else _adopt_text_encoder(mod, kind, dev)
        if why is not None:
            warnings.warn(f"{attr} kept on the host module: {why}", RuntimeWarning, stacklevel=3)
        got.append(enc)
    host._regione_hip_text = tuple(got)
    return host._regione_hip_text


class _hip_text_encoders:
    """`with _hip_text_encoders(host, dev): host.encode_prompt(...)` - the host's own `encode_prompt` (tokenizers, `_get_clip_prompt_embeds`,
    `_get_t5_prompt_embeds`: its code, untouched) runs with `text_encoder` / `text_encoder_2` bound to the adopted HIP encoders; the
    bindings are undone on exit, an exception included."""

    def __init__(self, host, dev):
        self.host, self.dev, self.saved = host, dev, []

    def __enter__(self):
        d = self.host.__dict__
        for (attr, _), enc in zip(_TEXT_ENCODERS, hip_text_encoders_for(self.host, self.dev)):
            if enc is not None:
                self.saved.append((attr, d.get(attr, _NO_HIP_VAE)))
                d[attr] = enc                  # the instance dict: no pipeline __setattr__ (diffusers would re-register the component)
        return self

    def __exit__(self, *a):
        d = self.host.__dict__
        for attr, orig in reversed(self.saved):
            if orig is _NO_HIP_VAE:
                del d[attr]
            else:
                d[attr] = orig
        self.saved = []
        return False


_QWEN_TEXT_HOSTS = ("QwenImageEditPipeline", "QwenImageEditPlusPipeline")


def hip_qwen_text_encoder_for(host, dev):
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
    top_k, top_p and repetition_penalty); absent, it is False; a value that is not a bool raises ValueError."""
    if host.__dict__.get("_regione_hip_text", _NO_HIP_VAE) is False:
        return None
    cached = host.__dict__.get("_regione_hip_qwen_text", _NO_HIP_VAE)
    if cached is not _NO_HIP_VAE:
        return cached
    fmt = host.__dict__.get("_regione_hip_text_weights", "bf16")
    if fmt not in ("bf16", "fp8"):
        raise ValueError(f"pipe._regione_hip_text_weights = {fmt!r}: \"bf16\" and \"fp8\" are accepted")
    sampling = host.__dict__.get("_regione_hip_text_sampling", False)
    if not isinstance(sampling, bool):
        raise ValueError(f"pipe._regione_hip_text_sampling = {sampling!r}: True and False are accepted")
    mod = getattr(host, "text_encoder", None)
    enc = None
    if type(mod).__name__ == "Qwen2_5_VLForConditionalGeneration" and getattr(mod, "config", None) is not None:
        from . import qwen_text_encoder as QT
        why = QT.qwen25vl_refusal(mod.config)
        if why is None and any("lora" in n.lower() for n, _ in mod.named_modules()):
            why = "PEFT / LoRA layers in the module"
        if why is None:
            try:
                enc = QT.HipQwen25VLTextEncoder(mod, dev, weights=fmt, **({"sampling": True} if sampling else {}))
            except _lib.RegionEHipError as e:
                why = str(e)
        if why is not None:
            warnings.warn(f"text_encoder kept on the host module: {why}", RuntimeWarning, stacklevel=3)
        elif host.__dict__.get("_regione_hip_vision", _NO_HIP_VAE) is not False:
            from . import qwen_vision as QV
            why = QV.vision_refusal(mod.config)
            if why is None:
                try:
                    enc.vision = QV.HipQwen25VLVisionTower(mod, dev)
                except _lib.RegionEHipError as e:
                    why = str(e)
            if why is not None:
                warnings.warn(f"vision tower kept on the host module: {why}", RuntimeWarning, stacklevel=3)
    host._regione_hip_qwen_text = enc
    return enc


class _hip_qwen_text_encoder:
    """`with _hip_qwen_text_encoder(host, dev): host.encode_prompt(...)` - the host's own `encode_prompt` (the template, the processor,
    `_get_qwen_prompt_embeds`, `_extract_masked_hidden`: its code, untouched) runs with `text_encoder` bound to the adopted HIP encoder,
    which answers what that code touches (the call, `.dtype`, `.device`, `.config`); the binding is undone on exit, an exception included."""

    def __init__(self, host, dev):
        self.host, self.dev, self.saved = host, dev, None

    def __enter__(self):
        enc = hip_qwen_text_encoder_for(self.host, self.dev)
        if enc is not None:
            d = self.host.__dict__
            self.saved = (d.get("text_encoder", _NO_HIP_VAE),)
            d["text_encoder"] = enc                # the instance dict: no pipeline __setattr__ (diffusers would re-register the component)
        return self

    def __exit__(self, *a):
        if self.saved is not None:
            d = self.host.__dict__
            if self.saved[0] is _NO_HIP_VAE:
                del d["text_encoder"]
            else:
                d["text_encoder"] = self.saved[0]
            self.saved = None
        return False


class _hip_vae_encode:
    """`with _hip_vae_encode(host, dev): host.prepare_latents(...)` - the host's own `prepare_latents` (resize, `_encode_vae_image`,
    `retrieve_latents`, shift / scale, packing: its code, untouched) runs with `vae.encode` answered by the HIP encoder for single 4-D
    images; anything else (batches, 5-D video-style inputs) falls through to the module's own method.  The binding is undone on exit."""

    def __init__(self, host, dev):
        self.host, self.dev = host, dev

    def __enter__(self):
        self.enc = hip_vae_encoder_for(self.host, self.dev)
        if self.enc is None:
            return self
        vae, enc, dev = self.host.vae, self.enc, self.dev
        self.orig = vae.__dict__.get("encode", _NO_HIP_VAE)
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
        vae.encode = encode
        return self

    def __exit__(self, *a):
        if self.enc is not None:
            if self.orig is _NO_HIP_VAE:
                del self.host.vae.__dict__["encode"]
            else:
                self.host.vae.encode = self.orig
        return False


def _decode_image(host, vae, lat, dev):
    """`vae.decode(lat, return_dict=False)[0]` - on the HIP decoder when the host's VAE is an AutoencoderKL (one image per call)."""
    hv = hip_vae_for(host, dev)
    if hv is not None and lat.dim() == 4 and lat.shape[0] == 1:
        return hv.decode(lat.to(dev))
    return vae.decode(lat, return_dict=False)[0]


def _decode_qwen_image(host, vae, z, dev):
    """`vae.decode(z, return_dict=False)[0][:, :, 0]` of the Qwen pipelines (QwenImageEdit/inplace.py:437-451) - on the HIP decoder when the
    host's VAE was adopted and the call is one it covers, else on the host module (with a warning naming the reason)."""
    from . import qwen_vae as Q
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
        from .image_ops import HipImageOps
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
    from . import qwen_vae as Q
    io = hip_image_ops_for(host, dev, "postprocess") if output_type == "pil" else None
    hv = hip_vae_for(host, dev) if io is not None else None
    if isinstance(hv, Q.HipQwenVaeDecoder) and hv.out_dtype == torch.bfloat16 and _qwen_vae_refusal(vae, z, "decode") is None:
        return [io.to_pil(hv.decode_u8(z.to(dev)))]
    return host.image_processor.postprocess(_decode_qwen_image(host, vae, z, dev), output_type=output_type)


def _qwen2vl_processor_refusal(own) -> Optional[str]:
    """Why the device does not restate this VLM image processor (None: it is transformers' PIL backend with the Qwen2-VL defaults, the
    arithmetic the kernels restate)."""
    from .image_ops import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
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


class _hip_qwen_image_processor:
    """`with _hip_qwen_image_processor(host, dev, twins): host.encode_prompt(...)` - the host's own code runs with
    `processor.image_processor` bound (in the processor's instance dict) to a _HipQwen2VLImageProcessor; undone on exit, an exception
    included.  `twins`: id(PIL image) -> its uint8 twin on the device, so an image this call made on the device is not uploaded again."""

    def __init__(self, host, dev, twins=None):
        self.host, self.dev, self.twins, self.proc = host, dev, {} if twins is None else twins, None

    def __enter__(self):
        proc = getattr(self.host, "processor", None)
        own = getattr(proc, "image_processor", None)
        io = hip_image_ops_for(self.host, self.dev, "vlm") if own is not None and hasattr(proc, "__dict__") else None
        if io is None or _qwen2vl_processor_refusal(own) is not None:
            return self
        tower = getattr(hip_qwen_text_encoder_for(self.host, self.dev), "vision", None)
        if type(tower).__name__ != "HipQwen25VLVisionTower":     # the rows stay on the device: only the HIP tower is known to read them there
            return self
        Kp = tower.Kp if tower.Kp != tower.K else None
        self.proc, self.saved = proc, proc.__dict__.get("image_processor", _NO_HIP_VAE)
        proc.__dict__["image_processor"] = _HipQwen2VLImageProcessor(own, io, self.twins, Kp)
        return self

    def __exit__(self, *a):
        if self.proc is not None:
            if self.saved is _NO_HIP_VAE:
                del self.proc.__dict__["image_processor"]
            else:
                self.proc.__dict__["image_processor"] = self.saved
            self.proc = None
        return False


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
    if trace is not None:
        kw["trace"] = trace
    latents = eng(**_loop_extras(kw, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs))[0]
    clk.mark("loop_s")
    # 7. decode (inplace.py:396-410)
    if output_type == "latent":
        out = latents
    else:
        vae = host.vae
        lat = host._unpack_latents(latents.to(vae.dtype if hasattr(vae, "dtype") else latents.dtype), height, width,
                                   host.vae_scale_factor)
        lat = lat / vae.config.scaling_factor + vae.config.shift_factor
        out = _postprocess_image(host, vae, lat, dev, output_type)
    if hasattr(host, "maybe_free_model_hooks"):
        host.maybe_free_model_hooks()
    clk.mark("decode_s")
    return HostedOutput(out, clk.out) if return_dict else (out,)


class _HostConnector:
    """Step1X-Edit's text path in front of the trunk - the [EXT] Qwen2 `connector` (token refiner conditioned on the
    TIMESTEP, so it runs once per computed step) and, in v1p2, `text_token_mapping` - stays on the host transformer
    (Step1XEdit/inplace.py:514-516, Step1XEditV1P2/inplace.py:602-609); the engine's `connector` hook calls this object
    and gets (context tokens, pooled vector rows) back.  Masks / text embeddings are bound per CFG branch."""

    def __init__(self, host_tr, dev, masks, text=None):
        self.tr, self.dev, self.masks, self.text = host_tr, dev, masks, text

    def _one(self, enc, timestep, row):
        mask = self.masks[row]
        hdev = enc.device if mask is None else mask.device
        e, y = self.tr.connector(enc.to(hdev), timestep.to(hdev), mask)
        ttm = getattr(self.tr, "text_token_mapping", None)
        if ttm is not None and self.text is not None and self.text[row] is not None:       # v1p2 :606-609
            emb, tmask = self.text[row]
            e = e + ttm(emb) * tmask[:, :, None]
        return _bf(e, self.dev), _bf(y, self.dev)

    def __call__(self, encoder_hidden_states, timestep, prompt_embeds_mask=None, tag=None):
        if tag is not None:                                   # sequential CFG (v1p2): one branch per call
            return self._one(encoder_hidden_states, timestep, 0 if tag == "cond" else 1)
        outs = [self._one(encoder_hidden_states[b:b + 1], timestep[b:b + 1], b) for b in range(encoder_hidden_states.shape[0])]
        return torch.cat([o[0] for o in outs], 0), [o[1] for o in outs]                    # batched CFG (v1p1)


def hip_step1x_connector_for(host, dev):
    """The host transformer's `connector` adopted onto the HIP kernels (regione_amd/step1x_connector.py), once
    per host pipeline and kept on it as `_regione_hip_connector`.  A `connector` that is not the public Qwen2Connector layout at all (no
    module, other parameter names) is left alone silently: None.  The layout with something the kernels do not cover (`connector_refusal`:
    head dim != 128, widths that are no multiples of 64, non-bf16 weights, missing / extra / mis-shaped parameters, PEFT / LoRA layers)
    stays the host's, with one warning naming the reason; `pipe._regione_hip_connector = False` before the first call keeps the host
    module on purpose, silently.  An adopted connector is checked against the module at every call (`HipStep1XConnector.stale`: parameter
    names, the tensors behind them, their versions): after a `load_lora_weights`, a `.to()` or a weight swap on `transformer.connector` it
    is adopted again, or refused with its warning.  A refusal is not looked at again: `del pipe._regione_hip_connector` has a repaired
    module considered."""
    cached = host.__dict__.get("_regione_hip_connector", _NO_HIP_VAE)
    if cached is False or cached is None:
        return None
    conn = getattr(getattr(host, "transformer", None), "connector", None)
    if cached is not _NO_HIP_VAE and not cached.stale(conn):
        return cached
    from . import step1x_connector as SC
    hip = None
    if SC.is_connector_layout(conn):
        why = SC.connector_refusal(conn)
        if why is None:
            try:
                hip = SC.HipStep1XConnector(conn, dev)
            except _lib.RegionEHipError as e:
                why = str(e)
        if why is not None:
            warnings.warn(f"connector kept on the host module: {why}", RuntimeWarning, stacklevel=3)
    host._regione_hip_connector = hip
    return hip


class _HipConnector:
    """`_HostConnector`'s call signature over the adopted connector (`hip_step1x_connector_for`): both CFG branches are prepared once per
    edit (`HipStep1XConnector.prepare`) and advanced together once per computed step (`step`), whichever way the engine asks - the batched
    v1p1 call with both rows, or v1p2's one call per branch `tag` (the second branch of a step is served from the first one's launch).
    `prepare` runs again when the embeddings handed in change - `callback_on_step_end` may replace `prompt_embeds` - keyed on the
    tensors themselves, their versions and shapes, like Step1XEditTransformer2DModel._batched_inputs.  v1p2's `ttm(emb) * tmask` does
    not depend on t either: `bind_text` evaluates it once per edit (a GEMM when `text_token_mapping` is one nn.Linear and the mask a run
    of ones then zeros, the host module once otherwise) and every step adds it with rgn_add_bf16, the eager op's rounding."""

    def __init__(self, hip, host_tr, dev, masks, embeds, text=None):
        self.hip, self.tr, self.dev, self.masks, self.text = hip, host_tr, dev, list(masks), text
        self.src = list(embeds)                    # the tensor each branch was last handed (held: identity is the key)
        self.key, self.gen, self.last, self.ttm = None, 0, None, [None] * len(self.src)

    @staticmethod
    def parse(masks, embeds):
        """(None, the valid length of every branch) when this call's embeddings and masks are what `prepare` takes, else (the reason, None).
        The one device-to-host read of each mask: `prepare` is handed the lengths."""
        from . import step1x_connector as SC
        ns = []
        for name, m, e in zip(("prompt", "negative prompt"), masks, embeds):
            if not isinstance(e, torch.Tensor) or e.dim() != 3 or e.shape[0] != 1:
                return f"{name} embeddings of shape {tuple(getattr(e, 'shape', ()))} (one [1, L, in] tensor per branch is covered)", None
            n = SC.mask_prefix(m, e.shape[1])
            if n is None:
                return f"a {name} mask that is not a run of ones followed by zeros over the {e.shape[1]} tokens", None
            ns.append(n)
        return None, ns

    def bind_text(self):
        ttm = getattr(self.tr, "text_token_mapping", None)
        if ttm is None or self.text is None:
            return
        from . import step1x_connector as SC
        for row, pair in enumerate(self.text):
            if pair is None:
                continue
            emb, tmask = pair
            L, K = emb.shape[1], emb.shape[2]
            n = SC.mask_prefix(tmask, L)
            wb = self.hip.adopt_ttm(ttm) if emb.dtype == torch.bfloat16 and n is not None else None
            if wb is None:
                with torch.no_grad():
                    self.ttm[row] = _bf(ttm(emb) * tmask[:, :, None], self.dev)[0].contiguous()
                continue
            Kp = wb[0].shape[1]
            x = emb.detach()[0].to(self.dev).contiguous()
            xp = torch.empty(L, Kp, dtype=torch.bfloat16, device=self.dev)
            _lib.check(_lib.lib().rgn_cast_pad_rows(ops._p(x), ops.BF16, x.stride(0), ops._p(xp), L, K, Kp, ops._stream()), "rgn_cast_pad_rows")
            out = torch.empty(L, self.hip.h, dtype=torch.bfloat16, device=self.dev)
            ops.gemm(xp, wb[0], wb[1], out)
            if n < L:                                 # `* tmask` of the padded rows
                _lib.check(_lib.lib().rgn_fill_zero(ops._p(out[n:]), (L - n) * self.hip.h * 2, ops._stream()), "rgn_fill_zero")
            self.ttm[row] = out

    def _prepared(self, keys, rows):
        def ver(t):
            return None if t.is_inference() else t._version
        key = tuple((id(t), ver(t), tuple(t.shape)) for t in keys)
        if key != self.key:
            self.hip.prepare(rows, self.masks)
            self.key, self.held, self.last = key, list(keys), None          # held: an id stays this tensor's while it is the key
            self.gen += 1

    def _step(self, timestep):
        tt = tuple(float(v) for v in timestep.detach().cpu().float().reshape(-1))
        if len(tt) == 1:
            tt = tt * len(self.masks)
        k = (self.gen, tt)
        if self.last is None or self.last[0] != k:
            outs = self.hip.step(torch.tensor(tt))
            for row, (e, _) in enumerate(outs):
                if self.ttm[row] is not None:                                                # v1p2 :606-609
                    ops.add_bf16(e[0], self.ttm[row], out=e[0])
            ev = torch.cuda.Event()
            ev.record()
            self.last = (k, outs, torch.cuda.current_stream(), ev)
        elif torch.cuda.current_stream() != self.last[2]:
            torch.cuda.current_stream().wait_event(self.last[3])        # a branch running on a side stream reads the other stream's launch
        return self.last[1]

    def __call__(self, encoder_hidden_states, timestep, prompt_embeds_mask=None, tag=None):
        if tag is not None:                                   # sequential CFG (v1p2): one branch per call
            row = 0 if tag == "cond" else 1
            self.src[row] = encoder_hidden_states
            self._prepared(self.src, [t[0] for t in self.src])
            return self._step(timestep)[row]
        B = encoder_hidden_states.shape[0]                    # batched CFG (v1p1): the rows of one [B, L, in] stack
        self._prepared([encoder_hidden_states], [encoder_hidden_states[b] for b in range(B)])
        outs = self._step(timestep)
        return self.hip.out.view(B, -1, self.hip.h), [o[1] for o in outs]


def _hosted_step1x(host, eng, image=None, prompt=None, negative_prompt=None, true_cfg_scale: float = 6.0, height=None, width=None,
                   num_inference_steps: int = 28, guidance_scale: float = 6.0, num_images_per_prompt: int = 1, generator=None,
                   latents=None, prompt_embeds=None, prompt_embeds_mask=None, negative_prompt_embeds=None,
                   negative_prompt_embeds_mask=None, output_type: str = "pil", return_dict: bool = True,
                   timesteps_truncate: float = 0.93, process_norm_power: float = 0.4, size_level=None, trace=None, sigmas=None,
                   callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), enable_thinking_mode=None,
                   enable_reflection_mode=None, max_try_cnt=None, **unused):
    """Step1XEditPipeline / Step1XEditPipelineV1P2 `__call__` around the engine loop (Step1XEdit/inplace.py:185-330,:437-455;
    Step1XEditV1P2/inplace.py:214-300).  Not hosted: v1p2's thinking / reflection retry loop (VLM prompting, :192-212) - the
    v1p2 switches `enable_thinking_mode` / `enable_reflection_mode` / `max_try_cnt` (Step1XEditV1P2/inplace.py:107-109) are
    accepted when they switch that loop OFF (the reference driver's own call, src/Step1X-Edit-v1p2/main.py:42-43,:69-77),
    True raises NotImplementedError; left unspecified the hosted call runs ONE attempt without reflection (the reference's
    signature default is reflection on: stated deviation)."""
    unused = _lora_call(host, eng, unused, "joint_attention_kwargs")
    v1p2 = _host_name(host).endswith("V1P2")
    think = dict(enable_thinking_mode=enable_thinking_mode, enable_reflection_mode=enable_reflection_mode, max_try_cnt=max_try_cnt)
    if v1p2:
        for k in ("enable_thinking_mode", "enable_reflection_mode"):
            if think[k]:
                raise NotImplementedError(f"{_host_name(host)}.__call__: {k}=True (the VLM thinking / reflection retry loop, "
                                          "Step1XEditV1P2/inplace.py:192-212) is not hosted by the HIP loop; pass False")
        if enable_reflection_mode is None:
            # the reference's signature default is reflection ON (Step1XEditV1P2/inplace.py:108): a caller that leaves it unspecified
            # gets ONE attempt here - say so instead of deviating silently (advisor finding, round 4)
            import warnings
            warnings.warn(f"{_host_name(host)}.__call__: enable_reflection_mode left unspecified - the reference defaults to True (a VLM "
                          "reflection retry loop), the HIP-hosted call runs ONE attempt without reflection; pass "
                          "enable_reflection_mode=False to acknowledge", stacklevel=3)
    else:                                   # v1p1 has no such arguments: a caller passing them gets the usual refusal
        unused = dict(unused, **{k: v for k, v in think.items() if v is not None})
    _refuse_unused(_host_name(host) + ".__call__", unused)
    dev = eng.transformer.device
    clk = _Clock(dev)
    exec_dev = getattr(host, "_execution_device", dev)
    _one_image_only(prompt, num_images_per_prompt)
    # 1. image (host.encode_image resizes, keeps the reference image for the VLM, remembers how to undo the resize)
    args = (image, width, height, size_level, exec_dev, 1) if v1p2 else (image, width, height, exec_dev, 1)
    image, ref_image, img_info, width, height = host.encode_image(*args)
    # 2./3. prompts through the host's VLM encoder
    has_neg = negative_prompt is not None or (negative_prompt_embeds is not None and negative_prompt_embeds_mask is not None)
    if not has_neg:
        negative_prompt = "" if image is not None else STEP1X_DEFAULT_NEGATIVE
    if v1p2:          # encode_prompt returns a record: embedding / mask / txt_ids / text_embeds / text_masks (:241-254)
        pos = host.encode_prompt(ref_image=ref_image, prompt=prompt, device=exec_dev, num_images_per_prompt=1)
        neg = host.encode_prompt(ref_image=ref_image, prompt=negative_prompt, device=exec_dev, num_images_per_prompt=1)
        prompt_embeds, prompt_embeds_mask = pos.embedding, pos.mask
        negative_prompt_embeds, negative_prompt_embeds_mask = neg.embedding, neg.mask
        text = [(pos.text_embeds, pos.text_masks), (neg.text_embeds, neg.text_masks)]
        dtype = pos.embedding.dtype
    else:
        prompt_embeds, prompt_embeds_mask, _ = host.encode_prompt(
            ref_image=ref_image, prompt=prompt, prompt_embeds=prompt_embeds, prompt_embeds_mask=prompt_embeds_mask,
            device=exec_dev, num_images_per_prompt=1)
        negative_prompt_embeds, negative_prompt_embeds_mask, _ = host.encode_prompt(
            ref_image=ref_image, prompt=negative_prompt, prompt_embeds=negative_prompt_embeds,
            prompt_embeds_mask=negative_prompt_embeds_mask, device=exec_dev, num_images_per_prompt=1)
        text, dtype = None, prompt_embeds.dtype
    # 4. latents
    pl = (image, 1, eng.transformer.cfg_model.in_channels // 4, height, width, dtype, exec_dev, generator)
    with _hip_vae_encode(host, dev):
        latents, image_latents, _, _ = host.prepare_latents(*pl) if v1p2 else host.prepare_latents(*pl, latents)
    # the connector: the adopted HIP one (prepared once per edit, advanced per computed step), or the host module per branch per step
    masks, embeds = [prompt_embeds_mask, negative_prompt_embeds_mask], [prompt_embeds, negative_prompt_embeds]
    hip = hip_step1x_connector_for(host, dev)
    if hip is not None:
        why, n_valid = _HipConnector.parse(masks, embeds)
        if why is not None:
            warnings.warn(f"connector kept on the host module for this call: {why}", RuntimeWarning, stacklevel=3)
            hip = None
    if hip is not None:
        connector = _HipConnector(hip, host.transformer, dev, n_valid, embeds, text)
        connector.bind_text()
    else:
        connector = _HostConnector(host.transformer, dev, masks, text)
    clk.mark("encode_s")
    # 5.-6. loop on the engine; the connector feeds it per computed step
    tr = eng.transformer
    prev = tr.__dict__.get("connector")
    tr.connector = connector
    try:
        kw = dict(image=_bf(image_latents, dev), prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds,
                  pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, height=height, width=width,
                  num_inference_steps=num_inference_steps, true_cfg_scale=true_cfg_scale, guidance_scale=guidance_scale,
                  latents=_bf(latents, dev), return_dict=False, timesteps_truncate=timesteps_truncate,
                  process_norm_power=process_norm_power)
        if trace is not None:
            kw["trace"] = trace
        latents = eng(**_loop_extras(kw, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs))[0]
    finally:
        if prev is None:
            tr.__dict__.pop("connector", None)
        else:
            tr.connector = prev
    clk.mark("loop_s")
    # 7. decode (:437-446)
    if output_type == "latent":
        out = latents
    else:
        vae = host.vae
        lat = host._unpack_latents(latents.to(getattr(vae, "dtype", latents.dtype)), height, width, host.vae_scale_factor)
        lat = lat / vae.config.scaling_factor + vae.config.shift_factor
        out = _postprocess_image(host, vae, lat, dev, output_type)
        out = host._output_process_image(out, img_info)
    if hasattr(host, "maybe_free_model_hooks"):
        host.maybe_free_model_hooks()
    clk.mark("decode_s")
    return HostedOutput(out, clk.out) if return_dict else (out,)


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
    ref_w, ref_h = ref.size if hasattr(ref, "size") and not isinstance(ref, torch.Tensor) else (ref.shape[-1], ref.shape[-2])
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
            iw, ih = img.size if hasattr(img, "size") and not isinstance(img, torch.Tensor) else (img.shape[-1], img.shape[-2])
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
    if trace is not None:
        kw["trace"] = trace
    latents = eng(**_loop_extras(kw, sigmas, callback_on_step_end, callback_on_step_end_tensor_inputs))[0]
    clk.mark("loop_s")
    if output_type == "latent":
        out = latents
    else:                                                                                  # QwenImageEdit/inplace.py:437-451
        vae = host.vae
        lat = host._unpack_latents(latents, height, width, host.vae_scale_factor).to(vae.dtype)
        mean = torch.tensor(vae.config.latents_mean).view(1, vae.config.z_dim, 1, 1, 1).to(lat.device, lat.dtype)
        inv_std = 1.0 / torch.tensor(vae.config.latents_std).view(1, vae.config.z_dim, 1, 1, 1).to(lat.device, lat.dtype)
        out = _postprocess_qwen_image(host, vae, lat / inv_std + mean, dev, output_type)
    if hasattr(host, "maybe_free_model_hooks"):
        host.maybe_free_model_hooks()
    clk.mark("decode_s")
    return HostedOutput(out, clk.out) if return_dict else (out,)


_HOSTED = {"FluxKontextPipeline": _hosted_flux, "Step1XEditPipeline": _hosted_step1x, "Step1XEditPipelineV1P2": _hosted_step1x,
           "QwenImageEditPipeline": _hosted_qwen, "QwenImageEditPlusPipeline": _hosted_qwen}


def is_engine_pipeline(pipe) -> bool:
    """True for a regione_amd.harness pipeline (latent-level, HIP transformer); False for a stock host pipeline."""
    from .harness import flux as HF
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

    @torch.no_grad()
    def __call__(self, *a, **kw):
        if a:
            raise TypeError("pass the pipeline arguments by keyword (image=..., prompt=...)")
        return self._call(self.host, self._regione_engine, **kw)


HostedFluxKontextPipeline = HostedPipeline          # round-1 name


def _host_name(pipe) -> str:
    cls = getattr(pipe, "_regione_host_class", None) or pipe.__class__
    return cls.__name__


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
    return eng


def swap_host_class(pipe):
    """Hook (1) of the reference (`pipeline.__class__ = RegionE<...>Pipeline`, inplace.py:53-62) on the HOST object: a
    subclass of the host's own class whose `__call__` is the hosted call.  The user keeps calling `pipe(...)`."""
    if getattr(pipe, "_regione_host_class", None) is not None:
        return pipe
    base = pipe.__class__
    call = _HOSTED[base.__name__]

    @torch.no_grad()
    def __call__(self, *a, **kw):
        if a:
            raise TypeError("pass the pipeline arguments by keyword (image=..., prompt=...)")
        return call(self, self._regione_engine, **kw)
    pipe._regione_host_class = base
    pipe.__class__ = type("RegionE" + base.__name__, (base,), {"__call__": __call__})
    return pipe


def restore_host_class(pipe):
    base = getattr(pipe, "_regione_host_class", None)
    if base is not None:
        pipe.__class__ = base
        pipe._regione_host_class = None
    return pipe
