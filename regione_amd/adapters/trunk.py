"""The trunk: a host transformer's weights onto the engine (`adopt_engine`) - per-family parameter-name maps, the strict layout check,
and LoRA (PEFT layers merged on the device at adoption, re-merged by `lora_sync` when the adapter state changes)."""
from __future__ import annotations

import re
from typing import Dict, Iterable, Iterator, Optional, Tuple

import torch

from .. import ops
from ..synth import FluxConfig, flux_param_shapes

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
    from ..harness import flux as HF, qwen as HQ, step1x as HS
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
