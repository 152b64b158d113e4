"""The text encoders of FLUX.1 Kontext on the HIP kernels (`encode_prompt`).

`encode_prompt` (reference call sites FluxKontext/inplace.py:185-211) runs diffusers' `_get_clip_prompt_embeds` - the [EXT] transformers
`CLIPTextModel`, `pooler_output` - and `_get_t5_prompt_embeds` - the [EXT] `T5EncoderModel` (v1.1 gated-GELU layout), `last_hidden_state`.
Both are restated here on the library's kernels, rounding where the eager bf16 modules round:

  T5 layer   n = rms_norm_rows(h)                   T5LayerNorm (fp32 variance, bf16(x * rsqrt) * w)
             qkv = n @ [q; k; v]^T                  one rgn_gemm_group over the concatenated weight
             a = text_attention(qkv, bias table)    scale 1, the relative-position bias of block 0 shared by every layer
             h = h + a @ o^T                        RGN_EPI_GATE_RESID with a gate of ones = torch's bf16 `h + linear(a)`
             ff = n2 @ [wi_1; wi_0]^T               RGN_EPI_GELU from column d_ff: the linear half, then gelu_new(wi_0 n2)
             h = h + geglu(ff) @ wo^T               bf16(gelu * linear), then the gated residual again
  CLIP layer affine LayerNorm, q/k/v with biases in one GEMM, causal attention with scale 1/8, out_proj + residual, fc1, quick_gelu,
             fc2 + residual; final LayerNorm; the pooled row picked on the device (argmax(input_ids) or the first eos, as transformers).

Adoption takes a transformers module (or its state dict plus config) with strict name and shape checks; q, k, v (and T5's wi_1, wi_0)
are concatenated once.  T5's `wo` may arrive in fp32 (`_keep_in_fp32_modules`): it is cast to bf16 once, with a warning.  The T5 bias
table [H][2 Lmax - 1] is built at adoption with transformers' own `compute_bias` arithmetic on the module's device and copied: the bucket
of distances 16, 32 and 64 depends on the last bit of a float32 `log`, so it is not recomputed elsewhere.

There is no eager fallback inside: what the kernels do not implement (an attention mask, hidden states of every layer, L > Lmax, another
activation) raises RegionEHipError, and the adapter (regione_amd.adapters, components.py) keeps the host module for layouts it cannot adopt.
Activation buffers are kept for the last sequence length only; every call returns freshly allocated outputs.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional

import torch

from . import _lib, ops

_p, _stream = ops._p, ops._stream


class TextEncoderOutput:
    """What diffusers reads of a transformers encoder output: `.last_hidden_state`, `.pooler_output` (CLIP) and `[0]`."""

    def __init__(self, last_hidden_state: torch.Tensor, pooler_output: Optional[torch.Tensor] = None):
        self.last_hidden_state, self.pooler_output = last_hidden_state, pooler_output

    def to_tuple(self):
        return tuple(t for t in (self.last_hidden_state, self.pooler_output) if t is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]


def _refuse(what: str, why: str):
    raise _lib.RegionEHipError(f"{what}: {why}")


def _source(module_or_state_dict, config, device, what):
    """(state dict, config, device, module or None) of a transformers module or of a state dict plus its config."""
    if isinstance(module_or_state_dict, dict):
        if config is None:
            _refuse(what, "a state dict needs its config")
        return module_or_state_dict, config, torch.device(device or "cuda"), None
    m = module_or_state_dict
    sd = m.state_dict()
    dev = device
    if dev is None:
        dev = next(iter(sd.values())).device
    return sd, config or m.config, torch.device(dev), m


def _check_names(what: str, sd: Dict[str, torch.Tensor], want: Dict[str, tuple], optional=()):
    lora = [k for k in sd if "lora_" in k or ".base_layer." in k]
    if lora:
        _refuse(what, f"PEFT / LoRA layers in the module ({lora[:3]})")
    unknown = [k for k in sd if k not in want]
    if unknown:
        _refuse(what, f"state dict entries it does not know: {unknown[:6]}")
    missing = [k for k in want if k not in sd and k not in optional]
    if missing:
        _refuse(what, f"parameters missing from the state dict: {missing[:6]}")
    for k, shape in want.items():
        if k in sd and tuple(sd[k].shape) != shape:
            _refuse(what, f"{k} has shape {tuple(sd[k].shape)}, the config needs {shape}")


def _bf16_only(what: str, sd: Dict[str, torch.Tensor], allow_fp32=()):
    bad = [f"{k} ({v.dtype})" for k, v in sd.items() if v.dtype != torch.bfloat16 and not (k.endswith(allow_fp32) and v.dtype == torch.float32)]
    if bad:
        _refuse(what, f"non-bf16 weights: {bad[:3]} (the kernels take bf16 weights)")


def _check_k(what, **dims):
    bad = {k: v for k, v in dims.items() if v % 64}
    if bad:
        _refuse(what, f"GEMM reduction widths {bad} must be multiples of 64")


class _Buffers:
    """Activation buffers of ONE sequence length (the last one seen): a new length replaces the set, it does not add to it."""

    def __init__(self, device):
        self.device, self.L, self.t = device, None, {}

    def get(self, L: int, shapes: Dict[str, tuple]) -> Dict[str, torch.Tensor]:
        if L != self.L:
            self.t = {}
            self.t = {k: torch.empty(s, dtype=torch.bfloat16, device=self.device) for k, s in shapes.items()}
            self.L = L
        return self.t


class _HipTextEncoder:
    what = "text encoder"

    @property
    def dtype(self):
        return torch.bfloat16

    def _ids(self, input_ids, attention_mask, output_hidden_states, kw):
        if attention_mask is not None:
            _refuse(self.what, "attention_mask is not implemented (diffusers' FLUX prompt encoders pass none)")
        if output_hidden_states:
            _refuse(self.what, "output_hidden_states=True is not implemented (only the last hidden state is computed)")
        if kw:
            _refuse(self.what, f"arguments {sorted(kw)} are not implemented")
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() not in (1, 2):
            _refuse(self.what, "input_ids must be a [B, L] or [L] tensor")
        ids = input_ids.reshape(-1, input_ids.shape[-1]).to(self.device, torch.int64).contiguous()
        L = ids.shape[1]
        if not 1 <= L <= self.max_length:
            _refuse(self.what, f"sequence length {L} outside [1, {self.max_length}] (Lmax of this adoption)")
        return ids

    def _embed(self, ids_row, out, pos=None):
        L = ids_row.shape[0]
        rc = _lib.lib().rgn_text_embed(_p(ids_row), L, _p(self.tok), self.tok.shape[0], _p(pos), 0 if pos is None else pos.shape[0],
                                       _p(out), self.d, _stream())
        _lib.check(rc, "rgn_text_embed")

    def _rms(self, x, w, out):
        rc = _lib.lib().rgn_rms_norm_rows(_p(x), x.stride(0), _p(w), _p(out), out.stride(0), x.shape[0], self.d, self.eps, _stream())
        _lib.check(rc, "rgn_rms_norm_rows")

    def _attention(self, qkv, out, L, scale, causal, bias=None):
        rc = _lib.lib().rgn_text_attention_bf16(_p(qkv), _p(out), L, self.H, float(scale), int(causal), _p(bias), self.max_length, _stream())
        _lib.check(rc, "rgn_text_attention_bf16")


# ----------------------------------------------------------------------------------------------------------------------------------
def t5_bias_table(rel_bias_weight: torch.Tensor, Lmax: int, num_buckets: int, max_distance: int, attention=None) -> torch.Tensor:
    """[H, 2 Lmax - 1] bf16 (the weight's dtype): entry [h, r + Lmax - 1] = the bias of relative position r = j - i.  Built by
    transformers' own arithmetic on the weight's device: `attention.compute_bias(Lmax, Lmax)` when the module is at hand, else the same
    `_relative_position_bucket` + embedding on a [Lmax, Lmax] grid; row i = Lmax - 1 holds r <= 0, row 0 holds r >= 1."""
    if attention is not None:
        v = attention.compute_bias(Lmax, Lmax, device=rel_bias_weight.device)[0]          # [H, Lmax, Lmax]
    else:
        from transformers.models.t5.modeling_t5 import T5Attention
        dev = rel_bias_weight.device
        ctx = torch.arange(Lmax, dtype=torch.long, device=dev)[:, None]
        mem = torch.arange(Lmax, dtype=torch.long, device=dev)[None, :]
        b = T5Attention._relative_position_bucket(mem - ctx, bidirectional=True, num_buckets=num_buckets, max_distance=max_distance)
        v = torch.nn.functional.embedding(b, rel_bias_weight).permute(2, 0, 1)
    return torch.cat([v[:, Lmax - 1, :], v[:, 0, 1:]], dim=1).contiguous()


def t5_param_shapes(cfg) -> Dict[str, tuple]:
    d, inner, F, H = cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff, cfg.num_heads
    s = {"shared.weight": (cfg.vocab_size, d), "encoder.embed_tokens.weight": (cfg.vocab_size, d), "encoder.final_layer_norm.weight": (d,)}
    for i in range(cfg.num_layers):
        b = f"encoder.block.{i}.layer."
        for n in "qkv":
            s[f"{b}0.SelfAttention.{n}.weight"] = (inner, d)
        s[f"{b}0.SelfAttention.o.weight"] = (d, inner)
        if i == 0:
            s[f"{b}0.SelfAttention.relative_attention_bias.weight"] = (cfg.relative_attention_num_buckets, H)
        s[f"{b}0.layer_norm.weight"] = (d,)
        s[f"{b}1.DenseReluDense.wi_0.weight"] = (F, d)
        s[f"{b}1.DenseReluDense.wi_1.weight"] = (F, d)
        s[f"{b}1.DenseReluDense.wo.weight"] = (d, F)
        s[f"{b}1.layer_norm.weight"] = (d,)
    return s


def t5_refusal(cfg) -> Optional[str]:
    """Why a T5 config is not one the kernels implement (None: it is)."""
    if getattr(cfg, "model_type", None) != "t5":
        return f"model_type {getattr(cfg, 'model_type', None)!r} (a T5 encoder is covered)"
    if getattr(cfg, "is_decoder", False):
        return "a T5 decoder stack (the encoder is covered)"
    if not getattr(cfg, "is_gated_act", False) or getattr(cfg, "dense_act_fn", None) != "gelu_new":
        return (f"feed-forward {getattr(cfg, 'feed_forward_proj', None)!r}: only the v1.1 gated-GELU layout (gelu_new) is implemented, "
                "not a non-gated or ReLU T5")
    if cfg.d_kv != 64:
        return f"head dim {cfg.d_kv} (the attention kernel is head-dim 64)"
    return None


class HipT5EncoderModel(_HipTextEncoder):
    """`T5EncoderModel(input_ids)` on the HIP kernels: `.last_hidden_state` [B, L, d_model] bf16.  Lmax = `max_length` (FLUX: 512)."""
    what = "HipT5EncoderModel"

    def __init__(self, module_or_state_dict, device=None, config=None, max_length: int = 512):
        sd, cfg, dev, mod = _source(module_or_state_dict, config, device, self.what)
        why = t5_refusal(cfg)
        if why:
            _refuse(self.what, why)
        if not 1 <= max_length <= 4096:
            _refuse(self.what, f"max_length {max_length} outside [1, 4096]")
        self.config, self.device, self.max_length = cfg, dev, int(max_length)
        self.d, self.H, self.F, self.eps = cfg.d_model, cfg.num_heads, cfg.d_ff, float(cfg.layer_norm_epsilon)
        self.inner = self.H * 64
        _check_k(self.what, d_model=self.d, inner=self.inner, d_ff=self.F)
        want = t5_param_shapes(cfg)
        _check_names(self.what, sd, want, optional=("shared.weight", "encoder.embed_tokens.weight"))
        _bf16_only(self.what, sd, allow_fp32=(".wo.weight",))
        emb = [sd[k] for k in ("shared.weight", "encoder.embed_tokens.weight") if k in sd]
        if not emb:
            _refuse(self.what, "neither shared.weight nor encoder.embed_tokens.weight is in the state dict")
        if len(emb) == 2 and emb[0].data_ptr() != emb[1].data_ptr() and not torch.equal(emb[0], emb[1].to(emb[0].device)):
            _refuse(self.what, "shared.weight and encoder.embed_tokens.weight differ (T5EncoderModel ties them)")
        fp32_wo = [k for k, v in sd.items() if k.endswith(".wo.weight") and v.dtype == torch.float32]
        if fp32_wo:
            warnings.warn(f"{self.what}: {len(fp32_wo)} feed-forward `wo` weights arrive in fp32 (transformers' _keep_in_fp32_modules); "
                          "cast to bf16 once at adoption", RuntimeWarning, stacklevel=2)

        def w(k):
            return sd[k].to(dev, torch.bfloat16).contiguous()
        self.tok = emb[0].to(dev, torch.bfloat16).contiguous()
        self.layers = []
        for i in range(cfg.num_layers):
            b = f"encoder.block.{i}.layer."
            a = b + "0.SelfAttention."
            self.layers.append(dict(
                ln1=w(b + "0.layer_norm.weight"),
                wqkv=torch.cat([sd[a + n + ".weight"].to(dev, torch.bfloat16) for n in "qkv"]).contiguous(),
                wo_attn=w(a + "o.weight"),
                ln2=w(b + "1.layer_norm.weight"),
                wi=torch.cat([sd[b + "1.DenseReluDense.wi_1.weight"].to(dev, torch.bfloat16),
                              sd[b + "1.DenseReluDense.wi_0.weight"].to(dev, torch.bfloat16)]).contiguous(),
                wo_ff=w(b + "1.DenseReluDense.wo.weight")))
        self.final_ln = w("encoder.final_layer_norm.weight")
        rb = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
        attn0 = mod.encoder.block[0].layer[0].SelfAttention if mod is not None else None
        self.bias_table = t5_bias_table(rb, self.max_length, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance,
                                        attention=attn0).to(dev, torch.bfloat16).contiguous()
        self.ones = torch.ones(self.d, dtype=torch.bfloat16, device=dev)
        self.buf = _Buffers(dev)

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True, **kw):
        ids = self._ids(input_ids, attention_mask, output_hidden_states, kw)
        B, L = ids.shape
        t = self.buf.get(L, dict(h=(L, self.d), n=(L, self.d), qkv=(L, 3 * self.inner), a=(L, self.inner), ff=(L, 2 * self.F),
                                 g=(L, self.F)))
        h, n, qkv, a, ff, g = t["h"], t["n"], t["qkv"], t["a"], t["ff"], t["g"]
        out = torch.empty(B, L, self.d, dtype=torch.bfloat16, device=self.device)
        lib = _lib.lib()
        for bi in range(B):
            self._embed(ids[bi], h)
            for p in self.layers:
                self._rms(h, p["ln1"], n)
                ops.gemm(n, p["wqkv"], None, qkv)
                self._attention(qkv, a, L, 1.0, False, self.bias_table)
                ops.gemm(a, p["wo_attn"], None, h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
                self._rms(h, p["ln2"], n)
                ops.gemm(n, p["wi"], None, ff, epilogue=ops.EPI_GELU, gelu_from_col=self.F)
                _lib.check(lib.rgn_geglu_bf16(_p(ff), ff.stride(0), _p(g), g.stride(0), L, self.F, _stream()), "rgn_geglu_bf16")
                ops.gemm(g, p["wo_ff"], None, h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
            self._rms(h, self.final_ln, out[bi])
        res = TextEncoderOutput(out)
        return res if return_dict else res.to_tuple()


# ----------------------------------------------------------------------------------------------------------------------------------
def clip_param_shapes(cfg) -> Dict[str, tuple]:
    d, F = cfg.hidden_size, cfg.intermediate_size
    s = {"embeddings.token_embedding.weight": (cfg.vocab_size, d), "embeddings.position_embedding.weight": (cfg.max_position_embeddings, d),
         "final_layer_norm.weight": (d,), "final_layer_norm.bias": (d,)}
    for i in range(cfg.num_hidden_layers):
        b = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[f"{b}self_attn.{n}.weight"], s[f"{b}self_attn.{n}.bias"] = (d, d), (d,)
        for n in ("layer_norm1", "layer_norm2"):
            s[f"{b}{n}.weight"], s[f"{b}{n}.bias"] = (d,), (d,)
        s[f"{b}mlp.fc1.weight"], s[f"{b}mlp.fc1.bias"] = (F, d), (F,)
        s[f"{b}mlp.fc2.weight"], s[f"{b}mlp.fc2.bias"] = (d, F), (d,)
    return s


def clip_refusal(cfg) -> Optional[str]:
    """Why a CLIP text config is not one the kernels implement (None: it is)."""
    if getattr(cfg, "model_type", None) != "clip_text_model":
        return f"model_type {getattr(cfg, 'model_type', None)!r} (a CLIP text model is covered)"
    if getattr(cfg, "hidden_act", None) != "quick_gelu":
        return f"hidden_act {getattr(cfg, 'hidden_act', None)!r} (quick_gelu is implemented)"
    if cfg.hidden_size % cfg.num_attention_heads or cfg.hidden_size // cfg.num_attention_heads != 64:
        return f"head dim {cfg.hidden_size / cfg.num_attention_heads:g} (the attention kernel is head-dim 64)"
    if getattr(cfg, "eos_token_id", None) is None:
        return "no eos_token_id in the config (the pooled row is chosen by it)"
    return None


def pooled_index(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """CLIPTextModel's pooled position per row (the rule rgn_text_pool_row applies on the device): argmax(input_ids) when
    eos_token_id == 2, else the first position of eos_token_id (0 when there is none)."""
    ids = input_ids.to(torch.int)
    return ids.argmax(dim=-1) if eos_token_id == 2 else (ids == eos_token_id).int().argmax(dim=-1)


class HipClipTextModel(_HipTextEncoder):
    """`CLIPTextModel(input_ids)` on the HIP kernels: `.last_hidden_state` [B, L, d] and `.pooler_output` [B, d], bf16.
    Lmax = max_position_embeddings (CLIP-L: 77)."""
    what = "HipClipTextModel"

    def __init__(self, module_or_state_dict, device=None, config=None):
        sd, cfg, dev, _ = _source(module_or_state_dict, config, device, self.what)
        why = clip_refusal(cfg)
        if why:
            _refuse(self.what, why)
        if any(k.startswith("text_model.") for k in sd):
            sd = {k[len("text_model."):] if k.startswith("text_model.") else k: v for k, v in sd.items()}
        self.config, self.device, self.max_length = cfg, dev, int(cfg.max_position_embeddings)
        self.d, self.F, self.H, self.eps = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, float(cfg.layer_norm_eps)
        self.eos = int(cfg.eos_token_id)
        _check_k(self.what, hidden_size=self.d, intermediate_size=self.F)
        _check_names(self.what, sd, clip_param_shapes(cfg))
        _bf16_only(self.what, sd)

        def w(k):
            return sd[k].to(dev, torch.bfloat16).contiguous()

        def cat(b, kind):
            return torch.cat([sd[f"{b}self_attn.{n}_proj.{kind}"].to(dev, torch.bfloat16) for n in "qkv"]).contiguous()
        self.tok, self.pos = w("embeddings.token_embedding.weight"), w("embeddings.position_embedding.weight")
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            b = f"encoder.layers.{i}."
            self.layers.append(dict(
                ln1=(w(b + "layer_norm1.weight"), w(b + "layer_norm1.bias")), wqkv=cat(b, "weight"), bqkv=cat(b, "bias"),
                wo=w(b + "self_attn.out_proj.weight"), bo=w(b + "self_attn.out_proj.bias"),
                ln2=(w(b + "layer_norm2.weight"), w(b + "layer_norm2.bias")),
                w1=w(b + "mlp.fc1.weight"), b1=w(b + "mlp.fc1.bias"), w2=w(b + "mlp.fc2.weight"), b2=w(b + "mlp.fc2.bias")))
        self.final_ln = (w("final_layer_norm.weight"), w("final_layer_norm.bias"))
        self.scale = (self.d // self.H) ** -0.5
        self.ones = torch.ones(self.d, dtype=torch.bfloat16, device=dev)
        self.buf = _Buffers(dev)

    def _ln(self, x, gb, out):
        rc = _lib.lib().rgn_layer_norm_rows(_p(x), x.stride(0), _p(gb[0]), _p(gb[1]), _p(out), out.stride(0), x.shape[0], self.d, self.eps,
                                            _stream())
        _lib.check(rc, "rgn_layer_norm_rows")

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True, **kw):
        ids = self._ids(input_ids, attention_mask, output_hidden_states, kw)
        B, L = ids.shape
        t = self.buf.get(L, dict(h=(L, self.d), n=(L, self.d), qkv=(L, 3 * self.d), a=(L, self.d), f=(L, self.F)))
        h, n, qkv, a, f = t["h"], t["n"], t["qkv"], t["a"], t["f"]
        out = torch.empty(B, L, self.d, dtype=torch.bfloat16, device=self.device)
        pooled = torch.empty(B, self.d, dtype=torch.bfloat16, device=self.device)
        lib = _lib.lib()
        for bi in range(B):
            self._embed(ids[bi], h, self.pos)
            for p in self.layers:
                self._ln(h, p["ln1"], n)
                ops.gemm(n, p["wqkv"], p["bqkv"], qkv)
                self._attention(qkv, a, L, self.scale, True)
                ops.gemm(a, p["wo"], p["bo"], h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
                self._ln(h, p["ln2"], n)
                ops.gemm(n, p["w1"], p["b1"], f)
                _lib.check(lib.rgn_quick_gelu_bf16(_p(f), _p(f), f.numel(), _stream()), "rgn_quick_gelu_bf16")
                ops.gemm(f, p["w2"], p["b2"], h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
            self._ln(h, self.final_ln, out[bi])
            rc = lib.rgn_text_pool_row(_p(ids[bi]), L, self.eos, _p(out[bi]), self.d, self.d, _p(pooled[bi]), _stream())
            _lib.check(rc, "rgn_text_pool_row")
        res = TextEncoderOutput(out, pooled)
        return res if return_dict else res.to_tuple()
