"""The vision tower of the Qwen2.5-VL prompt encoder on the HIP kernels (`encode_prompt` of Qwen-Image-Edit).

`get_image_features` of the [EXT] transformers `Qwen2_5_VLForConditionalGeneration` runs `Qwen2_5_VisionTransformerPretrainedModel` over
the condition images' patches.  The tower is restated here on the library's kernels, rounding where the eager bf16 module rounds:

  patches x = cast_pad_rows(pixel_values)            `.to(bfloat16)`, K = C * 2 * p * p padded with zero columns to a multiple of 64
          h = x @ patch^T                            the Conv3d with stride = kernel as ONE rgn_gemm_group; `out_rows` writes each patch at its
                                                     place in the window order (the module's `hidden_states[window_index]`)
  block   n = rms_norm_rows(h)                       Qwen2_5_VLRMSNorm
          qkv = n @ qkv^T + b                        one GEMM: [L, 3 H Dp], all q heads | all k heads | all v heads, head width padded to Dp
          vision_rope(qkv, cos, sin)                 apply_rotary_pos_emb_vision on the q and k columns, in place (fp32, one rounding)
          a = vision_attention(qkv, items)           non-causal, inside the segments of `cu_window_seqlens` (window blocks) or `cu_seqlens`
                                                     (fullatt_block_indexes); scale = real head width ^ -0.5
          h = h + (a @ proj^T + b)                   RGN_EPI_GATE_RESID with a gate of ones = torch's bf16 `h + linear(a)`
          ff = n2 @ [gate; up]^T + [bg; bu]          one GEMM, then swiglu: bf16(bf16(silu(gate)) * up)
          h = h + (swiglu(ff) @ down^T + b)          the gated residual again
  merger  m = gelu_erf(rms_norm_rows(h).view(-1, 4 d) @ mlp.0^T + b);  pooled = m @ mlp.2^T + b, `out_rows` = window_index: the rows land
          in the module's original, un-windowed order (`merged[argsort(window_index)]`)

Padding is done once, at adoption, with zeros: the head width to a multiple of 32 (qkv weight rows and bias entries per head, proj weight
columns), the MLP width to a multiple of 64 (gate / up rows and biases, down columns; silu(0) * 0 = 0), the patch-embedding K to a multiple
of 64.  A padded column only ever adds an exact zero to an fp32 sum, so no real output changes by a bit.

Per call the host side asks the installed transformers (on the CPU) for what the module's `forward` computes - `get_vision_position_ids`,
`get_vision_window_index`, `get_vision_cu_seqlens` - builds the rotary table with the module's own `rotary_pos_emb` arithmetic and
`inv_freq` buffer in ITS dtype (a `.to(bfloat16)` module carries a bf16-rounded buffer and gets bf16 tables, which the eager forward
uses; upcast to fp32 after), cuts the two item tables of rgn_vision_attention_bf16 and copies everything to the device once.  Tables and
activation buffers are kept for the last `grid_thw` only; every call returns freshly allocated outputs.

There is no eager fallback inside: what the kernels do not implement (videos, another activation, non-bf16 weights, LoRA layers, more
than `max_patches` rows) raises RegionEHipError before any launch, and the adapter keeps the host's tower for configs `vision_refusal` names.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib, ops
from .text_encoders import TextEncoderOutput, _Buffers, _bf16_only, _check_names, _refuse, _source

_p, _stream = ops._p, ops._stream

VISUAL = "model.visual."
EPS = 1e-6                                            # Qwen2_5_VLVisionBlock / Qwen2_5_VLPatchMerger build their norms with eps=1e-6
ITEM_Q = 64                                           # queries per attention item (ATTN_BQ of csrc/attn_tile.h)


def _vision_config(cfg):
    return getattr(cfg, "vision_config", None) or cfg


def padded_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def vision_refusal(cfg) -> Optional[str]:
    """Why a Qwen2.5-VL vision config (the composite config or its vision_config) is not one the kernels implement (None: it is)."""
    vc = _vision_config(cfg)
    if getattr(vc, "hidden_act", None) != "silu":
        return f"hidden_act {getattr(vc, 'hidden_act', None)!r} (silu is implemented)"
    d, H = vc.hidden_size, vc.num_heads
    if d % 64:
        return f"hidden_size {d} is not a multiple of 64"
    if H < 1 or d % H:
        return f"hidden_size {d} is not divisible by num_heads {H}"
    hd = d // H
    if hd % 8 or hd > 128:
        return f"head width {hd} (a multiple of 8, at most 128)"
    if (H * padded_to(hd, 32)) % 64:
        return f"{H} heads of padded width {padded_to(hd, 32)}: the attention width is not a multiple of 64"
    if vc.out_hidden_size % 8:
        return f"out_hidden_size {vc.out_hidden_size} is not a multiple of 8"
    return None


def vision_param_shapes(cfg, prefix: str = "") -> Dict[str, tuple]:
    vc = _vision_config(cfg)
    d, F, m = vc.hidden_size, vc.intermediate_size, vc.spatial_merge_size ** 2
    s = {"patch_embed.proj.weight": (d, vc.in_channels, vc.temporal_patch_size, vc.patch_size, vc.patch_size),
         "merger.ln_q.weight": (d,), "merger.mlp.0.weight": (m * d, m * d), "merger.mlp.0.bias": (m * d,),
         "merger.mlp.2.weight": (vc.out_hidden_size, m * d), "merger.mlp.2.bias": (vc.out_hidden_size,)}
    for i in range(vc.depth):
        b = f"blocks.{i}."
        s[b + "norm1.weight"], s[b + "norm2.weight"] = (d,), (d,)
        s[b + "attn.qkv.weight"], s[b + "attn.qkv.bias"] = (3 * d, d), (3 * d,)
        s[b + "attn.proj.weight"], s[b + "attn.proj.bias"] = (d, d), (d,)
        for n in ("gate_proj", "up_proj"):
            s[f"{b}mlp.{n}.weight"], s[f"{b}mlp.{n}.bias"] = (F, d), (F,)
        s[b + "mlp.down_proj.weight"], s[b + "mlp.down_proj.bias"] = (d, F), (d,)
    return {prefix + k: v for k, v in s.items()}


# ---- padding (once, at adoption) ----------------------------------------------------------------------------------------------------------
def _pad_dim(t: torch.Tensor, dim: int, n: int) -> torch.Tensor:
    if t.shape[dim] == n:
        return t.contiguous()
    shape = list(t.shape)
    shape[dim] = n - t.shape[dim]
    return torch.cat([t, t.new_zeros(shape)], dim=dim).contiguous()


def padded_widths(cfg):
    """(Dp, Fp, Kp): the head width padded to a multiple of 32, the MLP width and the patch-embedding K to multiples of 64."""
    vc = _vision_config(cfg)
    K = vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2
    return padded_to(vc.hidden_size // vc.num_heads, 32), padded_to(vc.intermediate_size, 64), padded_to(K, 64)


def pad_weights(sd: Dict[str, torch.Tensor], cfg) -> Dict[str, torch.Tensor]:
    """The tower's parameters (bare names) in the layout the kernels read, zero-padded: per block `wqkv` [3 H Dp, d], `bqkv` [3 H Dp],
    `wproj` [d, H Dp], `wgu` [2 Fp, d] = [gate; up], `bgu` [2 Fp], `wdown` [d, Fp]; `patch` [d, Kp]; the rest as they are."""
    vc = _vision_config(cfg)
    d, H, F = vc.hidden_size, vc.num_heads, vc.intermediate_size
    hd = d // H
    Dp, Fp, Kp = padded_widths(cfg)
    out = {"patch": _pad_dim(sd["patch_embed.proj.weight"].reshape(d, -1), 1, Kp)}
    for i in range(vc.depth):
        b, o = f"blocks.{i}.", f"blocks.{i}."
        out[o + "ln1"], out[o + "ln2"] = sd[b + "norm1.weight"].contiguous(), sd[b + "norm2.weight"].contiguous()
        out[o + "wqkv"] = _pad_dim(sd[b + "attn.qkv.weight"].reshape(3, H, hd, d), 2, Dp).reshape(3 * H * Dp, d)
        out[o + "bqkv"] = _pad_dim(sd[b + "attn.qkv.bias"].reshape(3, H, hd), 2, Dp).reshape(3 * H * Dp)
        out[o + "wproj"] = _pad_dim(sd[b + "attn.proj.weight"].reshape(d, H, hd), 2, Dp).reshape(d, H * Dp)
        out[o + "bproj"] = sd[b + "attn.proj.bias"].contiguous()
        out[o + "wgu"] = torch.cat([_pad_dim(sd[f"{b}mlp.{n}.weight"], 0, Fp) for n in ("gate_proj", "up_proj")]).contiguous()
        out[o + "bgu"] = torch.cat([_pad_dim(sd[f"{b}mlp.{n}.bias"], 0, Fp) for n in ("gate_proj", "up_proj")]).contiguous()
        out[o + "wdown"] = _pad_dim(sd[b + "mlp.down_proj.weight"], 1, Fp)
        out[o + "bdown"] = sd[b + "mlp.down_proj.bias"].contiguous()
    for k, n in (("merger.ln", "merger.ln_q.weight"), ("merger.w0", "merger.mlp.0.weight"), ("merger.b0", "merger.mlp.0.bias"),
                 ("merger.w2", "merger.mlp.2.weight"), ("merger.b2", "merger.mlp.2.bias")):
        out[k] = sd[n].contiguous()
    return out


def unpad_weights(pw: Dict[str, torch.Tensor], cfg) -> Dict[str, torch.Tensor]:
    """The inverse of `pad_weights`: the module's own names and shapes (the pad regions dropped)."""
    vc = _vision_config(cfg)
    d, H, F = vc.hidden_size, vc.num_heads, vc.intermediate_size
    hd = d // H
    Dp, Fp, Kp = padded_widths(cfg)
    K = vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2
    sd = {"patch_embed.proj.weight": pw["patch"][:, :K].reshape(d, vc.in_channels, vc.temporal_patch_size, vc.patch_size, vc.patch_size)}
    for i in range(vc.depth):
        b = f"blocks.{i}."
        sd[b + "norm1.weight"], sd[b + "norm2.weight"] = pw[b + "ln1"], pw[b + "ln2"]
        sd[b + "attn.qkv.weight"] = pw[b + "wqkv"].reshape(3, H, Dp, d)[:, :, :hd].reshape(3 * d, d)
        sd[b + "attn.qkv.bias"] = pw[b + "bqkv"].reshape(3, H, Dp)[:, :, :hd].reshape(3 * d)
        sd[b + "attn.proj.weight"] = pw[b + "wproj"].reshape(d, H, Dp)[:, :, :hd].reshape(d, d)
        sd[b + "attn.proj.bias"] = pw[b + "bproj"]
        sd[b + "mlp.gate_proj.weight"], sd[b + "mlp.up_proj.weight"] = pw[b + "wgu"][:F], pw[b + "wgu"][Fp:Fp + F]
        sd[b + "mlp.gate_proj.bias"], sd[b + "mlp.up_proj.bias"] = pw[b + "bgu"][:F], pw[b + "bgu"][Fp:Fp + F]
        sd[b + "mlp.down_proj.weight"], sd[b + "mlp.down_proj.bias"] = pw[b + "wdown"][:, :F], pw[b + "bdown"]
    for k, n in (("merger.ln", "merger.ln_q.weight"), ("merger.w0", "merger.mlp.0.weight"), ("merger.b0", "merger.mlp.0.bias"),
                 ("merger.w2", "merger.mlp.2.weight"), ("merger.b2", "merger.mlp.2.bias")):
        sd[n] = pw[k]
    return sd


# ---- host-side tables (no kernel) -----------------------------------------------------------------------------------------------------------
def default_inv_freq(cfg) -> torch.Tensor:
    """Qwen2_5_VisionRotaryEmbedding(head_dim // 2).inv_freq in fp32 (used when no module is at hand)."""
    vc = _vision_config(cfg)
    dim = vc.hidden_size // vc.num_heads // 2
    return 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))


def attention_items(cu_seqlens) -> torch.Tensor:
    """int32 [n_items, 4] = (q0, n_q, k_lo, k_hi) of rgn_vision_attention_bf16: every segment [a, b) of `cu_seqlens` cut into runs of at
    most 64 queries whose keys are the segment - no item crosses a segment, every row lies in exactly one item."""
    cu = [int(v) for v in cu_seqlens]
    rows = [(q0, min(ITEM_Q, b - q0), a, b) for a, b in zip(cu[:-1], cu[1:]) for q0 in range(a, b, ITEM_Q)]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def vision_tables(cfg, inv_freq: torch.Tensor, grid_thw) -> Dict[str, torch.Tensor]:
    """What Qwen2_5_VisionTransformerPretrainedModel.forward computes from `grid_thw` before its first block, on the CPU:
      cos, sin          fp32 [N, head width]: the `position_embeddings` the blocks receive (window order), computed in inv_freq's dtype
      window_index      int64 [N / merge^2];  patch_rows int64 [N]: the window-order row of every patch
      cu_seqlens / cu_window_seqlens  the segment lists of a full-attention / a window block;  items_full / items_window  their item tables"""
    from transformers.vision_utils import get_vision_cu_seqlens, get_vision_position_ids, get_vision_window_index
    vc = _vision_config(cfg)
    grid = torch.as_tensor(grid_thw).detach().cpu().to(torch.int64).reshape(-1, 3)
    unit = vc.spatial_merge_size ** 2
    pos = get_vision_position_ids(grid, vc.spatial_merge_size)
    cu = get_vision_cu_seqlens(grid)
    window_index, cu_win = get_vision_window_index(grid, spatial_merge_size=vc.spatial_merge_size, window_size=vc.window_size,
                                                   patch_size=vc.patch_size)
    N = pos.shape[0]
    rot = (pos.unsqueeze(-1) * inv_freq.cpu()).flatten(1)                         # Qwen2_5_VisionRotaryEmbedding.forward
    rot = rot.reshape(N // unit, unit, -1)[window_index, :, :].reshape(N, -1)
    emb = torch.cat((rot, rot), dim=-1)
    reverse = torch.argsort(window_index)
    patch_rows = (reverse[:, None] * unit + torch.arange(unit)[None, :]).reshape(-1)
    return dict(cos=emb.cos().float().contiguous(), sin=emb.sin().float().contiguous(), window_index=window_index.to(torch.int64).contiguous(),
                patch_rows=patch_rows.to(torch.int64).contiguous(), cu_seqlens=cu, cu_window_seqlens=cu_win,
                items_full=attention_items(cu.tolist()), items_window=attention_items(cu_win.tolist()))


class HipQwen25VLVisionTower:
    """`Qwen2_5_VisionTransformerPretrainedModel(pixel_values, grid_thw)` on the HIP kernels.  Adopts the tower of a
    Qwen2_5_VLForConditionalGeneration (`model.visual.*`), the tower itself, or a state dict of either with its config.  Returns an object
    with `.pooler_output` [N / merge^2, out_hidden_size] (the merged rows in the module's original order) and `.last_hidden_state` [N, d]
    (window order, as the module's), both freshly allocated bf16.  `pixel_values`: fp32 or bf16 [N, K] as the image processor returns
    them, or bf16 [N, Kp] rows whose columns [K, Kp) the caller has zeroed (they skip rgn_cast_pad_rows and are not checked)."""
    what = "HipQwen25VLVisionTower"

    def __init__(self, module_or_state_dict, device=None, config=None, max_patches: int = 16384):
        sd, cfg, dev, mod = _source(module_or_state_dict, config, device, self.what)
        why = vision_refusal(cfg)
        if why:
            _refuse(self.what, why)
        if max_patches < 1:
            _refuse(self.what, f"max_patches {max_patches} < 1")
        vc = _vision_config(cfg)
        self.config, self.device, self.max_patches = vc, dev, int(max_patches)
        if any(k.startswith(VISUAL) for k in sd):
            sd = {k[len(VISUAL):]: v for k, v in sd.items() if k.startswith(VISUAL)}
        _check_names(self.what, sd, vision_param_shapes(cfg))
        _bf16_only(self.what, sd)
        self.d, self.H, self.F, self.out = vc.hidden_size, vc.num_heads, vc.intermediate_size, vc.out_hidden_size
        self.hd, self.unit, self.depth = self.d // self.H, vc.spatial_merge_size ** 2, vc.depth
        self.Dp, self.Fp, self.Kp = padded_widths(cfg)
        self.K = vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2
        self.scale = self.hd ** -0.5
        self.full = set(int(i) for i in vc.fullatt_block_indexes)
        self.w = {k: v.to(dev) for k, v in pad_weights({k: v.detach() for k, v in sd.items()}, cfg).items()}
        tower = None
        if mod is not None:
            tower = getattr(getattr(mod, "model", mod), "visual", None) or getattr(mod, "visual", None) or mod
        rot = getattr(tower, "rotary_pos_emb", None)
        # the module's own inv_freq buffer in its own dtype (a `.to(bfloat16)` of the module rounds it; the eager forward uses that one)
        self.inv_freq = rot.inv_freq.detach().cpu() if rot is not None else default_inv_freq(cfg)
        self.ones = torch.ones(self.d, dtype=torch.bfloat16, device=dev)
        self.buf = _Buffers(dev)
        self._tab_key, self._tab = None, None

    @property
    def dtype(self):
        return torch.bfloat16

    # ---- host-side preparation (no kernel) -------------------------------------------------------------------------------------------
    def _tables(self, grid_thw):
        if not isinstance(grid_thw, torch.Tensor) or grid_thw.dim() != 2 or grid_thw.shape[1] != 3 or grid_thw.shape[0] < 1:
            _refuse(self.what, "grid_thw must be a [n_images, 3] tensor")
        grid = grid_thw.detach().cpu().to(torch.int64)
        key = tuple(tuple(int(v) for v in r) for r in grid.tolist())
        m = self.config.spatial_merge_size
        for t, h, w in key:
            if t != 1:
                _refuse(self.what, f"grid {(t, h, w)}: videos (t != 1) are not implemented")
            if h < m or w < m or h % m or w % m:
                _refuse(self.what, f"grid {(t, h, w)}: h and w must be positive multiples of spatial_merge_size {m}")
        N = sum(h * w for _, h, w in key)
        if N > self.max_patches:
            _refuse(self.what, f"{N} patches exceed max_patches {self.max_patches} of this adoption")
        if key != self._tab_key:
            tab = vision_tables(self.config, self.inv_freq, grid)
            self._tab = {k: tab[k].to(self.device) for k in ("cos", "sin", "window_index", "patch_rows", "items_full", "items_window")}
            self._tab_key = key
        return key, N, self._tab

    def _rms(self, x, w, out):
        rc = _lib.lib().rgn_rms_norm_rows(_p(x), x.stride(0), _p(w), _p(out), out.stride(0), x.shape[0], self.d, EPS, _stream())
        _lib.check(rc, "rgn_rms_norm_rows")

    # ---- the call --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, pixel_values, grid_thw, return_dict=True, **kw):
        if kw:
            _refuse(self.what, f"arguments {sorted(kw)} are not implemented")
        key, N, tab = self._tables(grid_thw)
        # bf16 rows already padded to the GEMM's K ([N, Kp]: HipImageOps.to_patch_rows(out="padded_bf16")) are the patch GEMM's operand as
        # they stand.  CALLER'S OBLIGATION: the columns [K, Kp) are zero - they are not looked at (a device read), and anything else there
        # is multiplied into the patch embedding.
        padded = isinstance(pixel_values, torch.Tensor) and self.Kp != self.K and pixel_values.dtype == torch.bfloat16 and \
            tuple(pixel_values.shape) == (N, self.Kp)
        if not padded and (not isinstance(pixel_values, torch.Tensor) or pixel_values.dim() != 2 or tuple(pixel_values.shape) != (N, self.K)):
            _refuse(self.what, f"pixel_values of shape {tuple(getattr(pixel_values, 'shape', ()))} for grid_thw {list(key)} (rows [{N}, {self.K}], or bf16 [{N}, {self.Kp}] zero-padded by the caller)")
        if pixel_values.dtype not in (torch.float32, torch.bfloat16):
            _refuse(self.what, f"pixel_values of dtype {pixel_values.dtype} (fp32 or bf16)")
        x = pixel_values.detach().to(self.device).contiguous()
        d, H, Dp, Fp, w = self.d, self.H, self.Dp, self.Fp, self.w
        M = N // self.unit
        t = self.buf.get(key, dict(xp=(N, self.Kp), h=(N, d), n=(N, d), qkv=(N, 3 * H * Dp), a=(N, H * Dp), ff=(N, 2 * Fp), g=(N, Fp),
                                   m=(M, self.unit * d)))
        xp, h, n, qkv, a, ff, g, m1 = (t[k] for k in ("xp", "h", "n", "qkv", "a", "ff", "g", "m"))
        lib = _lib.lib()
        if padded:
            xp = x
        else:
            _lib.check(lib.rgn_cast_pad_rows(_p(x), ops._dt(x), x.stride(0), _p(xp), N, self.K, self.Kp, _stream()), "rgn_cast_pad_rows")
        ops.gemm(xp, w["patch"], None, h, out_rows=tab["patch_rows"])
        cos, sin = tab["cos"], tab["sin"]
        for i in range(self.depth):
            b = f"blocks.{i}."
            items = tab["items_full"] if i in self.full else tab["items_window"]
            self._rms(h, w[b + "ln1"], n)
            ops.gemm(n, w[b + "wqkv"], w[b + "bqkv"], qkv)
            rc = lib.rgn_vision_rope_bf16(_p(qkv), qkv.stride(0), _p(cos), _p(sin), N, H, self.hd, Dp, _stream())
            _lib.check(rc, "rgn_vision_rope_bf16")
            rc = lib.rgn_vision_attention_bf16(_p(qkv), _p(a), N, H, Dp, float(self.scale), _p(items), items.shape[0], _stream())
            _lib.check(rc, "rgn_vision_attention_bf16")
            ops.gemm(a, w[b + "wproj"], w[b + "bproj"], h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
            self._rms(h, w[b + "ln2"], n)
            ops.gemm(n, w[b + "wgu"], w[b + "bgu"], ff)
            _lib.check(lib.rgn_swiglu_bf16(_p(ff), ff.stride(0), _p(g), g.stride(0), N, Fp, _stream()), "rgn_swiglu_bf16")
            ops.gemm(g, w[b + "wdown"], w[b + "bdown"], h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
        last = torch.empty(N, d, dtype=torch.bfloat16, device=self.device)
        last.copy_(h)                                                             # a device-to-device copy, no kernel
        self._rms(h, w["merger.ln"], n)
        ops.gemm(n.view(M, self.unit * d), w["merger.w0"], w["merger.b0"], m1)
        _lib.check(lib.rgn_gelu_erf_bf16(_p(m1), _p(m1), m1.numel(), _stream()), "rgn_gelu_erf_bf16")
        pooled = torch.empty(M, self.out, dtype=torch.bfloat16, device=self.device)
        ops.gemm(m1, w["merger.w2"], w["merger.b2"], pooled, out_rows=tab["window_index"])
        res = TextEncoderOutput(last, pooled)
        return res if return_dict else res.to_tuple()
