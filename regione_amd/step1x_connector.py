"""Step1X-Edit's per-step `connector` on the HIP kernels (VERDICT.md unbuilt #2).

A hosted `Step1XEditPipeline` / `Step1XEditPipelineV1P2` calls `transformer.connector(x, t, mask)` once per CFG branch per computed step
(Step1XEdit/inplace.py:514-516, Step1XEditV1P2/inplace.py:602-609).  The [EXT] module (`Qwen2Connector` of the public Step1X-Edit
transformer: a two-block token refiner conditioned on the timestep) is restated here on the library's kernels, rounding where the eager
bf16 module rounds.  With m = mask[..., None]:

  once per edit (`prepare`, both branches)
      mean = masked_mean_rows(x, n_valid)                      `(x m).sum(1) / m.sum(1)`
      y    = gemv(masked_mean_rows(x, n_valid, 1 + scale_factor), global_proj_out)
      cemb = gemv(silu(gemv(mean, c_embedder.linear_1)), c_embedder.linear_2)
      x0   = x @ input_embedder^T + b                          rgn_gemm_group, both branches as two problems sharing W
      items                                                    the connector item table of rgn_vision_attention_bf16 (below)
      P0   = block 0's attention branch up to self_attn_proj   (none of it depends on t)
  per computed step (`step`)
      c     = gemv(silu(gemv(sinusoid(t), t_embedder.mlp.0)), t_embedder.mlp.2) + cemb          rgn_add_bf16
      gates = gemv(silu(c), adaLN_modulation.1) per block      gate_msa | gate_mlp
      x     = x0 + gate_msa P0                                 rgn_gate_resid_rows (block 0); later blocks: the branch below, fused
      x     = x + gate_mlp (silu(LN2(x) @ fc1^T + b) @ fc2^T + b)                               RGN_EPI_GATE_RESID
  the attention branch of a block
      qkv = LN1(x) @ qkv^T + b;  head_rms_norm(qkv);  a = vision_attention(qkv, items, Dp = 128);  a @ proj^T + b

The attention mask of the module is `A[i, j] = mask[i] & mask[j]`, then `A[:, 0] = True`: a valid query row sees the valid keys, a
padded one key 0 alone.  For a mask of n leading ones that is the item table (q0, n_q, 0, n) for runs of at most 64 valid rows and
(q0, n_q, 0, 1) for runs of padded rows (`connector_items`); a padded row's output is v[0] of its head, bit for bit.

Masks must be a run of ones followed by zeros with at least one 1 (`mask_prefix`; None = all valid): the caller keeps the host module
for anything else.  Every state-dict name of the layout is in `NAMES` below - a maintainer with the fork at hand corrects a name in one
place.  There is no eager fallback inside: what the kernels do not implement raises RegionEHipError before any launch
(`connector_refusal` names the reason for the adapter).  Buffers are kept for the last tuple of sequence lengths only.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib, ops
from .text_encoders import _Buffers, _refuse

_p, _stream = ops._p, ops._stream

EPS = 1e-6                       # LayerNorm and RMSNorm of the refiner blocks
HEAD_DIM = 128
ITEM_Q = 64                      # queries per attention item (ATTN_BQ of csrc/attn_tile.h)
FREQ_DIM = 256                   # TimestepEmbedder's sinusoid width

# ---- the one table of state-dict names ({i} = block index) ------------------------------------------------------------------------------------
BLOCK = "S.individual_token_refiner.blocks.{i}."
NAMES = dict(
    embed="S.input_embedder", t0="S.t_embedder.mlp.0", t2="S.t_embedder.mlp.2", c1="S.c_embedder.linear_1", c2="S.c_embedder.linear_2",
    pool="global_proj_out", scale="scale_factor",
    ln1=BLOCK + "norm1", ln2=BLOCK + "norm2", qkv=BLOCK + "self_attn_qkv", qn=BLOCK + "self_attn_q_norm", kn=BLOCK + "self_attn_k_norm",
    proj=BLOCK + "self_attn_proj", fc1=BLOCK + "mlp.fc1", fc2=BLOCK + "mlp.fc2", ada=BLOCK + "adaLN_modulation.1")


def connector_param_shapes(cfg) -> Dict[str, tuple]:
    """name -> shape of every parameter of the layout for `cfg` (in_channels, hidden_size, heads_num, depth, pooled_dim)."""
    i_, h, p = cfg.in_channels, cfg.hidden_size, cfg.pooled_dim
    hd = h // cfg.heads_num
    s = {}

    def lin(key, n, k, **fmt):
        s[NAMES[key].format(**fmt) + ".weight"], s[NAMES[key].format(**fmt) + ".bias"] = (n, k), (n,)
    lin("embed", h, i_), lin("t0", h, FREQ_DIM), lin("t2", h, h), lin("c1", h, i_), lin("c2", h, h), lin("pool", p, i_)
    s[NAMES["scale"]] = (1,)
    for i in range(cfg.depth):
        for k in ("ln1", "ln2"):
            s[NAMES[k].format(i=i) + ".weight"], s[NAMES[k].format(i=i) + ".bias"] = (h,), (h,)
        for k in ("qn", "kn"):
            s[NAMES[k].format(i=i) + ".weight"] = (hd,)
        lin("qkv", 3 * h, h, i=i), lin("proj", h, h, i=i), lin("fc1", 4 * h, h, i=i), lin("fc2", h, 4 * h, i=i), lin("ada", 2 * h, h, i=i)
    return s


def _state_dict(module_or_state_dict) -> Optional[Dict[str, torch.Tensor]]:
    if isinstance(module_or_state_dict, dict):
        return module_or_state_dict
    sd = getattr(module_or_state_dict, "state_dict", None)
    return sd() if callable(sd) else None


def _plain(name: str) -> str:
    """A state-dict name with PEFT's wrapper levels removed (`x.base_layer.weight` -> `x.weight`)."""
    return name.replace(".base_layer.", ".")


def is_connector_layout(module_or_state_dict) -> bool:
    """Whether this is the Qwen2Connector layout at all (by parameter names): its token refiner under `S.` and the pooled projection."""
    sd = _state_dict(module_or_state_dict)
    if not sd:
        return False
    names = {_plain(k) for k in sd}
    return NAMES["embed"] + ".weight" in names and NAMES["pool"] + ".weight" in names and NAMES["qkv"].format(i=0) + ".weight" in names


def connector_config(module_or_state_dict):
    """(in_channels, hidden_size, heads_num, depth, pooled_dim) read off the parameter shapes of the layout."""
    sd = {_plain(k): v for k, v in _state_dict(module_or_state_dict).items()}
    h, i_ = (int(v) for v in sd[NAMES["embed"] + ".weight"].shape)
    hd = int(sd[NAMES["qn"].format(i=0) + ".weight"].shape[0]) if NAMES["qn"].format(i=0) + ".weight" in sd else HEAD_DIM
    depth = 0
    while NAMES["qkv"].format(i=depth) + ".weight" in sd:
        depth += 1
    heads = getattr(module_or_state_dict, "heads_num", None) or (h // hd if hd and h % hd == 0 else 0)
    return SimpleNamespace(in_channels=i_, hidden_size=h, heads_num=int(heads), depth=depth, pooled_dim=int(sd[NAMES["pool"] + ".weight"].shape[0]),
                           head_dim=hd)


def connector_refusal(module_or_state_dict) -> Optional[str]:
    """Why a module (or state dict) of the Qwen2Connector layout is not one the kernels run (None: it is)."""
    sd = _state_dict(module_or_state_dict)
    if not is_connector_layout(sd):
        return "not the Qwen2Connector layout (S.input_embedder / S.individual_token_refiner.blocks / global_proj_out)"
    lora = [k for k in sd if "lora_" in k or ".base_layer." in k]
    mods = getattr(module_or_state_dict, "named_modules", None)
    if not lora and callable(mods):
        lora = [n for n, _ in mods() if "lora" in n.lower()]
    if lora:
        return f"PEFT / LoRA layers in the module ({lora[:3]})"
    cfg = connector_config(sd)
    if cfg.head_dim != HEAD_DIM or cfg.heads_num < 1 or cfg.heads_num * HEAD_DIM != cfg.hidden_size:
        return f"head dim {cfg.head_dim} with {cfg.heads_num} heads at hidden_size {cfg.hidden_size} (heads of {HEAD_DIM} are implemented)"
    bad = {k: v for k, v in (("in_channels", cfg.in_channels), ("hidden_size", cfg.hidden_size), ("pooled_dim", cfg.pooled_dim)) if v % 64}
    if bad:
        return f"widths {bad} are not multiples of 64"
    want = connector_param_shapes(cfg)
    unknown = [k for k in sd if k not in want]
    if unknown:
        return f"extra parameters the layout does not know: {unknown[:6]}"
    missing = [k for k in want if k not in sd]
    if missing:
        return f"parameters missing from the state dict: {missing[:6]}"
    for k, shape in want.items():
        if tuple(sd[k].shape) != shape:
            return f"{k} has shape {tuple(sd[k].shape)}, the layout needs {shape}"
    nb = [f"{k} ({v.dtype})" for k, v in sd.items() if v.dtype != torch.bfloat16]
    if nb:
        return f"non-bf16 weights: {nb[:3]} (the kernels take bf16 weights)"
    return None


# ---- host-side tables (no kernel) -----------------------------------------------------------------------------------------------------------
def connector_items(L: int, n_valid: int, base: int = 0) -> torch.Tensor:
    """int32 [n_items, 4] = (q0, n_q, k_lo, k_hi) of rgn_vision_attention_bf16 for one sequence of L rows whose first n_valid are valid,
    stored at rows [base, base + L): valid rows in runs of at most 64 queries against keys [base, base + n_valid), padded rows in runs
    against key `base` alone.  Every row lies in exactly one item."""
    if not 1 <= n_valid <= L:
        raise ValueError(f"connector_items: n_valid {n_valid} outside [1, {L}]")
    rows = [(base + q0, min(ITEM_Q, n_valid - q0), base, base + n_valid) for q0 in range(0, n_valid, ITEM_Q)]
    rows += [(base + q0, min(ITEM_Q, L - q0), base, base + 1) for q0 in range(n_valid, L, ITEM_Q)]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def mask_prefix(mask, L: int) -> Optional[int]:
    """n_valid of a mask that is a run of ones followed by zeros with at least one 1 (None = all valid -> L); None for anything else
    (holes, left padding, all zeros, other values, another length).  One device-to-host read of L elements."""
    if mask is None:
        return L
    if isinstance(mask, int):                                   # a length the caller has parsed already
        return mask if 1 <= mask <= L else None
    if not isinstance(mask, torch.Tensor) or mask.numel() != L:
        return None
    m = mask.detach().reshape(-1).to("cpu", torch.float32)
    if not bool(((m == 0) | (m == 1)).all()):
        return None
    n = int(m.sum().item())
    if n < 1 or not bool((m[:n] == 1).all()):
        return None
    return n


def _adopt(t: torch.Tensor, dev) -> torch.Tensor:
    """The host's tensor itself when it is already bf16, contiguous and on the device; a copy otherwise."""
    t = t.detach()
    if t.device == dev and t.dtype == torch.bfloat16 and t.is_contiguous():
        return t
    return t.to(dev, torch.bfloat16).contiguous()


class HipStep1XConnector:
    """`Qwen2Connector(x, t, mask)` on the HIP kernels, split into the part that does not depend on t (`prepare`, once per edit, every
    CFG branch at once) and the part that does (`step`, once per computed step).  Adopts the module or its state dict.

        c = HipStep1XConnector(pipe.transformer.connector, "cuda")
        c.prepare([cond_rows, uncond_rows], [cond_mask, uncond_mask])
        for t in computed_steps:
            (enc_c, y_c), (enc_u, y_u) = c.step(t)          # enc [1, L, hidden] (fresh), y [1, pooled]

    `hoist=False` recomputes the t-invariant part in every `step` and takes block 0's gated residual in the GEMM epilogue, the way a
    direct restatement of the module would: the two give the same bits (tests/test_gpu_step1x_connector.py)."""
    what = "HipStep1XConnector"

    def __init__(self, module_or_state_dict, device=None, hoist: bool = True):
        why = connector_refusal(module_or_state_dict)
        if why:
            _refuse(self.what, why)
        sd = _state_dict(module_or_state_dict)
        dev = torch.device(device) if device is not None else next(iter(sd.values())).device
        if dev.type != "cuda":
            _refuse(self.what, f"device {dev} (the kernels need a HIP device: there is no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.cfg = cfg = connector_config(sd)
        self.device, self.hoist = dev, bool(hoist)
        self.i, self.h, self.H, self.depth, self.pooled = cfg.in_channels, cfg.hidden_size, cfg.heads_num, cfg.depth, cfg.pooled_dim
        w = {k: _adopt(v, dev) for k, v in sd.items()}
        # what was adopted: the host's tensors (held, so that identity is a key) and their versions - `stale` compares a later state dict
        self._src = {k: (v, v._version) for k, v in sd.items()}
        self._ttm = None

        def lin(key, **fmt):
            n = NAMES[key].format(**fmt)
            return w[n + ".weight"], w[n + ".bias"]
        self.embed, self.t0, self.t2, self.c1, self.c2, self.pool = (lin(k) for k in ("embed", "t0", "t2", "c1", "c2", "pool"))
        self.blocks = []
        for i in range(self.depth):
            b = {k: lin(k, i=i) for k in ("ln1", "ln2", "qkv", "proj", "fc1", "fc2", "ada")}
            b["qn"], b["kn"] = (w[NAMES[k].format(i=i) + ".weight"] for k in ("qn", "kn"))
            self.blocks.append(b)
        # `mean * (1 + scale_factor)`: the bf16 sum the eager op computes, as the kernel's scalar
        self.y_scale = float((1 + sd[NAMES["scale"]].detach().to("cpu", torch.bfloat16))[0])
        self.scale = HEAD_DIM ** -0.5
        self.buf = _Buffers(dev)
        self._Ls = None

    @property
    def dtype(self):
        return torch.bfloat16

    def stale(self, module_or_state_dict) -> bool:
        """Whether the module no longer is what was adopted: other parameter names (a LoRA loaded since), another tensor, device or dtype
        behind a name (`.to()`, a weight swap), or an in-place update of one (the version counter).  Host arithmetic only."""
        sd = _state_dict(module_or_state_dict)
        if sd is None or set(sd) != set(self._src):
            return True
        return any(sd[k].data_ptr() != v.data_ptr() or sd[k]._version != ver or sd[k].dtype != v.dtype or sd[k].device != v.device
                   for k, (v, ver) in self._src.items())

    def adopt_ttm(self, ttm):
        """v1p2's `text_token_mapping` when it is one bf16 nn.Linear onto the hidden width: (weight [hidden, Kp], bias or None) on the
        device, K zero-padded to a GEMM reduction width (exact zeros in the fp32 sums); None for any other module.  Kept until the
        module's weight is replaced or updated."""
        if type(ttm) is not torch.nn.Linear or ttm.weight.dtype != torch.bfloat16 or ttm.weight.shape[0] != self.h or \
                (ttm.bias is not None and ttm.bias.dtype != torch.bfloat16):
            return None
        c = self._ttm
        if c is None or c[0] is not ttm.weight or c[1] != ttm.weight._version:
            K = ttm.weight.shape[1]
            wp = torch.zeros(self.h, ops.padded(K), dtype=torch.bfloat16)
            wp[:, :K] = ttm.weight.detach().cpu()
            c = self._ttm = (ttm.weight, ttm.weight._version, wp.to(self.device),
                             None if ttm.bias is None else ttm.bias.detach().to(self.device).contiguous())
        return c[2], c[3]

    # ---- kernels ------------------------------------------------------------------------------------------------------------------------
    def _ln(self, x, gb, out):
        rc = _lib.lib().rgn_layer_norm_rows(_p(x), x.stride(0), _p(gb[0]), _p(gb[1]), _p(out), out.stride(0), x.shape[0], self.h, EPS, _stream())
        _lib.check(rc, "rgn_layer_norm_rows")

    def _group(self, A, wb, out, gates=None, resid=None):
        """One launch for every branch: out[rows of b] = epilogue(A[rows of b] @ W^T + bias), the branches as problems sharing W."""
        probs = []
        for b, (o, L) in enumerate(zip(self._off, self._Ls)):
            g = None if gates is None else gates[b]
            probs.append(ops.Problem(A[o:o + L], wb[0], wb[1], out[o:o + L], g, None if resid is None else resid[o:o + L]))
        ops.gemm_group(probs, epilogue=ops.EPI_BIAS if gates is None else ops.EPI_GATE_RESID)

    def _attention_branch(self, blk, x, out, gates=None):
        """LN1 -> qkv -> per-head RMSNorm -> attention -> self_attn_proj of one block into `out`: the bare projection (gates None), or
        x + gate_msa * projection in the GEMM epilogue."""
        t = self._t
        self._ln(x, blk["ln1"], t["n"])
        self._group(t["n"], blk["qkv"], t["qkv"])
        ops.head_rms_norm_(t["qkv"], blk["qn"], blk["kn"], self.H, EPS)
        rc = _lib.lib().rgn_vision_attention_bf16(_p(t["qkv"]), _p(t["a"]), self._Ltot, self.H, HEAD_DIM, float(self.scale), _p(self._items),
                                                  self._items.shape[0], _stream())
        _lib.check(rc, "rgn_vision_attention_bf16")
        self._group(t["a"], blk["proj"], out, gates, None if gates is None else x)

    def _mlp(self, blk, x, out, gates):
        t = self._t
        self._ln(x, blk["ln2"], t["n"])
        self._group(t["n"], blk["fc1"], t["ff"])
        _lib.check(_lib.lib().rgn_silu_bf16(_p(t["ff"]), _p(t["g"]), t["ff"].numel(), _stream()), "rgn_silu_bf16")
        self._group(t["g"], blk["fc2"], out, gates, x)

    def _invariant(self):
        """Everything that does not depend on t: embedded tokens, pooled context, c_embedder's output, y; with `hoist`, block 0's projected
        attention branch."""
        t, B = self._t, len(self._Ls)
        mean, ymean = torch.empty(B, self.i, dtype=torch.bfloat16, device=self.device), torch.empty(B, self.i, dtype=torch.bfloat16, device=self.device)
        for b, (o, L, n) in enumerate(zip(self._off, self._Ls, self._n)):
            ops.masked_mean_rows(t["xin"][o:o + L], n, 1.0, out=mean[b])
            # `mean * (1 + scale_factor)`: the same kernel over the one row it just wrote (bf16(mean / 1) is mean), not over x again
            ops.masked_mean_rows(mean[b:b + 1], 1, self.y_scale, out=ymean[b])
        self._y = ops.gemv(ymean, *self.pool)
        self._cemb = ops.gemv(ops.gemv(mean, *self.c1), *self.c2, silu_input=True)
        self._group(t["xin"], self.embed, t["x0"])
        if self.hoist:
            self._attention_branch(self.blocks[0], t["x0"], t["p0"])

    # ---- once per edit ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self, enc_rows: Sequence[torch.Tensor], masks: Optional[Sequence] = None):
        """Bind the embeddings of every CFG branch ([L, in] or [1, L, in] each, bf16 or fp32) and their masks (None, a run of ones then
        zeros, or the valid length as an int when the caller has parsed the mask already) and compute what does not depend on the
        timestep."""
        rows = [e[0] if e.dim() == 3 and e.shape[0] == 1 else e for e in enc_rows]
        if not 1 <= len(rows) <= 4:
            _refuse(self.what, f"{len(rows)} branches (1 to 4 are covered)")
        masks = list(masks) if masks is not None else [None] * len(rows)
        if len(masks) != len(rows):
            _refuse(self.what, f"{len(masks)} masks for {len(rows)} branches")
        Ls, ns = [], []
        for e, m in zip(rows, masks):
            if not isinstance(e, torch.Tensor) or e.dim() != 2 or e.shape[1] != self.i or e.shape[0] < 1 or e.dtype not in (torch.bfloat16, torch.float32):
                _refuse(self.what, f"embeddings of shape {tuple(getattr(e, 'shape', ()))} / dtype {getattr(e, 'dtype', None)} ([L, {self.i}] rows, bf16 or fp32)")
            n = mask_prefix(m, e.shape[0])
            if n is None:
                _refuse(self.what, "a mask that is not a run of ones followed by zeros with at least one 1")
            Ls.append(int(e.shape[0]))
            ns.append(n)
        self._Ls, self._n = tuple(Ls), tuple(ns)
        self._off = tuple(sum(Ls[:b]) for b in range(len(Ls)))
        self._Ltot = Lt = sum(Ls)
        h = self.h
        self._t = t = self.buf.get(self._Ls, dict(xin=(Lt, self.i), x0=(Lt, h), p0=(Lt, h), x=(Lt, h), n=(Lt, h), qkv=(Lt, 3 * h), a=(Lt, h),
                                                  ff=(Lt, 4 * h), g=(Lt, 4 * h)))
        for e, o, L in zip(rows, self._off, Ls):
            e = e.detach()
            if e.dtype == torch.bfloat16:
                t["xin"][o:o + L].copy_(e if e.is_contiguous() else e.contiguous())       # one copy (host-to-device or device-to-device)
            else:
                e = e.to(self.device).contiguous()
                rc = _lib.lib().rgn_cast_pad_rows(_p(e), ops.F32, e.stride(0), _p(t["xin"][o:o + L]), L, self.i, self.i, _stream())
                _lib.check(rc, "rgn_cast_pad_rows")
        self._items = torch.cat([connector_items(L, n, o) for L, n, o in zip(Ls, ns, self._off)]).to(self.device)
        self._y = self._cemb = None
        if self.hoist:
            self._invariant()
        return self

    # ---- once per computed step ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, t) -> List[tuple]:
        """The connector's outputs at timestep(s) t (a number, or a tensor of one value or one per branch): [(enc [1, L, hidden], y [1,
        pooled])] per branch; enc is freshly allocated."""
        if self._Ls is None:
            _refuse(self.what, "step() before prepare()")
        from .harness.flux import timestep_embedding
        B = len(self._Ls)
        tt = torch.as_tensor(t).detach().to("cpu", torch.float32).reshape(-1)
        if tt.numel() == 1:
            tt = tt.expand(B)
        if tt.numel() != B:
            _refuse(self.what, f"{tt.numel()} timesteps for {B} branches")
        if not self.hoist:
            self._invariant()
        bufs, h = self._t, self.h
        emb = timestep_embedding(tt, FREQ_DIM).to(torch.bfloat16).to(self.device)          # the host sinusoid, as in the trunk
        c = ops.gemv(ops.gemv(emb, *self.t0), *self.t2, silu_input=True)
        ops.add_bf16(c, self._cemb, out=c)
        out = torch.empty(self._Ltot, h, dtype=torch.bfloat16, device=self.device)
        x = bufs["x0"]
        for i, blk in enumerate(self.blocks):
            gates = ops.gemv(c, *blk["ada"], silu_input=True)                              # [B, 2 h] = gate_msa | gate_mlp
            msa, mlp = [gates[b, :h] for b in range(B)], [gates[b, h:] for b in range(B)]
            if i == 0 and self.hoist:
                for b, (o, L) in enumerate(zip(self._off, self._Ls)):
                    ops.gate_resid_rows(bufs["p0"][o:o + L], msa[b], x[o:o + L], out=bufs["x"][o:o + L])
            else:
                self._attention_branch(blk, x, bufs["x"], msa)
            x = bufs["x"]
            self._mlp(blk, x, out if i == self.depth - 1 else x, mlp)
        self.out = out                                                                     # all branches' rows, [sum L, hidden]
        return [(out[o:o + L].unsqueeze(0), self._y[b:b + 1]) for b, (o, L) in enumerate(zip(self._off, self._Ls))]
