"""Step1X-Edit's connector, the text path that runs in front of the trunk once per computed step: the two objects the engine's `connector`
hook may be bound to (the host module per branch, or the adopted HIP connector) and the adoption itself."""
from __future__ import annotations

import torch

from .. import _lib, ops
from .components import _UNSET, _adopt_or_keep, _bf, _memo


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
    cached = _memo(host, "_regione_hip_connector")
    if cached is False or cached is None:
        return None
    conn = getattr(getattr(host, "transformer", None), "connector", None)
    if cached is not _UNSET and not cached.stale(conn):
        return cached
    from .. import step1x_connector as SC
    hip = None
    if SC.is_connector_layout(conn):
        hip = _adopt_or_keep("connector", SC.connector_refusal(conn), lambda: SC.HipStep1XConnector(conn, dev), stacklevel=3)
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
        from .. import step1x_connector as SC
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
        from .. import step1x_connector as SC
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

