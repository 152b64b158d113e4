"""The language model of the Qwen2.5-VL prompt encoder on the HIP kernels (`encode_prompt` of Qwen-Image-Edit).

`encode_prompt` of QwenImageEditPipeline / QwenImageEditPlusPipeline runs diffusers' `_get_qwen_prompt_embeds`: the [EXT] transformers
`Qwen2_5_VLForConditionalGeneration` over the prompt template, the condition images' tokens and the instruction, reading
`hidden_states[-1]`.  The decoder stack is restated here on the library's kernels, rounding where the eager bf16 module rounds:

  layer   n = rms_norm_rows(h)                       Qwen2_5_VLRMSNorm (fp32 variance, w * bf16(x * rsqrt))
          qkv = n @ [q; k; v]^T + [bq; bk; bv]       one rgn_gemm_group over the concatenated weight: [L, (Hq + 2 Hkv) 128]
          mrope(qkv, cos, sin)                       apply_multimodal_rotary_pos_emb on the q and k columns, in place
          a = lm_attention(qkv)                      causal, grouped-query (query head h reads KV head h / (Hq / Hkv)), scale 1/sqrt(128)
          h = h + a @ o^T                            RGN_EPI_GATE_RESID with a gate of ones = torch's bf16 `h + linear(a)`
          ff = n2 @ [gate; up]^T                     one GEMM, then swiglu: bf16(bf16(silu(gate)) * up)
          h = h + swiglu(ff) @ down^T                the gated residual again
  final   rms_norm_rows(h)                           `model.language_model.norm`

Positions are the adopted module's own: `module.model.compute_3d_position_ids(...)` with the caller's arguments (None -> the plain arange
of Qwen2_5_VLTextModel.forward); the cos / sin tables are built on the CPU with the module's `rotary_emb` arithmetic and `inv_freq`
buffer, the `mrope_section` selection applied once, cast to bf16 and copied in one host-to-device copy per call.  The vision tower is
`vision=`, a HipQwen25VLVisionTower (regione_amd/qwen_vision.py: the tower on the same kernels; the adapter passes one), or with
`vision=None` the host's eager module (`get_image_features`); its embeddings are placed at the image-token rows by rgn_scatter_rows.

`generate` is transformers' greedy search on the same weights (csrc/decode.hip), ONE decode loop for 1 <= B <= max_batch rows: the prefill
above, row by row, with the k | v columns of every layer appended to the row's KV cache [layers][B][cap, 2 Hkv 128] after mRoPE
(rgn_lm_kv_append_bf16) and the final norm on the last row only, then per new token the decode step of `_DecodeStep` (the step is
described there, once) at M = B rows; this loop's middle of a layer is rgn_mrope_bf16, rgn_lm_kv_append_bf16_rows and
rgn_lm_decode_attention_bf16_rows against the rows' caches, and the step's head writes the tokens into the device id row the next
rgn_text_embed reads.  New token k sits at max(prompt positions) + 1 + k on all three axes (`decode_position_ids`).  The loop is a `for`
over `max_new_tokens`; the host reads the ids every `sync_every` tokens to look for EOS.

`weights="fp8"` stores the four packed matrices of every layer (q|k|v, o, gate|up, down) as OCP e4m3fn with one fp32 scale per output
channel (ops.quantize_w8, after the concatenation: the scale is per row, so the concatenation of the parts' quantisations is the
quantisation of the concatenation), layer by layer on the device; norms, the q|k|v bias, the embedding and `lm_head` stay bf16.  The prefill
is unchanged (ops.gemm takes the scale from the weight tensor, rgn_gemm_group converts exactly and scales the accumulator); the decode loop
calls rgn_lm_gemv_w8_rows instead of rgn_lm_gemv_bf16_rows: half the bytes per token for those matrices.  Opt-in: the default is "bf16".

`sampling=True` (opt-in; the default refuses what it refused before) lets `generate` honour a decoding configuration: `do_sample`,
`temperature`, `top_k`, `top_p` and `repetition_penalty`, each taken from the module's generation_config when the argument is None, as
transformers does.  The pick is then rgn_lm_head_argmax_rows for the fp32 logits followed by ONE rgn_lm_pick_rows on the same stream (at
B = 1 the one block of rgn_lm_pick: penalty over a byte map of the ids so far, temperature, top-k, top-p, argmax or the inverse CDF at a
uniform read from a device buffer filled before the loop), which overwrites the id slot: still no token visits the host inside a step.
The uniforms come from `generator=` / `uniforms=`, not from torch.multinomial: a seed gives transformers' distribution, not transformers'
tokens.

`max_batch=N` (opt-in, 1 <= N <= 8; the default 1 refuses what it refused before) lets `generate` take `input_ids [B, L]` with B <= N
left-padded rows, as transformers' batched greedy search does: rows prefill one after another over their valid tokens into their own
caches, then every step decodes all B rows from ONE stream of the weights (the `_rows` kernels of csrc/decode.hip from B = 2 on).  The
batch is invariant: row b's tokens and fp32 logits are bit for bit those of the B = 1 call on row b's unpadded prompt.  A row is finished
after its first EOS and holds `pad_token_id` from then on (`assemble_sequences`); B = 1 under such an adoption keeps the one-row rules.
Sampling over a batch is refused (rgn_lm_pick is one sequence) unless the adoption also sets `batch_sampling=True`.

`batch_sampling=True` (opt-in; needs `sampling=True` and `max_batch > 1`; without it every refusal is what it was) lets a batch of B >= 2
rows take the decoding configuration of `sampling=True`, ONE configuration for the whole batch as in transformers: per step
rgn_lm_head_argmax_rows writes the fp32 [B, V] logits and ONE rgn_lm_pick_rows (one block per row, each on a CU of its own, row b bit for
bit rgn_lm_pick on row b) writes the B tokens into the id row the next rgn_text_embed reads.  `uniforms=` is then [max_new_tokens, B],
time-major like the new ids.  The byte map is [B, V], row b marked over that row's VALID prompt ids only: the left padding is not marked.
This is a deliberate difference from transformers, whose RepetitionPenaltyLogitsProcessor gathers at the pad positions too and so, for
Qwen (the pad id is also an EOS id), penalises an EOS in padded rows only; not marking it is what keeps the batch invariant: for given
`uniforms`, row b's tokens, fp32 logits and scores are bit for bit those of the B = 1 sampled call on row b's unpadded prompt with
`uniforms[:, b]`.  A configuration that is greedy as before runs the greedy launches unchanged.  Not measured: real checkpoints.

`batch_kernels="mfma"` (opt-in; the default "fma" is the object described above in every respect and refuses `max_batch` > 8 as before)
accepts `max_batch` in 1..32 and runs the weight-streaming layers of EVERY decode step, B = 1 included, on the MFMA row GEMM of
csrc/decode.hip (lm_gemm_rows_kernel): rgn_lm_gemm_rows_bf16 / rgn_lm_gemm_rows_w8 for the four projections and rgn_lm_head_argmax_wide for
`lm_head`.  A weight byte is loaded once per step for all rows, straight into the B operand of v_mfma_f32_16x16x32_bf16 (fp8 bytes are
widened exactly to bf16 in registers; the scale multiplies the folded sum once); the rows sit in LDS as bf16.  The per-row entries
rgn_lm_kv_append_bf16_rows and rgn_lm_decode_attention_bf16_rows are called in groups of at most 8 rows with offset pointers, and the pick
is ONE rgn_lm_pick_wide (the kernel of rgn_lm_pick_rows with up to 32 blocks); nothing crosses rows there, so every row keeps its bits.
The batch stays invariant over the whole range: row b's tokens, fp32 logits and processed scores are bit for bit those of the B = 1 call
of the SAME adoption on that prompt alone.  Against an "fma" adoption
the sums differ in their last bits (another summation order), so tokens agree wherever the top-2 logit gap is not within that error.
`weights="fp8"`, `sampling=True` and `batch_sampling=True` combine with it as before (`uniforms` [T, B], the byte map [B, V]); the prefill,
the KV layout, EOS / pad assembly and `sync_every` are untouched.  KV memory: 28 layers x cap x 2 x 4 x 128 bf16 = 235 MB per row at
cap = 4096, so 7.5 GB at 32 rows.  Not measured: real checkpoints.

`lookup=True` (opt-in; the default refuses `prompt_lookup_num_tokens` as before, word for word) lets a one-sequence greedy `generate`
take transformers' `prompt_lookup_num_tokens=K` and `max_matching_ngram_size` (default 2) and the extension `draft_tokens=` (a 1-D int64
guess of the whole continuation, new token 0 first; alone it takes the family's largest K).  The speculative loop (`_generate_lookup`;
the plain loop is untouched and runs when neither argument is given) keeps prompt and new ids in ONE device run and carries up to K
drafted tokens as extra rows of a step: the step of `_DecodeStep` at M = R = drafts + 1 (row b of its entries is bit for bit the one-row
call), with its own middle: rgn_mrope_bf16 over R consecutive table rows, ONE rgn_lm_kv_append_bf16 of R rows, and
rgn_lm_verify_attention_bf16 - R <= 8 queries against the one cache, query r over n + r rows, K and V of a 64-key slice loaded once for
all of them, row r bit for bit rgn_lm_decode_attention_bf16 at n + r (groups of 8 queries under "mfma").  rgn_lm_lookup_step, one block
after the head, accepts the
drafts that equal the argmax before them (the first mismatch ends the run), writes the token after them and drafts the next step's
rows: the rule of transformers' PromptLookupCandidateGenerator over the run so far (n-gram sizes from the largest down, the lowest
matching window with a non-empty continuation), or the caller's guess; never past max_new_tokens.  The host reads that kernel's small
result once per step (the accepted tokens: its look for EOS).  Every kept token and its fp32 logits row are bit for bit what the plain
loop of the SAME adoption gives; rejected cache rows and logits rows are overwritten by later steps.  K <= 7 under "fma", <= 31 under
"mfma"; B > 1, sampling, a penalty and output_scores are refused by name.  `last_lookup_stats` = steps, drafted, accepted, tokens.
Not measured: the acceptance rate on a real checkpoint (a seeded model's rate means nothing).

`lookup_sampling=True` (opt-in; needs `lookup=True` and `sampling=True`; without it the refusal above stays word for word) lets that
loop run under the decoding configuration of `sampling=True`: do_sample, temperature, top_k, top_p, repetition_penalty, `uniforms=` /
`generator=` and `output_scores`.  The rule is the one transformers' `_assisted_decoding` applies to a candidate generator without
logits: the processors run on row i over the ids up to and including the drafts before it, a token is picked per row, drafts are kept
up to the first mismatch.  Here a step's head always writes its R fp32 rows; rgn_lm_pick_verify, ONE launch of one block per row, picks
row r under the byte map seen U drafts[0, r) (the map the plain loop has there exactly when those drafts were accepted) with
uniforms[k + r] - the uniforms are indexed by new-token position, so the result does not depend on K, on the drafts or on how many
were accepted - and never writes the map; rgn_lm_lookup_step_mark accepts against the picks and marks the tokens the step settles.
Every kept token, its fp32 logits row and its processed scores row are BIT FOR BIT those of the plain sampled `generate` of the same
adoption with the same `uniforms` - not merely the same distribution.  Under the switch `prompt_lookup_num_tokens` and
`max_matching_ngram_size` left at None take the adopted module's generation_config values (what transformers does), so a caller that
passes no decoding argument drafts as that config says.  A configuration that is greedy as before takes the greedy lookup path launch
for launch.  Still refused by name: B > 1, K outside the family's range, assistant_model, everything `_pick_plan` refuses.
Not measured: the acceptance rate on a real checkpoint, and therefore any speed-up of a real thinking run; at 0 % acceptance the path
is slower than the plain loop by construction.

There is no eager fallback inside: what the kernels do not implement raises RegionEHipError before any launch, and the adapter
(regione_amd.adapters, components.py) keeps the host module for configs `qwen25vl_refusal` names.  Activation buffers are kept for the last length
only; every call returns freshly allocated outputs.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Dict, Optional

import torch

from . import _lib, ops
from .text_encoders import _Buffers, _HipTextEncoder, _bf16_only, _check_k, _check_names, _refuse, _source

_p, _stream = ops._p, ops._stream

HEAD_DIM = 128
LM = "model.language_model."
NOT_ADOPTED = ("lm_head.", "model.visual.")                  # lm_head.weight: adopted by the first generate()
WEIGHT_FORMATS = ("bf16", "fp8")                             # of the layers' projection matrices (`weights=`)


class QwenTextEncoderOutput:
    """What diffusers reads of the Qwen2.5-VL output: `.hidden_states[-1]` (and `.last_hidden_state`, the same tensor: the final hidden
    state AFTER the final norm, which is what transformers returns as the last entry).  The EARLIER entries of `hidden_states` (the
    embeddings and the per-layer states) are ABSENT: the tuple has that one element."""

    def __init__(self, last_hidden_state: torch.Tensor, with_hidden_states: bool):
        self.last_hidden_state = last_hidden_state
        self.hidden_states = (last_hidden_state,) if with_hidden_states else None

    def to_tuple(self):
        return tuple(t for t in (self.last_hidden_state, self.hidden_states) if t is not None)

    def __getitem__(self, i):
        if isinstance(i, str):
            return getattr(self, i)
        return self.to_tuple()[i]


def _text_config(cfg):
    return getattr(cfg, "text_config", None) or cfg


def qwen25vl_refusal(cfg) -> Optional[str]:
    """Why a Qwen2.5-VL config (the composite one or its text_config) is not one the kernels implement (None: it is)."""
    tc = _text_config(cfg)
    if getattr(tc, "model_type", None) not in ("qwen2_5_vl", "qwen2_5_vl_text"):
        return f"model_type {getattr(tc, 'model_type', None)!r} (the Qwen2.5-VL language model is covered)"
    d, hq, hkv = tc.hidden_size, tc.num_attention_heads, tc.num_key_value_heads
    if d % hq or d // hq != HEAD_DIM:
        return f"head dim {d / hq:g} (the attention kernel is head-dim {HEAD_DIM})"
    if hkv < 1 or hq % hkv:
        return f"{hq} query heads over {hkv} KV heads (Hq % Hkv != 0)"
    rope = getattr(tc, "rope_parameters", None) or {}
    if rope.get("rope_type", "default") != "default":
        return f"rope_type {rope.get('rope_type')!r} (the default RoPE is implemented)"
    sec = list(rope.get("mrope_section") or [])
    if len(sec) != 3 or 2 * sum(sec) != HEAD_DIM:
        return f"mrope_section {sec} (three sections summing to {HEAD_DIM // 2})"
    if "sliding_attention" in (getattr(tc, "layer_types", None) or []):
        return "sliding-window layers (full causal attention is implemented)"
    if getattr(tc, "hidden_act", None) != "silu":
        return f"hidden_act {getattr(tc, 'hidden_act', None)!r} (silu is implemented)"
    bad = {k: v for k, v in dict(hidden_size=d, intermediate_size=tc.intermediate_size).items() if v % 64}
    if bad:
        return f"widths {bad} are not multiples of 64"
    return None


def qwen25vl_param_shapes(cfg) -> Dict[str, tuple]:
    tc = _text_config(cfg)
    d, F, hq, hkv = tc.hidden_size, tc.intermediate_size, tc.num_attention_heads, tc.num_key_value_heads
    s = {LM + "embed_tokens.weight": (tc.vocab_size, d), LM + "norm.weight": (d,)}
    for i in range(tc.num_hidden_layers):
        b = f"{LM}layers.{i}."
        for n, rows in (("q", hq * HEAD_DIM), ("k", hkv * HEAD_DIM), ("v", hkv * HEAD_DIM)):
            s[f"{b}self_attn.{n}_proj.weight"], s[f"{b}self_attn.{n}_proj.bias"] = (rows, d), (rows,)
        s[f"{b}self_attn.o_proj.weight"] = (d, hq * HEAD_DIM)
        s[f"{b}mlp.gate_proj.weight"], s[f"{b}mlp.up_proj.weight"], s[f"{b}mlp.down_proj.weight"] = (F, d), (F, d), (d, F)
        s[f"{b}input_layernorm.weight"], s[f"{b}post_attention_layernorm.weight"] = (d,), (d,)
    return s


def default_inv_freq(cfg) -> torch.Tensor:
    """Qwen2_5_VLRotaryEmbedding.compute_default_rope_parameters on the CPU (used when no module is at hand)."""
    base = _text_config(cfg).rope_parameters["rope_theta"]
    return 1.0 / (base ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.float) / HEAD_DIM))


def mrope_tables(inv_freq: torch.Tensor, position_ids: torch.Tensor, mrope_section) -> torch.Tensor:
    """[2, B, L, 128] bf16 on the CPU: (cos, sin) of Qwen2_5_VLRotaryEmbedding.forward for `position_ids` [3, B, L] in fp32, then the
    `mrope_section` selection of apply_multimodal_rotary_pos_emb (chunk i of the channel axis from position axis i % 3), then the cast."""
    inv = inv_freq.detach().float().cpu()
    pos = position_ids.detach().cpu()
    inv_e = inv[None, None, :, None].expand(3, pos.shape[1], -1, 1)
    pos_e = pos[:, :, None, :].float()
    freqs = (inv_e @ pos_e).transpose(2, 3)
    emb = torch.cat((freqs, freqs), dim=-1)
    sec = list(mrope_section) * 2
    pick = lambda t: torch.cat([m[i % 3] for i, m in enumerate(t.split(sec, dim=-1))], dim=-1)
    return torch.stack([pick(emb.cos()), pick(emb.sin())]).to(torch.bfloat16).contiguous()


def decode_position_ids(prompt_position_ids: torch.Tensor, n_new: int) -> torch.Tensor:
    """[3, B, n_new] int64 on the CPU: the positions transformers gives the tokens `generate` appends.  Qwen2_5_VLModel keeps
    `rope_deltas = max(prompt position_ids over the three axes) + 1 - L` from the prefill and uses `cache_position + rope_deltas` on every
    axis afterwards: new token k sits at max + 1 + k."""
    pos = prompt_position_ids.detach().cpu()
    top = pos.amax(dim=(0, 2))                                                   # [B]
    new = top[:, None] + 1 + torch.arange(int(n_new), dtype=pos.dtype)[None, :]
    return new[None].expand(3, -1, -1).contiguous()


class QwenGenerateOutput:
    """`generate(..., return_dict_in_generate=True)`: `.sequences` [1, L + n_new] int64 and, with `output_logits=True`, `.logits`, a tuple
    of n_new fp32 [1, V] tensors (the raw lm_head outputs the tokens were picked from); None otherwise.  Under `sampling=True`,
    `output_scores=True` adds `.scores`, the same shape: the processed scores of rgn_lm_pick (-inf where top-k / top-p filtered).  Over a
    batch of B rows every one of these has B rows."""

    def __init__(self, sequences, logits=None, scores=None):
        self.sequences, self.logits, self.scores = sequences, logits, scores

    def __getitem__(self, k):
        return getattr(self, k)


# arguments of transformers' generate that change WHICH token is picked: refused by name (greedy search is what the kernels implement)
SAMPLING_ARGS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "repetition_penalty",
                 "encoder_repetition_penalty", "no_repeat_ngram_size", "length_penalty", "diversity_penalty", "penalty_alpha",
                 "num_beam_groups", "num_return_sequences", "bad_words_ids", "force_words_ids", "suppress_tokens", "begin_suppress_tokens",
                 "sequence_bias", "logits_processor", "stopping_criteria", "min_new_tokens", "min_length", "guidance_scale",
                 "exponential_decay_length_penalty", "renormalize_logits", "constraints", "prefix_allowed_tokens_fn", "assistant_model")

# what a `sampling=True` adoption implements of them (rgn_lm_pick), and what its generate takes besides
PICK_ARGS = ("temperature", "top_k", "top_p", "repetition_penalty")
PICK_EXTRA = ("generator", "uniforms", "output_scores")
# the generation_config fields such an adoption still refuses, with the value (besides None) that switches each off
CONFIG_OFF = dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, encoder_repetition_penalty=1.0, no_repeat_ngram_size=0,
                  length_penalty=1.0, diversity_penalty=0.0, penalty_alpha=None, num_beam_groups=1, num_return_sequences=1,
                  bad_words_ids=None, force_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, sequence_bias=None,
                  min_new_tokens=0, min_length=0, guidance_scale=1.0, exponential_decay_length_penalty=None, renormalize_logits=False,
                  constraints=None)


# what a `lookup=True` adoption's generate takes besides: transformers' two prompt-lookup arguments and a caller's guess of the continuation
LOOKUP_ARGS = ("prompt_lookup_num_tokens", "max_matching_ngram_size", "draft_tokens")
MAX_NGRAM = 8                                                                    # rgn_lm_lookup_step: 1 <= max_ngram <= 8


def lookup_plan(what, look, wide):
    """(K, max_ngram, guess) of one speculative generate from its LOOKUP_ARGS, every refusal by name: K drafts at most per step (1..7 on
    the "fma" row kernels, 1..31 on "mfma": a step carries K + 1 rows), the largest n-gram tried (transformers' default 2), and the
    guess (a 1-D int64 tensor) or None.  `draft_tokens` alone takes the family's largest K."""
    top = (MAX_WIDE_BATCH if wide else MAX_BATCH) - 1
    K, ngram, guess = look.get("prompt_lookup_num_tokens"), look.get("max_matching_ngram_size"), look.get("draft_tokens")
    if K is None and guess is None:
        _refuse(what, "max_matching_ngram_size without prompt_lookup_num_tokens (it sizes the n-grams of the prompt lookup)")
    if K is None:
        K = top
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= top:
        _refuse(what, f"prompt_lookup_num_tokens={K!r} (an int in [1, {top}] under batch_kernels=\"{'mfma' if wide else 'fma'}\": a step "
                      f"verifies K drafts as K + 1 rows)")
    if ngram is None:
        ngram = 2
    if isinstance(ngram, bool) or not isinstance(ngram, int) or not 1 <= ngram <= MAX_NGRAM:
        _refuse(what, f"max_matching_ngram_size={ngram!r} (an int in [1, {MAX_NGRAM}])")
    if guess is not None:
        if not isinstance(guess, torch.Tensor) or guess.dtype != torch.int64 or guess.dim() != 1 or guess.numel() < 1:
            _refuse(what, "draft_tokens must be a 1-D int64 tensor with at least one id (a guess of the continuation, new token 0 first)")
    return K, ngram, guess


class PickPlan:
    """The resolved decoding configuration of one generate under `sampling=True` (the arguments of rgn_lm_pick)."""

    def __init__(self, sample, penalty, temperature, top_k, top_p, uniforms, generator, output_scores):
        self.sample, self.penalty, self.temperature, self.top_k, self.top_p = sample, penalty, temperature, top_k, top_p
        self.uniforms, self.generator, self.output_scores = uniforms, generator, output_scores

    @property
    def greedy_as_before(self):                                                  # nothing rgn_lm_head_argmax does not already do
        return not self.sample and self.penalty == 1.0 and not self.output_scores


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def valid_lengths(attention_mask: Optional[torch.Tensor], B: int, L: int, what: str = "HipQwen25VLTextEncoder"):
    """Valid length per row of a [B, L] mask that is a run of ones followed by zeros (right padding); anything else is refused."""
    if attention_mask is None:
        return [L] * B
    m = attention_mask.detach().cpu()
    if tuple(m.shape) != (B, L):
        _refuse(what, f"attention_mask of shape {tuple(m.shape)} for input_ids [{B}, {L}]")
    m = m != 0
    n = m.sum(dim=1)
    want = torch.arange(L)[None, :] < n[:, None]
    if not torch.equal(m, want):
        _refuse(what, "attention_mask is not a run of ones followed by zeros (left padding and holes are not implemented: rows are "
                      "processed over their valid prefix)")
    if int(n.min()) < 1:
        _refuse(what, "attention_mask with an empty row")
    return [int(v) for v in n]


def image_rows(input_ids: torch.Tensor, lengths, image_token_id: int, n_embeds: int, what: str = "HipQwen25VLTextEncoder"):
    """Per batch row, the positions of `image_token_id` (CPU); the placeholder count over the batch must equal the embedding rows, as
    transformers' get_placeholder_mask requires."""
    ids = input_ids.detach().cpu()
    hit = ids == image_token_id
    total = int(hit.sum())
    if total != n_embeds:
        raise ValueError(f"Image features and image tokens do not match, tokens: {total}, features: {n_embeds}")
    rows = []
    for b, n in enumerate(lengths):
        if bool(hit[b, n:].any()):
            _refuse(what, "image tokens in the padded part of a row")
        rows.append(torch.nonzero(hit[b, :n]).flatten())
    return rows


# ---- generate over a batch (`max_batch=`): the host rules of transformers' greedy search for several rows -----------------------------
MAX_BATCH = 8                                                                    # RGN_LM_MAX_BATCH of include/regione_hip.h
MAX_WIDE_BATCH = 32                                                              # RGN_LM_MAX_WIDE_BATCH: the rows of batch_kernels="mfma"
BATCH_KERNELS = ("fma", "mfma")                                                  # what multiplies the rows of a decode step (`batch_kernels=`)


def left_valid_lengths(attention_mask: Optional[torch.Tensor], B: int, L: int, what: str = "HipQwen25VLTextEncoder"):
    """Valid length per row of a [B, L] mask that is a run of zeros followed by a run of ones (left padding, the decoder-only convention
    of a batched generate), or all ones; right padding, holes and an empty row are refused by name."""
    if attention_mask is None:
        return [L] * B
    m = attention_mask.detach().cpu() if isinstance(attention_mask, torch.Tensor) else None
    if m is None or tuple(m.shape) != (B, L):
        _refuse(what, f"attention_mask of shape {tuple(getattr(attention_mask, 'shape', ()))} for input_ids [{B}, {L}]")
    m = m != 0
    n = m.sum(dim=1)
    if int(n.min()) < 1:
        _refuse(what, "attention_mask with an empty row")
    if not torch.equal(m, torch.arange(L)[None, :] >= (L - n)[:, None]):
        if torch.equal(m, torch.arange(L)[None, :] < n[:, None]):
            _refuse(what, "attention_mask with right padding: a batched generate takes left padding (zeros, then ones), as transformers' "
                          "decoder-only generate does")
        _refuse(what, "attention_mask with holes: every row must be a run of zeros followed by a run of ones (left padding)")
    return [int(v) for v in n]


def image_rows_left(input_ids: torch.Tensor, lengths, image_token_id: int, n_embeds: int, what: str = "HipQwen25VLTextEncoder"):
    """`image_rows` for left-padded rows: per batch row, the positions of `image_token_id` counted from the row's FIRST VALID token (the
    row the prefill sees).  Embedding rows are assigned in row order, as transformers' masked scatter does; the placeholder count over
    the batch must equal the embedding rows."""
    ids = input_ids.detach().cpu()
    L = ids.shape[1]
    hit = ids == image_token_id
    total = int(hit.sum())
    if total != n_embeds:
        raise ValueError(f"Image features and image tokens do not match, tokens: {total}, features: {n_embeds}")
    rows = []
    for b, n in enumerate(lengths):
        if bool(hit[b, :L - n].any()):
            _refuse(what, "image tokens in the padded part of a row")
        rows.append(torch.nonzero(hit[b, L - n:]).flatten())
    return rows


def resolve_pad_token_id(pad_token_id, generation_config, eos):
    """The id that fills a finished row: the argument, else generation_config.pad_token_id, else the first EOS id (transformers'
    fallback, taken without its warning); None with no EOS at all - then no row ever finishes and nothing is padded."""
    if pad_token_id is None:
        pad_token_id = getattr(generation_config, "pad_token_id", None)
    if isinstance(pad_token_id, torch.Tensor):
        pad_token_id = int(pad_token_id.flatten()[0])
    if pad_token_id is None and eos:
        pad_token_id = eos[0]
    return None if pad_token_id is None else int(pad_token_id)


def eos_cuts(new_ids: torch.Tensor, eos):
    """Per row of time-major new ids [k, B] (CPU): the number of new tokens up to and including the row's first EOS, None without one."""
    k, B = new_ids.shape
    hit = torch.zeros(k, B, dtype=torch.bool)
    for e in eos:
        hit |= new_ids == e
    return [int(torch.nonzero(hit[:, b])[0]) + 1 if bool(hit[:, b].any()) else None for b in range(B)]


def assemble_sequences(prompt_ids: torch.Tensor, new_ids: torch.Tensor, eos, pad_token_id):
    """transformers' batched greedy search over ids the device has already decoded: `prompt_ids` [B, L] and time-major `new_ids` [k, B]
    (CPU).  A row is finished after its first EOS and holds `pad_token_id` from then on; the search stops after the step at which the
    last row finishes.  Returns (sequences [B, L + n_new], n_new): n_new is the largest cut over the rows, or k if some row never
    finished.  What the device decoded for a finished row is overwritten here."""
    k, B = new_ids.shape
    cuts = eos_cuts(new_ids, eos) if eos else [None] * B
    n_new = max(cuts) if all(c is not None for c in cuts) else k
    new = new_ids[:n_new].t().clone()
    for b, c in enumerate(cuts):
        if c is not None and c < n_new:
            new[b, c:] = pad_token_id
    return torch.cat([prompt_ids.to(torch.int64), new.to(torch.int64)], dim=1), n_new


def _bound(fn, name, *args):
    """(`fn` with `args` bound, `name`): the arguments are converted to their ctypes objects once, a host array to a pointer to its
    memory (what is written into the array later is what the call reads), so that calling the result marshals nothing."""
    conv = [a if isinstance(a, ctypes._Pointer) else ctypes.cast(a, t) if isinstance(a, ctypes.Array) else t(a)
            for t, a in zip(fn.argtypes, args, strict=True)]
    return functools.partial(fn, *conv), name


def _row_buffers(enc, M):
    """The shapes of the activation buffers of M rows through the stack."""
    return dict(h=(M, enc.d), n=(M, enc.d), qkv=(M, enc.qkv_cols), a=(M, enc.Hq * HEAD_DIM), ff=(M, 2 * enc.F), g=(M, enc.F))


class _DecodeStep:
    """The decode step of one generate, chosen once: M rows through the stack against KV caches (csrc/decode.hip).  The plain loop runs
    it at M = B, the lookup loop at M = R = drafts + 1; row m of every entry below is bit for bit the one-row call, and at M = 1 a `_rows`
    entry launches the one-row kernels (it is the one-row entry), so one sequence decodes on the GEMVs tuned for it.

      rgn_text_embed                     the M ids picked last, read from the device id run
      layer   rgn_rms_norm_rows          at M rows
              linear(q|k|v) + bias       `linear` is rgn_lm_gemv_bf16_rows, rgn_lm_gemv_w8_rows under weights="fp8" (half the bytes per token
                                         for those matrices), or under batch_kernels="mfma" rgn_lm_gemm_rows_bf16 / rgn_lm_gemm_rows_w8
              the loop's middle          mRoPE, the append of the k | v columns to the cache(s), attention against them: the loop's own
              linear(o)                  with the two roundings of `h + linear(a)` for the residual add
              rgn_rms_norm_rows, linear(gate|up), rgn_swiglu_bf16, linear(down) with the residual add
      final   rgn_rms_norm_rows          over the M rows
      head    rgn_lm_head_argmax_rows over `lm_head` (fp32 logits, the lowest index on a tie), rgn_lm_head_argmax_wide under "mfma"

    Every launch of a layer outside the middle, and the final norm, takes the same arguments at every step: `launches` converts them once
    (`_bound`), so that a step only calls ready objects.  The embedding, the middle and the head's call (its token and logits rows move)
    stay with the loop; the head's entry and workspace size are chosen here."""

    def __init__(self, enc, lib):
        self.enc, self.lib, self.wide, self.fp8 = enc, lib, enc.batch_kernels == "mfma", enc.weights == "fp8"
        # the linear layer of this adoption: a weight is the leading argument(s) of its entry, (W,) or (W8, scale): `wp`
        if self.fp8:
            self.linear, self.linear_name = (lib.rgn_lm_gemm_rows_w8, "rgn_lm_gemm_rows_w8") if self.wide else \
                (lib.rgn_lm_gemv_w8_rows, "rgn_lm_gemv_w8_rows")
        else:
            self.linear, self.linear_name = (lib.rgn_lm_gemm_rows_bf16, "rgn_lm_gemm_rows_bf16") if self.wide else \
                (lib.rgn_lm_gemv_bf16_rows, "rgn_lm_gemv_bf16_rows")
        self.head, self.head_name = (lib.rgn_lm_head_argmax_wide, "rgn_lm_head_argmax_wide") if self.wide else \
            (lib.rgn_lm_head_argmax_rows, "rgn_lm_head_argmax_rows")

    def wp(self, w):
        return (w.data_ptr(), ops._wscale(w).data_ptr()) if self.fp8 else (w.data_ptr(),)

    def head_workspace_bytes(self, M):
        V = self.enc.tok.shape[0]
        return self.lib.rgn_lm_head_wide_workspace_bytes(V, M) if self.wide else M * self.lib.rgn_lm_head_workspace_bytes(V)

    def launches(self, c, M, st):
        """([(before, after) per layer], final norm) for M rows in the buffers `c`: the bound launches before a layer's middle (rms,
        q|k|v), those after it (o, rms, gate|up, swiglu, down) and the final norm, each a (ready call, entry name)."""
        e, lin, name, wp = self.enc, self.linear, self.linear_name, self.wp
        d, F, eps, qc, ad = e.d, e.F, e.eps, e.qkv_cols, e.Hq * HEAD_DIM
        ph, pn, pqkv, pa, pff, pg = (c[k].data_ptr() for k in ("h", "n", "qkv", "a", "ff", "g"))
        rms, swiglu = self.lib.rgn_rms_norm_rows, self.lib.rgn_swiglu_bf16
        lp = [([_bound(rms, "rgn_rms_norm_rows", ph, d, p["ln1"].data_ptr(), pn, d, M, d, eps, st),
                _bound(lin, name, *wp(p["wqkv"]), pn, d, p["bqkv"].data_ptr(), None, 0, pqkv, qc, M, qc, d, st)],
               [_bound(lin, name, *wp(p["wo"]), pa, ad, None, ph, d, ph, d, M, d, ad, st),
                _bound(rms, "rgn_rms_norm_rows", ph, d, p["ln2"].data_ptr(), pn, d, M, d, eps, st),
                _bound(lin, name, *wp(p["wgu"]), pn, d, None, None, 0, pff, 2 * F, M, 2 * F, d, st),
                _bound(swiglu, "rgn_swiglu_bf16", pff, 2 * F, pg, F, M, F, st),
                _bound(lin, name, *wp(p["wdown"]), pg, F, None, ph, d, ph, d, M, d, F, st)]) for p in e.layers]
        return lp, _bound(rms, "rgn_rms_norm_rows", ph, d, e.final_ln.data_ptr(), pn, d, M, d, eps, st)


class _PickState:
    """The device state of a sampled pick (a PickPlan that is not greedy as before) over the B rows of `ids` [B, L], for steps that write
    at most M logits rows (the plain loop: M = B; the lookup loop: B = 1, M = K + 1): the byte map `seen` [B, V], zeroed once and marked
    over each row's VALID prompt ids only (the left padding is never marked); `zrows` [M, V], where the head writes when the caller keeps
    no logits; the pick workspace of M rows; `scores` [T, B, V] under output_scores; and the uniforms, `plan.uniforms` or torch.rand(T, B)
    from the generator (on its device, then moved), filled before the loop: the kernels have no generator and index it by position."""

    def __init__(self, lib, plan, ids, lens, T, M, V, keep_logits, st):
        (B, L), dev, ck = ids.shape, ids.device, _lib.check
        self.ws_1 = lib.rgn_lm_pick_workspace_bytes(V)
        self.ws_bytes = M * self.ws_1
        self.seen = torch.empty(B, V, dtype=torch.uint8, device=dev)
        self.zrows = None if keep_logits else torch.empty(M, V, dtype=torch.float32, device=dev)
        self.ws = torch.empty((self.ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
        self.scores = torch.empty(T, B, V, dtype=torch.float32, device=dev) if plan.output_scores else None
        uni = plan.uniforms
        if plan.sample and uni is None:
            g = plan.generator
            uni = torch.rand(T, B, dtype=torch.float32, generator=g, device=dev if g is None else g.device).to(dev)
        ck(lib.rgn_fill_zero(_p(self.seen), B * V, st), "rgn_fill_zero")
        for b, n in enumerate(lens):
            ck(lib.rgn_lm_seen_mark(ids.data_ptr() + 8 * (b * L + L - n), n, _p(self.seen[b]), V, st), "rgn_lm_seen_mark")
        self.uniforms = uni                                                      # kept: the loop reads it through `pu`
        self.pu = uni.data_ptr() if plan.sample else None
        self.how = (plan.penalty, int(plan.sample), plan.temperature, plan.top_k, plan.top_p)


def _generate_result(seq, n_new, logits, scores, as_dict):
    """What a generate returns: `seq`, or under return_dict_in_generate a QwenGenerateOutput with the first n_new of the [T, B, V]
    `logits` / `scores` rows (None: not asked for)."""
    if not as_dict:
        return seq
    return QwenGenerateOutput(seq, tuple(logits[k] for k in range(n_new)) if logits is not None else None,
                              tuple(scores[k] for k in range(n_new)) if scores is not None else None)


class HipQwen25VLTextEncoder(_HipTextEncoder):
    """`Qwen2_5_VLForConditionalGeneration(input_ids, attention_mask, pixel_values, image_grid_thw, output_hidden_states=True)` with the
    language model on the HIP kernels.  Returns an object with `.last_hidden_state` [B, L, d] bf16 and `.hidden_states`, a ONE-element
    tuple whose `[-1]` is that final hidden state after the final norm - the earlier entries transformers returns (embeddings, per-layer
    states) are absent.  Padded positions are zero rows."""
    what = "HipQwen25VLTextEncoder"

    def __init__(self, module_or_state_dict, device=None, config=None, max_length: int = 4096, vision=None, weights: str = "bf16",
                 sampling: bool = False, max_batch: int = 1, batch_sampling: bool = False, batch_kernels: str = "fma", lookup: bool = False,
                 lookup_sampling: bool = False):
        if weights not in WEIGHT_FORMATS:
            _refuse(self.what, f"weights={weights!r} (the layer matrices are kept as one of {WEIGHT_FORMATS})")
        if not isinstance(sampling, bool):
            _refuse(self.what, f"sampling={sampling!r} (True or False)")
        if not isinstance(batch_kernels, str) or batch_kernels not in BATCH_KERNELS:
            _refuse(self.what, f"batch_kernels={batch_kernels!r} (one of {BATCH_KERNELS}: the vector-ALU row kernels, or the MFMA row GEMM)")
        if not isinstance(lookup, bool):
            _refuse(self.what, f"lookup={lookup!r} (True or False)")
        wide = batch_kernels == "mfma"
        if isinstance(max_batch, bool) or not isinstance(max_batch, int) or not 1 <= max_batch <= (MAX_WIDE_BATCH if wide else MAX_BATCH):
            if wide:
                _refuse(self.what, f"max_batch={max_batch!r} under batch_kernels=\"mfma\" (an int in [1, {MAX_WIDE_BATCH}]: the rows one "
                                   "generate decodes from one weight stream on the MFMA row GEMM)")
            _refuse(self.what, f"max_batch={max_batch!r} (an int in [1, {MAX_BATCH}]: the rows one generate decodes from one weight stream)")
        if not isinstance(batch_sampling, bool):
            _refuse(self.what, f"batch_sampling={batch_sampling!r} (True or False)")
        if batch_sampling and not sampling:
            _refuse(self.what, "batch_sampling=True without sampling=True (it is the decoding configuration of sampling=True over a batch)")
        if batch_sampling and max_batch == 1:
            _refuse(self.what, "batch_sampling=True with max_batch=1 (it needs max_batch > 1: one row takes the one-sequence pick)")
        if not isinstance(lookup_sampling, bool):
            _refuse(self.what, f"lookup_sampling={lookup_sampling!r} (True or False)")
        if lookup_sampling and not lookup:
            _refuse(self.what, "lookup_sampling=True without lookup=True (it is the speculative loop of lookup=True under a sampled pick)")
        if lookup_sampling and not sampling:
            _refuse(self.what, "lookup_sampling=True without sampling=True (it is the decoding configuration of sampling=True over drafted rows)")
        self.lookup_sampling = lookup_sampling
        self.weights, self.sampling, self.max_batch, self.batch_sampling = weights, sampling, max_batch, batch_sampling
        self.batch_kernels, self.lookup, self.last_lookup_stats = batch_kernels, lookup, None
        sd, cfg, dev, mod = _source(module_or_state_dict, config, device, self.what)
        self.vision = vision                               # a HipQwen25VLVisionTower, or None: the adopted module's eager tower
        why = qwen25vl_refusal(cfg)
        if why:
            _refuse(self.what, why)
        if not 1 <= max_length <= 4096:
            _refuse(self.what, f"max_length {max_length} outside [1, 4096]")
        tc = _text_config(cfg)
        self.config, self.device, self.max_length, self.module = cfg, dev, int(max_length), mod
        self.d, self.F, self.Hq, self.Hkv, self.eps = tc.hidden_size, tc.intermediate_size, tc.num_attention_heads, tc.num_key_value_heads, \
            float(tc.rms_norm_eps)
        self.qkv_cols = (self.Hq + 2 * self.Hkv) * HEAD_DIM
        self.scale = HEAD_DIM ** -0.5
        self.mrope_section = list(tc.rope_parameters["mrope_section"])
        self.image_token_id, self.video_token_id = getattr(cfg, "image_token_id", None), getattr(cfg, "video_token_id", None)
        _check_k(self.what, hidden_size=self.d, intermediate_size=self.F, attention_width=self.Hq * HEAD_DIM)
        lm = {k: v for k, v in sd.items() if not k.startswith(NOT_ADOPTED)}           # lm_head.* / model.visual.*: known, not adopted here
        _check_names(self.what, lm, qwen25vl_param_shapes(cfg))
        _bf16_only(self.what, lm)

        def w(k):
            return lm[LM + k].to(dev, torch.bfloat16).contiguous()

        def cat(b, names, kind):
            return torch.cat([lm[f"{LM}{b}{n}.{kind}"].to(dev, torch.bfloat16) for n in names]).contiguous()
        # "fp8": each packed matrix is quantised on the device as soon as it is there; its bf16 form is dropped before the next one
        mat = ops.quantize_w8 if weights == "fp8" else (lambda t: t)
        self.tok = w("embed_tokens.weight")                                            # in place: no copy when it is already there
        self.layers = []
        for i in range(tc.num_hidden_layers):
            b = f"layers.{i}."
            qkv = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")
            self.layers.append(dict(
                ln1=w(b + "input_layernorm.weight"), wqkv=mat(cat(b, qkv, "weight")), bqkv=cat(b, qkv, "bias"),
                wo=mat(w(b + "self_attn.o_proj.weight")), ln2=w(b + "post_attention_layernorm.weight"),
                wgu=mat(cat(b, ("mlp.gate_proj", "mlp.up_proj"), "weight")), wdown=mat(w(b + "mlp.down_proj.weight"))))
        self.final_ln = w("norm.weight")
        # the module's own inv_freq buffer (a `.to(bfloat16)` of the module rounds it; the eager forward then uses the rounded one)
        rot = getattr(getattr(getattr(mod, "model", None), "language_model", None), "rotary_emb", None) if mod is not None else None
        self.inv_freq = rot.inv_freq.detach().float().cpu() if rot is not None else default_inv_freq(cfg)
        self.ones = torch.ones(self.d, dtype=torch.bfloat16, device=dev)
        self.buf = _Buffers(dev)
        # generate(): lm_head is adopted at the first call (encode-only users do not pay for it); the KV cache is kept like the buffers
        self._tied = bool(getattr(cfg, "tie_word_embeddings", False) or getattr(tc, "tie_word_embeddings", False))
        self._lm_head_src = None if self._tied else sd.get("lm_head.weight")      # a reference, not a copy
        self.lm_head = None
        self.kv = _Buffers(dev)
        self.kv_lookup = _Buffers(dev)                                              # the speculative loop's own set (lookup=True)

    @property
    def generation_config(self):
        """The adopted module's own `generation_config` (the object `generate` reads its defaults from; None when adopted from a state
        dict): what a caller written against the module - Step1X-Edit's thinker - finds where it looks for it."""
        return getattr(self.module, "generation_config", None)

    # ---- host-side preparation (no kernel) -----------------------------------------------------------------------------------------
    def position_ids_for(self, input_ids, attention_mask=None, image_grid_thw=None, position_ids=None, mm_token_type_ids=None,
                         text_from_mask=False):
        """[3, B, L] int64: the caller's `position_ids`, else what the adopted module computes (`model.compute_3d_position_ids`), else
        the arange of Qwen2_5_VLTextModel.forward - or, with `text_from_mask` (a left-padded batch of generate), the text positions
        transformers' generate derives from the mask: cumsum(mask) - 1 on every axis, 0 on the padding."""
        B, L = input_ids.shape
        if position_ids is None:
            if self.module is None:
                _refuse(self.what, "adopted from a state dict (no module to ask for the 3-D positions): pass position_ids")
            position_ids = self.module.model.compute_3d_position_ids(
                input_ids=input_ids, image_grid_thw=image_grid_thw, video_grid_thw=None, inputs_embeds=None, attention_mask=attention_mask,
                past_key_values=None, mm_token_type_ids=mm_token_type_ids)
            if position_ids is None and text_from_mask and attention_mask is not None:
                m = attention_mask.detach().cpu().long()
                position_ids = (m.cumsum(-1) - 1).masked_fill(m == 0, 0)[None].expand(3, -1, -1)
            elif position_ids is None:
                position_ids = torch.arange(L).view(1, 1, -1).expand(3, B, -1)
        if position_ids.ndim == 2:
            position_ids = position_ids[None, ...].expand(3, position_ids.shape[0], -1)
        elif position_ids.ndim == 3 and position_ids.shape[0] == 4:
            position_ids = position_ids[1:]
        if tuple(position_ids.shape) != (3, B, L):
            _refuse(self.what, f"position_ids of shape {tuple(position_ids.shape)} for input_ids [{B}, {L}]")
        return position_ids

    def _prepare(self, input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids, image_embeds, kw,
                 left=False):
        for k in ("pixel_values_videos", "video_grid_thw", "second_per_grid_ts"):
            if kw.get(k) is not None:
                _refuse(self.what, f"{k}: videos are not implemented")
        for k in ("past_key_values", "inputs_embeds", "labels"):
            if kw.get(k) is not None:
                _refuse(self.what, f"{k} is not implemented (one prefill pass over input_ids)")
        for k in ("use_cache", "output_attentions"):
            if kw.get(k):
                _refuse(self.what, f"{k}=True is not implemented")
        known = ("pixel_values_videos", "video_grid_thw", "second_per_grid_ts", "past_key_values", "inputs_embeds", "labels", "use_cache",
                 "output_attentions")
        extra = sorted(k for k in kw if k not in known)
        if extra:
            _refuse(self.what, f"arguments {extra} are not implemented")
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2:
            _refuse(self.what, "input_ids must be a [B, L] tensor")
        B, L = input_ids.shape
        if not 1 <= L <= self.max_length:
            _refuse(self.what, f"sequence length {L} outside [1, {self.max_length}] (max_length of this adoption)")
        ids_cpu = input_ids.detach().cpu()
        if self.video_token_id is not None and bool((ids_cpu == self.video_token_id).any()):
            _refuse(self.what, "video tokens in input_ids: videos are not implemented")
        lengths = (left_valid_lengths if left else valid_lengths)(attention_mask, B, L, self.what)
        if pixel_values is not None and image_embeds is not None:
            _refuse(self.what, "pass pixel_values or image_embeds, not both")
        if pixel_values is not None and self.module is None and self.vision is None:
            _refuse(self.what, "adopted from a state dict (no vision tower at hand): pass image_embeds instead of pixel_values")
        if left:                                           # a batch: the module's position code runs on CPU copies (no eager kernel is launched)
            cpu = lambda v: v.detach().cpu() if isinstance(v, torch.Tensor) else v
            pos = self.position_ids_for(ids_cpu, cpu(attention_mask), cpu(image_grid_thw), cpu(position_ids), cpu(mm_token_type_ids),
                                        text_from_mask=True)
        else:
            pos = self.position_ids_for(input_ids, attention_mask, image_grid_thw, position_ids, mm_token_type_ids)
        tables = mrope_tables(self.inv_freq, pos, self.mrope_section)
        return ids_cpu, lengths, tables, pos

    def _image_embeds(self, pixel_values, image_grid_thw, image_embeds):
        if pixel_values is not None and self.vision is not None:       # the vision tower on the HIP kernels
            image_embeds = self.vision(pixel_values, image_grid_thw).pooler_output
        elif pixel_values is not None:                     # the host's eager module, as in Qwen2_5_VLModel.forward
            image_embeds = self.module.get_image_features(pixel_values, image_grid_thw).pooler_output
        if image_embeds is None:
            return None
        if isinstance(image_embeds, (tuple, list)):
            image_embeds = torch.cat(list(image_embeds), dim=0)
        if image_embeds.dim() != 2 or image_embeds.shape[1] != self.d:
            _refuse(self.what, f"image embeddings of shape {tuple(image_embeds.shape)} (rows of width {self.d})")
        return image_embeds.to(self.device, torch.bfloat16).contiguous()

    def _prefill_row(self, t, ids_row, n, cos, sin, emb=None, idx=None, cache=None):
        """The decoder stack over one row of n valid tokens in the buffers `t`; returns (h, n-scratch) BEFORE the final norm.  With `cache`
        ([layers, cap, 2 Hkv 128]) the k | v columns of every layer are appended as rows [0, n) after mRoPE (generate's prefill)."""
        lib = _lib.lib()
        h, nn, qkv, a, ff, g = (t[k][:n] for k in ("h", "n", "qkv", "a", "ff", "g"))
        self._embed(ids_row, h)
        if emb is not None:
            rc = lib.rgn_scatter_rows(_p(emb), _p(idx), _p(h), emb.shape[0], self.d * 2, _stream())
            _lib.check(rc, "rgn_scatter_rows")
        for li, p in enumerate(self.layers):
            self._rms(h, p["ln1"], nn)
            ops.gemm(nn, p["wqkv"], p["bqkv"], qkv)
            rc = lib.rgn_mrope_bf16(_p(qkv), qkv.stride(0), _p(cos), _p(sin), n, self.Hq, self.Hkv, _stream())
            _lib.check(rc, "rgn_mrope_bf16")
            if cache is not None:
                rc = lib.rgn_lm_kv_append_bf16(_p(qkv), qkv.stride(0), _p(cache[li]), cache.shape[1], 0, n, self.Hq, self.Hkv, _stream())
                _lib.check(rc, "rgn_lm_kv_append_bf16")
            rc = lib.rgn_lm_attention_bf16(_p(qkv), _p(a), n, self.Hq, self.Hkv, float(self.scale), _stream())
            _lib.check(rc, "rgn_lm_attention_bf16")
            ops.gemm(a, p["wo"], None, h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
            self._rms(h, p["ln2"], nn)
            ops.gemm(nn, p["wgu"], None, ff)
            _lib.check(lib.rgn_swiglu_bf16(_p(ff), ff.stride(0), _p(g), g.stride(0), n, self.F, _stream()), "rgn_swiglu_bf16")
            ops.gemm(g, p["wdown"], None, h, epilogue=ops.EPI_GATE_RESID, gate=self.ones, resid=h)
        return h, nn

    # ---- the call --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None, position_ids=None, mm_token_type_ids=None,
                 output_hidden_states=False, return_dict=True, image_embeds=None, **kw):
        ids_cpu, lengths, tables, _ = self._prepare(input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids,
                                                    image_embeds, kw)
        B, L = ids_cpu.shape
        emb = self._image_embeds(pixel_values, image_grid_thw, image_embeds)
        rows = None
        if emb is not None:
            if self.image_token_id is None:
                _refuse(self.what, "the config has no image_token_id")
            rows = image_rows(ids_cpu, lengths, int(self.image_token_id), emb.shape[0], self.what)
            idx = torch.cat(rows).to(self.device)
        ids = input_ids.to(self.device, torch.int64).contiguous()
        tab = tables.to(self.device)                                              # the one host-to-device copy of the tables
        Lb = max(lengths)
        t = self.buf.get(Lb, _row_buffers(self, Lb))
        out = torch.empty(B, L, self.d, dtype=torch.bfloat16, device=self.device)
        lib = _lib.lib()
        if min(lengths) < L:                                                      # padded positions are zero rows
            _lib.check(lib.rgn_fill_zero(_p(out), out.numel() * 2, _stream()), "rgn_fill_zero")
        at = 0
        for bi, n in enumerate(lengths):
            k = rows[bi].numel() if rows is not None else 0
            h, nn = self._prefill_row(t, ids[bi, :n], n, tab[0, bi], tab[1, bi], emb[at:at + k] if k else None, idx[at:at + k] if k else None)
            at += k
            self._rms(h, self.final_ln, out[bi, :n])
        res = QwenTextEncoderOutput(out, bool(output_hidden_states))
        return res if return_dict else res.to_tuple()

    # ---- greedy generate: the prefill above with a KV cache per row, then decode steps over the B rows (csrc/decode.hip) ------------
    def _generate_args(self, input_ids, attention_mask, max_new_tokens, eos_token_id, do_sample, sync_every, kw):
        """Every refusal of `generate`, before any launch; returns the eos ids (a possibly empty list)."""
        gc = getattr(self.module, "generation_config", None)
        if do_sample or (do_sample is None and getattr(gc, "do_sample", False)):
            _refuse(self.what, "do_sample: sampling is not implemented (greedy search only" +
                    ("; the module's generation_config.do_sample is true, pass do_sample=False to decode greedily)" if not do_sample else ")"))
        beams = kw.get("num_beams")
        if (beams is not None and beams != 1) or (beams is None and (getattr(gc, "num_beams", 1) or 1) > 1):
            _refuse(self.what, "num_beams > 1: beam search is not implemented (greedy search only)")
        for k in SAMPLING_ARGS:
            if kw.get(k) is not None:
                _refuse(self.what, f"{k}: sampling and penalty arguments are not implemented (greedy search only)")
        if kw.get("past_key_values") is not None:
            _refuse(self.what, "past_key_values: generate keeps its own KV cache")
        if kw.get("streamer") is not None:
            _refuse(self.what, "streamer is not implemented (the tokens stay on the device between host reads)")
        for k in ("pixel_values_videos", "video_grid_thw", "second_per_grid_ts"):
            if kw.get(k) is not None:
                _refuse(self.what, f"{k}: videos are not implemented")
        known = SAMPLING_ARGS + ("num_beams", "past_key_values", "streamer", "pixel_values_videos", "video_grid_thw", "second_per_grid_ts",
                                 "use_cache")
        extra = sorted(k for k in kw if k not in known)
        if extra:
            _refuse(self.what, f"arguments {extra} are not implemented")
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2:
            _refuse(self.what, "input_ids must be a [B, L] tensor")
        B, L = input_ids.shape
        lengths = None
        if B != 1 and self.max_batch > 1:                                         # a batch: left padding, one cache per row
            if not 1 <= B <= self.max_batch:
                _refuse(self.what, f"input_ids with B = {B}: this adoption takes 1 <= B <= max_batch = {self.max_batch}")
            if self.sampling and not self.batch_sampling:
                _refuse(self.what, f"sampling=True with B = {B}: rgn_lm_pick is one sequence (batched picking is not implemented)")
            lengths = left_valid_lengths(attention_mask, B, L, self.what)
        else:
            if B != 1:
                _refuse(self.what, f"input_ids with B = {B}: generate is implemented for B == 1")
            if attention_mask is not None and (tuple(attention_mask.shape) != (B, L) or not bool((attention_mask.detach().cpu() != 0).all())):
                _refuse(self.what, "attention_mask must be all ones for generate (no padding inside a KV cache)")
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
            _refuse(self.what, "max_new_tokens is required and must be an int >= 1 (the decode loop is a `for` over it)")
        if lengths is None and L + max_new_tokens > self.max_length:
            _refuse(self.what, f"L + max_new_tokens = {L + max_new_tokens} exceeds max_length {self.max_length} of this adoption")
        for b, n in enumerate(lengths or ()):
            if n + max_new_tokens > self.max_length:
                _refuse(self.what, f"row {b}: n + max_new_tokens = {n + max_new_tokens} exceeds max_length {self.max_length} of this adoption")
        if isinstance(sync_every, bool) or not isinstance(sync_every, int) or sync_every < 1:
            _refuse(self.what, "sync_every must be an int >= 1")
        if eos_token_id is None:                                                  # transformers' default; an explicit [] asks for no EOS
            eos_token_id = getattr(gc, "eos_token_id", None)
        if eos_token_id is None:
            return []
        if isinstance(eos_token_id, torch.Tensor):
            eos_token_id = eos_token_id.flatten().tolist()
        eos = [eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)
        if not all(isinstance(e, int) and not isinstance(e, bool) for e in eos):
            _refuse(self.what, "eos_token_id must be an int or a list of ints")
        return eos

    def _pick_plan(self, do_sample, max_new_tokens, kw, B=1):
        """`sampling=True`: the decoding configuration of this call - an argument, else the module's generation_config field, else off -
        and every refusal that goes with it, before any launch.  `kw` holds the PICK_ARGS / PICK_EXTRA arguments of the call.  A batch
        (`batch_sampling=True`, B >= 2) shares the one configuration; its `uniforms` are [max_new_tokens, B]."""
        gc = getattr(self.module, "generation_config", None)
        if self.tok.shape[0] > 1 << 20:
            _refuse(self.what, f"a vocabulary of {self.tok.shape[0]} under sampling=True (rgn_lm_pick takes V <= 1048576)")
        for k, off in CONFIG_OFF.items():
            v = getattr(gc, k, None)
            if v is not None and v != off:
                _refuse(self.what, f"generation_config.{k} = {v!r} of the adopted module is not implemented (only None"
                        + (f" or {off!r}" if off is not None else "") + " would not change the tokens)")

        def take(k):
            v = kw.get(k)
            return getattr(gc, k, None) if v is None else v
        if do_sample is None:
            do_sample = bool(getattr(gc, "do_sample", False))
        if not isinstance(do_sample, bool):
            _refuse(self.what, f"do_sample={do_sample!r} (True, False or None)")
        penalty, temperature, top_k, top_p = take("repetition_penalty"), take("temperature"), take("top_k"), take("top_p")
        if penalty is not None and not (_number(penalty) and 0 < penalty < float("inf")):
            _refuse(self.what, f"repetition_penalty={penalty!r} (a number > 0)")
        if temperature is not None and not (_number(temperature) and 0 < temperature < float("inf")):
            _refuse(self.what, f"temperature={temperature!r} (a number > 0)")
        if top_k is not None and not (isinstance(top_k, int) and not isinstance(top_k, bool) and 1 <= top_k < 2 ** 31):
            _refuse(self.what, f"top_k={top_k!r} (an int >= 1)")
        if top_p is not None and not (_number(top_p) and 0 < top_p <= 1):
            _refuse(self.what, f"top_p={top_p!r} (a number in (0, 1])")
        generator, uniforms, scores = kw.get("generator"), kw.get("uniforms"), kw.get("output_scores")
        if generator is not None and uniforms is not None:
            _refuse(self.what, "generator= and uniforms= together (one source of the uniforms)")
        if generator is not None and not isinstance(generator, torch.Generator):
            _refuse(self.what, f"generator={type(generator).__name__} (a torch.Generator)")
        if uniforms is not None:
            here = torch.device(self.device)
            there = uniforms.device if isinstance(uniforms, torch.Tensor) else None
            shape = (max_new_tokens,) if B == 1 else (max_new_tokens, B)
            if there is None or tuple(uniforms.shape) != shape or uniforms.dtype != torch.float32 or not uniforms.is_contiguous() \
                    or there.type != here.type or (here.index is not None and there.index not in (None, here.index)):
                if B > 1:
                    _refuse(self.what, f"uniforms must be a contiguous float32 tensor of shape ({max_new_tokens}, {B}) on "
                                       f"{torch.device(self.device)} (time-major: one uniform in [0, 1) per new token and row)")
                _refuse(self.what, f"uniforms must be a contiguous float32 tensor of shape ({max_new_tokens},) on {torch.device(self.device)} "
                                   "(one uniform in [0, 1) per new token)")
        if scores is not None and not isinstance(scores, bool):
            _refuse(self.what, f"output_scores={scores!r} (True or False)")
        return PickPlan(do_sample, float(penalty or 1.0), float(temperature or 1.0), int(top_k or 0), float(top_p or 1.0), uniforms, generator,
                        bool(scores))

    def _adopt_lm_head(self):
        """`lm_head.weight` [V, d] bf16 on the device, adopted at the first generate; the token embedding under tie_word_embeddings."""
        if self.lm_head is not None:
            return self.lm_head
        if self._tied:
            self.lm_head = self.tok
            return self.lm_head
        w = self._lm_head_src
        if w is None:
            _refuse(self.what, "lm_head.weight is missing from the adopted state dict: generate needs it")
        if w.dtype != torch.bfloat16 or tuple(w.shape) != tuple(self.tok.shape):
            _refuse(self.what, f"lm_head.weight is {w.dtype} {tuple(w.shape)}, the kernels take bf16 {tuple(self.tok.shape)}")
        self.lm_head = w.detach().to(self.device, torch.bfloat16).contiguous()
        return self.lm_head

    # The preparation of both decode loops, every refusal before any launch.  It comes in three calls, in this order, because the lookup
    # loop's own refusals sit between them and which refusal a bad call gets first is behaviour.
    def _decoding_args(self, input_ids, attention_mask, max_new_tokens, eos_token_id, do_sample, sync_every, kw):
        """(eos ids, the pad_token_id argument, the PICK_ARGS / PICK_EXTRA arguments or None), each split off `kw` where the adoption
        takes it (a default adoption refuses them as before), and `_generate_args` over the rest."""
        pad_arg = kw.pop("pad_token_id", None) if self.max_batch > 1 else None
        if not self.sampling:                                                     # without the opt-in every refusal is what it was
            return self._generate_args(input_ids, attention_mask, max_new_tokens, eos_token_id, do_sample, sync_every, kw), pad_arg, None
        mine = {k: kw.pop(k) for k in PICK_ARGS + PICK_EXTRA if k in kw}
        return self._generate_args(input_ids, attention_mask, max_new_tokens, eos_token_id, False, sync_every, kw), pad_arg, mine

    def _sampled_pick(self, do_sample, max_new_tokens, mine, B):
        """The PickPlan of a call whose pick is not the head's argmax; None without `sampling=True` and for a configuration that is
        greedy as before, which runs the greedy launches unchanged."""
        if mine is None:
            return None
        plan = self._pick_plan(do_sample, max_new_tokens, mine, B)
        return None if plan.greedy_as_before else plan

    def _prompt_inputs(self, input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids, image_embeds, T,
                       pad_arg, eos):
        """(ids_cpu, lens, prompt tables [2, B, L, 128], decode tables [2, B, T, 128], pad id, lm_head, image embeddings, their rows per
        batch row, those rows as one device index) of left-padded rows; the last three are None without images."""
        ids_cpu, lens, tables, pos = self._prepare(input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids,
                                                   image_embeds, {}, left=True)
        pad = resolve_pad_token_id(pad_arg, getattr(self.module, "generation_config", None), eos)
        new_tables = mrope_tables(self.inv_freq, decode_position_ids(pos, T), self.mrope_section)
        head = self._adopt_lm_head()                                               # may refuse: nothing has been launched yet
        emb = self._image_embeds(pixel_values, image_grid_thw, image_embeds)
        rows = idx = None
        if emb is not None:
            if self.image_token_id is None:
                _refuse(self.what, "the config has no image_token_id")
            rows = image_rows_left(ids_cpu, lens, int(self.image_token_id), emb.shape[0], self.what)
            idx = torch.cat(rows).to(self.device)
        return ids_cpu, lens, tables, new_tables, pad, head, emb, rows, idx

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, pixel_values=None, image_grid_thw=None, max_new_tokens=None, eos_token_id=None,
                 do_sample=None, return_dict_in_generate=False, output_logits=False, mm_token_type_ids=None, image_embeds=None,
                 position_ids=None, sync_every=8, **kw):
        """transformers' greedy `generate` for B rows, 1 <= B <= max_batch: LongTensor [B, L + n_new], the prompts followed by the new
        tokens.  A row is cut after its first `eos_token_id` (an int or a list; EOS included; None: the module's
        generation_config.eos_token_id, []: no EOS); n_new is the largest cut (max_new_tokens if a row never finished) and a row that
        finished earlier holds the pad id from its cut on (`assemble_sequences`) - one row is cut, never padded.
        Each row is prefilled over its valid tokens by `_prefill_row` into its own cache at rows [0, n_b) - no padded key is ever in a
        cache, so decode needs no mask - then every step is the decode step of `_DecodeStep` at M = B, the B rows from ONE stream of the
        weights, with this loop's middle of a layer: rgn_mrope_bf16 at the step's table rows, then rgn_lm_kv_append_bf16_rows and
        rgn_lm_decode_attention_bf16_rows over the rows' caches, in groups of at most 8 rows.  The step's head
        picks INTO the device id row the next rgn_text_embed reads (new ids [T, B] and decode RoPE tables [T, B, 128] time-major, so a
        step's rows are contiguous): no token visits the host inside a step.  The host reads the ids back every `sync_every` tokens to
        look for EOS (never without one); the result does not depend on `sync_every`.  The device keeps decoding finished rows (a fixed
        launch count, no dependence on device data).  Row b's tokens and fp32 logits are bit for bit those of the B = 1 call on row b's
        unpadded prompt.  `.logits` (output_logits=True) is a tuple of n_new fp32 [B, V] tensors; rows past a sequence's EOS are not
        meaningful.
        Under `max_batch=N` the call takes 2 <= B <= N rows with a left-padded `attention_mask` (zeros, then ones) and `pad_token_id`
        (None: generation_config.pad_token_id, else the first EOS id); one row takes an all-ones mask under every adoption.
        Under `sampling=True` the call also takes do_sample, temperature, top_k, top_p, repetition_penalty (None: the module's
        generation_config value, else off), generator= or uniforms= (fp32 [max_new_tokens] on the device) and output_scores=True: unless
        that configuration is greedy as before, the head writes the fp32 [B, V] logits and ONE rgn_lm_pick_rows per step turns them into
        the step's id row, still without a host read inside a step; `.scores` is a tuple of n_new fp32 [B, V] tensors.
        Under `batch_sampling=True` a batch takes those arguments too, one configuration for all rows: uniforms= is then a contiguous
        fp32 [max_new_tokens, B] on the device (time-major, like the new ids), generator= fills torch.rand(T, B) once before the loop -
        so with a generator a row's stream of uniforms depends on B and on the row's place in the batch.  For given `uniforms`, row b is
        bit for bit the B = 1 call on its unpadded prompt with uniforms[:, b].  The byte map of the repetition penalty is [B, V], zeroed
        once; row b sees that row's valid prompt ids and its own new tokens, the left padding is NOT marked (transformers gathers at the
        pad positions too).  Finished rows keep being picked; scores past a row's EOS are not meaningful.
        Under `lookup=True` one sequence also takes prompt_lookup_num_tokens=, max_matching_ngram_size= and draft_tokens=: with one of
        them the call is `_generate_lookup` (drafted tokens verified as extra rows of a step; the same sequences and logits, bit for bit),
        without them it is this loop unchanged.
        Under `lookup_sampling=True` that call also takes the decoding configuration of `sampling=True` (bit for bit the plain sampled
        loop's sequences, logits and scores for the same uniforms), and prompt_lookup_num_tokens / max_matching_ngram_size left at None
        take the module's generation_config values."""
        look = {k: kw.pop(k) for k in LOOKUP_ARGS if k in kw} if self.lookup else {}   # without lookup=True they are refused as before
        if self.lookup_sampling:                                                  # transformers' rule: an argument, else the config's field
            gc = getattr(self.module, "generation_config", None)
            for k in LOOKUP_ARGS[:2]:
                if look.get(k) is None and getattr(gc, k, None) is not None:
                    look[k] = getattr(gc, k)
        self.last_lookup_stats = None                                             # of the last generate: None after a plain one
        if any(v is not None for v in look.values()):
            return self._generate_lookup(look, input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, eos_token_id, do_sample,
                                         return_dict_in_generate, output_logits, mm_token_type_ids, image_embeds, position_ids, sync_every, kw)
        eos, pad_arg, mine = self._decoding_args(input_ids, attention_mask, max_new_tokens, eos_token_id, do_sample, sync_every, kw)
        plan = self._sampled_pick(do_sample, max_new_tokens, mine, input_ids.shape[0])
        T = int(max_new_tokens)
        ids_cpu, lens, tables, new_tables, pad, head, emb, rows, idx = self._prompt_inputs(
            input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids, image_embeds, T, pad_arg, eos)
        B, L = ids_cpu.shape
        lib, dev, d, V = _lib.lib(), self.device, self.d, self.tok.shape[0]
        nmax = max(lens)
        cap, kvw, nl = nmax + T, 2 * self.Hkv * HEAD_DIM, len(self.layers)
        step = _DecodeStep(self, lib)
        ws_a = B * lib.rgn_lm_decode_attention_workspace_bytes(self.Hq, cap)
        ws_h = step.head_workspace_bytes(B)
        head_rows, head_name = step.head, step.head_name
        groups = [(g0, min(MAX_BATCH, B - g0)) for g0 in range(0, B, MAX_BATCH)]  # at most 8 rows per launch of a per-row entry
        c = self.kv.get((B, cap), dict(cache=(nl, B, cap, kvw), **_row_buffers(self, B), ws_a=((ws_a + 1) // 2,), ws_h=((ws_h + 1) // 2,)))
        t = self.buf.get(nmax, _row_buffers(self, nmax))
        ids = input_ids.to(dev, torch.int64).contiguous()
        new = torch.empty(T, B, dtype=torch.int64, device=dev)                    # time-major: a step's B ids are contiguous
        logits = torch.empty(T, B, V, dtype=torch.float32, device=dev) if output_logits else None
        tab, ntab = tables.to(dev), new_tables.transpose(1, 2).contiguous().to(dev)                       # [2, B, L, 128], [2, T, B, 128]
        st, ck = _stream(), _lib.check
        pn, pnew = c["n"].data_ptr(), new.data_ptr()

        scores = None
        if plan is None:
            def pick(k):                                                          # tokens k of the B rows from the normalised rows in c["n"]
                ck(head_rows(_p(head), pn, d, B, V, d, pnew + 8 * B * k, 1, None if logits is None else _p(logits[k]), V, _p(c["ws_h"]), ws_h, st),
                   head_name)
        else:
            # the pick of this generate, chosen once: lm_head writes the fp32 rows, ONE rgn_lm_pick_rows turns them into the step's id row
            pk = _PickState(lib, plan, ids, lens, T, B, V, logits is not None, st)
            pick_rows, pick_name, pick_groups = (lib.rgn_lm_pick_wide, "rgn_lm_pick_wide", [(0, B)]) if step.wide else \
                (lib.rgn_lm_pick_rows, "rgn_lm_pick_rows", groups)
            seen, zrows, pick_ws, scores, ws_1, pu = pk.seen, pk.zrows, pk.ws, pk.scores, pk.ws_1, pk.pu
            pen, smp, tmp, tk, tp = pk.how

            def pick(k):
                z = logits[k] if logits is not None else zrows
                ck(head_rows(_p(head), pn, d, B, V, d, pnew + 8 * B * k, 1, _p(z), V, _p(c["ws_h"]), ws_h, st), head_name)
                for g0, Bg in pick_groups:                                        # rows never meet: one launch or several, every row keeps its bits
                    ck(pick_rows(z.data_ptr() + 4 * V * g0, V, Bg, V, seen.data_ptr() + V * g0, V, pen, smp, tmp, tk, tp,
                                 None if pu is None else pu + 4 * (B * k + g0), pnew + 8 * (B * k + g0), 1,
                                 None if scores is None else scores[k].data_ptr() + 4 * V * g0, V, pick_ws.data_ptr() + ws_1 * g0, Bg * ws_1, st),
                       pick_name)
        at = 0
        for b, n in enumerate(lens):                                              # rows prefill one after another on the existing kernels
            k = rows[b].numel() if rows is not None else 0
            h, _ = self._prefill_row(t, ids[b, L - n:], n, tab[0, b, L - n:], tab[1, b, L - n:], emb[at:at + k] if k else None,
                                     idx[at:at + k] if k else None, cache=c["cache"][:, b])
            at += k
            self._rms(h[n - 1:n], self.final_ln, c["n"][b:b + 1])                 # the final norm on the last row only
        pick(0)
        ph, pqkv, pa, pws = (c[k].data_ptr() for k in ("h", "qkv", "a", "ws_a"))
        ptok, pcos, psin = self.tok.data_ptr(), ntab[0].data_ptr(), ntab[1].data_ptr()
        Hq, Hkv, scale, qc, ad = self.Hq, self.Hkv, float(self.scale), self.qkv_cols, self.Hq * HEAD_DIM
        cstride = cap * kvw
        row0, nn = (ctypes.c_int * B)(), (ctypes.c_int * B)()                     # host arrays: the entries copy them into the launch
        # This loop's middle of a layer: mRoPE (its table row moves with the step), then per group of rows the append to the rows' caches
        # and the attention against them over the host arrays, bound once like the step's own launches and run with those after mRoPE.
        append, attend = lib.rgn_lm_kv_append_bf16_rows, lib.rgn_lm_decode_attention_bf16_rows
        layers, (final_norm, final_name) = step.launches(c, B, st)
        lp = []
        ws_1a = ws_a // B                                                         # a row's attention partials: a multiple of 8 x 65 bytes
        ints = ctypes.POINTER(ctypes.c_int)
        at_row = lambda arr, g0: ctypes.cast(ctypes.byref(arr, 4 * g0), ints)     # the group's slice of a host int array
        for i, (before, after) in enumerate(layers):
            pc = c["cache"][i].data_ptr()
            kv = [_bound(append, "rgn_lm_kv_append_bf16_rows", pqkv + 2 * qc * g0, qc, pc + 2 * cstride * g0, cstride, cap, at_row(row0, g0), Bg,
                         Hq, Hkv, st) for g0, Bg in groups]
            kv += [_bound(attend, "rgn_lm_decode_attention_bf16_rows", pqkv + 2 * qc * g0, qc, pc + 2 * cstride * g0, cstride, pa + 2 * ad * g0, ad,
                          at_row(nn, g0), Bg, Hq, Hkv, scale, pws + ws_1a * g0, Bg * ws_1a, st) for g0, Bg in groups]
            lp.append((before, kv + after))
        mrope = functools.partial(lib.rgn_mrope_bf16, ctypes.c_void_p(pqkv), ctypes.c_int(qc))
        mtail = (ctypes.c_int(B), ctypes.c_int(Hq), ctypes.c_int(Hkv), ctypes.c_void_p(st))
        n_new = T
        for k in range(1, T + 1):                                                 # bounded by max_new_tokens, never by device data
            if eos and (k % sync_every == 0 or k == T):                           # the host's look at the ids: the only synchronisation
                cuts = eos_cuts(new[:k].cpu(), eos)
                if all(cut is not None for cut in cuts):
                    n_new = max(cuts)
                    break
            if k == T:
                break
            for b, n in enumerate(lens):                                          # the tokens picked last: row n + k - 1 of each cache
                row0[b], nn[b] = n + k - 1, n + k
            tb = 256 * B * (k - 1)
            cos, sin = ctypes.c_void_p(pcos + tb), ctypes.c_void_p(psin + tb)
            ck(lib.rgn_text_embed(pnew + 8 * B * (k - 1), B, ptok, V, None, 0, ph, d, st), "rgn_text_embed")
            for before, after in lp:
                for launch, name in before:
                    ck(launch(), name)
                ck(mrope(cos, sin, *mtail), "rgn_mrope_bf16")
                for launch, name in after:
                    ck(launch(), name)
            ck(final_norm(), final_name)
            pick(k)
        seq, n_new = assemble_sequences(ids_cpu, new[:n_new].cpu(), eos, pad)
        return _generate_result(seq.to(input_ids.device), n_new, logits, scores, return_dict_in_generate)

    # ---- greedy generate with drafted tokens verified in one step (lookup=True; csrc/decode.hip: lm_verify_attention_kernel) ----------
    def _generate_lookup(self, look, input_ids, attention_mask, pixel_values, image_grid_thw, max_new_tokens, eos_token_id, do_sample,
                         return_dict_in_generate, output_logits, mm_token_type_ids, image_embeds, position_ids, sync_every, kw):
        """Greedy `generate` for ONE sequence whose steps carry drafted tokens: the sequences and fp32 `logits` of the plain loop of the
        same adoption, bit for bit, in fewer steps when drafts are accepted.  A step at settled length n with k' drafts runs R = k' + 1
        rows - the last settled token and the drafts, contiguous in the device id run `seq` (prompt, then new tokens) - through the
        decode step of `_DecodeStep` at M = R (row b of its entries has the bits of the one-row call), with this loop's middle of a
        layer: rgn_mrope_bf16 over R consecutive table rows, and ONE rgn_lm_kv_append_bf16 of R rows at cache row n - 1 followed by
        rgn_lm_verify_attention_bf16 (query r over n + r cache rows; groups of 8 queries under "mfma").  The head writes R argmaxes (and,
        with output_logits, the fp32 rows straight into logits[k : k + R]); rgn_lm_lookup_step keeps the drafts the argmaxes confirm,
        writes the token after them and drafts for the next step (`prompt_lookup_num_tokens`: transformers' n-gram lookup in the
        sequence so far; `draft_tokens`: the caller's guess); the host reads its (a, k', tokens) buffer, the one copy of a step, and
        looks for EOS there.  Cache rows and logits rows of rejected drafts are overwritten by later steps.  The prefill's pick is the
        first such step with R = 1.  `last_lookup_stats`: steps (decode steps after the prefill), drafted and accepted (drafts over
        those steps) and tokens (new tokens decoded before the EOS cut: 1 + steps + accepted).
        Under `lookup_sampling=True`, for a configuration that is not greedy as before, the claim is against the plain SAMPLED loop
        with the same `uniforms` (sequences, logits and processed scores): the head always writes the R fp32 rows, rgn_lm_pick_verify
        picks row r under the byte map seen U drafts[0, r) with uniforms[k + r] and leaves the map alone, rgn_lm_lookup_step_mark
        accepts against those picks and marks what the step settles.  The map is zeroed once and rgn_lm_seen_mark runs over the prompt
        once; scores rows of rejected drafts are overwritten like the logits rows."""
        eos, pad_arg, mine = self._decoding_args(input_ids, attention_mask, max_new_tokens, eos_token_id, do_sample, sync_every, kw)
        if input_ids.shape[0] != 1:
            _refuse(self.what, f"prompt_lookup_num_tokens / draft_tokens with B = {input_ids.shape[0]}: drafts are verified for one sequence (B == 1)")
        plan = self._sampled_pick(do_sample, max_new_tokens, mine, 1)            # a PickPlan: the step's picks are rgn_lm_pick_verify's
        if plan is not None and not self.lookup_sampling:                        # None: today's greedy path, launch for launch
            _refuse(self.what, "prompt_lookup_num_tokens / draft_tokens with sampling, a repetition penalty or output_scores: drafts are "
                               "verified against greedy search only")
        K, max_ngram, guess = lookup_plan(self.what, look, self.batch_kernels == "mfma")
        T = int(max_new_tokens)
        ids_cpu, lens, tables, new_tables, pad, head, emb, _, idx = self._prompt_inputs(
            input_ids, attention_mask, pixel_values, image_grid_thw, position_ids, mm_token_type_ids, image_embeds, T, pad_arg, eos)
        L = ids_cpu.shape[1]
        if lens[0] != L:                                                          # `_generate_args` takes one row with an all-ones mask only
            _refuse(self.what, "prompt_lookup_num_tokens / draft_tokens with a padded row: the id run of the lookup is the unpadded prompt")
        lib, dev, d, V = _lib.lib(), self.device, self.d, self.tok.shape[0]
        Rm, cap, kvw, nl = K + 1, L + T, 2 * self.Hkv * HEAD_DIM, len(self.layers)
        groups = {R: [(g0, min(MAX_BATCH, R - g0)) for g0 in range(0, R, MAX_BATCH)] for R in range(1, Rm + 1)}
        step = _DecodeStep(self, lib)
        ws_a = min(Rm, MAX_BATCH) * lib.rgn_lm_decode_attention_workspace_bytes(self.Hq, cap)          # the groups run one after another
        ws_h = step.head_workspace_bytes(Rm)
        head_rows, head_name = step.head, step.head_name
        c = self.kv_lookup.get((Rm, cap), dict(cache=(nl, cap, kvw), **_row_buffers(self, Rm), ws_a=((ws_a + 1) // 2,), ws_h=((ws_h + 1) // 2,)))
        t = self.buf.get(L, _row_buffers(self, L))
        ids = input_ids.to(dev, torch.int64).contiguous()
        seq = torch.empty(L + T, dtype=torch.int64, device=dev)                   # ONE run: the prompt ids, then the new tokens
        seq[:L].copy_(ids[0])
        heads = torch.empty(MAX_WIDE_BATCH, dtype=torch.int64, device=dev)        # the argmax after each row of a step
        res = torch.empty(2 + MAX_WIDE_BATCH, dtype=torch.int64, device=dev)      # a, k', the accepted tokens
        logits = torch.empty(T, 1, V, dtype=torch.float32, device=dev) if output_logits else None
        gdev = guess.detach().to(dev).contiguous() if guess is not None else None
        pguess, nguess = (gdev.data_ptr(), gdev.numel()) if gdev is not None else (None, 0)
        tab, ntab = tables.to(dev), new_tables.transpose(1, 2).contiguous().to(dev)                       # [2, 1, L, 128], [2, T, 1, 128]
        st, ck = _stream(), _lib.check
        ph, pn, pqkv, pa, pws = (c[k].data_ptr() for k in ("h", "n", "qkv", "a", "ws_a"))
        pseq, pheads, pres, pwh = seq.data_ptr(), heads.data_ptr(), res.data_ptr(), c["ws_h"].data_ptr()
        plog = logits.data_ptr() if logits is not None else None
        limit = L + T
        scores = None
        if plan is not None:
            # the picks of this generate, chosen once: the head always writes the R fp32 rows, ONE rgn_lm_pick_verify turns them into the
            # R picks (row r under seen U drafts[0, r), uniform k + r), rgn_lm_lookup_step_mark accepts against them and marks
            pk = _PickState(lib, plan, ids, lens, T, Rm, V, logits is not None, st)
            scores, ws_p, pu = pk.scores, pk.ws_bytes, pk.pu
            pen, smp, tmp, tk, tp = pk.how
            pseen, ppick, pz = pk.seen.data_ptr(), pk.ws.data_ptr(), None if pk.zrows is None else pk.zrows.data_ptr()
            pscores = None if scores is None else scores.data_ptr()

        def settle(n, R, k):
            """The head over the R normalised rows of c["n"] (logits rows k..k + R - 1), accept + propose, the step's one host read."""
            if plan is None:
                ck(head_rows(_p(head), pn, d, R, V, d, pheads, 1, None if plog is None else plog + 4 * V * k, V, pwh, ws_h, st), head_name)
                ck(lib.rgn_lm_lookup_step(pseq, n, R, pheads, 1, limit, K, max_ngram, pguess, nguess, L, pres, st), "rgn_lm_lookup_step")
            else:
                z = pz if plog is None else plog + 4 * V * k
                ck(head_rows(_p(head), pn, d, R, V, d, pheads, 1, z, V, pwh, ws_h, st), head_name)
                ck(lib.rgn_lm_pick_verify(z, V, R, V, pseen, pseq + 8 * n, pen, smp, tmp, tk, tp, None if pu is None else pu + 4 * k, pheads, 1,
                                          None if pscores is None else pscores + 4 * V * k, V, ppick, ws_p, st), "rgn_lm_pick_verify")
                ck(lib.rgn_lm_lookup_step_mark(pseq, n, R, pheads, 1, limit, K, max_ngram, pguess, nguess, L, pres, pseen, V, st),
                   "rgn_lm_lookup_step_mark")
            out = res[:2 + R].tolist()
            return out[0], out[1], out[2:3 + out[0]]

        h, _ = self._prefill_row(t, ids[0], L, tab[0, 0], tab[1, 0], emb, idx, cache=c["cache"])
        self._rms(h[L - 1:L], self.final_ln, c["n"][0:1])                         # the final norm on the last row only
        _, kd, new = settle(L, 1, 0)                                              # the prefill's pick: a step of one row, nothing to accept
        ptok, pcos, psin = self.tok.data_ptr(), ntab[0].data_ptr(), ntab[1].data_ptr()
        Hq, Hkv, scale, qc, ad = self.Hq, self.Hkv, float(self.scale), self.qkv_cols, self.Hq * HEAD_DIM
        I, P, Fl = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
        plans = {}

        def plan_for(R):
            """The launches of a step of R rows, built once: per layer the step's own before mRoPE, this loop's middle - the three whose
            arguments move with the step (mRoPE's table rows, the append's cache row, each verify group's n0: leading arguments bound, the
            tail ready) - and the step's own after it."""
            layers, final = step.launches(c, R, st)
            lp = []
            for i, (before, after) in enumerate(layers):
                pc = c["cache"][i].data_ptr()
                lp.append((
                    before,
                    functools.partial(lib.rgn_lm_kv_append_bf16, P(pqkv), I(qc), P(pc), I(cap)),
                    [(functools.partial(lib.rgn_lm_verify_attention_bf16, P(pqkv + 2 * qc * g0), I(qc), P(pc), P(pa + 2 * ad * g0), I(ad)), g0,
                      (I(Rg), I(Hq), I(Hkv), Fl(scale), P(pws), ctypes.c_size_t(ws_a), P(st))) for g0, Rg in groups[R]],
                    after))
            return lp, final, (I(R), I(Hq), I(Hkv), P(st))

        mrope = functools.partial(lib.rgn_mrope_bf16, P(pqkv), I(qc))
        k, steps, drafted, accepted = 1, 0, 0, 0                                   # k new tokens are settled
        while k < T and not (eos and any(tok in eos for tok in new)):             # bounded by max_new_tokens: every step settles >= 1
            R, n = kd + 1, L + k                                                  # rows: new token k - 1 and the kd drafts after it
            if R not in plans:
                plans[R] = plan_for(R)
            lp, (final_norm, final_name), tail = plans[R]
            cos, sin, row0 = P(pcos + 256 * (k - 1)), P(psin + 256 * (k - 1)), I(n - 1)
            ck(lib.rgn_text_embed(pseq + 8 * (n - 1), R, ptok, V, None, 0, ph, d, st), "rgn_text_embed")
            for before, append, verify, after in lp:
                for launch, name in before:
                    ck(launch(), name)
                ck(mrope(cos, sin, *tail), "rgn_mrope_bf16")
                ck(append(row0, *tail), "rgn_lm_kv_append_bf16")
                for attend, g0, vtail in verify:
                    ck(attend(I(n + g0), *vtail), "rgn_lm_verify_attention_bf16")
                for launch, name in after:
                    ck(launch(), name)
            ck(final_norm(), final_name)
            a, kn, toks = settle(n, R, k)
            steps, drafted, accepted, k, kd = steps + 1, drafted + kd, accepted + a, k + a + 1, kn
            new += toks
        self.last_lookup_stats = dict(steps=steps, drafted=drafted, accepted=accepted, tokens=len(new))
        out, n_new = assemble_sequences(ids_cpu, torch.tensor(new, dtype=torch.int64).view(-1, 1), eos, pad)
        return _generate_result(out.to(input_ids.device), n_new, logits, scores, return_dict_in_generate)
