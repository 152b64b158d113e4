"""ctypes binding of libregione_hip.so (the C ABI declared in include/regione_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a symbol cannot be
resolved this module raises at import/first use - loudly - instead of degrading to eager torch.
"""
from __future__ import annotations

import ctypes as C
import os

# torch ships its own libamdhip64; it must be in the process BEFORE libregione_hip.so is dlopen'ed so
# that both resolve to the same HIP runtime (loading ours first binds /opt/rocm's copy and the two
# runtimes then disagree about the device: "no ROCm-capable device is detected").
import torch  # noqa: F401

from . import build as _build
from .build import LIB_PATH

# developer A/B switch: load another build of the SAME C ABI (never a fallback - it must exist)
LIB_PATH = os.environ.get("RGN_LIB", LIB_PATH)

_c_void_p, _c_int, _c_float = C.c_void_p, C.c_int, C.c_float



class QkvEpilogue(C.Structure):
    """struct rgn_qkv_epilogue (include/regione_hip.h)."""
    _fields_ = [("wq", _c_void_p), ("wk", _c_void_p), ("cos_q", _c_void_p), ("sin_q", _c_void_p), ("cos_k", _c_void_p),
                ("sin_k", _c_void_p), ("kv_rows", _c_void_p), ("k_slab", _c_void_p), ("vt_slab", _c_void_p),
                ("row_base", _c_int), ("skv_pad", _c_int), ("k_col", _c_int), ("v_col", _c_int), ("q_col", _c_int),
                ("heads", _c_int), ("eps", _c_float), ("fp16_roundtrip", _c_int)]


_qkv_p = C.POINTER(QkvEpilogue)


class GemmProblem(C.Structure):
    """struct rgn_gemm_problem (include/regione_hip.h): one problem of rgn_gemm_group, the one GEMM entry point."""
    _fields_ = [("A", _c_void_p), ("W", _c_void_p), ("wscale", _c_void_p), ("bias", _c_void_p), ("C", _c_void_p),
                ("gate", _c_void_p), ("resid", _c_void_p), ("qkv", _qkv_p), ("out_rows", _c_void_p), ("lda", _c_int), ("ldc", _c_int),
                ("M", _c_int), ("ldw", _c_int), ("ascale", _c_void_p)]


_prob_p = C.POINTER(GemmProblem)


class BlockWeight(C.Structure):
    """struct rgn_block_weight (include/regione_hip.h): W, its fp8 per-channel scale (NULL = bf16 weights) and the bias."""
    _fields_ = [("W", _c_void_p), ("wscale", _c_void_p), ("bias", _c_void_p)]


class MmditBlock(C.Structure):
    """struct rgn_mmdit_block (include/regione_hip.h): one masked MMDiT block, the descriptor of rgn_mmdit_double_block /
    rgn_mmdit_single_block.  lib() compares its size with rgn_mmdit_block_bytes()."""
    _fields_ = ([("x", _c_void_p), ("nrm", _c_void_p), ("wide", _c_void_p), ("ldx", _c_int), ("ldnrm", _c_int), ("ldwide", _c_int),
                 ("T", _c_int), ("M", _c_int), ("d", _c_int), ("d_ff", _c_int), ("heads", _c_int), ("adaln", _c_void_p), ("adaln_txt", _c_void_p)]
                + [(n, BlockWeight) for n in ("w_kvq", "w_add_kvq", "w_out", "w_add_out", "ff_w1", "ffc_w1", "ff_w2", "ffc_w2", "w_kvqm", "w_po")]
                + [(n, _c_void_p) for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k", "k_slab", "vt_slab", "kv_rows", "cos_q", "sin_q",
                                            "cos_k", "sin_k")]
                + [("skv", _c_int), ("skv_pad", _c_int), ("score_bound", _c_float), ("rowbands", _c_int), ("out_rows", _c_int), ("branches", _c_int),
                   ("gemm_ws", _c_void_p), ("gemm_ws_bytes", C.c_size_t), ("attn_ws", _c_void_p), ("attn_ws_bytes", C.c_size_t)])


_block_p = C.POINTER(MmditBlock)


class LoraTerm(C.Structure):
    """struct rgn_lora_term (include/regione_hip.h): one `scale * B A` term of rgn_lora_merge_bf16 (A [r, K], B [N, r] fp32 on the device)."""
    _fields_ = [("A", _c_void_p), ("B", _c_void_p), ("r", _c_int), ("scale", _c_float)]


_term_p = C.POINTER(LoraTerm)

# name -> argtypes (restype is always int unless listed in _RESTYPE)
SIGNATURES = {
    "rgn_version": [],
    "rgn_abi_struct_bytes": [],
    "rgn_plan_override": [C.c_char_p, _c_int],
    "rgn_plan_override_get": [C.c_char_p, C.POINTER(C.c_int)],
    "rgn_gemm_last_plan": [],
    "rgn_attention_last_plan": [],
    "rgn_attention_plan_query": [_c_int, _c_int, _c_int, C.c_size_t],
    "rgn_gemm_plan_query": [C.POINTER(C.c_int), _c_int, _c_int, _c_int, _c_int, _c_int, C.c_size_t],
    "rgn_rowband_fork": [_c_void_p],
    "rgn_rowband_join": [_c_void_p],
    "rgn_rowband_query": [C.POINTER(C.c_int), _c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "rgn_rowband_side_launches": [],
    "rgn_last_error": [],
    "rgn_device_info": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)],
    "rgn_arp_partition": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_float, _c_float,
                          _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                          _c_void_p, _c_void_p, _c_void_p],
    "rgn_morph_compact": [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "rgn_gather_rows": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_scatter_rows": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_euler_step": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_float, _c_float, _c_int,
                       _c_int, _c_void_p],
    "rgn_avd_apply": [_c_void_p, _c_int, _c_void_p, _c_float, _c_int, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_cfg_combine": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_float, _c_int, _c_float, _c_int, _c_int, _c_void_p],
    "rgn_gemm_workspace_bytes": [],
    "rgn_gemm_group": [_prob_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_gemv_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int,
                      _c_void_p],
    "rgn_rms_norm_rows": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_silu_bf16": [_c_void_p, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_add_bf16": [_c_void_p, _c_void_p, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_sel_rows": [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p],
    "rgn_fill_zero": [_c_void_p, C.c_size_t, _c_void_p],
    "rgn_ln_modulate": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_int, _c_void_p,
                        _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "rgn_ln_modulate_segs": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_int, C.POINTER(_c_int),
                             C.POINTER(_c_void_p), C.POINTER(_c_void_p), _c_void_p],
    # fp8 activations: row quantiser and the LN-modulate forms that write fp8 rows + row scales (csrc/norm.hip)
    "rgn_quantize_rows_a8": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_ln_modulate_a8": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_float, _c_int, _c_void_p,
                           _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "rgn_ln_modulate_segs_a8": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_float, _c_int, C.POINTER(_c_int),
                                C.POINTER(_c_void_p), C.POINTER(_c_void_p), _c_void_p],
    # mx8 rows: e4m3fn bytes + one E8M0 scale byte per 32 values (x, ldx, q, ldq, s, lds, col0, M, K, stream)
    "rgn_quantize_rows_mx8": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_qk_norm_rope_store": [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p,
                               _c_void_p, _c_void_p, _c_void_p, _c_float, _c_void_p, _c_void_p, _c_void_p,
                               _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p],
    "rgn_attention": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                      _c_float, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_attention_bounded": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                              _c_float, _c_float, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_attention_workspace_bytes": [_c_int, _c_int],
    # f4: VAE decoder (implicit-GEMM convolutions + row kernels, csrc/vae.hip)
    "rgn_conv_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int,
                      _c_void_p, C.POINTER(C.c_int), _c_void_p],
    "rgn_conv_s2_bf16": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p],
    "rgn_conv_up2_bf16": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_void_p,
                          C.POINTER(C.c_int), _c_void_p],
    "rgn_groupnorm_workspace_bytes": [],
    "rgn_groupnorm_partial_bytes": [],
    "rgn_groupnorm_silu": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_float, _c_int, _c_void_p, _c_int, _c_void_p],
    "rgn_upsample2x": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_softmax_rows": [_c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_vae_attention_bf16": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_nchw_to_padded": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_padded_to_nchw": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_padded_to_nchw_cvt": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_rms_norm_silu": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p],
    # f4: text encoders of FLUX.1 Kontext (CLIP-L, T5-XXL; csrc/text.hip)
    "rgn_text_attention_bf16": [_c_void_p, _c_void_p, _c_int, _c_int, _c_float, _c_int, _c_void_p, _c_int, _c_void_p],
    "rgn_text_embed": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p],
    "rgn_geglu_bf16": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_quick_gelu_bf16": [_c_void_p, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_layer_norm_rows": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_text_pool_row": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p],
    # f4: language model of the Qwen2.5-VL prompt encoder (csrc/text.hip)
    "rgn_lm_attention_bf16": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_mrope_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_swiglu_bf16": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    # f4: greedy decode of that language model (csrc/decode.hip)
    "rgn_lm_gemv_bf16": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_lm_gemv_w8": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_lm_kv_append_bf16": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_lm_decode_attention_bf16": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_lm_decode_attention_workspace_bytes": [_c_int, _c_int],
    "rgn_lm_head_argmax": [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_lm_head_workspace_bytes": [_c_int],
    # the same step for B <= 8 sequences from one stream of the weights; per-sequence lengths are host int arrays
    "rgn_lm_gemv_bf16_rows": [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_lm_gemv_w8_rows": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                            _c_void_p],
    "rgn_lm_head_argmax_rows": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p,
                                C.c_size_t, _c_void_p],
    "rgn_lm_kv_append_bf16_rows": [_c_void_p, _c_int, _c_void_p, C.c_size_t, _c_int, C.POINTER(_c_int), _c_int, _c_int, _c_int, _c_void_p],
    "rgn_lm_decode_attention_bf16_rows": [_c_void_p, _c_int, _c_void_p, C.c_size_t, _c_void_p, _c_int, C.POINTER(_c_int), _c_int, _c_int,
                                          _c_int, _c_float, _c_void_p, C.c_size_t, _c_void_p],
    # drafts of one sequence verified in one step (lookup=True)
    "rgn_lm_verify_attention_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_void_p,
                                     C.c_size_t, _c_void_p],
    "rgn_lm_lookup_step": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p,
                           _c_void_p],
    # the same step under sampling and a penalty (lookup_sampling=True): the step's picks, then accept + propose + marks
    "rgn_lm_lookup_step_mark": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p,
                                _c_void_p, _c_int, _c_void_p],
    "rgn_lm_pick_verify": [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, _c_void_p, _c_float, _c_int, _c_float, _c_int, C.c_double, _c_void_p,
                           _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, C.c_size_t, _c_void_p],
    # the wide step: 1 <= B <= 32 rows on the MFMA row GEMM (batch_kernels="mfma")
    "rgn_lm_gemm_rows_bf16": [_c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_lm_gemm_rows_w8": [_c_void_p, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_int,
                            _c_void_p],
    "rgn_lm_head_argmax_wide": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p,
                                C.c_size_t, _c_void_p],
    "rgn_lm_head_wide_workspace_bytes": [_c_int, _c_int],
    "rgn_lm_pick_wide": [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, C.c_size_t, _c_float, _c_int, _c_float, _c_int, C.c_double, _c_void_p,
                         _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_lm_seen_mark": [_c_void_p, _c_int, _c_void_p, _c_int, _c_void_p],
    "rgn_lm_pick": [_c_void_p, _c_int, _c_void_p, _c_float, _c_int, _c_float, _c_int, C.c_double, _c_void_p, _c_void_p, _c_void_p,
                    _c_void_p, C.c_size_t, _c_void_p],
    "rgn_lm_pick_workspace_bytes": [_c_int],
    "rgn_lm_pick_rows": [_c_void_p, _c_int, _c_int, _c_int, _c_void_p, C.c_size_t, _c_float, _c_int, _c_float, _c_int, C.c_double, _c_void_p,
                         _c_void_p, _c_int, _c_void_p, _c_int, _c_void_p, C.c_size_t, _c_void_p],
    # f4: vision tower of the Qwen2.5-VL prompt encoder (csrc/vision.hip)
    "rgn_vision_attention_bf16": [_c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_float, _c_void_p, _c_int, _c_void_p],
    "rgn_vision_rope_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_int, _c_int, _c_void_p],
    "rgn_gelu_erf_bf16": [_c_void_p, _c_void_p, C.c_size_t, _c_void_p],
    "rgn_cast_pad_rows": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    # f4: Step1X-Edit's per-step connector (csrc/connector.hip)
    "rgn_masked_mean_rows": [_c_void_p, _c_int, _c_int, _c_int, _c_int, _c_float, _c_void_p, _c_void_p],
    "rgn_head_rms_norm_bf16": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_float, _c_void_p],
    "rgn_gate_resid_rows": [_c_void_p, _c_int, _c_void_p, _c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _c_void_p],
    # a10: one masked MMDiT block per call (csrc/block.hip)
    "rgn_mmdit_double_block": [_block_p, _c_void_p],
    "rgn_mmdit_single_block": [_block_p, _c_void_p],
    "rgn_mmdit_block_bytes": [],
    # a11: LoRA merge into a bf16 weight at adoption (csrc/lora.hip)
    "rgn_lora_merge_bf16": [_c_void_p, _c_int, _c_void_p, _c_int, _c_int, _c_int, _term_p, _c_int, _c_void_p],
    # a12: image pre- and post-processing, bit-exact with the host's PIL / numpy / torch code (csrc/image.hip)
    "rgn_image_resample_u8": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_image_u8_to_nchw_bf16": [_c_void_p, _c_void_p, _c_int, _c_int, _c_void_p, _c_void_p],
    "rgn_image_patchify_u8": [_c_void_p, _c_int, _c_int, _c_void_p, _c_void_p, _c_int, _c_int, _c_void_p],
    "rgn_image_bf16_to_u8": [_c_void_p, _c_int, _c_int, _c_void_p, _c_int, _c_int, _c_void_p],
}
_RESTYPE = {"rgn_last_error": C.c_char_p, "rgn_abi_struct_bytes": C.c_size_t, "rgn_attention_workspace_bytes": C.c_size_t,
            "rgn_gemm_workspace_bytes": C.c_size_t, "rgn_groupnorm_workspace_bytes": C.c_size_t,
            "rgn_groupnorm_partial_bytes": C.c_size_t, "rgn_lm_decode_attention_workspace_bytes": C.c_size_t,
            "rgn_lm_head_workspace_bytes": C.c_size_t, "rgn_lm_pick_workspace_bytes": C.c_size_t,
            "rgn_lm_head_wide_workspace_bytes": C.c_size_t,
            "rgn_rowband_side_launches": C.c_longlong, "rgn_mmdit_block_bytes": C.c_size_t}

_lib = None


class RegionEHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raise if the native library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RegionEHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); there is no CPU fallback.")
    if os.path.abspath(LIB_PATH) == os.path.abspath(_build.LIB_PATH) and os.path.isdir(_build.CSRC):
        # the in-tree library beside its sources: it must be the build of THESE sources (a stale .so would make every measurement and
        # parity claim about the tree a claim about something else)
        built, now = _build.built_from(), _build.csrc_hash()
        if built and built != now:
            raise RegionEHipError(f"{LIB_PATH} was built from kernel sources {built}, the tree holds {now}: rebuild with "
                                  "`python -m regione_amd.build` (or `__graft_entry__.build()`)")
    h = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(h, name)           # AttributeError if the symbol is missing: loud by design
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, C.c_int)
    # the ctypes mirrors of the structs passed by pointer must be the library's layout (a library built from another header)
    want = C.sizeof(QkvEpilogue) * 1000 + C.sizeof(GemmProblem)
    if h.rgn_abi_struct_bytes() != want:
        raise RegionEHipError(f"{LIB_PATH}: struct layout {h.rgn_abi_struct_bytes()} != the Python binding's {want} "
                              f"(library ABI version {h.rgn_version()}): rebuild with `python -m regione_amd.build --force`")
    if h.rgn_mmdit_block_bytes() != C.sizeof(MmditBlock):
        raise RegionEHipError(f"{LIB_PATH}: sizeof(rgn_mmdit_block) {h.rgn_mmdit_block_bytes()} != the Python binding's {C.sizeof(MmditBlock)}: "
                              "rebuild with `python -m regione_amd.build --force`")
    _lib = h
    return h


import contextlib as _contextlib

PLAN_KEYS = ("gemm_pieces", "gemm_geometry", "gemm_asm", "gemm_quarter", "attn_waves", "attn_split", "attn_streamk", "attn_asm", "rowbands")


@_contextlib.contextmanager
def plan_override(**knobs):
    """Force launch-plan knobs for the duration of a `with` block (rgn_plan_override, include/regione_hip.h) - tests and sweep
    tools only; every knob returns to the value it HAD on exit (nested blocks and an RGN_PLAN_OVERRIDE preset survive).

        with _lib.plan_override(gemm_pieces=3, gemm_geometry=256): ops.gemm(...)"""
    h = lib()
    before = {}
    try:
        for k, v in knobs.items():
            old = C.c_int(-1)
            check(h.rgn_plan_override_get(k.encode(), C.byref(old)), f"rgn_plan_override_get({k})")
            check(h.rgn_plan_override(k.encode(), int(v)), f"rgn_plan_override({k})")
            before[k] = old.value
        yield
    finally:
        for k, old in before.items():
            h.rgn_plan_override(k.encode(), old)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().rgn_last_error().decode(errors="replace")
        raise RegionEHipError(f"{what or 'libregione_hip'} failed (rc={rc}): {msg}")
