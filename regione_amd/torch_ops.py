"""`torch.ops.regione_mi.*` - the hot-path ops registered as PyTorch custom ops.

SURVEY.md section 8(b) names this surface ("exposed to Python through PyTorch-ROCm custom ops"): the same
entry points of libregione_hip.so that `regione_amd.ops` calls through ctypes, registered with
`torch.library` so that they are dispatcher-visible (`torch.ops.regione_mi.arp_partition(...)`), carry
schemas with their mutation annotations (`Tensor(a!)`), and have fake (meta) implementations for tracing.
The native boundary stays the C ABI of include/regione_hip.h; nothing here computes - every op forwards to
the HIP library and raises if it is missing (no CPU fallback).

Two registrations of the SAME schemas (`SCHEMAS` below), mutually exclusive in one process (same operator names):
  * C++ (default when regione_amd/lib/libregione_torch.so is built): `TORCH_LIBRARY(regione_mi, m)` + `TORCH_LIBRARY_IMPL(regione_mi,
    CUDA, m)` in csrc/torch_binding.cpp, linked against libregione_hip.so - `torch.ops.load_library(path)` alone makes
    `torch.ops.regione_mi.*` resolve (C++ / AOT callers need no Python); this module then only adds the fake kernels;
  * Python `torch.library` over the ctypes wrappers (`RGN_TORCH_OPS=py`; the A/B, and the fallback when the C++ library is absent).
`RGN_TORCH_OPS=cpp` insists on the C++ registration (raises when the library is missing), `=0` sends the calls straight to
`regione_amd.ops` (no dispatcher).

This IS the surface the engine runs on: the family patch sets (`regione_amd/<Family>/inplace.py`, `utils.py`) and the
attention processors (`harness/*.py`) call these ops through the dispatcher (`R = torch.ops.regione_mi`); only the
[EXT] block bodies around them (LayerNorm-modulate, FeedForward / out-projection GEMMs) call `regione_amd.ops` directly.
fp8 weights: the per-output-channel scale rides on the weight tensor as a Python attribute (`ops.quantize_w8`), which a C++
kernel cannot see - the projection ops therefore take it as an explicit optional argument (`w_scale`), and the engine-side
accessor `R` fills it in from the attribute.

    import regione_amd.torch_ops            # registers the ops (idempotent)
    e, u, mask = torch.ops.regione_mi.arp_partition(sample, v, cond, dt_final, 0.88, 64, 64, True)

| op | replaces (reference file:line) |
|---|---|
| arp_partition        | token_selector + the one-step estimate, FluxKontext/utils.py:282-354, inplace.py:650-651 |
| gather_rows          | ids_gather, utils.py:260-279 |
| scatter_rows_        | ids_scatter, utils.py:240-257 |
| split_euler_step     | scheduler update incl. the split update of partition / refresh steps, inplace.py:648-680 |
| avd_apply            | `cache = ids_gather(cache, ids); noise_pred = cache * ratio`, inplace.py:315-318 |
| cfg_combine          | inplace.py:364; Step1XEdit/inplace.py:401-410; QwenImageEdit/inplace.py:401-405 |
| kv_partial_update_   | `_partially_linear` x2 + norm_k + RoPE into the K / V^T caches, inplace.py:734-794, fused_kernels.py:81-101 |
| kv_partial_update_pair_ | the same for the two streams of a double-stream block (one launch), inplace.py:734-794 |
| region_attention     | flash_attn_func / SDPA of the edited-token queries against the full cache, inplace.py:796-806 |
| mmdit_double_block_  | one whole masked double-stream block (BLOCK_SCHEMAS), inplace.py:518-524 with :704-824 inside |
| mmdit_single_block_  | one whole masked single-stream block, inplace.py:549-555 with :704-824 inside |
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

import os as _os

NS = "regione_mi"
CPP_LIB = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "lib", "libregione_torch.so")
_mode = _os.environ.get("RGN_TORCH_OPS", "")
if _mode in ("", "1"):
    _mode = "cpp" if _os.path.exists(CPP_LIB) else "py"
if _mode == "cpp":
    if not _os.path.exists(CPP_LIB):
        raise ops._lib.RegionEHipError(f"RGN_TORCH_OPS=cpp but {CPP_LIB} is not built (python -m regione_amd.build)")
    _h = ops._lib.lib()                             # libregione_hip.so first (the binding links against it by $ORIGIN rpath)
    torch.ops.load_library(CPP_LIB)                 # TORCH_LIBRARY(regione_mi) + CUDA kernels: defined by the library itself
    # a binding compiled against another regione_hip.h than the HIP library next to it would misread the structs it passes by
    # pointer (advisor finding, round 4): both carry the header's ABI stamp - compare before any op can run
    import ctypes as _C
    _b = _C.CDLL(CPP_LIB)
    _b.rgn_torch_binding_struct_bytes.restype = _C.c_size_t
    if (_b.rgn_torch_binding_abi_version(), _b.rgn_torch_binding_struct_bytes()) != (_h.rgn_version(), _h.rgn_abi_struct_bytes()):
        raise ops._lib.RegionEHipError(
            f"{CPP_LIB} was built against ABI {_b.rgn_torch_binding_abi_version()} / struct bytes {_b.rgn_torch_binding_struct_bytes()}, "
            f"libregione_hip.so is {_h.rgn_version()} / {_h.rgn_abi_struct_bytes()}: rebuild (python -m regione_amd.build --force)")
    _b.rgn_torch_binding_block_bytes.restype = _C.c_size_t
    if _b.rgn_torch_binding_block_bytes() != _h.rgn_mmdit_block_bytes():
        raise ops._lib.RegionEHipError(
            f"{CPP_LIB} was built with sizeof(rgn_mmdit_block) = {_b.rgn_torch_binding_block_bytes()}, libregione_hip.so has "
            f"{_h.rgn_mmdit_block_bytes()}: rebuild (python -m regione_amd.build --force)")
    _lib = None
else:
    _lib = torch.library.Library(NS, "FRAGMENT")   # (the dispatcher omits trailing arguments that equal their schema default:
    # every implementation below therefore repeats the defaults)
REGISTRATION = {"cpp": "cpp", "py": "py"}.get(_mode, "py")      # which one this process holds ("0" still registers py)
_defined = set()
SCHEMAS = {}


ROW_SCHEMAS = {}                # the row kernels of the Step1X connector: registered alike, listed apart (SCHEMAS is the region-op surface)
_row_defined = set()


def _define(name: str, schema: str, impl, fake, schemas=SCHEMAS, names=_defined):
    if name in names:
        return
    schemas[name] = schema
    if _lib is not None:
        _lib.define(f"{name}{schema}")
        torch.library.impl(_lib, name, "CUDA")(impl)
    torch.library.register_fake(f"{NS}::{name}")(fake)
    names.add(name)


# ---- region ops ---------------------------------------------------------------------------------
def _arp(sample, model_output, cond, dt_final, threshold, h_tok, w_tok, erosion_dilation=True):
    e, u, mask, _, _ = ops.arp_partition(sample, model_output, cond, dt_final, threshold, h_tok, w_tok, erosion_dilation)
    return e, u, mask


def _arp_fake(sample, model_output, cond, dt_final, threshold, h_tok, w_tok, erosion_dilation=True):
    L = h_tok * w_tok
    k = torch.library.get_ctx().new_dynamic_size()          # K_e is data dependent
    return (sample.new_empty((1, k), dtype=torch.int64), sample.new_empty((1, L - k), dtype=torch.int64),
            sample.new_empty((L,), dtype=torch.uint8))


_define("arp_partition",
        "(Tensor sample, Tensor? model_output, Tensor cond, float dt_final, float threshold, int h_tok, int w_tok, "
        "bool erosion_dilation=True) -> (Tensor, Tensor, Tensor)", _arp, _arp_fake)

_define("gather_rows", "(Tensor x, Tensor ids) -> Tensor", ops.gather_rows,
        lambda x, ids: x.new_empty((1, ids.numel(), x.shape[-1]) if x.dim() == 3 else (ids.numel(), x.shape[-1])))


def _scatter(src, ids, dst):
    ops.scatter_rows_(src, ids, dst)


_define("scatter_rows_", "(Tensor src, Tensor ids, Tensor(a!) dst) -> ()", _scatter, lambda src, ids, dst: None)

_define("split_euler_step", "(Tensor sample, Tensor v, float dt, Tensor? mask=None, float dt_direct=0.0) -> Tensor",
        lambda sample, v, dt, mask=None, dt_direct=0.0: ops.euler_step(sample, v, dt, mask, dt_direct),
        lambda sample, v, dt, mask=None, dt_direct=0.0: torch.empty_like(v))

_define("avd_apply", "(Tensor cache, float ratio, Tensor? ids=None, bool round_ratio=False) -> Tensor",
        lambda cache, ratio, ids=None, round_ratio=False: ops.avd_apply(cache, ratio, ids, round_ratio),
        lambda cache, ratio, ids=None, round_ratio=False: (
            torch.empty_like(cache) if ids is None else
            cache.new_empty((1, ids.numel(), cache.shape[-1]) if cache.dim() == 3 else (ids.numel(), cache.shape[-1]))))

_define("cfg_combine", "(Tensor pos, Tensor neg, float scale, int mode=0, float power=0.4) -> Tensor",
        lambda pos, neg, scale, mode=0, power=0.4: ops.cfg_combine(pos, neg, scale, mode, power),
        lambda pos, neg, scale, mode=0, power=0.4: torch.empty_like(pos))


# ---- Region-Instruction KV cache ------------------------------------------------------------------
def _epi(x, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, row_base, eps, fp16_roundtrip):
    d = heads * 128
    return ops.qkv_epilogue(wq=norm_q, wk=norm_k, rope_q=(cos_q, sin_q), rope_k=(cos_k, sin_k), k_slab=k_cache,
                            vt_slab=vt_cache, H=heads, k_col=0, v_col=d, q_col=2 * d, kv_rows=kv_rows, row_base=row_base,
                            eps=eps, fp16_roundtrip=fp16_roundtrip, rows=x.shape[0])


def _scaled(w, w_scale):
    """An fp8 weight whose scale arrived as an explicit argument (a caller without the Python attribute) gets it attached."""
    if w_scale is not None and getattr(w, "_rgn_scale", None) is None:
        w._rgn_scale = w_scale
    return w


def _kv_update(x, w_kvq, b_kvq, q_out, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, row_base=0,
               eps=1e-6, fp16_roundtrip=False, gelu_from_col=-1, w_scale=None):
    w_kvq = _scaled(w_kvq, w_scale)
    epi = _epi(x, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, row_base, eps, fp16_roundtrip)
    ops.gemm_qkv(x, w_kvq, b_kvq, q_out, epi, gelu_from_col=3 * heads * 128 if gelu_from_col < 0 else gelu_from_col)


_define("kv_partial_update_",
        "(Tensor x, Tensor w_kvq, Tensor? b_kvq, Tensor(a!) q_out, Tensor norm_q, Tensor norm_k, Tensor cos_q, Tensor sin_q, "
        "Tensor cos_k, Tensor sin_k, Tensor? kv_rows, Tensor(b!) k_cache, Tensor(c!) vt_cache, int heads, int row_base=0, "
        "float eps=1e-6, bool fp16_roundtrip=False, int gelu_from_col=-1, Tensor? w_scale=None) -> ()", _kv_update, lambda *a, **k: None)


def _kv_update_pair(x_img, w_img, b_img, out_img, norm_q_img, norm_k_img, x_txt, w_txt, b_txt, out_txt, norm_q_txt, norm_k_txt,
                    cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, txt_len, eps=1e-6, fp16_roundtrip=False,
                    w_scale_img=None, w_scale_txt=None):
    w_img, w_txt = _scaled(w_img, w_scale_img), _scaled(w_txt, w_scale_txt)
    e_img = _epi(x_img, norm_q_img, norm_k_img, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, txt_len, eps, fp16_roundtrip)
    e_txt = _epi(x_txt, norm_q_txt, norm_k_txt, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, 0, eps, False)
    ops.gemm_qkv_pair(x_img, w_img, b_img, out_img, e_img, x_txt, w_txt, b_txt, out_txt, e_txt)


# both streams of a double-stream block in one launch: image rows sit behind the `txt_len` text rows of the shared
# [text ; image] sequence (cache rows, rotary rows); only the image rows are ever partial (fp16 round trip, quirk A-3)
_define("kv_partial_update_pair_",
        "(Tensor x_img, Tensor w_img, Tensor? b_img, Tensor(a!) out_img, Tensor norm_q_img, Tensor norm_k_img, "
        "Tensor x_txt, Tensor w_txt, Tensor? b_txt, Tensor(b!) out_txt, Tensor norm_q_txt, Tensor norm_k_txt, "
        "Tensor cos_q, Tensor sin_q, Tensor cos_k, Tensor sin_k, Tensor? kv_rows, Tensor(c!) k_cache, Tensor(d!) vt_cache, "
        "int heads, int txt_len, float eps=1e-6, bool fp16_roundtrip=False, Tensor? w_scale_img=None, Tensor? w_scale_txt=None) -> ()",
        _kv_update_pair, lambda *a, **k: None)


def _kv_update_group(x, w, w_scale, b, out, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads, row_base,
                     eps=1e-6, fp16_roundtrip=(), gelu_from_col=-1):
    rt = list(fp16_roundtrip) or [False] * len(x)
    if len(w_scale):
        w = [_scaled(wi, si) for wi, si in zip(w, w_scale)]
    probs = [ops.Problem(x[i], w[i], b[i], out[i],
                         epi=_epi(x[i], norm_q[i], norm_k[i], cos_q[i], sin_q[i], cos_k[i], sin_k[i], kv_rows[i], k_cache[i], vt_cache[i],
                                  heads, int(row_base[i]), eps, bool(rt[i]))) for i in range(len(x))]
    ops.gemm_group(probs, epilogue=3, gelu_from_col=0 if gelu_from_col < 0 else gelu_from_col)


# the projections of up to four (stream, CFG branch) problems in ONE launch: per problem its activations, weights (shared
# between the branches of a stream), RMSNorm weights, rotary tables, cache-row list and K / V^T cache (one per branch)
_define("kv_partial_update_group_",
        "(Tensor[] x, Tensor[] w_kvq, Tensor?[] w_scale, Tensor?[] b_kvq, Tensor(a!)[] q_out, Tensor[] norm_q, Tensor[] norm_k, "
        "Tensor[] cos_q, Tensor[] sin_q, Tensor[] cos_k, Tensor[] sin_k, Tensor?[] kv_rows, Tensor(b!)[] k_cache, Tensor(c!)[] vt_cache, "
        "int heads, int[] row_base, float eps=1e-6, int[] fp16_roundtrip=[], int gelu_from_col=-1) -> ()", _kv_update_group,
        lambda *a, **k: None)


def _region_attention(q, k_cache, vt_cache, out, skv, heads, scale=-1.0, score_bound=0.0):
    ops.attention(q, k_cache, vt_cache, out, skv, heads, scale if scale > 0 else None, score_bound=score_bound)


_define("region_attention",
        "(Tensor q, Tensor k_cache, Tensor vt_cache, Tensor(a!) out, int skv, int heads, float scale=-1.0, float score_bound=0.0) -> ()",
        _region_attention, lambda *a, **k: None)


def _workspace(like, kind):
    return ops.gemm_workspace(like.device) if kind == 0 else ops.attention_workspace(like.device)


# the scratch lane (kind 0 = GEMM split-K partials, 1 = attention KV-split partials) of `like`'s device and current stream: ONE
# provider for both ways a launch reaches the library (C++ ops and the ctypes wrappers)
_define("workspace", "(Tensor like, int kind) -> Tensor", _workspace,
        lambda like, kind: like.new_empty((1,), dtype=torch.float32))


# ---- Step1X-Edit connector row kernels (csrc/connector.hip) -----------------------------------------
def _head_rms_norm(qkv, wq, wk, heads, eps=1e-6):
    ops.head_rms_norm_(qkv, wq, wk, heads, eps)


def _gate_resid_rows(p, gate, resid, out):
    ops.gate_resid_rows(p, gate, resid, out)


_define("masked_mean_rows", "(Tensor x, int n_valid, float scale=1.0) -> Tensor",
        lambda x, n_valid, scale=1.0: ops.masked_mean_rows(x, n_valid, scale),
        lambda x, n_valid, scale=1.0: x.new_empty((x.shape[1],)), ROW_SCHEMAS, _row_defined)
_define("head_rms_norm_", "(Tensor(a!) qkv, Tensor wq, Tensor wk, int heads, float eps=1e-6) -> ()", _head_rms_norm,
        lambda *a, **k: None, ROW_SCHEMAS, _row_defined)
_define("gate_resid_rows_", "(Tensor p, Tensor gate, Tensor resid, Tensor(a!) out) -> ()", _gate_resid_rows,
        lambda *a, **k: None, ROW_SCHEMAS, _row_defined)


# ---- fp8 activations: the row quantiser (csrc/norm.hip) -----------------------------------------------
A8_SCHEMAS = {}                 # listed apart like ROW_SCHEMAS: SCHEMAS stays the region-op surface
_a8_defined = set()


def _quantize_rows_a8(x):
    q = ops.quantize_rows_a8(x)
    return q, q._rgn_scale


# x bf16 [M, K] -> (fp8 e4m3fn [M, K], fp32 row scales [M]); a caller attaches the scales (`q._rgn_scale = scale`) before ops.gemm
_define("quantize_rows_a8", "(Tensor x) -> (Tensor, Tensor)", _quantize_rows_a8,
        lambda x: (x.new_empty(x.shape, dtype=ops.FP8), x.new_empty((x.shape[0],), dtype=torch.float32)), A8_SCHEMAS, _a8_defined)


def _quantize_rows_mx8(x):
    q = ops.quantize_rows_mx8(x)
    return q, q._rgn_mx_scale


# x bf16 [M, K], K % 128 == 0 -> (fp8 e4m3fn [M, K], E8M0 block scales uint8 [M, K / 32]): "mx8 rows" of include/regione_hip.h; a caller
# attaches the scales (`q._rgn_mx_scale = s`).  Writing into columns of a wider buffer is ops.quantize_rows_mx8(x, out=, col=).
_define("quantize_rows_mx8", "(Tensor x) -> (Tensor, Tensor)", _quantize_rows_mx8,
        lambda x: (x.new_empty(x.shape, dtype=ops.FP8), x.new_empty((x.shape[0], x.shape[1] // 32), dtype=torch.uint8)),
        A8_SCHEMAS, _a8_defined)


# ---- one masked MMDiT block per call (csrc/block.hip) ------------------------------------------------
BLOCK_SCHEMAS = {}              # listed apart like ROW_SCHEMAS: SCHEMAS stays the region-op surface
_block_defined = set()
_BLOCK_TAIL = ("Tensor[] weights, Tensor?[] scales, Tensor?[] biases, Tensor[] norms, Tensor cos_q, Tensor sin_q, Tensor cos_k, Tensor sin_k, "
               "Tensor? kv_rows, Tensor(d!) k_cache, Tensor(e!) vt_cache, int T, int M, int heads, int skv, float score_bound, "
               "bool rowbands=False) -> ()")
DOUBLE_WEIGHTS = ("w_kvq", "w_add_kvq", "w_out", "w_add_out", "ff_w1", "ffc_w1", "ff_w2", "ffc_w2")     # order of `weights` / `scales` / `biases`
SINGLE_WEIGHTS = ("w_kvqm", "w_po")


def _need(ok, op, msg):
    if not ok:
        raise ops._lib.RegionEHipError(f"{op}: {msg}")


def _block_desc(op, x, nrm, wide, d_ff, names, shapes, weights, scales, biases, norms, n_norms, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache,
                vt_cache, T, M, heads, skv, score_bound, rowbands):
    """The extent checks of csrc/torch_binding.cpp:block_common / block_weight, then struct rgn_mmdit_block; returns (descriptor, keep-alive)."""
    L = ops._lib
    bf, dev = torch.bfloat16, x.device
    _need(x.is_cuda, op, "needs CUDA/HIP tensors: there is no CPU fallback")
    _need(heads > 0 and T >= 0 and M > 0, op, "heads > 0, T >= 0, M > 0")
    d, R = heads * 128, T + M
    _need(d_ff > 0, op, "d_ff must be positive")
    for t in (x, nrm, wide):
        _need(t.device == dev and t.dtype == bf and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= R, op,
              f"x / nrm / wide must be bf16 [>= T + M = {R} rows, cols] with unit column stride on one device")
    for t in (x, nrm, wide):                 # the descriptor carries row strides as int
        _need(t.shape[1] <= t.stride(0) < 2 ** 31, op, f"row stride {t.stride(0)} of x / nrm / wide out of range")
    _need(x.shape[1] == d and nrm.shape[1] == d, op, f"x / nrm need heads * 128 = {d} columns")
    _need(wide.shape[1] == 3 * d + d_ff, op, f"wide needs 3 d + d_ff = {3 * d + d_ff} columns [k | v | q | mlp], got {wide.shape[1]}")
    n = len(names)
    _need(len(weights) == n and len(scales) in (0, n) and len(biases) == n, op, f"{n} weights, {n} (or no) scales, {n} biases")
    ws = []
    for i, (name, (N, K)) in enumerate(zip(names, shapes)):
        w, sc, b = weights[i], (scales[i] if len(scales) else None), biases[i]
        _need(w.device == dev and tuple(w.shape) == (N, K) and w.is_contiguous() and w.dtype in (bf, ops.FP8), op,
              f"{name} must be a contiguous bf16 or fp8 [{N}, {K}] on the activations' device")
        _need((w.dtype == ops.FP8) == (sc is not None), op, f"{name}: an fp8 weight needs its per-output-channel scale, a bf16 weight takes none")
        _need(sc is None or (sc.dtype == torch.float32 and sc.numel() == N and sc.is_contiguous() and sc.device == dev), op,
              f"scale of {name} must be fp32 [{N}], contiguous")
        _need(b is None or (b.dtype == bf and b.dim() == 1 and b.numel() == N and b.is_contiguous() and b.device == dev), op,
              f"bias of {name} must be bf16 [{N}], contiguous")
        ws.append(L.BlockWeight(ops._p(w), ops._p(sc), ops._p(b)))
    _need(len(norms) == n_norms, op, f"{n_norms} per-head RMSNorm weight vectors")
    for t in norms:
        _need(t.device == dev and t.dtype == bf and t.numel() == 128 and t.is_contiguous(), op, "per-head RMSNorm weights: bf16 [128]")
    _need(cos_q.shape == sin_q.shape and cos_k.shape == sin_k.shape, op, "cos / sin of one rotary table differ in shape")
    for t in (cos_q, sin_q, cos_k, sin_k):
        _need(t.device == dev and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 128 and t.is_contiguous(), op,
              "rotary tables: fp32 [rows, 128], contiguous, on the activations' device")
    _need(cos_q.shape[0] >= R, op, f"rotary table of the queries has {cos_q.shape[0]} rows, the block needs {R}")
    _need(k_cache.device == dev and vt_cache.device == dev and k_cache.dtype == bf and vt_cache.dtype == bf and k_cache.dim() == 2 and
          vt_cache.dim() == 2 and k_cache.shape[1] == d and vt_cache.shape[0] == d and vt_cache.shape[1] == k_cache.shape[0] and
          k_cache.is_contiguous() and vt_cache.is_contiguous() and k_cache.shape[0] % 64 == 0, op,
          "K slab bf16 [skv_pad, d] / V^T slab bf16 [d, skv_pad], contiguous, skv_pad a multiple of 64")
    skv_pad = k_cache.shape[0]
    _need(1 <= skv <= skv_pad, op, f"skv = {skv} outside the cache slab's {skv_pad} rows")
    if kv_rows is not None:
        _need(kv_rows.device == dev and kv_rows.dtype == torch.int64 and kv_rows.dim() == 1 and kv_rows.is_contiguous() and kv_rows.numel() == R,
              op, f"kv_rows must be int64 [T + M = {R}], contiguous")
        _need(cos_k.shape[0] >= skv >= R, op, f"the key rotary table ({cos_k.shape[0]} rows) must cover the {skv} cache rows, which must hold "
                                              f"the {R} distinct rows kv_rows names")
    else:
        _need(R <= skv, op, f"identity cache rows [0, {R}) exceed skv = {skv}")
        _need(cos_k.shape[0] >= R, op, f"rotary table of the keys has {cos_k.shape[0]} rows, the block needs {R}")
    gws, aws = ops.gemm_workspace(dev), ops.attention_workspace(dev)
    b = L.MmditBlock()
    b.x, b.nrm, b.wide = ops._p(x), ops._p(nrm), ops._p(wide)
    b.ldx, b.ldnrm, b.ldwide = x.stride(0), nrm.stride(0), wide.stride(0)
    b.T, b.M, b.d, b.d_ff, b.heads = T, M, d, d_ff, heads
    for name, w in zip(names, ws):
        setattr(b, name, w)
    for name, t in zip(("norm_q", "norm_k", "norm_added_q", "norm_added_k"), norms):
        setattr(b, name, ops._p(t))
    b.k_slab, b.vt_slab, b.kv_rows = ops._p(k_cache), ops._p(vt_cache), ops._p(kv_rows)
    b.cos_q, b.sin_q, b.cos_k, b.sin_k = ops._p(cos_q), ops._p(sin_q), ops._p(cos_k), ops._p(sin_k)
    b.skv, b.skv_pad, b.score_bound, b.rowbands, b.out_rows, b.branches = skv, skv_pad, float(score_bound), int(bool(rowbands)), 0, 1
    b.gemm_ws, b.gemm_ws_bytes, b.attn_ws, b.attn_ws_bytes = ops._p(gws), gws.numel() * 4, ops._p(aws), aws.numel() * 4
    return b, (gws, aws)


def _adaln(op, v, like, n):
    _need(v.device == like.device and v.dtype == torch.bfloat16 and v.is_contiguous() and v.numel() == n, op,
          f"AdaLN vector must be bf16 [{n}], contiguous, on the activations' device (got {v.numel()} elements)")
    return ops._p(v)


def _double_block(x, nrm, wide, adaln_img, adaln_txt, weights, scales, biases, norms, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache,
                  T, M, heads, skv, score_bound, rowbands=False):
    import ctypes
    op = "mmdit_double_block_"
    _need(len(weights) == 8 and weights[4].dim() == 2, op, "8 weights, ff_w1 = [d_ff, d]")
    d, ff = heads * 128, weights[4].shape[0]
    shapes = ((3 * d, d), (3 * d, d), (d, d), (d, d), (ff, d), (ff, d), (d, ff), (d, ff))
    b, keep = _block_desc(op, x, nrm, wide, ff, DOUBLE_WEIGHTS, shapes, weights, scales, biases, norms, 4, cos_q, sin_q, cos_k, sin_k, kv_rows,
                          k_cache, vt_cache, T, M, heads, skv, score_bound, rowbands)
    b.adaln, b.adaln_txt = _adaln(op, adaln_img, x, 6 * d), _adaln(op, adaln_txt, x, 6 * d)
    ops._lib.check(ops._lib.lib().rgn_mmdit_double_block(ctypes.byref(b), ops._stream()), "rgn_mmdit_double_block")


def _single_block(x, nrm, wide, adaln, weights, scales, biases, norms, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, T, M, heads, skv,
                  score_bound, rowbands=False):
    import ctypes
    op = "mmdit_single_block_"
    _need(len(weights) == 2 and weights[1].dim() == 2, op, "2 weights, w_po = [d, d + d_ff]")
    d = heads * 128
    ff = weights[1].shape[1] - d
    b, keep = _block_desc(op, x, nrm, wide, ff, SINGLE_WEIGHTS, ((3 * d + ff, d), (d, d + ff)), weights, scales, biases, norms, 2, cos_q, sin_q,
                          cos_k, sin_k, kv_rows, k_cache, vt_cache, T, M, heads, skv, score_bound, rowbands)
    b.adaln = _adaln(op, adaln, x, 3 * d)
    ops._lib.check(ops._lib.lib().rgn_mmdit_single_block(ctypes.byref(b), ops._stream()), "rgn_mmdit_single_block")


_define("mmdit_double_block_", "(Tensor(a!) x, Tensor(b!) nrm, Tensor(c!) wide, Tensor adaln_img, Tensor adaln_txt, " + _BLOCK_TAIL,
        _double_block, lambda *a, **k: None, BLOCK_SCHEMAS, _block_defined)
_define("mmdit_single_block_", "(Tensor(a!) x, Tensor(b!) nrm, Tensor(c!) wide, Tensor adaln, " + _BLOCK_TAIL,
        _single_block, lambda *a, **k: None, BLOCK_SCHEMAS, _block_defined)


def registered() -> Tuple[str, ...]:
    return tuple(sorted(_defined))


def registered_row_ops() -> Tuple[str, ...]:
    return tuple(sorted(_row_defined))


def registered_block_ops() -> Tuple[str, ...]:
    return tuple(sorted(_block_defined))


def registered_a8_ops() -> Tuple[str, ...]:
    return tuple(sorted(_a8_defined))


def _sc(w):
    return ops._wscale(w)


def _scales(weights):
    sc = [_sc(w) for w in weights]
    return sc if any(s is not None for s in sc) else []


class _Dispatched:
    """The engine-side accessor of the registered ops (`R.<op>(...)` = `torch.ops.regione_mi.<op>(...)`): identical for both
    registrations; the three projection ops get the fp8 per-channel scale that rides on the weight tensor passed explicitly."""

    def __getattr__(self, name):
        return getattr(getattr(torch.ops, NS), name)

    @staticmethod
    def kv_partial_update_(x, w_kvq, *a, **kw):
        s = _sc(w_kvq)
        if s is not None:
            kw["w_scale"] = s
        return torch.ops.regione_mi.kv_partial_update_(x, w_kvq, *a, **kw)

    @staticmethod
    def kv_partial_update_pair_(x_img, w_img, b_img, out_img, nq_img, nk_img, x_txt, w_txt, *a, **kw):
        s0, s1 = _sc(w_img), _sc(w_txt)
        if s0 is not None or s1 is not None:
            kw.update(w_scale_img=s0, w_scale_txt=s1)
        return torch.ops.regione_mi.kv_partial_update_pair_(x_img, w_img, b_img, out_img, nq_img, nk_img, x_txt, w_txt, *a, **kw)

    @staticmethod
    def kv_partial_update_group_(x, w_kvq, b_kvq, q_out, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows, k_cache, vt_cache, heads,
                                 row_base, eps=1e-6, fp16_roundtrip=(), gelu_from_col=-1):
        sc = [_sc(w) for w in w_kvq]
        return torch.ops.regione_mi.kv_partial_update_group_(
            x, w_kvq, sc if any(s is not None for s in sc) else [], b_kvq, q_out, norm_q, norm_k, cos_q, sin_q, cos_k, sin_k, kv_rows,
            k_cache, vt_cache, heads, row_base, eps, [int(bool(f)) for f in fp16_roundtrip], gelu_from_col)

    # the block ops take the weights as a list: the scales that ride on fp8 weights go in a list beside it
    @staticmethod
    def mmdit_double_block_(x, nrm, wide, adaln_img, adaln_txt, weights, biases, *a, **kw):
        return torch.ops.regione_mi.mmdit_double_block_(x, nrm, wide, adaln_img, adaln_txt, weights, _scales(weights), biases, *a, **kw)

    @staticmethod
    def mmdit_single_block_(x, nrm, wide, adaln, weights, biases, *a, **kw):
        return torch.ops.regione_mi.mmdit_single_block_(x, nrm, wide, adaln, weights, _scales(weights), biases, *a, **kw)


class _Direct:
    """`RGN_TORCH_OPS=0`: the same names bound straight to regione_amd.ops (no dispatcher) - A/B switch only."""
    arp_partition = staticmethod(_arp)
    gather_rows = staticmethod(ops.gather_rows)
    scatter_rows_ = staticmethod(_scatter)
    split_euler_step = staticmethod(lambda sample, v, dt, mask=None, dt_direct=0.0: ops.euler_step(sample, v, dt, mask, dt_direct))
    avd_apply = staticmethod(ops.avd_apply)
    cfg_combine = staticmethod(ops.cfg_combine)
    kv_partial_update_ = staticmethod(_kv_update)
    kv_partial_update_pair_ = staticmethod(_kv_update_pair)
    region_attention = staticmethod(_region_attention)

    @staticmethod
    def kv_partial_update_group_(x, w_kvq, b_kvq, *a, **kw):
        return _kv_update_group(x, w_kvq, [], b_kvq, *a, **kw)

    @staticmethod
    def mmdit_double_block_(x, nrm, wide, adaln_img, adaln_txt, weights, biases, *a, **kw):
        return _double_block(x, nrm, wide, adaln_img, adaln_txt, weights, _scales(weights), biases, *a, **kw)

    @staticmethod
    def mmdit_single_block_(x, nrm, wide, adaln, weights, biases, *a, **kw):
        return _single_block(x, nrm, wide, adaln, weights, _scales(weights), biases, *a, **kw)


R = _Direct if _mode == "0" else _Dispatched()
Direct = _Direct        # the engine's fp8-activation trunks: their projections read fp8 rows + row scales, which the registered ops
                        # (bf16 rows by schema) do not take - the same rgn_gemm_group launches through regione_amd.ops
