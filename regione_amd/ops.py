"""Tensor-level wrappers over the C ABI (include/regione_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every arithmetic op of the hot
path runs in libregione_hip.so.  Wrappers pass raw device pointers + the current stream; they never
synchronise except where a host-visible count is explicitly requested.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch

from . import _lib

F32, BF16 = 0, 1
EPI_BIAS, EPI_GELU, EPI_GATE_RESID, EPI_QKV = 0, 1, 2, 3


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype} (fp32 / bf16 only)")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.RegionEHipError("regione_amd ops need CUDA/HIP tensors: there is no CPU fallback")
    return t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[1,L,D] or [L,D] -> contiguous [L,D] view."""
    if t.dim() == 3:
        assert t.shape[0] == 1, "region ops are per image (reference is batch-1, quirk A-5)"
        t = t[0]
    assert t.is_contiguous()
    return t


def padded(n: int, m: int = 64) -> int:
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------
# region ops
# ---------------------------------------------------------------------------------------------
def arp_partition(sample: torch.Tensor, model_output: Optional[torch.Tensor], cond: torch.Tensor,
                  dt_final: float, threshold: float, h_tok: int, w_tok: int, erosion_dilation: bool = True,
                  want_sim: bool = False):
    """token_selector + one-step estimate.  Returns (edited_ids i64[1,K], unedited_ids i64[1,L-K],
    mask u8[L], raw u8[L], sim f32[L] or None).  ONE 4-byte D2H read (K_e) - the only host sync the
    partition needs; every later launch of the image is shape-static."""
    s, c = _rows(sample), _rows(cond)
    mo = _rows(model_output) if model_output is not None else None
    L, D = s.shape
    dev = s.device
    if c.shape != s.shape or (mo is not None and mo.shape != s.shape) or h_tok * w_tok != L:
        raise _lib.RegionEHipError(f"arp_partition: sample {tuple(s.shape)}, model_output {None if mo is None else tuple(mo.shape)}, cond "
                                   f"{tuple(c.shape)} must all be [L, D] with L = h_tok * w_tok = {h_tok * w_tok}")
    e = torch.empty(L, dtype=torch.int64, device=dev)
    u = torch.empty(L, dtype=torch.int64, device=dev)
    raw = torch.empty(L, dtype=torch.uint8, device=dev)
    mask = torch.empty(L, dtype=torch.uint8, device=dev)
    sim = torch.empty(L, dtype=torch.float32, device=dev) if want_sim else None
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().rgn_arp_partition(_p(s), _dt(s), _p(mo), _dt(mo) if mo is not None else F32, _p(c), _dt(c),
                                      float(dt_final), float(threshold), L, D, h_tok, w_tok, int(erosion_dilation),
                                      _p(e), _p(u), _p(raw), _p(mask), _p(sim), _p(cnt), _stream())
    _lib.check(rc, "rgn_arp_partition")
    k = int(cnt.item())
    return e[:k].unsqueeze(0), u[: L - k].unsqueeze(0), mask, raw, sim


def morph_compact(raw_mask: torch.Tensor, erosion_dilation: bool = True):
    h, w = raw_mask.shape
    L = h * w
    dev = raw_mask.device
    e = torch.empty(L, dtype=torch.int64, device=dev)
    u = torch.empty(L, dtype=torch.int64, device=dev)
    mask = torch.empty(L, dtype=torch.uint8, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    rc = _lib.lib().rgn_morph_compact(_p(raw_mask.contiguous()), h, w, int(erosion_dilation), _p(e), _p(u), _p(mask),
                                      _p(cnt), _stream())
    _lib.check(rc, "rgn_morph_compact")
    k = int(cnt.item())
    return e[:k], u[: L - k], mask.view(h, w)


def gather_rows(x: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """ids_gather for [1,L,D] x, [1,K] ids -> [1,K,D]."""
    src = _rows(x)
    idv = ids.reshape(-1).contiguous()
    K = idv.numel()
    out = torch.empty((K, src.shape[1]), dtype=src.dtype, device=src.device)
    rc = _lib.lib().rgn_gather_rows(_p(src), _p(idv), _p(out), K, src.shape[1] * src.element_size(), _stream())
    _lib.check(rc, "rgn_gather_rows")
    return out.unsqueeze(0) if x.dim() == 3 else out


def scatter_rows_(src: torch.Tensor, ids: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """ids_scatter: dst[ids[k]] = src[k] in place; returns dst."""
    s, d = _rows(src), _rows(dst)
    idv = ids.reshape(-1).contiguous()
    if idv.dtype != torch.int64 or idv.numel() > s.shape[0] or s.shape[1] != d.shape[1] or s.dtype != d.dtype:
        raise _lib.RegionEHipError(f"scatter_rows_: {idv.numel()} {idv.dtype} ids for {s.shape[0]} source rows of width {s.shape[1]} -> {d.shape[1]}")
    rc = _lib.lib().rgn_scatter_rows(_p(s), _p(idv), _p(d), idv.numel(), s.shape[1] * s.element_size(), _stream())
    _lib.check(rc, "rgn_scatter_rows")
    return dst


def euler_step(sample: torch.Tensor, v: torch.Tensor, dt: float, mask: Optional[torch.Tensor] = None,
               dt_direct: float = 0.0) -> torch.Tensor:
    s, vv = _rows(sample), _rows(v)
    if mask is not None and (mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != s.shape[0]):
        raise _lib.RegionEHipError("euler_step: mask must be uint8 [L] (the third result of arp_partition)")
    out = torch.empty_like(vv)
    rc = _lib.lib().rgn_euler_step(_p(s), _dt(s), _p(vv), _dt(vv), _p(out), _p(mask), float(dt), float(dt_direct),
                                   s.shape[0], s.shape[1], _stream())
    _lib.check(rc, "rgn_euler_step")
    return out.unsqueeze(0) if v.dim() == 3 else out


def avd_apply(cache: torch.Tensor, ratio: float, ids: Optional[torch.Tensor] = None,
              round_ratio: bool = False) -> torch.Tensor:
    c = _rows(cache)
    if ids is not None and ids.dtype != torch.int64:
        raise _lib.RegionEHipError("avd_apply: ids must be int64")        # the kernel reads 8-byte indices
    idv = ids.reshape(-1).contiguous() if ids is not None else None
    K = idv.numel() if idv is not None else c.shape[0]
    out = torch.empty((K, c.shape[1]), dtype=c.dtype, device=c.device)
    rc = _lib.lib().rgn_avd_apply(_p(c), _dt(c), _p(idv), float(ratio), int(round_ratio), _p(out), K, c.shape[1],
                                  _stream())
    _lib.check(rc, "rgn_avd_apply")
    return out.unsqueeze(0) if cache.dim() == 3 else out


CFG_PLAIN, CFG_STEP1X_RESCALE, CFG_QWEN_NORM = 0, 1, 2


def cfg_combine(pos: torch.Tensor, neg: torch.Tensor, scale: float, mode: int = CFG_PLAIN, power: float = 0.4) -> torch.Tensor:
    p, n = _rows(pos), _rows(neg)
    out = torch.empty_like(p)
    rc = _lib.lib().rgn_cfg_combine(_p(p), _p(n), _p(out), _dt(p), float(scale), mode, float(power), p.shape[0],
                                    p.shape[1], _stream())
    _lib.check(rc, "rgn_cfg_combine")
    return out.unsqueeze(0) if pos.dim() == 3 else out


# ---------------------------------------------------------------------------------------------
# MMDiT block kernels
# ---------------------------------------------------------------------------------------------
_gemm_ws = {}
MAX_WS_LANES = 4          # scratch lanes kept per kind (device x stream), least recently used dropped


def _shared_lane(device, kind: int):
    """With the C++ registration active its lane table is the one provider (torch.ops.regione_mi.workspace): the block-body GEMMs
    launched from here share the buffer the fused projections use on the same stream.  None -> the Python table below."""
    import sys
    to = sys.modules.get("regione_amd.torch_ops")
    if to is None or getattr(to, "REGISTRATION", "py") != "cpp":
        return None
    probes = _shared_lane.__dict__.setdefault("probes", {})
    like = probes.get(str(device))
    if like is None:
        like = probes[str(device)] = torch.empty(0, dtype=torch.float32, device=device)
    return torch.ops.regione_mi.workspace(like, kind)


def _ws_lane(table: dict, device, make):
    """One scratch buffer per (device, stream), bounded LRU: two forwards running on two streams must not share split-K /
    KV-split partials, and a host calling from many short-lived streams must not pin 256 + 128 MiB per stream forever.  A
    dropped lane's memory goes back to the caching allocator, which keeps it off limits until the work enqueued on its
    stream has finished."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = table.pop(key, None)
    if buf is None:
        mine = [k for k in table if k[0] == key[0]]           # the bound is per device
        while len(mine) >= MAX_WS_LANES:
            table.pop(mine.pop(0))
        buf = make()
    table[key] = buf                     # most recently used last
    return buf


def gemm_workspace(device) -> torch.Tensor:
    """fp32 scratch for the round-aware GEMM schedule (one per device and stream, see _ws_lane)."""
    shared = _shared_lane(device, 0)
    if shared is not None:
        return shared
    return _ws_lane(_gemm_ws, device,
                    lambda: torch.empty(_lib.lib().rgn_gemm_workspace_bytes() // 4, dtype=torch.float32, device=device))


FP8 = torch.float8_e4m3fn


def quantize_w8(W: torch.Tensor):
    """bf16 weight [N, K] -> (fp8 e4m3fn [N, K], fp32 scale [N]): per-output-channel absmax / 448 (OCP e4m3fn max).  The
    scale travels ON the quantised tensor (`._rgn_scale`), so call sites keep passing one weight object."""
    w = W.float()
    scale = (w.abs().amax(dim=1).clamp_min(1e-12) / 448.0)
    q = (w / scale[:, None]).to(FP8).contiguous()
    q._rgn_scale = scale.contiguous()
    return q


def wrows(W: torch.Tensor, lo: Optional[int] = None, hi: Optional[int] = None) -> torch.Tensor:
    """W[lo:hi] (output channels) of a GEMM weight; for a quantised weight the per-channel scales are sliced with it (a plain
    slice of the tensor would lose the `_rgn_scale` attribute)."""
    v = W[lo:hi]
    s = getattr(W, "_rgn_scale", None)
    if s is not None:
        v._rgn_scale = s[lo:hi]
    return v


def _wscale(W: torch.Tensor) -> Optional[torch.Tensor]:
    if W.dtype != FP8:
        return None
    s = getattr(W, "_rgn_scale", None)
    if s is None:
        raise _lib.RegionEHipError("fp8 weight without its per-channel scale (use ops.quantize_w8; slices lose the attribute)")
    return s


def quantize_rows_a8(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 activations [M, K] -> fp8 e4m3fn [M, K] with one fp32 scale per ROW (rgn_quantize_rows_a8): the arithmetic of quantize_w8 per
    row - scale = max(amax|x|, 1e-12) / 448, q = e4m3fn(x / scale) - on the device, bit-identical to that torch expression on the CPU.
    The scales travel ON the result (`._rgn_scale`, fp32 [M]); `out` may be given (fp8 [M, K] with `._rgn_scale` [M] already attached)."""
    if x.dim() != 2 or x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise _lib.RegionEHipError(f"quantize_rows_a8: x must be bf16 [M, K] with unit column stride (got {x.dtype} {tuple(x.shape)})")
    M, K = x.shape
    if out is None:
        out = torch.empty((M, K), dtype=FP8, device=x.device)
        out._rgn_scale = torch.empty(M, dtype=torch.float32, device=x.device)
    sc = _a8_out(out, M, K, x.device, "quantize_rows_a8")
    rc = _lib.lib().rgn_quantize_rows_a8(_p(x), x.stride(0), _p(out), out.stride(0), _p(sc), M, K, _stream())
    _lib.check(rc, "rgn_quantize_rows_a8")
    return out


def _a8_out(out: torch.Tensor, M: int, K: int, dev, what: str) -> torch.Tensor:
    """The row-scale vector of an fp8 activation buffer the kernels are about to WRITE (extents checked here: the C ABI cannot)."""
    sc = getattr(out, "_rgn_scale", None)
    if out.dtype != FP8 or tuple(out.shape) != (M, K) or out.stride(1) != 1 or out.device != dev:
        raise _lib.RegionEHipError(f"{what}: out must be fp8 e4m3fn [{M}, {K}] on {dev} (got {out.dtype} {tuple(out.shape)} on {out.device})")
    if sc is None or sc.dtype != torch.float32 or sc.dim() != 1 or sc.numel() != M or not sc.is_contiguous() or sc.device != dev:
        raise _lib.RegionEHipError(f"{what}: an fp8 out carries its row scales as `._rgn_scale`, fp32 [{M}], contiguous, on {dev}")
    return sc


def mx8_rows(M: int, K: int, device) -> torch.Tensor:
    """An empty mx8 buffer (include/regione_hip.h, "mx8 rows"): fp8 e4m3fn [M, K] whose E8M0 block scales, uint8 [M, K / 32], travel ON it
    as `._rgn_mx_scale` - a name of their own, so that no consumer takes them for the fp32 row scales of `._rgn_scale`."""
    if K <= 0 or K % 128:
        raise _lib.RegionEHipError(f"mx8 rows: K = {K} must be a positive multiple of 128")
    q = torch.empty((M, K), dtype=FP8, device=device)
    q._rgn_mx_scale = torch.empty((M, K // 32), dtype=torch.uint8, device=device)
    return q


def mx8_arows(A: torch.Tensor, lo: Optional[int] = None, hi: Optional[int] = None) -> torch.Tensor:
    """A[lo:hi] (rows) of an mx8 buffer with its block scales sliced alike (a plain slice loses the attribute): the rows of a row band."""
    s = getattr(A, "_rgn_mx_scale", None)
    if s is None:
        raise _lib.RegionEHipError("mx8_arows: not an mx8 buffer (no `._rgn_mx_scale`; use ops.mx8_rows)")
    v = A[lo:hi]
    v._rgn_mx_scale = s[lo:hi]
    return v


def quantize_rows_mx8(x: torch.Tensor, out: Optional[torch.Tensor] = None, col: int = 0) -> torch.Tensor:
    """bf16 activations [M, K] -> mx8 rows (rgn_quantize_rows_mx8): e4m3fn bytes with one power-of-two scale per 32 consecutive values,
    the smallest that keeps the block's amax at or below 448 - bit-identical to tests/gemm_mx8_model.py.  `out` (from ops.mx8_rows, at
    least `col + K` columns wide) receives the rows at columns [col, col + K), `col` a multiple of 128; its other columns stay as they
    are.  Returns `out` (a new [M, K] buffer when none is given)."""
    if x.dim() != 2 or x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise _lib.RegionEHipError(f"quantize_rows_mx8: x must be bf16 [M, K] with unit column stride (got {x.dtype} {tuple(x.shape)})")
    M, K = x.shape
    if K <= 0 or K % 128 or col < 0 or col % 128:
        raise _lib.RegionEHipError(f"quantize_rows_mx8: K = {K} must be a positive multiple of 128, col = {col} a non-negative one")
    if out is None:
        if col:
            raise _lib.RegionEHipError("quantize_rows_mx8: a column offset needs the `out` buffer it refers to")
        out = mx8_rows(M, K, x.device)
    s = getattr(out, "_rgn_mx_scale", None)
    if out.dtype != FP8 or out.dim() != 2 or out.shape[0] != M or out.shape[1] < col + K or out.stride(1) != 1 or out.device != x.device:
        raise _lib.RegionEHipError(f"quantize_rows_mx8: out must be fp8 e4m3fn [{M}, >= {col + K}] on {x.device} "
                                   f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    if (s is None or s.dtype != torch.uint8 or s.dim() != 2 or s.shape[0] != M or s.shape[1] * 32 < col + K or s.stride(1) != 1
            or s.device != x.device):
        raise _lib.RegionEHipError(f"quantize_rows_mx8: an mx8 out carries its block scales as `._rgn_mx_scale`, uint8 [{M}, >= {(col + K) // 32}], "
                                   f"on {x.device} (use ops.mx8_rows)")
    rc = _lib.lib().rgn_quantize_rows_mx8(_p(x), x.stride(0), _p(out), out.stride(0), _p(s), s.stride(0), col, M, K, _stream())
    _lib.check(rc, "rgn_quantize_rows_mx8")
    return out


def arows(A: torch.Tensor, lo: Optional[int] = None, hi: Optional[int] = None) -> torch.Tensor:
    """A[lo:hi] (rows) of an activation matrix; for fp8 activations the row scales are sliced with it, as wrows does for weights."""
    v = A[lo:hi]
    s = getattr(A, "_rgn_scale", None)
    if s is not None:
        v._rgn_scale = s[lo:hi]
    return v


def _ascale(A: torch.Tensor) -> Optional[torch.Tensor]:
    if A.dtype != FP8:
        return None
    s = getattr(A, "_rgn_scale", None)
    if s is None:
        raise _lib.RegionEHipError("fp8 activations without their per-row scales (use ops.quantize_rows_a8 / an fp8 `out` of ops.ln_modulate; "
                                   "slice rows with ops.arows - a plain slice loses the attribute)")
    if s.dtype != torch.float32 or s.numel() != A.shape[0] or not s.is_contiguous() or s.device != A.device:
        raise _lib.RegionEHipError(f"fp8 activations [{A.shape[0]} rows]: `_rgn_scale` must be fp32 [{A.shape[0]}], contiguous, on {A.device}")
    return s


class Problem:
    """One problem of a GEMM launch: out[r] = epilogue(A @ W^T + bias) with its own gate / residual, Q/K/V epilogue or row scatter."""
    __slots__ = ("A", "W", "bias", "out", "gate", "resid", "epi", "out_rows")

    def __init__(self, A, W, bias, out, gate=None, resid=None, epi=None, out_rows=None):
        self.A, self.W, self.bias, self.out, self.gate, self.resid, self.epi, self.out_rows = A, W, bias, out, gate, resid, epi, out_rows


def _launch(problems, epilogue: int, gelu_from_col: int):
    """The one way from here to the GEMM kernel (rgn_gemm_group): drops the empty problems, fills one descriptor per problem - the W row
    stride from the tensor, the fp8 scale from the weight - borrows the stream's workspace and launches."""
    probs = [p for p in problems if p.A.shape[0] > 0]
    if not probs:
        return
    assert len(probs) <= 4
    N, K = probs[0].W.shape
    arr = (_lib.GemmProblem * len(probs))(*[
        _lib.GemmProblem(_p(p.A), _p(p.W), _p(_wscale(p.W)), _p(p.bias), _p(p.out), _p(p.gate), _p(p.resid),
                         ctypes.pointer(p.epi) if p.epi is not None else None, _p(p.out_rows), p.A.stride(0), p.out.stride(0),
                         p.A.shape[0], p.W.stride(0), _p(_ascale(p.A))) for p in probs])
    ws = gemm_workspace(probs[0].A.device)
    rc = _lib.lib().rgn_gemm_group(arr, len(probs), N, K, epilogue, gelu_from_col, _p(ws), ws.numel() * 4, _stream())
    _lib.check(rc, "rgn_gemm_group")


def _check_single(A, W, out):
    assert A.dtype in (torch.bfloat16, FP8) and out.dtype == torch.bfloat16 and W.dtype in (torch.bfloat16, FP8)
    K, N = A.shape[1], W.shape[0]
    assert A.stride(1) == 1 and W.stride(1) == 1 and out.stride(1) == 1 and W.shape[1] == K and out.shape[1] == N


def _check_pair(A0, W0, out0, A1, W1, out1):
    N, K = W0.shape
    assert W1.shape == (N, K) and W0.is_contiguous() and W1.is_contiguous()
    assert A0.shape[1] == K and A1.shape[1] == K and out0.shape[1] == N and out1.shape[1] == N
    for t in (A0, A1, out0, out1):
        assert t.stride(1) == 1 and t.dtype in ((torch.bfloat16, FP8) if t is A0 or t is A1 else (torch.bfloat16,))


def gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, *, epilogue: int = EPI_BIAS,
         gelu_from_col: int = 0, gate: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
         out_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = epilogue(A @ W^T + bias).  A [M,K] (row stride may exceed K), W [N,K] (bf16, or fp8 from quantize_w8; row stride may
    exceed K), out [*,N] view; r = out_rows[m] (int64) or m."""
    _check_single(A, W, out)
    if resid is not None:
        assert resid.stride(0) == out.stride(0) and resid.stride(1) == 1
    _launch((Problem(A, W, bias, out, gate, resid, None, out_rows),), epilogue, gelu_from_col)
    return out


def gemm_pair(A0, W0, b0, out0, A1, W1, b1, out1, *, epilogue: int = EPI_BIAS, gelu_from_col: int = 0,
              gate0=None, resid0=None, gate1=None, resid1=None):
    """Two GEMMs with equal (N, K) and epilogue in one launch: outI = epilogue(AI @ WI^T + bI)."""
    _check_pair(A0, W0, out0, A1, W1, out1)
    _launch((Problem(A0, W0, b0, out0, gate0, resid0), Problem(A1, W1, b1, out1, gate1, resid1)), epilogue, gelu_from_col)


def _check_bias(bias, N: int, dev, what: str):
    """The kernels read `bias` as bf16 [N] (8-byte vectors): the C ABI cannot know its length."""
    if bias is not None and (bias.dtype != torch.bfloat16 or bias.dim() != 1 or bias.numel() != N or not bias.is_contiguous() or bias.device != dev):
        raise _lib.RegionEHipError(f"{what}: bias must be bf16 [{N}], contiguous, on {dev} (got {bias.dtype} {tuple(bias.shape)} on {bias.device})")


def qkv_epilogue(*, wq, wk, rope_q, rope_k, k_slab, vt_slab, H: int, k_col: int, v_col: int, q_col: int,
                 kv_rows: Optional[torch.Tensor] = None, row_base: int = 0, eps: float = 1e-6, fp16_roundtrip: bool = False,
                 rows: Optional[int] = None):
    """Descriptor of the fused Q/K/V epilogue (struct rgn_qkv_epilogue); keeps its tensors alive.  `rows` = the row count M of
    the problem the descriptor belongs to: with it the extents the kernel will read are checked here (the same checks as
    csrc/torch_binding.cpp:epi) - rotary rows [row_base, row_base + M), kv_rows[row_base + m], identity cache rows inside the slab."""
    skv_pad = k_slab.shape[0]
    assert vt_slab.shape == (H * 128, skv_pad) and k_slab.shape[1] == H * 128 and k_slab.is_contiguous() and vt_slab.is_contiguous()
    for t in (rope_q[0], rope_q[1], rope_k[0], rope_k[1]):
        assert t.dtype == torch.float32 and t.shape[1] == 128 and t.is_contiguous()
    assert rope_q[0].shape == rope_q[1].shape and rope_k[0].shape == rope_k[1].shape, "cos / sin of one rotary table differ in shape"
    for w in (wq, wk):
        assert w.dtype == torch.bfloat16 and w.numel() == 128 and w.is_contiguous(), "per-head RMSNorm weights: bf16 [128]"
    # the kernel reads 8-byte indices: an int32 tensor would be read past its end and scatter K / V to garbage cache rows
    assert kv_rows is None or (kv_rows.dtype == torch.int64 and kv_rows.dim() == 1 and kv_rows.is_contiguous())
    dev = k_slab.device
    for t in (wq, wk, rope_q[0], rope_q[1], rope_k[0], rope_k[1], vt_slab) + ((kv_rows,) if kv_rows is not None else ()):
        if t.device != dev:
            raise _lib.RegionEHipError(f"fused Q/K/V epilogue: tensors on {t.device} and {dev} (one device per problem)")
    if rows is not None:
        need = row_base + int(rows)
        if row_base < 0 or rope_q[0].shape[0] < need:
            raise _lib.RegionEHipError(f"rotary table of the queries has {rope_q[0].shape[0]} rows, the problem needs {need}")
        if kv_rows is not None:
            if kv_rows.numel() < need:
                raise _lib.RegionEHipError(f"kv_rows has {kv_rows.numel()} entries, the problem needs {need}")
            # the VALUES of kv_rows are device data, unchecked (no host sync per launch): the caller guarantees max(kv_rows) <
            # min(rope_k rows, skv_pad); checked is the necessary condition (distinct scatter targets need that many rows)
            if rope_k[0].shape[0] < need or skv_pad < need:
                raise _lib.RegionEHipError(f"key rotary table ({rope_k[0].shape[0]} rows) / slab ({skv_pad} rows) cannot hold the {need} "
                                           "distinct cache rows kv_rows names")
        elif rope_k[0].shape[0] < need or need > skv_pad:
            raise _lib.RegionEHipError(f"identity cache rows [{row_base}, {need}) exceed the key rotary table / the slab's {skv_pad} rows")
    e = _lib.QkvEpilogue(_p(wq), _p(wk), _p(rope_q[0]), _p(rope_q[1]), _p(rope_k[0]), _p(rope_k[1]), _p(kv_rows),
                         _p(k_slab), _p(vt_slab), row_base, skv_pad, k_col, v_col, q_col, H, eps, int(fp16_roundtrip))
    e._keep = (wq, wk, rope_q, rope_k, kv_rows, k_slab, vt_slab)
    return e


def gemm_qkv(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epi, *,
             gelu_from_col: Optional[int] = None) -> torch.Tensor:
    """QKV (+ fused MLP half) projection whose epilogue normalises / rotates Q and K, places K and V^T in the
    cache slabs and leaves Q (and GELU(mlp)) in `out`: the plain projection + rgn_qk_norm_rope_store in one launch."""
    _check_single(A, W, out)
    _check_bias(bias, W.shape[0], A.device, "gemm_qkv")
    _launch((Problem(A, W, bias, out, epi=epi),), EPI_QKV, W.shape[0] if gelu_from_col is None else gelu_from_col)
    return out


def gemm_qkv_pair(A0, W0, b0, out0, epi0, A1, W1, b1, out1, epi1):
    """Both streams of a double block (image + text QKV projections) in one launch, fused Q/K/V epilogue."""
    _check_pair(A0, W0, out0, A1, W1, out1)
    _check_bias(b0, W0.shape[0], A0.device, "gemm_qkv_pair")
    _check_bias(b1, W0.shape[0], A0.device, "gemm_qkv_pair")
    _launch((Problem(A0, W0, b0, out0, epi=epi0), Problem(A1, W1, b1, out1, epi=epi1)), EPI_QKV, W0.shape[0])


def gemm_group(problems, *, epilogue: int = EPI_BIAS, gelu_from_col: int = 0):
    """Up to four GEMMs with equal (N, K), epilogue and weight format in ONE launch: the text / image streams of a double
    block x the cond / uncond CFG branches.  Problems may share W."""
    probs = [p for p in problems if p.A.shape[0] > 0]
    if not probs:
        return
    N, K = probs[0].W.shape
    for p in probs:
        assert p.W.shape == (N, K) and p.W.is_contiguous() and p.A.shape[1] == K and p.out.shape == (p.A.shape[0], N)
        for t in (p.A, p.out):
            assert t.stride(1) == 1 and t.dtype in ((torch.bfloat16, FP8) if t is p.A else (torch.bfloat16,))
        if p.resid is not None:
            assert p.resid.stride(0) == p.out.stride(0) and p.resid.stride(1) == 1
        _check_bias(p.bias, N, p.A.device, "gemm_group")
    _launch(probs, epilogue, gelu_from_col)


# row bands (rgn_rowband_fork / rgn_rowband_join, include/regione_hip.h): between fork and join on the current stream the GEMM and
# LN-modulate launches above / below run as two row bands on two streams; the harness forks after a block's attention and joins before
# the next one
def rowband_fork():
    _lib.check(_lib.lib().rgn_rowband_fork(_stream()), "rgn_rowband_fork")


def rowband_join():
    _lib.check(_lib.lib().rgn_rowband_join(_stream()), "rgn_rowband_join")


def rowband_query(Ms):
    """The band boundary for problems of `Ms` rows listed in memory order: (problem, row) - that problem's rows from `row` on are band 1,
    everything else band 0 - or None when nothing is cut.  Host arithmetic only (no GPU)."""
    n = len(Ms)
    which, row = ctypes.c_int(-1), ctypes.c_int(0)
    rc = _lib.lib().rgn_rowband_query((ctypes.c_int * n)(*[int(m) for m in Ms]), n, ctypes.byref(which), ctypes.byref(row))
    if rc < 0:
        _lib.check(rc, "rgn_rowband_query")
    return (which.value, row.value) if rc == 1 else None


def rowband_side_launches() -> int:
    return int(_lib.lib().rgn_rowband_side_launches())


def gemv(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], silu_input: bool = False,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    B, K = x.shape
    N = W.shape[0]
    assert W.is_contiguous() and x.stride(1) == 1
    if out is None:
        out = torch.empty((B, N), dtype=torch.bfloat16, device=x.device)
    rc = _lib.lib().rgn_gemv_bf16(_p(x), x.stride(0), _p(W), _p(bias), _p(out), out.stride(0), B, N, K,
                                  int(silu_input), _stream())
    _lib.check(rc, "rgn_gemv_bf16")
    return out


def rms_norm_rows(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    out = torch.empty_like(x)
    rc = _lib.lib().rgn_rms_norm_rows(_p(x), x.stride(0), _p(w), _p(out), out.stride(0), x.shape[0], x.shape[1], eps,
                                      _stream())
    _lib.check(rc, "rgn_rms_norm_rows")
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().rgn_silu_bf16(_p(x), _p(y), x.numel(), _stream()), "rgn_silu_bf16")
    return y


def add_bf16(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 a + b (one rounding, like torch) into `out` (default: a new tensor; may alias an input)."""
    assert a.dtype == b.dtype == torch.bfloat16 and a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty_like(a)
    assert out.dtype == torch.bfloat16 and out.numel() == a.numel() and out.is_contiguous()
    _lib.check(_lib.lib().rgn_add_bf16(_p(a), _p(b), _p(out), a.numel(), _stream()), "rgn_add_bf16")
    return out


def _bf16_rows(what: str, **tensors):
    """The row kernels read bf16 rows through 16-byte vectors: dtype, unit column stride and one device, checked where the C ABI cannot."""
    dev = None
    for k, t in tensors.items():
        if t.dtype != torch.bfloat16 or t.stride(-1) != 1 or (dev is not None and t.device != dev):
            raise _lib.RegionEHipError(f"{what}: {k} must be bf16 with unit column stride on one device (got {t.dtype}, strides {t.stride()}, {t.device})")
        dev = t.device


def masked_mean_rows(x: torch.Tensor, n_valid: int, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16(bf16(mean of the first `n_valid` rows of x [L, d]) * scale) -> [d] (rgn_masked_mean_rows): the connector's pooled context."""
    L, d = x.shape
    if out is None:
        out = torch.empty(d, dtype=torch.bfloat16, device=x.device)
    _bf16_rows("masked_mean_rows", x=x, out=out)
    if out.numel() != d:
        raise _lib.RegionEHipError(f"masked_mean_rows: out has {out.numel()} elements, x has {d} columns")
    rc = _lib.lib().rgn_masked_mean_rows(_p(x), x.stride(0), L, d, int(n_valid), float(scale), _p(out), _stream())
    _lib.check(rc, "rgn_masked_mean_rows")
    return out


def head_rms_norm_(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, H: int, eps: float = 1e-6) -> torch.Tensor:
    """Per-head RMSNorm (width 128) of the q and k columns of packed [L, >= 3 H 128] rows, in place (rgn_head_rms_norm_bf16)."""
    _bf16_rows("head_rms_norm_", qkv=qkv, wq=wq, wk=wk)
    if qkv.dim() != 2 or qkv.shape[1] < 3 * H * 128 or wq.numel() != 128 or wk.numel() != 128:
        raise _lib.RegionEHipError(f"head_rms_norm_: qkv {tuple(qkv.shape)} for {H} heads of 128, weights of {wq.numel()} / {wk.numel()} elements")
    rc = _lib.lib().rgn_head_rms_norm_bf16(_p(qkv), qkv.stride(0), _p(wq), _p(wk), qkv.shape[0], int(H), float(eps), _stream())
    _lib.check(rc, "rgn_head_rms_norm_bf16")
    return qkv


def gate_resid_rows(p: torch.Tensor, gate: torch.Tensor, resid: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 `resid + gate * p` with torch's two roundings (rgn_gate_resid_rows); p, resid [M, N], gate [N]; `out` may be resid."""
    if out is None:
        out = torch.empty_like(resid)
    _bf16_rows("gate_resid_rows", p=p, gate=gate, resid=resid, out=out)
    M, N = p.shape
    if tuple(resid.shape) != (M, N) or tuple(out.shape) != (M, N) or gate.numel() != N:
        raise _lib.RegionEHipError(f"gate_resid_rows: p {tuple(p.shape)}, resid {tuple(resid.shape)}, out {tuple(out.shape)}, gate of {gate.numel()}")
    rc = _lib.lib().rgn_gate_resid_rows(_p(p), p.stride(0), _p(gate), _p(resid), resid.stride(0), _p(out), out.stride(0), M, N, _stream())
    _lib.check(rc, "rgn_gate_resid_rows")
    return out


LORA_MAX_TERMS, LORA_MAX_RANK = 8, 1024          # RGN_LORA_MAX_TERMS / RGN_LORA_MAX_RANK


def lora_merge(dst: torch.Tensor, W: torch.Tensor, terms) -> torch.Tensor:
    """dst = bf16(W + sum_t scale_t * B_t A_t) (rgn_lora_merge_bf16: fp32 fma in term order, r ascending, ONE rounding to bf16).
    dst, W [N, K] bf16 with unit column stride (row ranges of packed tensors are fine; `dst is W` is the in-place form); `terms` a
    sequence of (A [r, K], B [N, r], scale) with A, B contiguous fp32 on W's device."""
    _bf16_rows("lora_merge", dst=dst, W=W)
    if dst.dim() != 2 or dst.shape != W.shape:
        raise _lib.RegionEHipError(f"lora_merge: dst {tuple(dst.shape)} and W {tuple(W.shape)} must be the same [N, K]")
    N, K = W.shape
    terms = list(terms)
    arr = (_lib.LoraTerm * max(len(terms), 1))()
    for i, (A, B, scale) in enumerate(terms):
        for name, t, shape in (("A", A, (A.shape[0], K)), ("B", B, (N, A.shape[0]))):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != W.device or tuple(t.shape) != shape:
                raise _lib.RegionEHipError(f"lora_merge: term {i} {name} must be contiguous fp32 {shape} on {W.device} "
                                           f"(got {t.dtype} {tuple(t.shape)} on {t.device})")
        arr[i] = _lib.LoraTerm(_p(A), _p(B), A.shape[0], float(scale))
    rc = _lib.lib().rgn_lora_merge_bf16(_p(dst), dst.stride(0) if N > 1 else max(dst.stride(0), K), _p(W),
                                        W.stride(0) if N > 1 else max(W.stride(0), K), N, K, arr, len(terms), _stream())
    _lib.check(rc, "rgn_lora_merge_bf16")
    return dst


def sel_rows(edited_ids: torch.Tensor, T: int) -> torch.Tensor:
    """int64 [T + K]: [0..T) then T + edited_ids - the cache rows of a region step (inplace.py:732-733)."""
    idv = edited_ids.reshape(-1)
    assert idv.dtype == torch.int64 and idv.is_contiguous()
    out = torch.empty(T + idv.numel(), dtype=torch.int64, device=idv.device)
    _lib.check(_lib.lib().rgn_sel_rows(_p(idv), idv.numel(), int(T), _p(out), _stream()), "rgn_sel_rows")
    return out


def zeros(shape, dtype=torch.bfloat16, device="cuda") -> torch.Tensor:
    """torch.empty + hipMemsetAsync on the current stream (no fill kernel)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    _lib.check(_lib.lib().rgn_fill_zero(_p(t), t.numel() * t.element_size(), _stream()), "rgn_fill_zero")
    return t


def cat_rows(parts, dim: int = 1) -> torch.Tensor:
    """torch.cat of contiguous pieces along `dim` when every piece is one contiguous run of the result (dim 0, or dim 1 of
    batch-1 tensors): device-to-device copies (hipMemcpyAsync), no concat kernel."""
    parts = list(parts)
    ref = parts[0]
    assert all(p.is_contiguous() and p.dtype == ref.dtype for p in parts) and (dim == 0 or all(p.shape[0] == 1 for p in parts))
    shape = list(ref.shape)
    shape[dim] = sum(p.shape[dim] for p in parts)
    out = torch.empty(shape, dtype=ref.dtype, device=ref.device)
    o = 0
    for p in parts:
        n = p.shape[dim]
        out.narrow(dim, o, n).copy_(p)
        o += n
    return out


def ln_modulate(x: torch.Tensor, out: torch.Tensor, shift1, scale1, split_row: int = 0, shift0=None, scale0=None,
                eps: float = 1e-6) -> torch.Tensor:
    M, d = x.shape
    if out.dtype == FP8:          # fp8 rows + row scales (`out._rgn_scale`): bit-identical to quantize_rows_a8 of the bf16 result
        sc = _a8_out(out, M, d, x.device, "ln_modulate")
        rc = _lib.lib().rgn_ln_modulate_a8(_p(x), x.stride(0), _p(out), out.stride(0), _p(sc), M, d, eps, split_row, _p(shift0),
                                           _p(scale0), _p(shift1), _p(scale1), _stream())
        _lib.check(rc, "rgn_ln_modulate_a8")
        return out
    rc = _lib.lib().rgn_ln_modulate(_p(x), x.stride(0), _p(out), out.stride(0), M, d, eps, split_row, _p(shift0),
                                    _p(scale0), _p(shift1), _p(scale1), _stream())
    _lib.check(rc, "rgn_ln_modulate")
    return out


def ln_modulate_segs(x: torch.Tensor, out: torch.Tensor, segs, eps: float = 1e-6) -> torch.Tensor:
    """LN * (1 + scale) + shift with up to four row segments: `segs` = [(end_row, shift, scale), ...], ascending, the last
    end_row == rows of x."""
    import ctypes as C
    M, d = x.shape
    n = len(segs)
    assert 1 <= n <= 4 and segs[-1][0] == M
    ends = (C.c_int * n)(*[int(s[0]) for s in segs])
    sh = (C.c_void_p * n)(*[_p(s[1]) for s in segs])
    sc = (C.c_void_p * n)(*[_p(s[2]) for s in segs])
    if out.dtype == FP8:
        rs = _a8_out(out, M, d, x.device, "ln_modulate_segs")
        rc = _lib.lib().rgn_ln_modulate_segs_a8(_p(x), x.stride(0), _p(out), out.stride(0), _p(rs), M, d, eps, n, ends, sh, sc, _stream())
        _lib.check(rc, "rgn_ln_modulate_segs_a8")
        return out
    rc = _lib.lib().rgn_ln_modulate_segs(_p(x), x.stride(0), _p(out), out.stride(0), M, d, eps, n, ends, sh, sc, _stream())
    _lib.check(rc, "rgn_ln_modulate_segs")
    return out


def qk_norm_rope_store(qkv: torch.Tensor, k_col: int, v_col: int, q_col: int, H: int, wq1, wk1, rope_q, rope_k,
                       k_slab: torch.Tensor, vt_slab: torch.Tensor, kv_rows: Optional[torch.Tensor] = None,
                       split_row: int = 0, wq0=None, wk0=None, eps: float = 1e-6):
    M = qkv.shape[0]
    skv_pad = k_slab.shape[0]
    assert vt_slab.shape == (H * 128, skv_pad) and k_slab.shape[1] == H * 128
    assert kv_rows is None or (kv_rows.dtype == torch.int64 and kv_rows.dim() == 1 and kv_rows.is_contiguous() and kv_rows.numel() >= M)
    rc = _lib.lib().rgn_qk_norm_rope_store(_p(qkv), qkv.stride(0), k_col, v_col, q_col, M, H, split_row, _p(wq0),
                                           _p(wk0), _p(wq1), _p(wk1), eps, _p(rope_q[0]), _p(rope_q[1]),
                                           _p(rope_k[0]), _p(rope_k[1]), _p(kv_rows), _p(k_slab), _p(vt_slab), skv_pad,
                                           _stream())
    _lib.check(rc, "rgn_qk_norm_rope_store")


_attn_ws = {}


def attention_workspace(device) -> torch.Tensor:
    """fp32 scratch for the round-aware attention schedule (allocated once per device and stream)."""
    shared = _shared_lane(device, 1)
    if shared is not None:
        return shared
    return _ws_lane(_attn_ws, device,
                    lambda: torch.empty(_lib.lib().rgn_attention_workspace_bytes(0, 0) // 4, dtype=torch.float32, device=device))


def attention(q: torch.Tensor, k_slab: torch.Tensor, vt_slab: torch.Tensor, out: torch.Tensor, skv: int, H: int,
              scale: Optional[float] = None, workspace: Optional[torch.Tensor] = None, score_bound: float = 0.0) -> torch.Tensor:
    """q / out: [Sq, H*128] views (row stride free, may alias).  `score_bound` > 0: the caller's guarantee that every
    |q . k| * scale is at most that (rgn_attention_bounded: no running max in the softmax)."""
    Sq = q.shape[0]
    if scale is None:
        scale = 1.0 / math.sqrt(128.0)
    if workspace is None:
        workspace = attention_workspace(q.device)
    rc = _lib.lib().rgn_attention_bounded(_p(q), q.stride(0), _p(k_slab), _p(vt_slab), k_slab.shape[0], _p(out), out.stride(0),
                                          Sq, skv, H, float(scale), float(score_bound), _p(workspace), workspace.numel() * 4,
                                          _stream())
    _lib.check(rc, "rgn_attention_bounded")
    return out


def device_info() -> Tuple[int, int, int]:
    import ctypes as C
    cu, clk, mem = C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(_lib.lib().rgn_device_info(C.byref(cu), C.byref(clk), C.byref(mem)), "rgn_device_info")
    return cu.value, clk.value, mem.value


# ---- the wide decode step: 1 <= B <= 32 rows on the MFMA row GEMM (csrc/decode.hip: lm_gemm_rows_kernel) -------------------------------
LM_MAX_WIDE_BATCH = 32                                                           # RGN_LM_MAX_WIDE_BATCH of include/regione_hip.h


def lm_gemm_rows(X: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y [B, N] bf16 = X [B, K] W^T (+ bias) (+ resid: the two roundings of `h + linear(a)`) for 1 <= B <= 32 rows from one stream of
    W [N, K]: bf16 (rgn_lm_gemm_rows_bf16) or an ops.quantize_w8 weight (rgn_lm_gemm_rows_w8).  Row strides are free (multiples of 8
    elements); `out` may be `resid`.  The C entry validates everything else."""
    B, N = X.shape[0], W.shape[0]
    if out is None:
        out = torch.empty(B, N, dtype=torch.bfloat16, device=X.device)
    tail = (_p(X), X.stride(0), _p(bias), _p(resid), resid.stride(0) if resid is not None else 0, _p(out), out.stride(0), B, N, W.shape[1],
            _stream())
    if W.dtype == FP8:
        _lib.check(_lib.lib().rgn_lm_gemm_rows_w8(_p(W), _p(_wscale(W)), *tail), "rgn_lm_gemm_rows_w8")
    else:
        _lib.check(_lib.lib().rgn_lm_gemm_rows_bf16(_p(W), *tail), "rgn_lm_gemm_rows_bf16")
    return out


def lm_head_argmax_wide(X: torch.Tensor, W: torch.Tensor, logits: bool = False):
    """(tokens [B] int64, fp32 logits [B, V] or None) of rgn_lm_head_argmax_wide: the argmax of X [B, K] W^T per row over W [V, K] bf16, the
    lowest index on a tie, for 1 <= B <= 32 rows."""
    lib = _lib.lib()
    B, V = X.shape[0], W.shape[0]
    nbytes = lib.rgn_lm_head_wide_workspace_bytes(V, B)
    ws = torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=X.device)
    tok = torch.empty(B, dtype=torch.int64, device=X.device)
    z = torch.empty(B, V, dtype=torch.float32, device=X.device) if logits else None
    rc = lib.rgn_lm_head_argmax_wide(_p(W), _p(X), X.stride(0), B, V, W.shape[1], _p(tok), 1, _p(z), V, _p(ws), nbytes, _stream())
    _lib.check(rc, "rgn_lm_head_argmax_wide")
    return tok, z
