"""The wide decode step on the GPU (regione_amd/csrc/decode.hip: lm_gemm_rows_kernel behind rgn_lm_gemm_rows_bf16, rgn_lm_gemm_rows_w8 and
rgn_lm_head_argmax_wide), pinned by the probes of tests/lm_rows_mfma_model.py (which tests/test_lm_rows_mfma_model.py shows to be sharp
against every named defect): exact integer and one-hot probes, all fp8 codes, row invariance against hostile neighbours, sentinel frames
with strides and Y aliasing resid, repeatability, the fp64 bound of the bf16 GEMM probes, lm_head logits / ties / outputs, and refusals.
Every call is strided (ldx = K + 8, ldy = ldr = N + pad) unless the test says otherwise.

The fp64 bounds, as the entries meet them, are printed before they are asserted (pytest -s)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_rows_mfma_model as M  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODEL_SHAPES = [(4608, 3584), (3584, 3584), (37888, 3584), (3584, 18944)]        # q|k|v, o, gate|up, down of Qwen2.5-VL-7B
SHAPES = M.TINY + MODEL_SHAPES
XPAD = 8


def _strided_x(p):
    X = torch.full((M.MAX_B, p.K + XPAD), M.SENT, device=DEV).to(M.BF16)
    X[:, :p.K] = p.X.to(DEV)
    return X


def _call(p, B, Y, X=None, resid="alias", ldy=None):
    """One entry call on device tensors; returns the status."""
    lib = _lib.lib()
    X = _strided_x(p) if X is None else X
    rs = Y if (resid == "alias" and p.resid is not None) else (resid if isinstance(resid, torch.Tensor) else None)
    bias = None if p.bias is None else p.bias.to(DEV)
    p._keep = (X, bias)
    tail = (X.data_ptr(), X.stride(0), ops._p(bias), ops._p(rs), rs.stride(0) if rs is not None else 0, Y.data_ptr(),
            Y.stride(0) if ldy is None else ldy, B, p.N, p.K, ops._stream())
    W = p.W.to(DEV)
    p._keep += (W,)
    if p.w8:
        ws = p.wscale.to(DEV).float().contiguous()
        p._keep += (ws,)
        return lib.rgn_lm_gemm_rows_w8(W.data_ptr(), ws.data_ptr(), *tail)
    return lib.rgn_lm_gemm_rows_bf16(W.data_ptr(), *tail)


def run(p, B, Y):
    Y = Y.to(DEV)
    _lib.check(_call(p, B, Y), "rgn_lm_gemm_rows")
    torch.cuda.synchronize()
    return Y


def run_head(p, B, logits=True, stride=1):
    lib = _lib.lib()
    X, W = _strided_x(p), p.W.to(DEV)
    V = p.N
    nb = lib.rgn_lm_head_wide_workspace_bytes(V, B)
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device=DEV)
    tok = torch.full((B * stride,), -1, dtype=torch.int64, device=DEV)
    z = torch.full((B, V + 3), M.SENT, dtype=torch.float32, device=DEV) if logits else None
    rc = lib.rgn_lm_head_argmax_wide(W.data_ptr(), X.data_ptr(), X.stride(0), B, V, p.K, tok.data_ptr(), stride, ops._p(z), V + 3, ws.data_ptr(),
                                     nb, ops._stream())
    _lib.check(rc, "rgn_lm_head_argmax_wide")
    torch.cuda.synchronize()
    if z is not None:
        assert bool((z[:, V:] == M.SENT).all())
    if stride > 1:
        assert bool((tok.view(B, stride)[:, 1:] == -1).all())
    return tok.view(B, stride)[:, 0].contiguous(), (z[:, :V].contiguous() if z is not None else None)


# ---- exact probes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w8", [False, True])
@pytest.mark.parametrize("N,K", M.TINY)
def test_integer_probe_is_exact_at_every_batch_in_a_sentinel_frame_with_y_aliasing_resid(N, K, w8):
    for B in M.BATCHES:
        assert M.check_integer(run, N, K, w8, B, dev=DEV), (N, K, w8, B)
    assert M.check_integer(run, N, K, w8, 17, resid=False, dev=DEV)              # the one-rounding epilogue


@pytest.mark.parametrize("w8", [False, True])
@pytest.mark.parametrize("N,K", MODEL_SHAPES)
def test_integer_probe_is_exact_at_the_model_shapes(N, K, w8):
    for B in (1, 17, 32):
        assert M.check_integer(run, N, K, w8, B, dev=DEV), (N, K, w8, B)


@pytest.mark.parametrize("w8", [False, True])
def test_one_hot_rows_return_every_weight_of_k_3584_itself(w8):
    assert M.check_index(run, 33, 3584, w8, dev=DEV)                             # 112 calls of 32 k: every k of every wave and chunk


def test_all_254_finite_fp8_codes_come_out_as_the_bf16_that_equals_them():
    assert M.check_codes(run)


def test_the_scale_multiplies_the_folded_sum_once():
    for B in (1, 17, 32):
        assert M.check_scale(run, B)


# ---- invariance, repeatability ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w8", [False, True])
@pytest.mark.parametrize("N,K", [M.TINY[-1], (3584, 3584), (96, 18944)])
def test_row_b_of_32_equals_the_call_on_row_b_alone_whatever_the_other_rows_hold(N, K, w8):
    assert M.check_invariance(run, N, K, w8, dev=DEV)


@pytest.mark.parametrize("w8", [False, True])
def test_two_calls_are_bit_identical(w8):
    p = M.with_pad(M.invariance_case(4608, 3584, w8, dev=DEV))
    a = run(p, 32, M.frames(p, 32))
    b = run(p, 32, M.frames(p, 32))
    assert M.same_bits(a, b)
    t1, z1 = run_head(M.invariance_case(4097, 3584, False, dev=DEV), 32)
    t2, z2 = run_head(M.invariance_case(4097, 3584, False, dev=DEV), 32)
    assert torch.equal(t1, t2) and torch.equal(z1.view(torch.int32), z2.view(torch.int32))


# ---- the fp64 bound of the bf16 GEMM probes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w8", [False, True])
@pytest.mark.parametrize("family", M.G.FAMILIES)
@pytest.mark.parametrize("N,K", SHAPES)
def test_bias_epilogue_is_within_the_fp64_bound(N, K, family, w8):
    p = M.with_pad(M.bound_case(N, K, family, w8, dev=DEV))
    Y = run(p, 32, M.frames(p, 32))
    r = M.bound_ratio(p, 32, Y)
    print(f"bound ratio N={N} K={K} {family} {'w8' if w8 else 'bf16'}: {r:.4f}")
    assert M.frame_intact(p, 32, Y) and r <= 1.0, r


# ---- lm_head ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", [(1, 64), (17, 128), (4097, 3584), (152064, 3584)])
def test_head_logits_are_within_the_fp64_bound_and_the_token_is_their_first_maximum(V, K):
    p = M.bound_case(V, K, "randn", False, dev=DEV)
    p.bias = None
    for B in ((32,) if V > 4097 else (1, 17, 32)):
        tok, z = run_head(p, B)
        lin, bound = M.head_bound(p, B)
        r = float(((z.double() - lin).abs() / (bound + 1e-30)).max())
        print(f"head bound ratio V={V} K={K} B={B}: {r:.4f}")
        assert r <= 1.0, (V, B, r)
        assert torch.equal(tok, torch.argmax(z, dim=1))                          # ties have probability 0 here; the tie rule is below
        assert all(float(z[b, tok[b]]) == float(z[b].max()) for b in range(B))


@pytest.mark.parametrize("V", [17, 97, 4097])
def test_head_ties_go_to_the_lowest_index(V):
    assert M.check_head_ties(run_head, V, dev=DEV)
    assert M.check_head_ties(run_head, V, K=2 * M.KW + 64, B=17, dev=DEV)


def test_head_row_b_of_32_equals_the_call_on_row_b_alone():
    assert M.check_head_invariance(run_head, 4097, 3584, dev=DEV)


def test_head_outputs_token_stride_and_no_logits():
    p = M.head_case(4097, 128, dev=DEV)
    M.plant(p, 3, (4096,))
    want, _ = M.head_expected(p, 32)
    a, _ = run_head(p, 32)
    b, z = run_head(p, 32, logits=False, stride=3)
    assert z is None and torch.equal(a, want) and torch.equal(b, want) and int(want[3]) == 4096


# ---- refusals: RGN_E_* before any launch, outputs intact -----------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_leave_the_outputs_intact():
    lib = _lib.lib()
    for w8 in (False, True):
        p = M.with_pad(M.integer_case(17, 128, w8, dev=DEV))
        Y0 = M.frames(p, 32)
        Y = Y0.clone()
        X = _strided_x(p)
        assert _call(p, 0, Y) != 0 and b"B outside [1, 32]" in lib.rgn_last_error()
        assert _call(p, 33, Y) != 0 and b"B outside [1, 32]" in lib.rgn_last_error()
        q = M.with_pad(M.integer_case(17, 128, w8, dev=DEV))
        q.K = 96
        assert _call(q, 2, Y, X=X) != 0 and b"multiple of 64" in lib.rgn_last_error()
        assert _call(p, 2, Y, X=X.view(-1)[1:].as_strided((32, p.K), (p.K + XPAD, 1))) != 0 and b"aligned" in lib.rgn_last_error()
        assert _call(p, 2, Y, X=X.as_strided((32, p.K), (p.K - 8, 1))) != 0 and b"strides" in lib.rgn_last_error()      # ldx < K
        assert _call(p, 2, Y, ldy=p.N - 1) != 0 and b"strides" in lib.rgn_last_error()                               # ldy < N, not a multiple of 8
        assert _call(p, 2, Y, ldy=16) != 0 and b"strides" in lib.rgn_last_error()                                    # ldy < N
        torch.cuda.synchronize()
        assert M.same_bits(Y, Y0)
    p = M.head_case(17, 128, dev=DEV)
    X, W = _strided_x(p), p.W.to(DEV)
    nb = lib.rgn_lm_head_wide_workspace_bytes(17, 32)
    ws = torch.zeros(nb // 4 + 1, dtype=torch.float32, device=DEV)
    tok = torch.full((32,), -1, dtype=torch.int64, device=DEV)

    def head(B=2, K=128, ldx=None, x=None, wsb=None, tokp=None):
        return lib.rgn_lm_head_argmax_wide(W.data_ptr(), (X if x is None else x).data_ptr(), X.stride(0) if ldx is None else ldx, B, 17, K,
                                           tok.data_ptr() if tokp is None else tokp, 1, None, 0, ws.data_ptr(), nb if wsb is None else wsb,
                                           ops._stream())
    assert head(B=0) != 0 and head(B=33) != 0 and head(K=96) != 0 and head(ldx=64) != 0 and head(wsb=8) != 0
    assert head(x=X.view(-1)[1:]) != 0 and head(tokp=tok.data_ptr() + 4) != 0
    assert lib.rgn_lm_head_wide_workspace_bytes(17, 33) == 0 and lib.rgn_lm_head_wide_workspace_bytes(17, 32) == 32 * 2 * 8
    torch.cuda.synchronize()
    assert bool((tok == -1).all()) and bool((ws == 0).all())
    assert head() == 0


def test_the_ops_wrappers_reach_the_entries():
    p = M.integer_case(40, 576, False, dev=DEV)
    Y = ops.lm_gemm_rows(p.X[:17], p.W, p.bias, p.resid[:17])
    assert M.same_bits(Y, M.expected_exact(p, 17))
    q = M.integer_case(40, 576, True, dev=DEV)
    W8 = q.W.view(ops.FP8)
    W8._rgn_scale = q.wscale
    out = q.resid[:17].clone()
    assert ops.lm_gemm_rows(q.X[:17], W8, q.bias, out, out=out) is out and M.same_bits(out, M.expected_exact(q, 17))
    h = M.head_case(97, 128, dev=DEV)
    M.plant(h, 2, (40, 96))
    tok, z = ops.lm_head_argmax_wide(h.X[:5], h.W, logits=True)
    want, zw = M.head_expected(h, 5)
    assert torch.equal(tok, want) and torch.equal(z, zw) and int(tok[2]) == 40
    assert ops.lm_head_argmax_wide(h.X[:5], h.W)[1] is None
