"""-m gpu: exact probes and the element-wise fp64 bound for rgn_gemm_group with fp8 activations (`ascale`; csrc/gemm.hip, kernel variant
AV = 10: both operands as e4m3fn bytes on v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales, row scale then channel scale in the epilogue).

Inputs, expected outputs, checks and the table of launch paths (A.TABLE / A.QKV_TABLE: M in {1, 130, 257} x N in {128, 384} x K in {128, 256,
640} on the 128 x 128 and the 256 x 256 geometry, quarter tiles, two-problem groups that share W, lda > K) come from tests/gemm_a8_model.py;
tests/test_gemm_a8_model.py shows on the CPU that the same checks notice six named defects.  One test is one row of the table:

  a. index probe: one-hot A rows against a W of distinct integer codes that depends on n and k asymmetrically, short-mantissa row and channel
     scales, integer bias - every output bit for bit, over as many passes as it takes for the rows to select every k.  Pins the lane -> k
     map of the A fragment against that of the W fragment, and the tile walk;
  b. all 254 finite e4m3fn codes in A and in W with power-of-two scales: bit for bit (-0, subnormals, +-448);
  c. scale-then-bias with scales that are no power of two; K-tile signatures (each K tile of 128 adds its own power of two);
  d. GELU from column 0, from a multiple of 8 inside a tile, from N (rows with the GELU epilogue);
  e. |out - lin| <= 2^-8 |lin| + (K + 2) 2^-22 S + 1e-30 on the quantised `randn` and `cancel` families; a repeated call is bit-identical;
  f. the integer Q/K/V case of G.qkv_case on fp8 operands: Q in out, K in the slab row kv_rows names, V^T at kvpos, sentinels elsewhere;
  g. every refusal: RegionEHipError, the destination untouched.
Every launch writes into a view of a sentinel-filled buffer (3 rows longer, 8 columns wider) that must be intact outside the problem, and
asserts rgn_gemm_last_plan() against the table."""
import pytest
import torch

import gemm_a8_model as A
import gemm_model as G
import plan_helpers
from regione_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = [r.name for r in A.TABLE]
EPI = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_GELU}


def _to(case):
    moved = {}                                                       # problems that share W keep sharing one tensor
    for p in case.probs:
        for k, v in list(p.__dict__.items()):
            if torch.is_tensor(v):
                setattr(p, k, moved.setdefault(id(v), v.to(DEV)))
    q = case.qkv
    if q is not None:
        for k, v in list(q.__dict__.items()):
            if torch.is_tensor(v):
                setattr(q, k, v.to(DEV))
        q.rope_q, q.rope_k = tuple(t.to(DEV) for t in q.rope_q), tuple(t.to(DEV) for t in q.rope_k)
    return case


def _a8(row, p):
    """The problem's A as an fp8 tensor that carries its row scales (dense, or a view with lda > K into a zero-filled buffer)."""
    a = p.A
    pad = row.feat.get("lda", 0)
    if pad:
        buf = torch.zeros((p.M + G.XR, row.K + pad), dtype=torch.uint8, device=DEV)
        buf[:p.M, :row.K] = a
        a = buf[:p.M, :row.K]
    a = a.view(ops.FP8)
    a._rgn_scale = p.ascale.contiguous()
    return a


def _w8(p):
    w = p.W.view(ops.FP8)
    w._rgn_scale = p.wscale
    return w


def _launch(row, case):
    """One call of ops.gemm / ops.gemm_group on the case under the knobs of the row: the destination buffers, whole."""
    probs, outs = [], []
    for p in case.probs:
        buf = p.out_init.clone()
        outs.append(buf)
        probs.append(ops.Problem(_a8(row, p), _w8(p), p.bias, buf[:p.M, :case.N]))
    plan_helpers.force(**row.knobs)
    if len(probs) == 1:
        q = probs[0]
        ops.gemm(q.A, q.W, q.bias, q.out, epilogue=EPI[case.epi], gelu_from_col=case.gelu_from)
    else:
        ops.gemm_group(probs, epilogue=EPI[case.epi], gelu_from_col=case.gelu_from)
    plan = _lib.lib().rgn_gemm_last_plan()
    assert plan == row.plan, f"{row.name}: plan {plan:#x}, the table says {row.plan:#x}"
    for p, buf in zip(case.probs, outs):
        assert G.outside_intact(p, buf, case.N), "wrote outside the problem's rows / columns"
    return outs


def _exact(row, case):
    case = _to(case)
    return G.check_exact(case, _launch(row, case))


# ---- a. index probe ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_index_probe(name):
    row = A.TABLE_BY_NAME[name]
    for shift in range(A.index_shifts(row)):
        assert _exact(row, A.index_case(row, shift=shift)) == 0, shift


def test_index_probe_notices_one_changed_weight():
    """The comparison itself: one W byte changed behind the back of the expected values shows in exactly the outputs that select it."""
    row = A.TABLE_BY_NAME["a8_256_m257_n384_k640"]
    c = _to(A.index_case(row, gelu_from=row.N))
    p = c.probs[0]
    f = G.f_onehot(p.M, row.K, DEV)
    n = next(n for n in range(301, row.N) if int(p.W[n, f[200]]) & 0x7f)      # a non-zero weight
    p.W[n, f[200]] ^= 0x80                                            # its sign: the pre-activation moves by 2 |w| ascale wscale >= 0.75
    rows = (f == f[200]).nonzero().flatten().tolist()
    out = _launch(row, c)[0]
    want, _ = G.expected(c, p)
    assert G.check_exact(c, [out]) == len(rows) >= 1 and (G.bits(out) != G.bits(want)).nonzero().tolist() == [[m, n] for m in rows]


# ---- b. byte codes;  c. scale order and K-tile signatures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_fp8_byte_codes_scale_then_bias_and_k_tile_signatures(name):
    row = A.TABLE_BY_NAME[name]
    seen_a, seen_w = 0, 0
    for shift in range(2):
        c = A.bytecode_case(row, shift=shift)
        seen_a, seen_w = max(seen_a, c.a_codes_seen), max(seen_w, c.w_codes_seen)
        assert _exact(row, c) == 0
    if max(row.Ms) >= 257:
        assert seen_a == 254 and seen_w == 254
    assert _exact(row, A.scale_bias_case(row)) == 0
    assert _exact(row, A.signature_case(row)) == 0


# ---- d. GELU columns -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in A.TABLE if r.epi == "gelu"])
def test_gelu_from_a_column(name):
    row = A.TABLE_BY_NAME[name]
    for frm in (0, None, row.N):                                      # None: a multiple of 8, not of 16, inside a tile
        assert _exact(row, A.index_case(row, halves=True, gelu_from=frm)) == 0, frm


# ---- e. fp64 bound -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.BOUND_ROWS)
def test_fp64_bound(name):
    row = A.TABLE_BY_NAME[name]
    for family in G.FAMILIES:
        c = _to(A.bound_case(row, family))
        outs = _launch(row, c)
        r = A.bound_ratio(c, outs)
        print(f"{name} {family}: worst err / bound {r:.3f}")
        assert r <= 1.0, (family, r)
        assert all(torch.equal(a, b) for a, b in zip(_launch(row, c), outs)), "a repeated call must be bit-identical"


# ---- f. fused Q/K/V epilogue ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in A.QKV_TABLE])
def test_fused_qkv_epilogue_placement(name):
    row = A.TABLE_BY_NAME[name]
    c = _to(A.qkv_case(row))
    q, p = c.qkv, c.probs[0]
    out, ks, vt = p.out_init.clone(), q.k_init.clone(), q.vt_init.clone()
    epi = ops.qkv_epilogue(wq=q.wq, wk=q.wk, rope_q=q.rope_q, rope_k=q.rope_k, k_slab=ks, vt_slab=vt, H=q.H, k_col=q.k_col, v_col=q.v_col,
                           q_col=q.q_col, kv_rows=q.kv_rows, row_base=q.row_base, eps=q.eps, fp16_roundtrip=q.f16, rows=p.M)
    plan_helpers.force(**row.knobs)
    ops.gemm_qkv(_a8(row, p), _w8(p), p.bias, out[:p.M, :c.N], epi, gelu_from_col=c.gelu_from)
    plan = _lib.lib().rgn_gemm_last_plan()
    assert plan == row.plan, f"{name}: plan {plan:#x}, the table says {row.plan:#x}"
    assert G.outside_intact(p, out, c.N)
    assert G.check_qkv(c, (out, ks, vt)) == 0


# ---- g. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_destination_alone():
    row = A.TABLE_BY_NAME["a8_128_m130_n128_k256"]
    c = _to(A.scale_bias_case(row))
    p = c.probs[0]
    a, w = _a8(row, p), _w8(p)
    out = p.out_init.clone()
    view = out[:p.M, :row.N]
    rows = torch.arange(p.M, device=DEV)
    other = torch.zeros(p.M, row.N, dtype=torch.bfloat16, device=DEV)
    gate = torch.ones(row.N, dtype=torch.bfloat16, device=DEV)
    wb = torch.zeros(row.N, row.K, dtype=torch.bfloat16, device=DEV)
    bare = p.A.view(ops.FP8)                                                                    # no `_rgn_scale`
    a192 = torch.zeros(p.M, 192, dtype=torch.uint8, device=DEV).view(ops.FP8)
    a192._rgn_scale = p.ascale
    w192 = torch.zeros(row.N, 192, dtype=torch.uint8, device=DEV).view(ops.FP8)
    w192._rgn_scale = p.wscale
    odd = torch.zeros(p.M, row.K + 8, dtype=torch.uint8, device=DEV)[:, :row.K].view(ops.FP8)       # rows 8 bytes off a 16-byte boundary
    odd._rgn_scale = p.ascale
    abf = torch.zeros(p.M, row.K, dtype=torch.bfloat16, device=DEV)
    calls = {
        "gate_resid": lambda: ops.gemm(a, w, p.bias, view, epilogue=ops.EPI_GATE_RESID, gate=gate, resid=view),
        "out_rows": lambda: ops.gemm(a, w, p.bias, view, out_rows=rows),
        "bf16_weights": lambda: ops.gemm(a, wb, p.bias, view),
        "missing_scale": lambda: ops.gemm(bare, w, p.bias, view),
        "k_192": lambda: ops.gemm(a192, w192, p.bias, view),
        "misaligned_rows": lambda: ops.gemm(odd, w, p.bias, view),
        "mixed_formats": lambda: ops.gemm_group([ops.Problem(a, w, p.bias, view), ops.Problem(abf, w, p.bias, other)]),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.RegionEHipError):
            call()
        torch.cuda.synchronize()
        assert G.mismatches(out, p.out_init) == 0, name
    ops.gemm(a, w, p.bias, view)                                                                # and the accepted call still works
    assert G.check_exact(c, [out]) == 0
