"""-m gpu: exact probes and element-wise fp64 bounds for rgn_gemm_group (csrc/gemm.hip) on every launch path of launch_mode / gemm_schedule:
the three geometries, FULL / PARTIAL / REDUCE, the two-stage, ring and fp8 loops (AV 0 / 1 / 8 / 9), gemm_reduce4w_kernel x 3 epilogues, the
8-wave reduce over 4-wave partials (fused Q/K/V), quarter tiles, whole rounds plus remainder (257 tiles), the K split of the 128 geometry,
groups, strided operands and the row scatter.

Inputs, expected outputs, checks and the table of launch paths (G.TABLE / G.QKV_TABLE: shape, weight format, epilogue, plan knobs, expected
plan word, and the comment block that lists the kernel instantiations against the rows) come from tests/gemm_model.py;
tests/test_gemm_model.py shows on the CPU that the same checks reject 19 named defects and that the table's plans are the planner's.  One
test is one row of the table:

  a. index probe (one-hot A, integer W that depends on n and k, integer bias; as many passes as it takes for the rows to select every
     k): every output bit for bit;
  b. K-tile signature probe (every 32-wide half step of a window of four K tiles adds its own power of two, the sign keyed by channel and
     K tile) and the count probe A = W = 1: bit for bit;
  c. epilogue probes on exact pre-activations: gated residual in place and out of place with the two roundings; GELU from column 0, from
     a multiple of 8 inside a tile, from N - linear columns exact, GELU columns one of the two bf16 neighbours of the fp64 tanh-GELU of
     bf16(lin), pre-activations on the halves in [-8, 8]; the row scatter leaves every unnamed row alone (rows scat*);
  d. fp8: all 254 finite e4m3fn codes x power-of-two scales; scale-then-bias with scales that are no power of two;
  e. |out - ref64| <= 2^-8 |ref64| + K 2^-23 sum|a w| + tiny on N(0, 1) sigma and on cancelling operands (rows with K <= 512); a repeated
     call is bit-identical;
  f. NaN outside the problem (A rows / columns, W rows, bias / gate / scale tails, residual frame, the split-K workspace) changes no bit;
  g. fused Q/K/V epilogue: Q in out, K in the slab row kv_rows names, V^T at kvpos - integer arithmetic, bit for bit, sentinels elsewhere.
Every launch writes into a view of a buffer prefilled with a sentinel (3 rows longer, 8 columns wider) and asserts rgn_gemm_last_plan()
against the table.  The margins measured on an MI355X are in profiles/r21_gemm_probes.txt.
"""
import pytest
import torch

import gemm_model as G
import plan_helpers
from regione_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
ALL = [r.name for r in G.TABLE]
EPI = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_GELU, "gate": ops.EPI_GATE_RESID}


def _dev_of(row):
    return DEV if row.feat.get("huge") else "cpu"           # the 257-tile and K = 15360 operands are built on the device


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


def _framed(t, rows, cols, fill, dtype=None, row0=0, col0=0):
    """t [r, c] as a view into a buffer [r + rows, c + cols] filled with `fill`, at (row0, col0)."""
    buf = torch.full((t.shape[0] + rows, t.shape[1] + cols), fill, dtype=dtype or t.dtype, device=DEV)
    view = buf[row0:row0 + t.shape[0], col0:col0 + t.shape[1]]
    view.copy_(t)
    return view


def _tail(v, fill):
    """v [N] as the head of a buffer 16 elements longer."""
    buf = torch.full((v.numel() + 16,), fill, dtype=v.dtype, device=DEV)
    buf[:v.numel()] = v
    return buf[:v.numel()]


def _operands(row, case, p, pad, poison):
    """A, W (with its scale), bias, gate of one problem: dense, or (pad) views into buffers whose surroundings hold zeros / (poison) NaN."""
    fill = NAN if poison else 0.0
    lda, ldw = row.feat.get("lda", 0), row.feat.get("ldw", 0)
    A, W, bias, gate, ws = p.A, p.W, p.bias, p.gate, p.wscale
    if pad or lda:
        A = _framed(A, G.XR, lda or 64, fill, row0=0, col0=8 if pad else 0)
    if ws is not None:
        if pad:
            W = _framed(W, 8, 0, 0x7f if poison else 0)                # 0x7f: the NaN code of e4m3fn
            ws = _tail(ws, fill)
        W = W.view(ops.FP8)
        W._rgn_scale = ws
    elif pad or ldw:
        W = _framed(W, 8 if pad else 0, ldw, fill)
    if pad:
        bias = _tail(bias, fill) if bias is not None else None
        gate = _tail(gate, fill) if gate is not None else None
    return A, W, bias, gate


def _launch(row, case, pad=False, poison=False):
    """One call of ops.gemm / ops.gemm_group on the case under the knobs of the row: the destination buffers, whole."""
    probs, outs = [], []
    for p in case.probs:
        buf = p.out_init.clone()
        outs.append(buf)
        if p.M == 0:
            probs.append(ops.Problem(p.A, p.W if p.wscale is None else p.W.view(ops.FP8), p.bias, buf[:0, :case.N]))
            continue
        A, W, bias, gate = _operands(row, case, p, pad, poison)
        out, resid = buf[:p.R, :case.N], None
        if case.epi == "gate":
            resid = out if case.inplace else _framed(p.resid, G.XR, G.XC, NAN if poison else 0.0)
        probs.append(ops.Problem(A, W, bias, out, gate, resid, None, p.out_rows))
    if poison:
        ops.gemm_workspace(torch.device(DEV)).fill_(NAN)
    plan_helpers.force(**row.knobs)
    if len(probs) == 1:
        q = probs[0]
        ops.gemm(q.A, q.W, q.bias, q.out, epilogue=EPI[case.epi], gelu_from_col=case.gelu_from, gate=q.gate, resid=q.resid, out_rows=q.out_rows)
    else:
        ops.gemm_group(probs, epilogue=EPI[case.epi], gelu_from_col=case.gelu_from)
    plan = _lib.lib().rgn_gemm_last_plan()
    assert plan == row.plan, f"{row.name}: plan {plan:#x}, the table says {row.plan:#x}"
    for p, buf in zip(case.probs, outs):
        assert G.outside_intact(p, buf, case.N), "wrote outside the problem's rows / columns"
    return outs


def _exact(row, case):
    case = _to(case)
    bad = G.check_exact(case, _launch(row, case))
    if case.epi == "gelu":
        print(f"{row.name} {case.kind} gelu_from={case.gelu_from}: GELU outputs not correctly rounded {100 * case.gelu_share:.2f} %")
    return bad


# ---- a. index probe;  b. signature and count probes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_index_probe(name):
    row = G.TABLE_BY_NAME[name]
    for shift in range(G.index_shifts(row)):                          # every k selected by some row
        assert _exact(row, G.index_case(row, _dev_of(row), shift=shift)) == 0, shift


def test_index_probe_notices_one_changed_weight():
    """The comparison itself: one W element changed behind the back of the expected values shows in exactly the outputs that select it."""
    row = G.TABLE_BY_NAME["f256_ring"]
    c = _to(G.index_case(row, gelu_from=row.N))
    p = c.probs[0]
    f, n = G.f_onehot(p.M, row.K, DEV), 301
    p.W[n, f[777]] += 2
    rows = (f == f[777]).nonzero().flatten().tolist()                 # 1100 rows, K = 512: rows 265 and 777
    out = _launch(row, c)[0]
    want, _ = G.expected(c, p)
    assert G.check_exact(c, [out]) == len(rows) == 2 and (G.bits(out) != G.bits(want)).nonzero().tolist() == [[m, n] for m in rows]


@pytest.mark.parametrize("name", ALL)
def test_k_tile_signature_and_count_probes(name):
    row = G.TABLE_BY_NAME[name]
    assert _exact(row, G.signature_case(row, _dev_of(row))) == 0
    assert _exact(row, G.count_case(row, _dev_of(row))) == 0


# ---- c. epilogue probes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in G.TABLE if r.epi == "gate"])
def test_gated_residual_in_place_and_out_of_place(name):
    row = G.TABLE_BY_NAME[name]
    for inplace in (True, False):
        assert _exact(row, G.index_case(row, inplace=inplace)) == 0, inplace


@pytest.mark.parametrize("name", [r.name for r in G.TABLE if r.epi == "gelu"])
def test_gelu_from_a_column(name):
    row = G.TABLE_BY_NAME[name]
    for frm in (0, None, row.N):                                      # None: a multiple of 8, not of 16, inside a tile
        assert _exact(row, G.index_case(row, halves=True, gelu_from=frm)) == 0, frm


# ---- d. fp8 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in G.TABLE if r.w8])
def test_fp8_byte_codes_and_scale_then_bias(name):
    row = G.TABLE_BY_NAME[name]
    c = G.bytecode_case(row)
    assert c.codes_seen == 254
    assert _exact(row, c) == 0
    assert _exact(row, G.scale_bias_case(row)) == 0


# ---- e. fp64 bound ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.BOUND_ROWS)
def test_fp64_bound(name):
    row = G.TABLE_BY_NAME[name]
    for family in G.FAMILIES:
        c = _to(G.bound_case(row, family))
        outs = _launch(row, c)
        r = G.bound_ratio(c, outs)
        print(f"{name} {family}: worst err / bound {r:.3f}")
        assert r <= 1.0, (family, r)
        assert all(torch.equal(a, b) for a, b in zip(_launch(row, c), outs)), "a repeated call must be bit-identical"


# ---- f. garbage outside the problem -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.GARBAGE_ROWS)
def test_garbage_outside_the_problem_changes_no_bit(name):
    row = G.TABLE_BY_NAME[name]
    c = _to(G.bound_case(row, "randn") if row.epi == "bias" else G.index_case(row))
    clean = _launch(row, c, pad=True)
    for p, buf in zip(c.probs, clean):
        assert bool(torch.isfinite(buf.float()).all())
    dirty = _launch(row, c, pad=True, poison=True)
    assert all(torch.equal(a, b) for a, b in zip(dirty, clean))
    if c.kind == "index":
        assert G.check_exact(c, clean) == 0


# ---- g. fused Q/K/V epilogue --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in G.QKV_TABLE])
def test_fused_qkv_epilogue_placement(name):
    row = G.TABLE_BY_NAME[name]
    c = _to(G.qkv_case(row))
    q, p = c.qkv, c.probs[0]
    out, ks, vt = p.out_init.clone(), q.k_init.clone(), q.vt_init.clone()
    epi = ops.qkv_epilogue(wq=q.wq, wk=q.wk, rope_q=q.rope_q, rope_k=q.rope_k, k_slab=ks, vt_slab=vt, H=q.H, k_col=q.k_col, v_col=q.v_col,
                           q_col=q.q_col, kv_rows=q.kv_rows, row_base=q.row_base, eps=q.eps, fp16_roundtrip=q.f16, rows=p.M)
    plan_helpers.force(**row.knobs)
    ops.gemm_qkv(p.A, p.W, p.bias, out[:p.M, :c.N], epi, gelu_from_col=c.gelu_from)
    plan = _lib.lib().rgn_gemm_last_plan()
    assert plan == row.plan, f"{name}: plan {plan:#x}, the table says {row.plan:#x}"
    assert G.outside_intact(p, out, c.N)
    assert G.check_qkv(c, (out, ks, vt)) == 0
