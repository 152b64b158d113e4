"""CPU: the checks of tests/gemm_a8_model.py have teeth, the table's plans are the planner's, and the fp8-activation refusals of
rgn_gemm_group come before any launch.

  * the unmutated emulation (K tiles of 128, (acc * ascale[m]) * wscale[n] + bias) passes every probe on every row of the table;
  * every defect of A.MUTANTS changes at least one probe output (the matrix mutant x probe is printed): K halves of a fragment swapped,
    lane groups permuted, the row scale of the tile row instead of the global row, both scales after the bias, the last K tile dropped,
    amax over K - 1 columns;
  * rgn_gemm_plan_query(w8 = 2) under each row's knobs returns the row's plan word, never a K split;
  * a plain fp32 CPU matmul of the quantised operands stays inside the fp64 bound (the reference alone meets the condition);
  * the quantiser model is ops.quantize_w8 per row, and every refusal returns RGN_E_UNSUPPORTED with a message (no GPU: validation only).
tests/test_gpu_gemm_a8_probes.py and tests/test_gpu_quantize_rows.py apply the same checks to the kernels."""
import ctypes as C

import pytest
import torch

import gemm_a8_model as A
import gemm_model as G
import plan_helpers
from regione_amd import _lib

CHECKS = ("index", "bytecode", "scale_bias", "signature", "epilogue", "bound", "qkv", "quantise")
MUTANT_ROWS = {
    "k_halves_swapped": ["a8_128_m130_n128_k128"], "lane_groups_permuted": ["a8_256_m130_n128_k128"],
    "row_scale_of_tile_row": ["a8_128_m257_n128_k128", "a8_quarter"], "scales_after_bias": ["a8_128_m130_n384_k256"],
    "last_k_tile_dropped": ["a8_256_m130_n384_k640", "a8_128_m1_n128_k128"], "amax_k_minus_1": ["a8_128_m130_n128_k128"],
}


def quantise_probe(mutant=None):
    """Violating bytes / scales of the (mutated) quantiser model against the torch expression on the rows of A.quant_rows."""
    bad = 0
    for K in (128, 3072):
        x = torch.stack(list(A.quant_rows(K).values()))
        q, s = A.quantize_rows(x, mutant)
        xf = x.float()
        ws = xf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
        wq = (xf / ws[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
        bad += int((q != wq).sum()) + int((s.view(torch.int32) != ws.view(torch.int32)).sum())
    return bad


def run_checks(row, mutant=None):
    res = {}
    if row.epi == "qkv":
        c = A.qkv_case(row)
        res["qkv"] = G.check_qkv(c, A.emulate(c, row, mutant)[0])
        return res
    res["index"] = 0
    for shift in sorted({0, A.index_shifts(row) - 1}):
        c = A.index_case(row, shift=shift)
        res["index"] += G.check_exact(c, A.emulate(c, row, mutant))
    for kind, make in (("bytecode", A.bytecode_case), ("scale_bias", A.scale_bias_case), ("signature", A.signature_case)):
        c = make(row)
        res[kind] = G.check_exact(c, A.emulate(c, row, mutant))
    res["epilogue"] = 0
    if row.epi == "gelu":
        for frm in (0, None, row.N):
            c = A.index_case(row, halves=True, gelu_from=frm)
            res["epilogue"] += G.check_exact(c, A.emulate(c, row, mutant))
    res["bound"] = 0
    for fam in G.FAMILIES:
        c = A.bound_case(row, fam)
        r = A.bound_ratio(c, A.emulate(c, row, mutant))
        res["bound_ratio_" + fam] = r
        res["bound"] += int(not r <= 1.0)
    return res


@pytest.mark.parametrize("name", [r.name for r in A.TABLE + A.QKV_TABLE])
def test_unmutated_emulation_passes_every_check(name):
    res = run_checks(A.TABLE_BY_NAME[name])
    print(name, res)
    assert all(v == 0 for k, v in res.items() if not k.startswith("bound_ratio")), res


def test_unmutated_quantiser_model_is_the_torch_expression():
    assert quantise_probe() == 0


def test_every_mutant_changes_some_probe_output():
    assert set(MUTANT_ROWS) == set(A.MUTANTS)
    lines, missed = [], []
    for mut in A.MUTANTS:
        total = dict.fromkeys(CHECKS, 0)
        for name in MUTANT_ROWS[mut]:
            for k, v in run_checks(A.TABLE_BY_NAME[name], mut).items():
                if k in total:
                    total[k] += v
        total["quantise"] = quantise_probe(mut)
        lines.append(f"{mut:<26s}" + "".join(f"{total[c]:>12d}" for c in CHECKS))
        if not any(total.values()):
            missed.append(mut)
    print("\nviolating elements, mutant x probe (rows: MUTANT_ROWS)\n" + " " * 26 + "".join(f"{c:>12s}" for c in CHECKS) + "\n" + "\n".join(lines))
    assert not missed, missed


def test_index_probe_selects_every_k_and_both_operands_see_every_code():
    for row in A.TABLE:
        if max(row.Ms) > 1:
            ks = torch.cat([G.f_onehot(max(row.Ms), row.K, "cpu", s) for s in range(A.index_shifts(row))])
            assert ks.unique().numel() == row.K, row.name
    c = A.bytecode_case(A.TABLE_BY_NAME["a8_128_m257_n384_k256"])
    assert c.a_codes_seen == 254 and c.w_codes_seen == 254


@pytest.mark.parametrize("name", [r.name for r in A.TABLE + A.QKV_TABLE])
def test_table_plan_is_the_planners(name):
    row = A.TABLE_BY_NAME[name]
    Ms, N, K, dw, w8 = A.plan_query_args(row)
    h = _lib.lib()
    h.rgn_plan_override(None, 0)
    try:
        plan_helpers.force(**row.knobs)
        got = h.rgn_gemm_plan_query((C.c_int * len(Ms))(*Ms), len(Ms), N, K, dw, w8, h.rgn_gemm_workspace_bytes())
    finally:
        h.rgn_plan_override(None, 0)
    assert got == row.plan, f"{name}: planner {got:#x}, table {row.plan:#x}"


def test_fp8_activation_plans_never_cut_k():
    """Whole-K tiles only: the trunk's shapes, a forced piece count and a long K all report one piece (bits 0-7 <= 1, bits 12-15 = 0)."""
    h = _lib.lib()
    ws = h.rgn_gemm_workspace_bytes()
    h.rgn_plan_override(None, 0)
    try:
        for Ms, N, K in (((8704,), 21504, 3072), ((8704,), 9216, 3072), ((1536,), 12288, 3072), ((512, 1536), 9216, 3072), ((300,), 128, 15360)):
            arr = (C.c_int * len(Ms))(*Ms)
            for knobs in ({}, dict(gemm_pieces=3), dict(gemm_geometry=128), dict(gemm_geometry=256)):
                h.rgn_plan_override(None, 0)
                plan_helpers.force(**knobs)
                plan = h.rgn_gemm_plan_query(arr, len(Ms), N, K, 1, 2, ws)
                assert plan >= 0 and (plan & 0xff) <= 1 and (plan >> 12) == 0, (Ms, N, K, knobs, hex(plan))
        assert h.rgn_gemm_plan_query((C.c_int * 1)(300), 1, 128, 192, 1, 2, ws) < 0          # K % 128
    finally:
        h.rgn_plan_override(None, 0)


@pytest.mark.parametrize("name", ["a8_128_m130_n128_k128", "a8_128_m257_n384_k640", "a8_256_m130_n384_k256", "a8_grp128"])
def test_fp32_cpu_matmul_stays_inside_the_fp64_bound(name):
    row = A.TABLE_BY_NAME[name]
    tab = G.e4m3fn_table().float()
    for fam in G.FAMILIES:
        c = A.bound_case(row, fam)
        outs = []
        for p in c.probs:
            got = p.out_init.clone()
            acc = tab[p.A.long()] @ tab[p.W.long()].t()
            got[:p.M, :c.N] = (acc * p.ascale[:, None] * p.wscale[None, :] + p.bias.float()).to(G.BF16)
            outs.append(got)
        r = A.bound_ratio(c, outs)
        print(f"{name} {fam}: fp32 CPU matmul worst err / bound {r:.3f}")
        assert r <= 1.0, (fam, r)


def test_quantiser_model_is_quantize_w8_per_row():
    from regione_amd import ops
    x = torch.stack(list(A.quant_rows(128).values()))
    q, s = A.quantize_rows(x)
    w = ops.quantize_w8(x)
    assert torch.equal(q, w.view(torch.uint8)) and torch.equal(s, w._rgn_scale)


def test_refusals_come_before_any_launch():
    """`ascale` needs fp8 weights, K % 128 == 0, 16-byte aligned rows, one of the BIAS / GELU / QKV epilogues, no row scatter and one A
    format per call: each returns RGN_E_UNSUPPORTED (-2) with a message, on never-dereferenced addresses (validation precedes every launch)."""
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()

    def prob(A_=P, W=P, C_=P, lda=128, ldc=64, M=8, ldw=0, wscale=P, ascale=P, out_rows=None, gate=None, resid=None):
        return _lib.GemmProblem(A_, W, wscale, None, C_, gate, resid, None, out_rows, lda, ldc, M, ldw, ascale)

    def group(probs, N=64, K=128, epilogue=0, gelu_from_col=0):
        arr = (_lib.GemmProblem * len(probs))(*probs)
        return h.rgn_gemm_group(arr, len(probs), N, K, epilogue, gelu_from_col, None, 0, None)
    assert group([prob(wscale=None)]) == -2 and "fp8 weights" in msg()
    assert group([prob(lda=64)], K=64) == -2 and "multiple of 128" in msg()
    assert group([prob(lda=192)], K=192) == -2 and "multiple of 128" in msg()
    assert group([prob(lda=136)]) == -2 and "16-byte aligned" in msg()
    assert group([prob(lda=64)]) == -2 and "16-byte aligned" in msg()                      # lda (bytes) < K
    assert group([prob(A_=P + 8)]) == -2 and "aligned" in msg()
    assert group([prob(gate=P, resid=P)], epilogue=2) == -2 and "epilogue" in msg()
    assert group([prob()], epilogue=4) == -2 and "epilogue" in msg()                       # RGN_EPI_CONV is not an rgn_gemm_group epilogue
    assert group([prob(out_rows=P)]) == -2 and "out_rows" in msg()
    assert group([prob(), prob(ascale=None, lda=64)]) == -2 and "same format" in msg()
    assert group([prob(M=0), prob(M=0, ascale=None)]) == 0                                 # empty problems are dropped first
