"""CPU: the checks of tests/gemm_model.py have teeth, and the table's plans are the planner's.

  * the unmutated emulation passes every check on every row of the table (the 257-tile rows as 5 tiles on 4 workgroup slots);
  * every mutant of G.MUTANTS is rejected by at least one check on at least one row (the matrix mutant x check is printed);
  * rgn_gemm_plan_query under each row's knobs returns the row's plan word (host arithmetic: no GPU);
  * for the fp64 bound, a plain fp32 CPU matmul of the same inputs stays inside the bound (the reference alone meets the condition).
tests/test_gpu_gemm_probes.py applies the same checks to the kernels."""
import ctypes as C

import pytest
import torch

import gemm_model as G
import plan_helpers
from regione_amd import _lib

CHECKS = ("index", "signature", "count", "epilogue", "bytecode", "scale_bias", "bound", "qkv")
# the rows a mutant is tried on: the smallest whose launch structure can express it
MUTANT_ROWS = {
    "piece_last_tile_dropped": ["pc256_av0"], "piece_boundary_tile_twice": ["pc256_av0"], "reduce_skips_piece": ["pc256_av0", "pc256c_w8"],
    "partial_slot_of_wrong_tile": ["r257_pieces"], "a_half_steps_swapped": ["f128_ragged"], "c_fragment_transposed": ["f128_ragged"],
    "group_m_two_tiles_swapped": ["f256_k192"], "quadrant_bits_exchanged": ["quarter_w8"], "edge_row_plus_one": ["f128_ragged"],
    "write_row_M": ["f128_ragged", "f128_w8"], "gelu_boundary_off_by_8": ["f256c_w8"], "bias_of_neighbour_tile": ["f128_ragged"],
    "group_uses_problem_0": ["grp128"], "scatter_to_m": ["scat128_perm"], "wscale_after_bias": ["f128_w8"], "e4m3fnuz_decode": ["f128_w8"],
    "kvpos_omitted": ["qkv256_pieces"], "cos_k_by_sequence_row": ["qkv256_pieces"], "rotation_pair_swapped": ["qkv256_pieces"],
}


def _cpu_row(name):
    row = G.TABLE_BY_NAME[name]
    return G.small_twin(row) if name.startswith("r257") else row


def epilogue_variants(row):
    """c. gated residual in place and out of place; GELU from column 0, from a multiple of 8 (not of 16) inside a tile, from N (none)."""
    if row.epi == "gate":
        return [dict(inplace=True), dict(inplace=False)]
    if row.epi == "gelu":
        return [dict(gelu_from=0, halves=True), dict(halves=True), dict(gelu_from=row.N, halves=True)]
    return []


def run_checks(row, mutant=None):
    """check -> violations (bound: 1 where the ratio exceeds 1) of the emulation of `row`."""
    res = {}
    if row.epi == "qkv":
        c = G.qkv_case(row)
        res["qkv"] = G.check_qkv(c, G.emulate(c, row, mutant)[0])
        return res
    res["index"] = 0
    for shift in sorted({0, G.index_shifts(row) - 1}):                # the first and the last pass over the k's
        c = G.index_case(row, shift=shift)
        res["index"] += G.check_exact(c, G.emulate(c, row, mutant))
    for kind, make in (("signature", G.signature_case), ("count", G.count_case)):
        c = make(row)
        res[kind] = G.check_exact(c, G.emulate(c, row, mutant))
    res["epilogue"] = 0
    for kw in epilogue_variants(row):
        c = G.index_case(row, **kw)
        res["epilogue"] += G.check_exact(c, G.emulate(c, row, mutant))
    if row.w8:
        c = G.bytecode_case(row)
        assert c.codes_seen == 254
        res["bytecode"] = G.check_exact(c, G.emulate(c, row, mutant))
        c = G.scale_bias_case(row)
        res["scale_bias"] = G.check_exact(c, G.emulate(c, row, mutant))
    if row.name in G.BOUND_ROWS:
        res["bound"] = 0
        for fam in G.FAMILIES:
            c = G.bound_case(row, fam)
            r = G.bound_ratio(c, G.emulate(c, row, mutant))
            res["bound_ratio_" + fam] = r
            res["bound"] += int(not r <= 1.0)
    return res


@pytest.mark.parametrize("name", [r.name for r in G.TABLE + G.QKV_TABLE])
def test_unmutated_emulation_passes_every_check(name):
    res = run_checks(_cpu_row(name))
    print(name, res)
    assert all(v == 0 for k, v in res.items() if not k.startswith("bound_ratio")), res


def test_every_mutant_is_rejected_by_some_check():
    assert set(MUTANT_ROWS) == set(G.MUTANTS)
    lines, missed = [], []
    for mut in G.MUTANTS:
        total = dict.fromkeys(CHECKS, 0)
        for name in MUTANT_ROWS[mut]:
            for k, v in run_checks(_cpu_row(name), mut).items():
                if k in total:
                    total[k] += v
        lines.append(f"{mut:<30s}" + "".join(f"{total[c]:>12d}" for c in CHECKS))
        if not any(total.values()):
            missed.append(mut)
    print("\nviolating elements, mutant x check (rows: MUTANT_ROWS)\n" + " " * 30 + "".join(f"{c:>12s}" for c in CHECKS) + "\n" + "\n".join(lines))
    assert not missed, missed


@pytest.mark.parametrize("name", [r.name for r in G.TABLE + G.QKV_TABLE])
def test_table_plan_is_the_planners(name):
    row = G.TABLE_BY_NAME[name]
    Ms, N, K, dw, w8 = G.plan_query_args(row)
    h = _lib.lib()
    h.rgn_plan_override(None, 0)
    try:
        plan_helpers.force(**row.knobs)
        got = h.rgn_gemm_plan_query((C.c_int * len(Ms))(*Ms), len(Ms), N, K, dw, w8, h.rgn_gemm_workspace_bytes())
    finally:
        h.rgn_plan_override(None, 0)
    assert got == row.plan, f"{name}: planner {got:#x}, table {row.plan:#x}"


def test_plan_word_reports_the_128_geometry_split_and_nothing_else_changes():
    """Bits 12-15 = pieces chosen by split128; 0 when unsplit, when there is no workspace, on the 256 geometry and under gemm_pieces = 1."""
    h = _lib.lib()
    one = (C.c_int * 1)(300)
    ws = h.rgn_gemm_workspace_bytes()
    h.rgn_plan_override(None, 0)
    try:
        plan_helpers.force(gemm_geometry=128)
        assert h.rgn_gemm_plan_query(one, 1, 200, 15360, 1, 0, ws) == 6 << 12
        assert h.rgn_gemm_plan_query(one, 1, 200, 15360, 1, 0, 0) == 0
        assert h.rgn_gemm_plan_query(one, 1, 200, 512, 1, 0, ws) == 0
        plan_helpers.force(gemm_pieces=1)
        assert h.rgn_gemm_plan_query(one, 1, 200, 15360, 1, 0, ws) == 0
        plan_helpers.force(gemm_pieces=-1, gemm_geometry=256)
        assert h.rgn_gemm_plan_query(one, 1, 200, 15360, 1, 0, ws) >> 12 == 0
    finally:
        h.rgn_plan_override(None, 0)


@pytest.mark.parametrize("name", G.BOUND_ROWS)
def test_fp32_cpu_matmul_stays_inside_the_fp64_bound(name):
    row = G.TABLE_BY_NAME[name]
    for fam in G.FAMILIES:
        c = G.bound_case(row, fam)
        outs = []
        for p in c.probs:
            got = p.out_init.clone()
            if p.M:
                acc = p.A.float() @ G.w_values(p).float().t()
                got[G._rows_of(p), :c.N] = (acc * (p.wscale if p.wscale is not None else 1.0) + p.bias.float()).to(G.BF16)
            outs.append(got)
        r = G.bound_ratio(c, outs)
        print(f"{name} {fam}: fp32 CPU matmul worst err / bound {r:.3f}")
        assert r <= 1.0, (fam, r)


def test_number_format_helpers():
    v = G.e4m3fn_table()
    assert torch.equal(torch.nan_to_num(v, nan=7e7).float(), torch.nan_to_num(torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float(), nan=7e7))
    x = torch.tensor([1.0, 1.001, -1.001, 3e-5, -8.0, 0.0, 1e-45, -1e-45], dtype=torch.float64)
    lo, hi = G.bf16_neighbours(x)
    assert bool((lo <= x).all()) and bool((x <= hi).all())
    assert lo[0] == hi[0] == 1.0 and lo[1] == 1.0 and hi[1] == 1.0078125 and lo[2] == -1.0078125 and hi[2] == -1.0 and lo[5] == hi[5] == 0.0
    assert hi[6] > 0 and lo[6] == 0 and lo[7] < 0 and hi[7] == 0
    r = torch.arange(64)
    assert torch.equal(G.kvpos(G.kvpos(r)), r) and int(G.kvpos(torch.tensor(4))) == 8
