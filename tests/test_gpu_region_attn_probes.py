"""-m gpu: exact probes and element-wise fp64 bounds for rgn_attention / rgn_attention_bounded (csrc/attn.hip) on every launch path of
attention_schedule: attention_kernel<4, 2> and <8, 3> (compiler-scheduled, ragged Skv, tail mask) unsplit and SPLIT,
attention_asm_kernel<0 | 1 | 2> with the running max and with the static shift, attention_asm64_kernel, attention_combine_kernel<128 | 256>,
attention_combine_sk_kernel, the stream-K two-segment loop, the XCD item map and the ragged last query block.

The inputs, the expected outputs, the checks and the table of launch paths (R.TABLE: shape, plan knobs, workspace, expected plan) come from
tests/region_attn_model.py; tests/test_region_attn_model.py shows on the CPU that the same checks reject a dropped key, a counted pad
key, a missing rescale, a dropped last tile of a piece, a run-boundary tile counted twice, a stale accumulator in the second stream-K
segment, a merge that ignores the piece maxima, a missing V^T group permutation, a wrong head and a ragged query block that reads the
next row - and that the plans of the table are what the scheduler chooses.  One test is one row of the table:

  a. counting probe (q = 0, integer V): every element equals, bit for bit, one of the two roundings of sum / Skv of its head;
  b. spike probe (one key 40 above the rest, at tile, piece and run edges): every row returns that V row bit for bit; on one row per
     kernel class also with O aliasing Q;
  c. wrong-head probe: V of head h is h + 1, head h returns h + 1 exactly (H = 3 and H = 24);
  d. |out - O_ref| <= 2^-8 A_ref + 2^-8 |O_ref| + 1e-6 element-wise against the fp64 softmax on N(0, 1) inputs, on logits of +-60 with
     the row maximum in the last key tile / on the first key, and on a staircase that keeps P above 1; the bounded path (score_bound = 66)
     on the same inputs; a repeated call is bit-identical;
  e. other garbage behind Skv (K rows NaN, V^T pad columns finite, the whole tile behind the padded length NaN) changes no bit.
Every launch builds the K slab and the V^T slab by hand (kvpos as written in include/regione_hip.h), with NaN in the K rows and 50.0 in
the V^T columns of no key, a Q whose row stride is wider than H * 128 and an O, prefilled with a sentinel, that is wider than H * 128 and
longer than Sq; it asserts rgn_attention_last_plan() against the table, and that the sentinel survives outside [Sq, H * 128].
The margins measured on an MI355X, next to the emulation's, are in profiles/r16_region_attn_probes.txt.
"""
import pytest
import torch

import plan_helpers
import region_attn_model as R
from regione_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENTINEL = 7.0
EXTRA_COLS, EXTRA_ROWS = 64, 3
ROWS = [r.name for r in R.TABLE]


def _slabs(c, poison):
    """K slab [skv_pad, H 128] and V^T slab [H 128, skv_pad], skv_pad one 64-row tile more than padded(Skv).  K rows >= Skv hold NaN.
    V^T column kvpos(r) holds key r; the columns of no key hold 50.0 (`poison`: -1e30, and NaN in the extra tile)."""
    H, Skv, _ = c.k.shape
    D, pad = H * 128, R.padded(Skv)
    ks = torch.full((pad + 64, D), NAN, dtype=torch.bfloat16, device=DEV)
    ks[:Skv] = c.k.permute(1, 0, 2).reshape(Skv, D)
    vt = torch.full((D, pad + 64), -1e30 if poison else 50.0, dtype=torch.bfloat16, device=DEV)
    if poison:
        vt[:, pad:] = NAN
    r = torch.arange(Skv, device=DEV)
    vt[:, R.kvpos(r)] = c.v.permute(0, 2, 1).reshape(D, Skv)
    return ks, vt


def _launch(row, c, bounded=False, poison=False, alias=False):
    """One call of ops.attention on the case (on the GPU) under the knobs and the workspace of the row: out [H, Sq, 128]."""
    H, Sq, _ = c.q.shape
    Skv, D = c.k.shape[1], H * 128
    assert (Sq, Skv, H) == (row.Sq, row.Skv, row.H)
    ks, vt = _slabs(c, poison)
    qbuf = torch.full((Sq + (EXTRA_ROWS if alias else 0), D + EXTRA_COLS), SENTINEL if alias else NAN, dtype=torch.bfloat16, device=DEV)
    qbuf[:Sq, :D] = c.q.permute(1, 0, 2).reshape(Sq, D)
    obuf = qbuf if alias else torch.full((Sq + EXTRA_ROWS, D + EXTRA_COLS), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ws = ops.attention_workspace(torch.device(DEV))
    assert ws.numel() * 4 >= row.ws
    plan_helpers.force(**row.knobs)
    ops.attention(qbuf[:Sq, :D], ks, vt, obuf[:Sq, :D], Skv, H, scale=c.scale, workspace=ws[:row.ws // 4],
                  score_bound=c.score_bound if bounded else 0.0)
    plan = _lib.lib().rgn_attention_last_plan()
    assert plan == R.expected_plan_bits(row), f"{row.name}: plan {plan:#x}, the table says {R.expected_plan_bits(row):#x}"
    assert bool((obuf[Sq:] == SENTINEL).all()) and bool((obuf[:Sq, D:] == SENTINEL).all()), "wrote outside [Sq, H * 128]"
    return obuf[:Sq, :D].reshape(Sq, H, 128).permute(1, 0, 2)


def _gpu(case):
    return R.to_device(case, DEV)


# ---- a. counting probe;  e. poison ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_counting_probe(name):
    row = R.TABLE_BY_NAME[name]
    c = _gpu(R.counting_case(row.Sq, row.Skv, row.H))
    for bounded in row.bounded:
        assert R.check_counting(c, _launch(row, c, bounded)) == 0, bounded


@pytest.mark.parametrize("name", ROWS)
def test_other_garbage_behind_skv_changes_no_bit(name):
    row = R.TABLE_BY_NAME[name]
    c = _gpu(R.bound_case("randn", row.Sq, row.Skv, row.H))
    for bounded in row.bounded:
        first = _launch(row, c, bounded)
        assert bool(torch.isfinite(first.float()).all())
        assert torch.equal(_launch(row, c, bounded, poison=True), first), bounded


# ---- b. spike probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_spike_probe(name):
    row = R.TABLE_BY_NAME[name]
    for j in R.spike_keys(row):
        c = _gpu(R.spike_case(row.Sq, row.Skv, row.H, j))
        for bounded in row.bounded:
            out = _launch(row, c, bounded)
            assert R.check_spike(c, out) == 0, (j, bounded)
            if name in R.CLASS_ROWS and j == row.Skv - 1:
                assert torch.equal(_launch(row, c, bounded, alias=True), out), "O aliasing Q changed the result"


# ---- c. wrong-head probe --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r.name for r in R.WRONG_HEAD_TABLE])
def test_wrong_head_probe(name):
    row = R.ALL_ROWS[name]
    c = _gpu(R.wrong_head_case(row.Sq, row.Skv, row.H))
    for bounded in row.bounded:
        assert R.check_wrong_head(c, _launch(row, c, bounded)) == 0, bounded


# ---- d. fp64 bound, element-wise; a repeated call is bit-identical ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ROWS)
def test_fp64_bound(name):
    row = R.TABLE_BY_NAME[name]
    rows = None if row.H * row.Sq * row.Skv <= 2 ** 26 else R.bound_rows(row.Sq).to(DEV)
    for family in R.FAMILIES:
        c = _gpu(R.bound_case(family, row.Sq, row.Skv, row.H))
        R.check_stress_shape(c, rows)                               # max |s| <= 64 <= score_bound in fp64; the maximum where the family puts it
        for bounded in row.bounded:
            out = _launch(row, c, bounded)
            r = R.bound_ratio(c, out, rows)                         # asserts that the fp64 reference is finite
            print(f"{name} {family} bounded={bounded}: worst err / bound {r:.3f}")
            assert r <= 1.0, (family, bounded, r)
            assert torch.equal(_launch(row, c, bounded), out), "a repeated call must be bit-identical"
