"""-m gpu: exact probes and element-wise fp64 bounds for the three sequence front ends of the flash-attention tile core
(csrc/attn_tile.h): rgn_text_attention_bf16, rgn_lm_attention_bf16, rgn_vision_attention_bf16.

The inputs, the expected outputs and the checks come from tests/attn_tile_model.py; tests/test_attn_tile_model.py shows on the CPU
that the same checks reject a dropped key, a counted pad key, a causal off-by-one, a shifted or edge-wrong bias read, a wrong
grouped-query head map and a missing rescale.  Lengths sit on the boundaries of the 32-key tile and the 64-query block (1, 31, 32, 33,
63, 64, 65, 97, 129) plus one long case per kernel; heads stay small.

  a. counting probe (q = 0, integer V): every element equals, bit for bit, one of the two roundings of sum / count;
  b. spike probe (text, bias table zero but +40 at one offset): the rows that see the spike return that V row bit for bit;
  c. head-map probe (LM): V of KV head g is g + 1, query head h returns h // (Hq / Hkv) + 1 exactly;
  d. |out - O_ref| <= 2^-8 A_ref + 2^-8 |O_ref| + 1e-6 element-wise against the fp64 softmax, on N(0, 1) inputs and on logits of +-60
     with the row maximum in the last key tile / on the first key;  f. and a repeated call on those inputs is bit-identical;
  e. NaN rows behind row L (and in a vision segment no item names) change no bit, and output rows nobody owns keep their sentinel.
The margins measured on an MI355X, next to the emulation's, are in profiles/r13_attn_tile_probes.txt.
"""
import pytest
import torch

import attn_tile_model as M
from regione_amd import _lib, ops
from regione_amd import qwen_vision as QV

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream
SENTINEL = 7.0
DEV = "cuda"
NAN = float("nan")


def _launch(case, qkv, o, L, items=None):
    """One call of the kernel of the case on a packed QKV buffer [rows >= L, (Hq + 2 Hkv) D] and O [rows >= L, Hq D]."""
    Hq, _, D = case.q.shape
    Hkv = case.k.shape[0]
    lib = _lib.lib()
    assert qkv.is_contiguous() and o.is_contiguous() and qkv.shape[0] >= L and o.shape[0] >= L
    assert qkv.shape[1] == (Hq + 2 * Hkv) * D and o.shape[1] == Hq * D
    if case.kind == "text":
        assert D == 64 and Hq == Hkv and (case.table is None or tuple(case.table.shape) == (Hq, 2 * case.Lmax - 1))
        rc = lib.rgn_text_attention_bf16(_p(qkv), _p(o), L, Hq, case.scale, int(case.causal), _p(case.table), case.Lmax, _stream())
        _lib.check(rc, "rgn_text_attention_bf16")
    elif case.kind == "lm":
        assert D == 128 and case.causal
        _lib.check(lib.rgn_lm_attention_bf16(_p(qkv), _p(o), L, Hq, Hkv, case.scale, _stream()), "rgn_lm_attention_bf16")
    else:
        assert items.dtype == torch.int32 and items.is_contiguous() and items.shape[1] == 4
        rc = lib.rgn_vision_attention_bf16(_p(qkv), _p(o), L, Hq, D, case.scale, _p(items), items.shape[0], _stream())
        _lib.check(rc, "rgn_vision_attention_bf16")


def _pack(c):
    """q [Hq, L, D], k, v [Hkv, L, D] -> the fused QKV GEMM layout [L, (Hq + 2 Hkv) D]."""
    return torch.cat([c.q, c.k, c.v], 0).permute(1, 0, 2).reshape(c.q.shape[1], -1).contiguous()


def _items(c):
    return QV.attention_items(M.cu_of(c.segs)).to(DEV) if c.kind == "vision" else None


def _run(case, items=None, tail=0, fill=NAN):
    """The kernel on the case (moved to the GPU): (case on the GPU, out [Hq, L, D], the whole O buffer).  `tail` rows of NaN follow
    row L of QKV, and as many rows of `fill` follow row L of O; O starts as `fill` everywhere."""
    c = M.to_device(case, DEV)
    Hq, L, D = c.q.shape
    qkv = torch.full((L + tail, (Hq + 2 * c.k.shape[0]) * D), NAN, dtype=torch.bfloat16, device=DEV)
    qkv[:L] = _pack(c)
    o = torch.full((L + tail, Hq * D), fill, dtype=torch.bfloat16, device=DEV)
    _launch(c, qkv, o, L, _items(c) if items is None else items)
    return c, o[:L].view(L, Hq, D).permute(1, 0, 2), o


# ---- a. counting probe ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,H", M.text_cases_LH())
def test_text_counting_probe(L, H):
    for causal in (False, True):
        for zero_table in (False, True):
            c, out, _ = _run(M.counting_case("text", L, H, H, 64, causal, zero_table))
            assert M.check_counting(c, out) == 0, (causal, zero_table)


@pytest.mark.parametrize("L,Hq,Hkv", M.lm_cases_LH())
def test_lm_counting_probe(L, Hq, Hkv):
    """Row i is the mean of keys 0 .. i: the diagonal of every row, and with it the wave-level skip of tiles above the wave's queries."""
    c, out, _ = _run(M.counting_case("lm", L, Hq, Hkv, 128, True))
    assert M.check_counting(c, out) == 0


@pytest.mark.parametrize("Dp", M.VISION_WIDTHS)
@pytest.mark.parametrize("segs", list(M.VISION_SEGS))
def test_vision_counting_probe(segs, Dp):
    segs = M.VISION_SEGS[segs]
    for H in M.HEADS:
        c, out, _ = _run(M.counting_case("vision", sum(segs), H, H, Dp, segs=segs))
        assert M.check_counting(c, out) == 0, H


def test_vision_counting_probe_long_segment():
    c, out, _ = _run(M.counting_case("vision", M.VISION_LONG, 1, 1, 96, segs=[M.VISION_LONG]))
    assert M.check_counting(c, out) == 0


def test_vision_counting_probe_items_of_1_63_and_64_queries_in_one_segment():
    items = torch.tensor([[0, 1, 0, 128], [1, 63, 0, 128], [64, 64, 0, 128]], dtype=torch.int32, device=DEV)
    c, out, _ = _run(M.counting_case("vision", 128, 3, 3, 64, segs=[128]), items=items)
    assert M.check_counting(c, out) == 0


def test_vision_counting_probe_width_80_in_96_keeps_the_pad_columns_zero():
    c, out, _ = _run(M.counting_case("vision", 195, 3, 3, 96, segs=[31, 1, 64, 65, 34], width=80))
    assert int((out[..., 80:] != 0).sum()) == 0
    assert M.check_counting(c, out) == 0


# ---- b. spike probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("L", M.SPIKE_LENGTHS)
def test_text_spike_probe(L, causal):
    """Lmax in {L, L + 3, 4096}: the window of the table starts Lmax - L entries in."""
    for Lmax in M.spike_lmaxes(L):
        for delta in M.spike_deltas(L, Lmax):
            c, out, _ = _run(M.spike_case(L, 3, delta, Lmax, causal))
            assert M.check_spike(c, out) == 0, (Lmax, delta)


# ---- c. head-map probe ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,Hq,Hkv", M.lm_cases_LH())
def test_lm_head_map_probe(L, Hq, Hkv):
    c, out, _ = _run(M.headmap_case(L, Hq, Hkv))
    assert M.check_headmap(c, out) == 0


# ---- d. fp64 bound, element-wise; f. repeat-call bit identity ---------------------------------------------------------------------------
def _bound_and_repeat(case, what):
    c, out, _ = _run(case)
    M.check_stress_shape(c)                                            # logits reach 50, the maximum where the family puts it
    r = M.bound_ratio(c, out)                                          # asserts that the fp64 reference is finite
    print(f"{case.kind} {case.family} {what}: worst err / bound {r:.3f}")
    assert r <= 1.0, (what, r)
    assert torch.equal(out, _run(case)[1]), "a repeated call must be bit-identical"
    return r


@pytest.mark.parametrize("L,H", M.text_cases_LH())
@pytest.mark.parametrize("family", M.FAMILIES)
def test_text_fp64_bound(family, L, H):
    for causal in (False, True):
        for bias in (False, True):
            _bound_and_repeat(M.bound_case("text", family, L, H, H, 64, causal, bias), f"L={L} H={H} causal={causal} bias={bias}")


@pytest.mark.parametrize("L,Hq,Hkv", M.lm_cases_LH())
@pytest.mark.parametrize("family", M.FAMILIES)
def test_lm_fp64_bound(family, L, Hq, Hkv):
    _bound_and_repeat(M.bound_case("lm", family, L, Hq, Hkv, 128, True), f"L={L} {Hq}/{Hkv}")


@pytest.mark.parametrize("segs", list(M.VISION_SEGS))
@pytest.mark.parametrize("family", M.FAMILIES)
def test_vision_fp64_bound(family, segs):
    for Dp in M.VISION_WIDTHS:
        _bound_and_repeat(M.bound_case("vision", family, sum(M.VISION_SEGS[segs]), 3, 3, Dp, segs=M.VISION_SEGS[segs]), f"{segs} Dp={Dp}")


@pytest.mark.parametrize("family", M.FAMILIES)
def test_vision_fp64_bound_long_segment_and_width_80_in_96(family):
    _bound_and_repeat(M.bound_case("vision", family, M.VISION_LONG, 1, 1, 96, segs=[M.VISION_LONG]), "long")
    _bound_and_repeat(M.bound_case("vision", family, 195, 3, 3, 96, segs=[31, 1, 64, 65, 34], width=80), "80 in 96")


# ---- e. poisoned tail -----------------------------------------------------------------------------------------------------------------
def _poisoned_tail(case):
    _, exact, _ = _run(case)
    _, out, o = _run(case, tail=64, fill=SENTINEL)
    L = case.q.shape[1]
    assert bool(torch.isfinite(exact.float()).all())
    assert torch.equal(out, exact), "NaN rows behind row L reached the output"
    assert bool((o[L:] == SENTINEL).all()), "rows behind row L were written"


@pytest.mark.parametrize("L", [1, 33, 97])
def test_text_ignores_poison_behind_row_L(L):
    for causal in (False, True):
        for bias in (False, True):
            _poisoned_tail(M.bound_case("text", "randn", L, 3, 3, 64, causal, bias))


@pytest.mark.parametrize("L", [1, 33, 97])
def test_lm_ignores_poison_behind_row_L(L):
    _poisoned_tail(M.bound_case("lm", "randn", L, 4, 2, 128, True))


@pytest.mark.parametrize("Dp", M.VISION_WIDTHS)
def test_vision_ignores_poison_behind_row_L_and_in_an_unnamed_segment(Dp):
    _poisoned_tail(M.bound_case("vision", "randn", 133, 3, 3, Dp, segs=[60, 70, 3]))
    # rows [33, 73) belong to no item: their q / k / v are NaN, their output rows keep the sentinel, the named rows do not change
    segs = [33, 40, 30]
    case = M.bound_case("vision", "randn", 103, 3, 3, Dp, segs=segs)
    items = QV.attention_items(M.cu_of(segs))
    named = items[items[:, 2] != 33].contiguous().to(DEV)
    assert named.shape[0] == 2
    _, whole, _ = _run(case)
    for t in (case.q, case.k, case.v):
        t[:, 33:73] = NAN
    _, out, o = _run(case, items=named, tail=64, fill=SENTINEL)
    assert torch.equal(out[:, :33], whole[:, :33]) and torch.equal(out[:, 73:], whole[:, 73:])
    assert bool((o[33:73] == SENTINEL).all()) and bool((o[103:] == SENTINEL).all())
