"""A model of the GEMM (regione_amd/csrc/gemm.hip: rgn_gemm_group) and the probes that pin every launch path of launch_mode /
gemm_schedule / plan_group / split128 / launch_gemm to the mathematics.  Plain torch, CPU or GPU tensors, no GPU import.

  TABLE / QKV_TABLE  one row per kernel class: shapes, weight format, epilogue, the plan knobs that make a problem of one to a few
                     tiles reach it, and the plan word rgn_gemm_last_plan / rgn_gemm_plan_query must report;
  *_case             probe inputs whose correct output is known EXACTLY from a closed form that holds no matrix product (one-hot A:
                     a gather of W; K-tile signatures: a sum of powers of two; all-ones: K), and the random / cancelling inputs of the
                     fp64 bound.  A case holds, per problem, A, W (bf16 values or e4m3fn byte codes + per-channel scales), bias, gate,
                     residual, out_rows, the prefilled destination and `lin`, the exact pre-activation in fp64;
  expected / check_* the checks: a count of violating elements (0 = pass) or a ratio (<= 1 = pass);
  emulate            a torch emulation that follows the tile / piece / quadrant structure of a row (tile map with GROUP_M, 64-wide K
                     tiles in two 32-wide half steps, K pieces -> fp32 partials per workspace slot -> reduce, quadrants of a parent
                     tile, clamped edge rows, epilogue per tile), with the named defects of MUTANTS.  A model of the scheme, not of any
                     kernel's instruction order.
tests/test_gpu_gemm_probes.py applies the checks to the kernels; tests/test_gemm_model.py applies the same functions to `emulate`, shows
that each mutant fails at least one of them and that every plan of the table is the planner's.
"""
from types import SimpleNamespace as NS

import torch

BF16 = torch.bfloat16
BK = 64
XR, XC = 3, 8                                   # rows / columns of the destination buffer behind the problem: they keep the sentinel
SENT_BITS = 0x1234                              # bf16 bit pattern of the sentinel (5.7e-28: no probe produces it)
BIG, QUARTER = 0x400, 0x100                     # bits of the plan word (include/regione_hip.h)
MUTANTS = ("piece_last_tile_dropped", "piece_boundary_tile_twice", "reduce_skips_piece", "partial_slot_of_wrong_tile",
           "a_half_steps_swapped", "c_fragment_transposed", "group_m_two_tiles_swapped", "quadrant_bits_exchanged",
           "edge_row_plus_one", "write_row_M", "gelu_boundary_off_by_8", "bias_of_neighbour_tile", "group_uses_problem_0",
           "scatter_to_m", "wscale_after_bias", "e4m3fnuz_decode", "kvpos_omitted", "cos_k_by_sequence_row", "rotation_pair_swapped")

# ---- the table of launch paths -------------------------------------------------------------------------------------------------------
# gemm_bf16_kernel<EPI, BM, BN, WM, WN, MODE, AV> instantiations that launch_mode / gemm_schedule can launch for the four non-conv
# epilogues (every EPI shares one template body; the rows spread BIAS / GELU / GATE_RESID over the classes, QKV_TABLE holds RGN_EPI_QKV),
# against the rows that are there for them:
#   <128,128,2,2> FULL    AV 0   f128_tiny f128_ragged f128_xcd f128_strided grp128 scat128_perm qkv128
#   <128,128,2,2> FULL    AV 8   f128_w8
#   <128,128,2,2> FULL    quarter = 1, AV 0   quarter_edges quarter_inside r257_quarter qkv_quarter;  AV 8   quarter_w8
#   <128,128,2,2> PARTIAL AV 0 + REDUCE (split128: no knob, the cost model splits K = 15360)   split128
#   <128,128,2,2> PARTIAL AV 8 + REDUCE (split128 does not look at the weight format: the fp8 text stream with a long K)   split128_w8
#   <256,256,2,4> FULL    AV 0   f256c f256c_k64 (default gemm_asm, K < 128 falls back) grp256c qkv256c;   AV 8   f256c_w8 f256_w8_k128 f256_w8_k192
#   <256,256,2,4> PARTIAL AV 0   pc256c_3 pc256_short1;   AV 8   pc256c_w8 pc256_w8_short
#   <256,256,2,4> REDUCE  (part4w = 0)   pc256c_3 pc256c_w8 pc256_short1 pc256_w8_short;   (part4w = 1, RGN_EPI_QKV)   qkv256_pieces;   (part4w = 0, RGN_EPI_QKV)   qkv256c_pieces
#   <256,256,2,2> FULL    AV 0 (two-stage loop, K = 128 / 192)   f256_k128 f256_k192 f256_strided scat256_sorted
#   <256,256,2,2> FULL    AV 1 (ring, K >= 256)   f256_ring f256_long grp256 r257_plain r257_quarter qkv256
#   <256,256,2,2> FULL    AV 9 (fp8 ring, K >= 256)   f256_w8_ring
#   <256,256,2,2> PARTIAL AV 0 (shortest piece 2 ... 3 K tiles)   pc256_av0 pc256_av0_uneven r257_pieces qkv256_pieces
#   <256,256,2,2> PARTIAL AV 1 (shortest piece >= 4)   pc256_av1_bias pc256_av1_gelu pc256_av1_gate pc256_long grp256_pieces scat256_pieces
#   <256,256,2,2> PARTIAL AV 9   pc256_w8_av9
#   gemm_reduce4w_kernel<BIAS>   pc256_av0 pc256_av1_bias r257_pieces scat256_pieces;  <GELU>   pc256_av0_uneven pc256_av1_gelu pc256_w8_av9;
#                        <GATE_RESID>   pc256_av1_gate pc256_long grp256_pieces
#   tile_offset != 0 (whole rounds plus remainder): r257_plain (one launch), r257_pieces, r257_quarter - probes (a), (b) only.
# Left out: the 128 geometry with whole rounds AND a split remainder (513 tiles x K >= 1024 with a cost-model split needs a 2 GB
# operand); a gemm_pieces value that leaves a piece without a K tile (not a production plan: nk / S >= 6); rgn_conv_* (pinned by
# tests/conv_model.py / tests/test_gpu_conv_probes.py), rgn_gemv_bf16 and the row-band launcher (pinned elsewhere).
G128, G256C, G256 = dict(gemm_geometry=128), dict(gemm_geometry=256, gemm_asm=0), dict(gemm_geometry=256)


def _row(name, Ms, N, K, w8, epi, knobs, plan, **feat):
    return NS(name=name, Ms=tuple(Ms), N=N, K=K, w8=bool(w8), epi=epi, knobs=dict(knobs), plan=plan, feat=feat, slots=None)


RAG, XCD, TINY = ((300,), 200, 192), ((1100,), 776, 512), ((1,), 8, 64)
GRP = (300, 0, 520, 8)
TABLE = [
    # plain launches
    _row("f128_tiny", *TINY, 0, "bias", G128, 0),                                                # <128,128,2,2> FULL, one row, one K tile
    _row("f128_ragged", *RAG, 0, "gate", G128, 0),                                               # <128,128,2,2> FULL, 3 x 2 ragged tiles
    _row("f128_xcd", *XCD, 0, "gelu", G128, 0),                                                  # 9 x 7 tiles: short last group, nb % 8 != 0
    _row("f128_w8", *RAG, 1, "bias", G128, 0),                                                   # <128,128,2,2> FULL AV 8
    _row("f256c", *XCD, 0, "gate", G256C, BIG | 1),                                              # <256,256,2,4> FULL, 5 x 4 tiles
    _row("f256c_w8", *RAG, 1, "gelu", G256C, BIG | 1),                                           # <256,256,2,4> FULL AV 8
    _row("f256c_k64", *TINY, 0, "bias", G256, BIG | 1),                                          # K < 128: <256,256,2,4> under the default gemm_asm
    _row("f256_k128", (300,), 200, 128, 0, "bias", G256, BIG | 1),                               # <256,256,2,2> FULL AV 0, the shortest loop
    _row("f256_k192", *RAG, 0, "gate", G256, BIG | 1),                                           # <256,256,2,2> FULL AV 0
    _row("f256_ring", *XCD, 0, "gelu", G256, BIG | 1),                                           # <256,256,2,2> FULL AV 1
    _row("f256_long", (520,), 264, 1536, 0, "bias", dict(G256, gemm_pieces=1), BIG | 1),         # AV 1, 24 K tiles: the rings wrap 8 / 12 times
    _row("f256_w8_ring", *XCD, 1, "bias", G256, BIG | 1),                                        # <256,256,2,2> FULL AV 9
    _row("f256_w8_k128", (300,), 200, 128, 1, "gate", G256, BIG | 1),                            # fp8, K < 256: back to <256,256,2,4> AV 8
    _row("f256_w8_k192", *RAG, 1, "bias", G256, BIG | 1),
    # K pieces on the 256 geometry (nk K tiles -> piece lengths)
    _row("pc256c_3", *XCD, 0, "gate", dict(G256C, gemm_pieces=3), BIG | 3),                      # 8 -> 3, 3, 2
    _row("pc256c_w8", (300,), 200, 320, 1, "bias", dict(G256C, gemm_pieces=2), BIG | 2),         # 5 -> 3, 2
    _row("pc256_av0", (300,), 200, 320, 0, "bias", dict(G256, gemm_pieces=2), BIG | 2),          # 5 -> 3, 2
    _row("pc256_av0_uneven", (520,), 264, 512, 0, "gelu", dict(G256, gemm_pieces=3), BIG | 3),   # 8 -> 3, 3, 2
    _row("pc256_av1_bias", *XCD, 0, "bias", dict(G256, gemm_pieces=2), BIG | 2),                 # 8 -> 4, 4
    _row("pc256_av1_gelu", *XCD, 0, "gelu", dict(G256, gemm_pieces=2), BIG | 2),
    _row("pc256_av1_gate", *XCD, 0, "gate", dict(G256, gemm_pieces=2), BIG | 2),
    _row("pc256_long", (520,), 264, 1536, 0, "gate", dict(G256, gemm_pieces=2), BIG | 2),        # 24 -> 12, 12: the ring wraps
    _row("pc256_short1", *RAG, 0, "bias", dict(G256, gemm_pieces=2), BIG | 2),                   # 3 -> 2, 1: 8-wave pieces and reduce
    _row("pc256_w8_av9", *XCD, 1, "gelu", dict(G256, gemm_pieces=2), BIG | 2),                   # 8 -> 4, 4
    _row("pc256_w8_short", (300,), 200, 320, 1, "gate", dict(G256, gemm_pieces=2), BIG | 2),     # 5 -> 3, 2: AV 8 pieces
    # quarter-tile remainder
    _row("quarter_edges", *XCD, 0, "bias", dict(G256, gemm_quarter=1), BIG | QUARTER | 1),       # 1100 = 1024 + 76, 776 = 768 + 8: early return
    _row("quarter_inside", (520,), 392, 256, 0, "gelu", dict(G256, gemm_quarter=1), BIG | QUARTER | 1),
    _row("quarter_w8", *RAG, 1, "gate", dict(G256, gemm_quarter=1), BIG | QUARTER | 1),
    # whole rounds plus remainder: 257 tiles of 256 x 256
    _row("r257_plain", (65792,), 256, 256, 0, "bias", G256, BIG | 1, huge=True),
    _row("r257_pieces", (65792,), 256, 256, 0, "bias", dict(G256, gemm_pieces=2), BIG | 2, huge=True),
    _row("r257_quarter", (65792,), 256, 256, 0, "bias", dict(G256, gemm_quarter=1), BIG | QUARTER | 1, huge=True),
    # K split on the 128 geometry: the cost model of split128 alone (bits 12-15 of the plan word)
    _row("split128", (300,), 128, 15360, 0, "bias", G128, 6 << 12, huge=True),                          # three 128-tiles, 240 K tiles -> 6 x 40
    _row("split128_w8", (300,), 128, 15360, 1, "bias", G128, 6 << 12, huge=True),                       # the same with fp8 W: PARTIAL AV 8
    # groups: four problems, the second empty, problems 0 and 2 share W, own bias / gate / resid
    _row("grp128", GRP, 200, 192, 0, "gate", G128, 0, share_w=True),
    _row("grp256c", GRP, 200, 192, 0, "gate", G256C, BIG | 1, share_w=True),
    _row("grp256", GRP, 264, 256, 0, "gate", G256, BIG | 1, share_w=True),
    _row("grp256_pieces", GRP, 264, 512, 0, "gate", dict(G256, gemm_pieces=2), BIG | 2, share_w=True),
    # single-problem features
    _row("f128_strided", *RAG, 0, "bias", G128, 0, lda=64, ldw=24),
    _row("f256_strided", *RAG, 0, "bias", G256, BIG | 1, lda=64, ldw=24),
    _row("scat256_sorted", *RAG, 0, "gate", G256, BIG | 1, scatter="sorted"),
    _row("scat128_perm", *RAG, 0, "bias", G128, 0, scatter="perm"),
    _row("scat256_pieces", *XCD, 0, "bias", dict(G256, gemm_pieces=2), BIG | 2, scatter="perm"),
]
# fused Q/K/V epilogue (H = 2: K, V, Q blocks of 256 columns, K = 256)
QKV_TABLE = [
    _row("qkv128", (200,), 768, 256, 0, "qkv", G128, 0, row_base=0, perm=False, f16=False),
    _row("qkv256c", (333,), 1024, 256, 0, "qkv", G256C, BIG | 1, row_base=0, perm=True, f16=False),          # + an MLP half of 256 columns
    _row("qkv256", (333,), 768, 256, 0, "qkv", G256, BIG | 1, row_base=48, perm=False, f16=False),
    _row("qkv256_pieces", (200,), 768, 256, 0, "qkv", dict(G256, gemm_pieces=2), BIG | 2, row_base=5, perm=True, f16=True),      # 4 -> 2, 2
    _row("qkv256c_pieces", (333,), 768, 256, 0, "qkv", dict(G256C, gemm_pieces=2), BIG | 2, row_base=0, perm=False, f16=True),      # 8-wave pieces: part4w = 0
    _row("qkv_quarter", (333,), 768, 256, 0, "qkv", dict(G256, gemm_quarter=1), BIG | QUARTER | 1, row_base=5, perm=True, f16=True),
]
TABLE_BY_NAME = {r.name: r for r in TABLE + QKV_TABLE}
BOUND_ROWS = [r.name for r in TABLE if r.K <= 512 and not r.feat.get("huge")]          # the bound is only sharp for short K
SMALL_ROWS = [r.name for r in TABLE if not r.feat.get("huge")]
GARBAGE_ROWS = SMALL_ROWS + [r.name for r in TABLE if r.name.startswith("split128")]          # f: every row but the 257-tile ones


def small_twin(row):
    """The logic of a 257-tile row at a size the CPU emulation affords: 5 tiles of 256 x 256 with 4 workgroup slots per round."""
    return NS(**{**row.__dict__, "Ms": (1280,), "slots": 4})


def plan_query_args(row):
    """(Ms, N, K, distinct_w, w8) for rgn_gemm_plan_query."""
    n = sum(1 for m in row.Ms if m > 0)
    return list(row.Ms), row.N, row.K, (n - 1 if row.feat.get("share_w") else n), int(row.w8)


# ---- number formats --------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int16)


def mismatches(got, want):
    return int((bits(got) != bits(want)).sum())


def sentinel(shape, dev):
    return torch.full(shape, SENT_BITS, dtype=torch.int16, device=dev).view(BF16)


def e4m3fn_table(dev="cpu", fnuz=False):
    """Value of every byte code in fp64 (NaN codes: NaN).  OCP e4m3fn: bias 7, no infinity, S.1111.111 = NaN; fnuz: bias 8, 0x80 = NaN."""
    c = torch.arange(256, device=dev)
    s, e, m = 1.0 - 2.0 * (c >> 7).double(), ((c >> 3) & 15).double(), (c & 7).double()
    b = 8.0 if fnuz else 7.0
    v = s * torch.where(e == 0, m / 8.0 * 2.0 ** (1.0 - b), (1.0 + m / 8.0) * torch.exp2(e - b))
    nan = (c == 0x80) if fnuz else ((c & 0x7f) == 0x7f)
    return torch.where(nan, torch.full_like(v, float("nan")), v)


def w_values(p, fnuz=False):
    """W [N, K] as fp64 values."""
    return e4m3fn_table(p.W.device, fnuz)[p.W.long()] if p.wscale is not None else p.W.double()


def _bf16_step(x, up):
    """The next bf16 above / below a finite non-zero bf16 x."""
    b = bits(x).int()
    pos = b >= 0
    nb = torch.where(pos == up, b + 1, b - 1)
    return nb.short().view(BF16)


def bf16_neighbours(x64):
    """(lo, hi): the largest bf16 <= x and the smallest bf16 >= x, as fp64 (equal where x is a bf16)."""
    r = x64.float().to(BF16)
    r64 = r.double()
    zero = r64 == 0
    safe = torch.where(zero, torch.ones_like(r), r)
    up, dn = _bf16_step(safe, True).double(), _bf16_step(safe, False).double()
    lo = torch.where(r64 <= x64, r64, dn)
    hi = torch.where(r64 >= x64, r64, up)
    tiny = 2.0 ** -133                                            # smallest bf16 subnormal: the neighbours of a value that rounds to 0
    lo = torch.where(zero, torch.where(x64 < 0, torch.full_like(x64, -tiny), torch.zeros_like(x64)), lo)
    hi = torch.where(zero, torch.where(x64 > 0, torch.full_like(x64, tiny), torch.zeros_like(x64)), hi)
    return lo, hi


FLUSH = 2.0 ** -126          # below the smallest normal fp32 the exp / rcp units flush: a GELU of that size may also come out as (signed) zero.
                             # It takes |x| > 10: allowed only where the integer index probe runs through a GELU row (case.allow_flush);
                             # the GELU probe proper (halves in [-8, 8], 17 orders above it) keeps the two-neighbour rule as it stands.


def gelu64(x):
    """tanh-GELU in fp64: 0.5 x (1 + tanh(u)) = x / (1 + exp(-2 u)), u = sqrt(2 / pi) (x + 0.044715 x^3).  The second form is the same
    function without the cancellation of 1 + tanh(u) at u << 0, where the first loses every digit even in fp64."""
    return x / (1.0 + torch.exp(-2.0 * 0.7978845608028654 * (x + 0.044715 * x ** 3)))


def kvpos(r):
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def f_onehot(M, K, dev, shift=0):
    """The k that row m selects: an odd stride, so K consecutive rows hit every k; row 0 selects k = 63 (an 8-, 32- and 64-element edge).
    A problem of M < K rows hits every k over the passes shift = 0 ... index_shifts - 1 (row m stands for row m + shift M)."""
    return (37 * (torch.arange(M, device=dev) + shift * M) + 63) % K


def index_shifts(row):
    """Passes of the index probe after which the largest problem of the row has selected every k."""
    return (row.K + max(row.Ms) - 1) // max(row.Ms)


def _onehot(M, K, dev, shift=0):
    A = torch.zeros(M, K, dtype=BF16, device=dev)
    A[torch.arange(M, device=dev), f_onehot(M, K, dev, shift)] = 1
    return A


def _int_codes(dev):
    """e4m3fn codes of the integers of magnitude <= 120 that the format holds (4 significant bits), ascending."""
    v = e4m3fn_table(dev)
    ok = (v == v.round()) & (v.abs() <= 120) & (torch.arange(256, device=dev) != 0x80)
    codes = torch.arange(256, device=dev)[ok]
    return codes[torch.argsort(v[ok])]


def _grid(N, K, dev, wid, mod, off):
    n, k = torch.arange(N, device=dev)[:, None], torch.arange(K, device=dev)[None, :]
    return (7 * n + 13 * k + 31 * wid) % mod - off


def _dest(case, p, row, i, dev, gen):
    """Destination of problem p: R rows (> M with a row scatter), gate / residual, the prefilled buffer."""
    M, N = p.M, row.N
    kind = row.feat.get("scatter")
    p.R, p.out_rows = M, None
    if kind and M > 0:
        p.R = M + M // 2
        perm = torch.randperm(p.R, generator=gen)[:M]
        p.out_rows = (perm.sort().values if kind == "sorted" else perm).to(dev)
    p.gate = p.resid = None
    p.out_init = sentinel((p.R + XR, N + XC), dev)
    if case.epi == "gate":
        p.gate = torch.randn(N, generator=gen).to(BF16).to(dev)
        p.resid = (torch.randn(p.R, N, generator=gen) * 4).to(BF16).to(dev)
        if case.inplace:
            p.out_init[:p.R, :N] = p.resid


def _case(row, kind, dev, epi=None, inplace=False, gelu_from=None, seed=0):
    epi = epi or row.epi
    if gelu_from is None:
        gelu_from = (row.N // 2) // 16 * 16 + 8 if row.N >= 24 else 0          # a multiple of 8, not of 16, inside a tile
    return NS(kind=kind, epi=epi, inplace=inplace, gelu_from=gelu_from if epi == "gelu" else 0, w8=row.w8, N=row.N, K=row.K, probs=[], qkv=None, allow_flush=False,
              gen=torch.Generator().manual_seed(1000 * seed + len(row.name) + row.K))


def _finish(case, row, dev, build):
    """Problems of the row; build(i, wid, M) -> (A, W, wscale, bias, lin).  Problems 0 and 2 of a `share_w` group share one W."""
    made = {}
    for i, M in enumerate(row.Ms):
        wid = 0 if (row.feat.get("share_w") and i == 2) else i
        A, W, ws, bias, lin = build(i, wid, M)
        if wid in made:
            W, ws = made[wid]
        made[wid] = (W, ws)
        p = NS(M=M, A=A, W=W, wscale=ws, bias=bias, lin=lin, wid=wid)
        _dest(case, p, row, i, dev, case.gen)
        case.probs.append(p)
    return case


def _scales(N, dev, i, pow2):
    """Per-channel scales: powers of two, or short mantissas that are no power of two - a product with a small integer and the sum with
    an integer bias stay exact in fp32, so a fused multiply-add and a separate multiply and add give the same bits."""
    tab = torch.tensor([0.5, 1.0, 2.0, 0.25, 4.0] if pow2 else [0.75, 1.5, 0.375, 1.25, 0.625], device=dev)
    return tab[(torch.arange(N, device=dev) + i) % 5].float()


def index_case(row, dev="cpu", halves=False, shift=0, **kw):
    """a. one-hot A, W[n, k] an integer in [-125, 125] that depends on n and k (fp8: the integers e4m3fn holds, times a short scale),
    integer bias: out[m, n] = epilogue(W[n, f(m)] (* scale[n]) + bias[n]).  halves: pre-activations on the grid of halves in [-8, 8]."""
    case = _case(row, "index", dev, **kw)
    case.allow_flush = not halves
    N, K = row.N, row.K

    def build(i, wid, M):
        ws = None
        if row.w8:
            codes = _int_codes(dev)
            if halves:
                v = e4m3fn_table(dev)
                codes = torch.arange(256, device=dev)[(v * 2 == (v * 2).round()) & (v.abs() <= 7.5)]
            W = codes[_grid(N, K, dev, wid, len(codes), 0)].to(torch.uint8)
            ws = _scales(N, dev, i, pow2=False) if not halves else torch.ones(N, device=dev)
        else:
            W = (_grid(N, K, dev, wid, 31, 15).double() / 2 if halves else _grid(N, K, dev, wid, 251, 125)).to(BF16)
        n = torch.arange(N, device=dev)
        bias = (((5 * n + 3 * i) % 3 - 1).double() / 2 if halves else ((5 * n + 3 * i) % 17 - 8)).to(BF16)
        A = _onehot(M, K, dev, shift)
        wv = w_values(NS(W=W, wscale=ws))
        lin = wv.t()[f_onehot(M, K, dev, shift)] * (ws.double() if ws is not None else 1.0) + bias.double()
        return A, W, ws, bias, lin
    return _finish(case, row, dev, build)


SIG_TILES = 4                                   # K tiles per signature pass: 8 half steps = the 8 significant bits of bf16


def _sig_sign(n, hs, wid):
    """Sign of W[n, k] in half step hs = k // 32: depends on the output channel AND on the K tile, so a W tile of another K tile (or of
    another problem's W) paired with the right A tile changes the sum."""
    return 1 - 2 * (((n * 5 + hs * 3 + n // 8 + wid) % 7) < 3).long()


def signature_case(row, dev="cpu", **kw):
    """b. Row m belongs to pass m % npass, whose window is K tiles [4 pass, 4 pass + 4): half step h of tile t of the window holds a
    single 1 in A and sign(n, j) 2^j in every W[n, k] of the half step, j = 2 (t - 4 pass) + h.  out[m, n] = sum_j sign(n, j) 2^j: every
    partial sum in any order is an integer below 256.  No bias (the null-bias path)."""
    case = _case(row, "signature", dev, **kw)
    N, K = row.N, row.K
    nk = K // BK
    npass = (nk + SIG_TILES - 1) // SIG_TILES

    def build(i, wid, M):
        k = torch.arange(K, device=dev)
        hs = k // 32                                                              # [K] half step
        n = torch.arange(N, device=dev)[:, None]
        Wv = _sig_sign(n, hs[None, :], wid) * (2 ** (hs % 8))[None, :]
        ws = None
        if row.w8:
            v = e4m3fn_table(dev)
            lut = torch.zeros(257, dtype=torch.long, device=dev)
            for val in [s * (1 << b) for s in (1, -1) for b in range(8)]:
                lut[val + 128] = int(torch.nonzero(v == val)[0])
            W = lut[Wv + 128].to(torch.uint8)
            ws = _scales(N, dev, i, pow2=True)
        else:
            W = Wv.to(BF16)
        m = torch.arange(M, device=dev)
        ps = (m % npass)[:, None]
        win = (k[None, :] // BK) // SIG_TILES == ps                               # [M, K] inside the row's window
        pos = ((m * 11 + 7)[:, None] + 5 * (k[None, :] // 32)) % 32               # position of the 1 inside each half step
        A = (win & ((k[None, :] % 32) == pos)).to(BF16)
        lin = torch.zeros(M, N, dtype=torch.float64, device=dev)
        for s in range(2 * SIG_TILES):                                            # the closed form: the half steps of the row's window
            h = 2 * SIG_TILES * ps + s                                            # [M, 1]
            lin += (h < 2 * nk) * _sig_sign(n.t(), h, wid).double() * 2.0 ** s
        return A, W, ws, None, lin * (ws.double() if ws is not None else 1.0)
    return _finish(case, row, dev, build)


def count_case(row, dev="cpu", **kw):
    """A = W = 1: out = K (every K of the table is a bf16)."""
    case = _case(row, "count", dev, **kw)
    assert float(torch.tensor(float(row.K)).to(BF16)) == row.K

    def build(i, wid, M):
        A = torch.ones(M, row.K, dtype=BF16, device=dev)
        W = torch.full((row.N, row.K), 0x38, dtype=torch.uint8, device=dev) if row.w8 else torch.ones(row.N, row.K, dtype=BF16, device=dev)
        ws = torch.ones(row.N, device=dev) if row.w8 else None
        return A, W, ws, None, torch.full((M, row.N), float(row.K), dtype=torch.float64, device=dev)
    return _finish(case, row, dev, build)


def bytecode_case(row, dev="cpu"):
    """d. every finite e4m3fn code (-0, the subnormals and +-448 included) in W, power-of-two scales, one-hot A, no bias:
    out = bf16(value * scale) exactly."""
    assert row.w8
    case = _case(row, "bytecode", dev, epi="bias")
    fin = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], device=dev)
    assert len(fin) == 254

    def build(i, wid, M):
        n, k = torch.arange(row.N, device=dev)[:, None], torch.arange(row.K, device=dev)[None, :]
        W = fin[(n + k + 3 * wid) % 254].to(torch.uint8)
        ws = torch.exp2(((torch.arange(row.N, device=dev) % 7) - 3).float())
        lin = w_values(NS(W=W, wscale=ws)).t()[f_onehot(M, row.K, dev)] * ws.double() + 0.0          # -0 + 0 = +0, as in the accumulator
        return _onehot(M, row.K, dev), W, ws, None, lin
    c = _finish(case, row, dev, build)
    sel = torch.cat([p.W[:, f_onehot(p.M, row.K, dev)].flatten() for p in c.probs if p.M > 0])
    c.codes_seen = int(sel.unique().numel())
    return c


def scale_bias_case(row, dev="cpu"):
    """d. scales that are no power of two and a bias of magnitude >= 3: (acc * scale) + bias and (acc + bias) * scale differ by
    |bias| (1 - scale) >= 0.75 on integers of magnitude <= 190 - more than any bf16 spacing there."""
    assert row.w8
    case = _case(row, "scale_bias", dev, epi="bias")
    codes = _int_codes(dev)

    def build(i, wid, M):
        W = codes[_grid(row.N, row.K, dev, wid, len(codes), 0)].to(torch.uint8)
        ws = torch.tensor([0.75, 0.375, 0.625], device=dev)[(torch.arange(row.N, device=dev) + i) % 3].float()
        n = torch.arange(row.N, device=dev)
        bias = (((n * 3 + i) % 6 + 3) * (1 - 2 * (n % 2))).to(BF16)
        lin = w_values(NS(W=W, wscale=ws)).t()[f_onehot(M, row.K, dev)] * ws.double() + bias.double()
        return _onehot(M, row.K, dev), W, ws, bias, lin
    return _finish(case, row, dev, build)


FAMILIES = ("randn", "cancel")
SIGMA = 0.5


def bound_case(row, family, dev="cpu"):
    """e. N(0, 1) sigma operands, or `cancel`: products of magnitude ~16 in adjacent pairs of opposite sign whose sum is ~2^-8 of them."""
    case = _case(row, "bound_" + family, dev, epi="bias", seed=1 + FAMILIES.index(family))      # the bound is on the sum: plain epilogue
    g, shared = case.gen, {}

    def build(i, wid, M):
        N, K = row.N, row.K
        if family == "randn":
            A, Wf = torch.randn(M, K, generator=g) * SIGMA, torch.randn(N, K, generator=g) * SIGMA
        else:
            A = (torch.randn(M, K // 2, generator=g) * 4).repeat_interleave(2, dim=1)
            y = torch.randn(N, K // 2, generator=g) * 4
            Wf = torch.stack([y, -y * (1 + torch.randn(N, K // 2, generator=g) * 2.0 ** -8)], dim=2).reshape(N, K)
        Wf = shared.setdefault(wid, Wf)
        A = A.to(BF16).to(dev)
        ws = None
        if row.w8:
            s = Wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
            W = (Wf / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).to(dev)
            ws = s.float().to(dev)
        else:
            W = Wf.to(BF16).to(dev)
        bias = torch.randn(N, generator=g).to(BF16).to(dev)
        wv = w_values(NS(W=W, wscale=ws))
        sc = ws.double() if ws is not None else 1.0
        lin = A.double() @ wv.t() * sc + bias.double()
        p_abs = A.double().abs() @ wv.abs().t() * sc
        return A, W, ws, bias, (lin, p_abs)
    c = _finish(case, row, dev, build)
    for p in c.probs:
        p.lin, p.S = p.lin
    return c


# ---- expected outputs and checks -----------------------------------------------------------------------------------------------------------
def _rows_of(p):
    return p.out_rows if p.out_rows is not None else torch.arange(p.M, device=p.A.device)


def epilogue_ref(case, p):
    """The epilogue on the exact pre-activation: (exact values [M, N] bf16, None) - or, for the GELU columns, (nearest, (lo, hi, mask))."""
    v = p.lin.float().to(BF16)                                                   # exact operands: one rounding
    if case.epi == "bias":
        return v, None
    if case.epi == "gate":
        t = (p.gate.float()[None, :] * v.float()).to(BF16)                       # bf16(gate * bf16(lin))
        return (p.resid[_rows_of(p)].float() + t.float()).to(BF16), None         # bf16(resid + .)
    assert case.epi == "gelu"
    y = gelu64(v.double())                                                       # GELU of the bf16-rounded value
    lo, hi = bf16_neighbours(y)
    mask = (torch.arange(case.N, device=v.device) >= case.gelu_from)[None, :].expand_as(v)
    return torch.where(mask, y.float().to(BF16), v), (lo, hi, mask)


def expected(case, p):
    """The whole destination buffer of problem p: the sentinel (or, in place, the residual) wherever the problem does not write."""
    want = p.out_init.clone()
    v, gel = epilogue_ref(case, p)
    want[_rows_of(p), :case.N] = v
    return want, gel


def outside_intact(p, got, N):
    """The destination buffer keeps its prefill outside the rows the problem names and behind column N."""
    frame = p.out_init.clone()
    if p.M:
        frame[_rows_of(p), :N] = got[_rows_of(p), :N]
    return mismatches(got, frame) == 0


def check_exact(case, outs):
    """Violating elements over all problems: bits against `expected` - in the GELU columns: not one of the two bf16 neighbours of the
    fp64 tanh-GELU.  Also returns the share of GELU outputs that are not correctly rounded."""
    bad = off = total = 0
    for p, got in zip(case.probs, outs):
        if p.M == 0:
            continue
        want, gel = expected(case, p)
        diff = bits(got) != bits(want)
        if gel is not None:
            lo, hi, mask = gel
            g = got[_rows_of(p), :case.N].double()
            ok = (g == lo) | (g == hi)
            if case.allow_flush:
                ok = ok | ((g == 0) & (lo.abs() < FLUSH))
            inner = torch.zeros_like(diff)
            inner[_rows_of(p), :case.N] = mask
            bad += int((diff & ~inner).sum()) + int((mask & ~ok).sum())
            off += int((diff & inner).sum())
            total += int(mask.sum())
        else:
            bad += int(diff.sum())
    case.gelu_share = off / total if total else 0.0
    return bad


def bound_ratio(case, outs):
    """e. worst |out - ref64| / (2^-8 |ref64| + K 2^-23 S + tiny) over the problem; the sentinel outside it must be intact (-> inf)."""
    worst = 0.0
    for p, got in zip(case.probs, outs):
        if p.M == 0:
            continue
        assert bool(torch.isfinite(p.lin).all())
        frame, rows = p.out_init.clone(), _rows_of(p)
        frame[rows, :case.N] = got[rows, :case.N]
        if mismatches(got, frame):
            return float("inf")
        bound = 2.0 ** -8 * p.lin.abs() + case.K * 2.0 ** -23 * p.S + 1e-30
        worst = max(worst, float(((got[rows, :case.N].double() - p.lin).abs() / bound).max()))
    return worst


# ---- the fused Q/K/V epilogue -------------------------------------------------------------------------------------------------------------
def _sign(n):
    return 1 - 2 * ((n * 11) % 7 >= 4).long()


def _rope_tab(rows, dev, salt):
    r, c = torch.arange(rows, device=dev)[:, None], torch.arange(128, device=dev)[None, :]
    t3 = torch.tensor([1.0, 0.0, -1.0], device=dev)                               # cos / sin in {0, +-1}, keyed by the table row
    cos = t3[(3 * r + c + c // 2 + salt) % 3]
    sin = t3[(r + 2 * c + c // 4 + salt) % 3]
    return cos.float().contiguous(), sin.float().contiguous()


def qkv_case(row, dev="cpu"):
    """g. one-hot A, W[n, k] = sign(n) 2^(k % 8): every head of every row has constant magnitude >= 1, its RMS-normalised value rounds
    to +-1 (eps = 1e-6), norm weights are distinct integers per channel, cos / sin in {0, +-1}: Q, K and V^T are integer arithmetic."""
    H, D, M = 2, 256, row.Ms[0]
    N, K, base = row.N, row.K, row.feat["row_base"]
    case = _case(row, "qkv", dev)
    case.gelu_from = 3 * D
    gen = case.gen
    skv = base + 2 * M
    skv_pad = (skv + 63) // 64 * 64
    kv_rows = None
    if row.feat["perm"]:
        kv_rows = torch.cat([torch.arange(base), base + torch.randperm(skv - base, generator=gen)[:M]]).to(dev)
    n, k = torch.arange(N, device=dev), torch.arange(K, device=dev)
    W = (_sign(n)[:, None] * (2 ** (k % 8))[None, :]).to(BF16)
    wq = (torch.arange(128, device=dev) + 1).to(BF16)
    wk = (128 - torch.arange(128, device=dev)).to(BF16)
    case.qkv = NS(H=H, D=D, k_col=0, v_col=D, q_col=2 * D, row_base=base, kv_rows=kv_rows, skv_pad=skv_pad, wq=wq, wk=wk, eps=1e-6,
                  rope_q=_rope_tab(base + M, dev, 0), rope_k=_rope_tab(skv_pad, dev, 1), f16=row.feat["f16"],
                  k_init=sentinel((skv_pad, D), dev), vt_init=sentinel((D, skv_pad), dev))
    A = _onehot(M, K, dev)
    lin = W.double().t()[f_onehot(M, K, dev)]
    p = NS(M=M, A=A, W=W, wscale=None, bias=torch.zeros(N, dtype=BF16, device=dev), lin=lin, wid=0, R=M, out_rows=None, gate=None, resid=None,
           out_init=sentinel((M + XR, N + XC), dev))
    case.probs.append(p)
    return case


def qkv_expected(case):
    """(out buffer, K slab, V^T slab, GELU neighbours of the MLP columns) by integer arithmetic: unit = sign(n), rotated pairs of
    unit * weight."""
    q, p = case.qkv, case.probs[0]
    dev, M, D = p.A.device, p.M, q.D
    m = torch.arange(M, device=dev)
    seq = q.row_base + m
    kr = q.kv_rows[seq] if q.kv_rows is not None else seq

    def rot(col0, w, tab, trow):
        u = (_sign(col0 + torch.arange(D, device=dev)).double() * w.double().repeat(q.H))[None, :].expand(M, D)
        cos, sin = tab[0][trow].double().repeat(1, q.H), tab[1][trow].double().repeat(1, q.H)
        a, b = u[:, 0::2], u[:, 1::2]
        o = torch.stack([a * cos[:, 0::2] + (-b) * sin[:, 0::2], b * cos[:, 1::2] + a * sin[:, 1::2]], dim=2).reshape(M, D)      # signed zeros as the kernel's
        return o.float().to(BF16)
    out, ks, vt = p.out_init.clone(), q.k_init.clone(), q.vt_init.clone()
    out[:M, q.q_col:q.q_col + D] = rot(q.q_col, q.wq, q.rope_q, seq)
    ks[kr] = rot(q.k_col, q.wk, q.rope_k, kr)
    vt[:, kvpos(kr)] = p.lin[:, q.v_col:q.v_col + D].float().to(BF16).t()
    gel = None
    if case.N > 3 * D:
        y = gelu64(p.lin[:, 3 * D:].float().to(BF16).double())
        gel = bf16_neighbours(y)
        out[:M, 3 * D:case.N] = y.float().to(BF16)
    return out, ks, vt, gel


def check_qkv(case, got):
    out, ks, vt = got
    wo, wk_, wv, gel = qkv_expected(case)
    p, D = case.probs[0], case.qkv.D
    bad = mismatches(ks, wk_) + mismatches(vt, wv)
    diff = bits(out) != bits(wo)
    if gel is not None:
        g = out[:p.M, 3 * D:case.N].double()
        bad += int(((g != gel[0]) & (g != gel[1])).sum())
        diff[:p.M, 3 * D:case.N] = False
    return bad + int(diff.sum())


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------------
def tile_coords(t, M, N, PB):
    """Tile t of one problem -> (tm, tn): GROUP_M row tiles share a column sweep; the last group may be short."""
    ntm, ntn = (M + PB - 1) // PB, (N + PB - 1) // PB
    G = 4 if PB >= 256 else 8
    per = G * ntn
    first = (t // per) * G
    gs = min(ntm - first, G)
    return first + (t % per) % gs, (t % per) // gs


def _gelu32(x):
    z = x * (-2.8853900817779268 * 0.7978845608028654 * 0.044715 * x * x - 2.8853900817779268 * 0.7978845608028654)
    return x / (1.0 + torch.exp2(z))


def emulate(case, row, mutant=None, slots=None):
    """What the launches of `row` write for `case`: a list of destination buffers (Q/K/V: (out, K slab, V^T slab))."""
    big, quarter = bool(row.plan & BIG), bool(row.plan & QUARTER)
    S = (row.plan & 0xff) if big else max(1, (row.plan >> 12) & 15)
    PB = 256 if big else 128
    slots = slots or row.slots or (256 if big else 512)
    probs = [p for p in case.probs if p.M > 0]
    dev = probs[0].A.device
    for p in probs:
        p.Af = p.A.float()
        p.Wf = w_values(p, fnuz=(mutant == "e4m3fnuz_decode")).float()
        p.out = p.out_init.clone()
    if case.qkv is not None:
        case.qkv.ks, case.qkv.vt = case.qkv.k_init.clone(), case.qkv.vt_init.clone()
    ends, nt = [], 0
    for p in probs:
        nt += ((p.M + PB - 1) // PB) * ((case.N + PB - 1) // PB)
        ends.append(nt)
    full = nt // slots * slots
    left = nt - full
    if left == 0:
        S, quarter = 1, False
    nk_all = case.K // BK
    ws = {}
    for t in range(nt):
        rem = t >= full and (S > 1 or quarter)
        unit = t - full if rem else t                                            # launch-local index = workspace slot
        pi = sum(1 for e in ends[:-1] if t >= e)
        p = probs[pi]
        tl = t - (ends[pi - 1] if pi else 0)
        tm, tn = tile_coords(tl, p.M, case.N, PB)
        om, on = tm, tn                                                          # the tile whose operands are read
        ntl = ends[pi] - (ends[pi - 1] if pi else 0)
        if mutant == "group_m_two_tiles_swapped" and tl < 2 and ntl >= 2:
            om, on = tile_coords(1 - tl, p.M, case.N, PB)
        if quarter and rem:
            blocks = []
            for qsub in range(4):
                hi, lo = qsub >> 1, qsub & 1
                ahi, alo = (lo, hi) if mutant == "quadrant_bits_exchanged" else (hi, lo)          # on the operand side only
                blocks.append((tm * 256 + hi * 128, tn * 256 + lo * 128, om * 256 + ahi * 128, on * 256 + alo * 128, 128))
        else:
            blocks = [(tm * PB, tn * PB, om * PB, on * PB, PB)]
        for m0, n0, am0, an0, B in blocks:
            if m0 >= p.M or n0 >= case.N:
                continue                                                         # a quadrant past the problem's edge
            ridx = am0 + torch.arange(B, device=dev)
            if mutant == "edge_row_plus_one" and am0 + B > p.M:
                ridx = ridx + 1
            a = p.Af[ridx.clamp(max=p.M - 1)]
            w = p.Wf[(an0 + torch.arange(B, device=dev)).clamp(max=case.N - 1)]
            split = rem and S > 1 and not quarter
            per = (nk_all + S - 1) // S if split else nk_all
            for sp in range(S if split else 1):
                k0 = sp * per
                nk = max(0, min(per, nk_all - k0))
                if split and mutant == "piece_last_tile_dropped":
                    nk -= 1
                if split and mutant == "piece_boundary_tile_twice" and sp > 0:
                    k0, nk = k0 - 1, nk + 1
                acc = torch.zeros(B, B, device=dev)
                for kt in range(k0, k0 + nk):
                    for kk in range(2):                                          # two 32-wide half steps per K tile
                        ka = kt * BK + 32 * ((1 - kk) if mutant == "a_half_steps_swapped" else kk)
                        kw = kt * BK + 32 * kk
                        acc = acc + a[:, ka:ka + 32] @ w[:, kw:kw + 32].t()
                ws[(unit, sp)] = acc
            if split:                                                            # reduce pass: 0 + p0 + p1 + ...
                slot = t if mutant == "partial_slot_of_wrong_tile" else unit
                acc = torch.zeros(B, B, device=dev)
                for sp in range(S - 1 if mutant == "reduce_skips_piece" else S):
                    acc = acc + ws.get((slot, sp), torch.full((B, B), float("nan"), device=dev))
            if mutant == "c_fragment_transposed":
                acc = acc.view(B // 16, 16, B // 16, 16).transpose(1, 3).reshape(B, B)
            _epilogue(case, p, probs[0], acc, m0, n0, B, mutant)
    if case.qkv is not None:
        return [(probs[0].out, case.qkv.ks, case.qkv.vt)]
    outs = {id(p): p.out for p in probs}
    return [outs.get(id(p), p.out_init) for p in case.probs]


def _epilogue(case, p, p0, acc, m0, n0, B, mutant):
    dev = acc.device
    src = p0 if mutant == "group_uses_problem_0" else p
    n = n0 + torch.arange(B, device=dev)
    okn = n < case.N
    nc = n.clamp(max=case.N - 1)
    nb = ((n + B) % case.N) if mutant == "bias_of_neighbour_tile" else nc
    bias = src.bias.float()[nb] if src.bias is not None else torch.zeros(B, device=dev)
    sv = p.wscale[nc] if p.wscale is not None else torch.ones(B, device=dev)
    c = (acc + bias) * sv if mutant == "wscale_after_bias" else acc * sv + bias
    m = m0 + torch.arange(B, device=dev)
    okm = (m <= p.M) if mutant == "write_row_M" else (m < p.M)
    if case.qkv is not None:
        return _qkv_epilogue(case, p, c, m[okm], n0, B, okm, mutant)
    v = c.to(BF16)
    if case.epi == "gelu":
        frm = case.gelu_from + (8 if mutant == "gelu_boundary_off_by_8" else 0)
        v = torch.where((n >= frm)[None, :], _gelu32(v.float()).to(BF16), v)
    mm = m[okm]
    orow = mm
    if p.out_rows is not None and mutant != "scatter_to_m":
        orow = p.out_rows[mm.clamp(max=p.M - 1)]
    if case.epi == "gate":
        t = (src.gate.float()[nc][None, :] * v.float()).to(BF16)
        v = (p.resid[orow.clamp(max=p.R - 1)][:, nc].float() + t[okm].float()).to(BF16)
    else:
        v = v[okm]
    p.out[orow[:, None], n[okn][None, :]] = v[:, okn]


def _qkv_epilogue(case, p, c, m, n0, B, okm, mutant):
    q, dev = case.qkv, c.device
    if q.f16 and n0 < q.q_col:
        c = c.half().float()
    v = c.to(BF16)[okm]
    seq = q.row_base + m
    kr = q.kv_rows[seq] if q.kv_rows is not None else seq
    for j0 in range(0, B, 128):
        nb, blk = n0 + j0, v[:, j0:j0 + 128]
        if nb >= case.N:
            continue
        if q.v_col <= nb < q.v_col + q.D:
            pos = kr if mutant == "kvpos_omitted" else kvpos(kr)
            hd = nb - q.v_col + torch.arange(128, device=dev)
            q.vt[hd[:, None], pos[None, :]] = blk.t()
        elif nb < q.q_col + q.D:
            k_tile = nb < q.q_col
            x = blk.float()
            r = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) * (1.0 / 128.0) + q.eps)
            w = (q.wk if k_tile else q.wq).float()[None, :]
            mm = ((x * r).to(BF16).float() * w).to(BF16).float()
            tab = q.rope_k if k_tile else q.rope_q
            trow = (seq if mutant == "cos_k_by_sequence_row" else kr) if k_tile else seq
            trow = trow.clamp(max=tab[0].shape[0] - 1)
            cos, sin = tab[0][trow], tab[1][trow]
            a, b = mm[:, 0::2], mm[:, 1::2]
            if mutant == "rotation_pair_swapped":
                a, b = b, a
            o = torch.stack([a * cos[:, 0::2] - b * sin[:, 0::2], b * cos[:, 1::2] + a * sin[:, 1::2]], dim=2).reshape(-1, 128).to(BF16)
            hc = nb - (q.k_col if k_tile else q.q_col)
            if k_tile:
                q.ks[kr[:, None], (hc + torch.arange(128, device=dev))[None, :]] = o
            else:
                p.out[m[:, None], (nb + torch.arange(128, device=dev))[None, :]] = o
        else:
            y = torch.where((nb + torch.arange(128, device=dev) >= case.gelu_from)[None, :], _gelu32(blk.float()).to(BF16), blk)
            p.out[m[:, None], (nb + torch.arange(128, device=dev))[None, :]] = y
