"""A model of the fp8-activation GEMM (regione_amd/csrc/gemm.hip: rgn_gemm_group with `ascale`, kernel variant AV = 10) and of the row
quantiser in front of it (csrc/norm.hip: rgn_quantize_rows_a8), with the probes that pin both to the mathematics.  Plain torch, CPU or GPU
tensors, no GPU import.  The number formats, the sentinel frame, the closed-form checks and the epilogue emulation are those of
tests/gemm_model.py (imported as G); this file adds what the new format adds:

  quantize_rows      the quantiser as a torch expression: scale = max(amax|x|, 1e-12) / 448 per row (fp32), q = e4m3fn_rne(f32(x) / scale);
  quant_rows         the input rows the quantiser is probed with (ties, subnormal results, amax in the last column, ...);
  TABLE / QKV_TABLE  M x N x K x geometry: the smallest shapes that reach every tile path of the variant (one K tile of 128 = prologue only,
                     two, an odd count; one row, a ragged tile, more than one tile; 128 x 128 tiles, 256 x 256 tiles, quarter tiles; groups);
  *_case             probe inputs whose correct output is known exactly from a closed form without a matrix product, and the quantised
                     random / cancelling inputs of the fp64 bound.  A problem holds A as e4m3fn byte codes + one fp32 scale per row, W as byte
                     codes + one scale per output channel, bias, the prefilled destination and `lin`, the exact pre-activation in fp64;
  emulate            the tile walk over K tiles of 128 and the scale order of the epilogue, (acc * ascale[m]) * wscale[n] + bias, with the
                     named defects of MUTANTS.
tests/test_gpu_gemm_a8_probes.py applies the checks to the kernels; tests/test_gemm_a8_model.py applies them to `emulate` and shows that
every mutant changes at least one probe output.
"""
from types import SimpleNamespace as NS

import torch

import gemm_model as G

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
BK8 = 128                                       # K tile of the fp8 x fp8 variant: 128 values = 128 bytes per row
MUTANTS = ("k_halves_swapped", "lane_groups_permuted", "row_scale_of_tile_row", "scales_after_bias", "last_k_tile_dropped", "amax_k_minus_1")
G128, G256 = dict(gemm_geometry=128), dict(gemm_geometry=256)
ONE = 0x38                                      # e4m3fn code of 1.0


# ---- the quantiser ----------------------------------------------------------------------------------------------------------------------
def quantize_rows(x, mutant=None):
    """bf16 [M, K] -> (codes uint8 [M, K], scale fp32 [M]): ops.quantize_w8 restated per row."""
    xf = x.float()
    src = xf[:, :-1] if mutant == "amax_k_minus_1" else xf
    scale = src.abs().amax(dim=1).clamp_min(1e-12) / 448.0
    return (xf / scale[:, None]).to(FP8).view(torch.uint8), scale


def a_values(p):
    """A [M, K] as fp64 values (without the row scale)."""
    return G.e4m3fn_table(p.A.device)[p.A.long()]


def quant_rows(K, seed=0):
    """name -> bf16 row [K] the quantiser must get right, bit for bit."""
    g = torch.Generator().manual_seed(77 + seed)
    rows = {}
    rows["randn"] = torch.randn(K, generator=g)
    rows["zero"] = torch.zeros(K)
    one = torch.zeros(K)
    one[K // 3] = -3.0
    rows["single_nonzero"] = one
    # amax = 448 exactly: scale = 1, so the stored values ARE the scaled values - every midpoint between two neighbouring e4m3fn values
    # (normal and subnormal; a bf16 holds each: 5 significant bits at most), with both signs, then values just off the midpoints
    v = G.e4m3fn_table()
    fin = torch.sort(v[(torch.arange(256) & 0x7f) != 0x7f].unique()).values
    mids = (fin[:-1] + fin[1:]) / 2
    ties = torch.cat([mids, mids * (1 + 2.0 ** -7), mids * (1 - 2.0 ** -7)]).to(BF16).float()
    t = torch.zeros(max(K, 0))
    n = min(K - 1, ties.numel())
    t[:n] = ties[torch.randperm(ties.numel(), generator=g)[:n]]
    t[K - 1] = 448.0
    rows["ties"] = t
    # results below the smallest normal e4m3fn (2^-6): a large amax and many small values
    sub = torch.randn(K, generator=g) * 2.0 ** -8
    sub[5] = 7.0
    rows["subnormal_results"] = sub
    last = torch.randn(K, generator=g) * 0.25
    last[K - 1] = -9.5
    rows["amax_last_column"] = last
    rows["tiny"] = torch.full((K,), 1e-20)          # amax below the clamp: scale = 1e-12 / 448
    return {k: r.to(BF16) for k, r in rows.items()}


# ---- the table of launch paths -----------------------------------------------------------------------------------------------------------
# gemm_bf16_kernel<EPI, BM, BN, WM, WN, MODE_FULL, 10>: <128,128,2,2> (plain and quarter = 1) and <256,256,2,4>, epilogues BIAS / GELU / QKV.
def _row(name, Ms, N, K, epi, knobs, plan, **feat):
    return NS(name=name, Ms=tuple(Ms), N=N, K=K, w8=True, epi=epi, knobs=dict(knobs), plan=plan, feat=feat, slots=None)


TABLE = []
for _gi, (_gn, _knobs, _plan) in enumerate((("128", G128, 0), ("256", G256, G.BIG | 1))):
    _i = 0
    for _M in (1, 130, 257):
        for _N in (128, 384):
            for _K in (128, 256, 640):
                TABLE.append(_row(f"a8_{_gn}_m{_M}_n{_N}_k{_K}", (_M,), _N, _K, "gelu" if (_i + _gi) % 2 else "bias", _knobs, _plan))
                _i += 1
TABLE += [
    _row("a8_quarter", (257,), 384, 640, "bias", dict(G256, gemm_quarter=1), G.BIG | G.QUARTER | 1),       # 2 x 2 parent tiles: quadrants past both edges
    _row("a8_quarter_gelu", (130,), 384, 256, "gelu", dict(G256, gemm_quarter=1), G.BIG | G.QUARTER | 1),
    _row("a8_grp128", (130, 257), 384, 256, "bias", G128, 0, share_w=False),
    _row("a8_grp256", (130, 257), 384, 640, "gelu", G256, G.BIG | 1, share_w=False),
    _row("a8_strided", (130,), 128, 256, "bias", G128, 0, lda=64),                                         # lda > K (bytes)
]
for _r in TABLE:
    if _r.name.startswith("a8_grp"):
        _r.feat["share_w"] = True               # the two problems share one W (text / image rows of one stream, the CFG branches)
QKV_TABLE = [
    _row("a8_qkv128", (200,), 768, 256, "qkv", G128, 0, row_base=0, perm=False, f16=False),
    _row("a8_qkv256", (333,), 1024, 256, "qkv", G256, G.BIG | 1, row_base=48, perm=True, f16=True),          # + an MLP half of 256 columns
    _row("a8_qkv_quarter", (333,), 768, 256, "qkv", dict(G256, gemm_quarter=1), G.BIG | G.QUARTER | 1, row_base=5, perm=True, f16=False),
]
TABLE_BY_NAME = {r.name: r for r in TABLE + QKV_TABLE}
BOUND_ROWS = [r.name for r in TABLE]


def plan_query_args(row):
    """(Ms, N, K, distinct_w, w8 = 2) for rgn_gemm_plan_query."""
    n = sum(1 for m in row.Ms if m > 0)
    return list(row.Ms), row.N, row.K, (1 if row.feat.get("share_w") else n), 2


def _share(row):
    """G._finish shares W between problems 0 and 2 of a `share_w` group; here a group has two problems that share it."""
    return row.feat.get("share_w")


def _finish(case, row, dev, build):
    made = {}
    for i, M in enumerate(row.Ms):
        wid = 0 if _share(row) else i
        A, asc, W, ws, bias, lin = build(i, wid, M)
        if wid in made:
            W, ws = made[wid]
        made[wid] = (W, ws)
        p = NS(M=M, A=A, ascale=asc, W=W, wscale=ws, bias=bias, lin=lin, wid=wid, R=M, out_rows=None, gate=None, resid=None,
               out_init=G.sentinel((M + G.XR, row.N + G.XC), dev))
        case.probs.append(p)
    return case


def _onehot(M, K, dev, shift=0, codes=None):
    """One-hot A as byte codes: row m holds `codes[m]` (default: 1.0) at k = G.f_onehot(m) and +0 elsewhere."""
    A = torch.zeros(M, K, dtype=torch.uint8, device=dev)
    A[torch.arange(M, device=dev), G.f_onehot(M, K, dev, shift)] = ONE if codes is None else codes
    return A


def _row_scales(M, dev, i, pow2, whole=False):
    tab = torch.tensor([2.0, 1.0, 4.0, 1.0, 2.0] if whole else [2.0, 0.5, 1.0, 4.0, 0.25] if pow2 else [1.5, 0.75, 1.25, 0.375, 0.625], device=dev)
    return tab[(3 * torch.arange(M, device=dev) + i) % 5].float()


def index_shifts(row):
    """Passes of the index probe: the rows of a problem of M >= 130 rows select every k over them; a one-row problem (whose point is
    the clamped tile edge, not the index map) runs six."""
    return min(G.index_shifts(row), 6) if max(row.Ms) == 1 else G.index_shifts(row)


def index_case(row, dev="cpu", halves=False, shift=0, **kw):
    """a. one-hot A (the code of 1.0), W[n, k] one of the integers e4m3fn holds, a function of n AND k that is not symmetric in them,
    row and channel scales with short mantissas that are no power of two, integer bias:
    out[m, n] = epilogue(W[n, f(m)] * ascale[m] * wscale[n] + bias[n]) - every product and the sum exact in fp32.
    halves: pre-activations on the grid of halves in [-8, 8] (the GELU probe), unit scales.
    Where the probe runs through a GELU row the row scales are 1, 2 and 4: the pre-activations then stay on the grid of eighths, like
    those of G.index_case, which holds no value in (-10.11, -10.06] - there fp32 exp2 overflows before the GELU itself goes subnormal,
    the one window that neither the two-neighbour rule nor G.FLUSH describes."""
    case = G._case(row, "index", dev, **kw)
    case.allow_flush = not halves
    N, K = row.N, row.K

    def build(i, wid, M):
        codes = G._int_codes(dev)
        if halves:
            v = G.e4m3fn_table(dev)
            codes = torch.arange(256, device=dev)[(v * 2 == (v * 2).round()) & (v.abs() <= 7.5)]
        W = codes[G._grid(N, K, dev, wid, len(codes), 0)].to(torch.uint8)
        ws = G._scales(N, dev, wid, pow2=False) if not halves else torch.ones(N, device=dev)
        asc = _row_scales(M, dev, i, pow2=False, whole=case.epi == "gelu") if not halves else torch.ones(M, device=dev)
        n = torch.arange(N, device=dev)
        bias = (((5 * n + 3 * i) % 3 - 1).double() / 2 if halves else ((5 * n + 3 * i) % 17 - 8)).to(BF16)
        wv = G.w_values(NS(W=W, wscale=ws))
        lin = wv.t()[G.f_onehot(M, K, dev, shift)] * asc.double()[:, None] * ws.double()[None, :] + bias.double()
        return _onehot(M, K, dev, shift), asc, W, ws, bias, lin
    return _finish(case, row, dev, build)


def bytecode_case(row, dev="cpu", shift=0):
    """b. every finite e4m3fn code (-0, the subnormals and +-448 included) in A AND in W, power-of-two scales, no bias: row m holds code
    a(m) at k = f(m), so out[m, n] = bf16(value(a(m)) value(W[n, f(m)]) ascale[m] wscale[n]) - a product of two 4-bit significands,
    exact in fp32 and in bf16."""
    case = G._case(row, "bytecode", dev, epi="bias")
    fin = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], device=dev)

    def build(i, wid, M):
        n, k = torch.arange(row.N, device=dev)[:, None], torch.arange(row.K, device=dev)[None, :]
        W = fin[(n + k + 3 * wid) % 254].to(torch.uint8)
        ws = torch.exp2(((torch.arange(row.N, device=dev) % 7) - 3).float())
        acodes = fin[(5 * torch.arange(M, device=dev) + 11 * i + 127 * shift) % 254].to(torch.uint8)
        asc = _row_scales(M, dev, i, pow2=True)
        A = _onehot(M, row.K, dev, shift, acodes)
        f = G.f_onehot(M, row.K, dev, shift)
        av = G.e4m3fn_table(dev)[acodes.long()]
        lin = av[:, None] * G.w_values(NS(W=W, wscale=ws)).t()[f] * asc.double()[:, None] * ws.double()[None, :] + 0.0
        return A, asc, W, ws, None, lin
    c = _finish(case, row, dev, build)
    c.a_codes_seen = int(torch.cat([p.A[torch.arange(p.M, device=dev), G.f_onehot(p.M, row.K, dev, shift)] for p in c.probs if p.M > 0]).unique().numel())
    c.w_codes_seen = int(torch.cat([p.W[:, G.f_onehot(p.M, row.K, dev, shift)].flatten() for p in c.probs if p.M > 0]).unique().numel())
    return c


def scale_bias_case(row, dev="cpu"):
    """c. row and channel scales that are no power of two and a bias of magnitude >= 3: (acc * ascale * wscale) + bias and
    (acc + bias) * ascale * wscale differ by |bias| |1 - ascale wscale| >= 3 * 0.0625 on values below 256 - not a rounding."""
    case = G._case(row, "scale_bias", dev, epi="bias")
    codes = G._int_codes(dev)

    def build(i, wid, M):
        W = codes[G._grid(row.N, row.K, dev, wid, len(codes), 0)].to(torch.uint8)
        ws = torch.tensor([0.75, 0.375, 0.625], device=dev)[(torch.arange(row.N, device=dev) + wid) % 3].float()
        asc = _row_scales(M, dev, i, pow2=False)
        n = torch.arange(row.N, device=dev)
        bias = (((n * 3 + i) % 6 + 3) * (1 - 2 * (n % 2))).to(BF16)
        lin = G.w_values(NS(W=W, wscale=ws)).t()[G.f_onehot(M, row.K, dev)] * asc.double()[:, None] * ws.double()[None, :] + bias.double()
        return _onehot(M, row.K, dev), asc, W, ws, bias, lin
    return _finish(case, row, dev, build)


def _pow2_lut(dev):
    """value + 256 -> e4m3fn code, for +-2^0 ... +-2^7."""
    v = G.e4m3fn_table(dev)
    lut = torch.zeros(513, dtype=torch.long, device=dev)
    for val in [s * (1 << b) for s in (1, -1) for b in range(8)]:
        lut[val + 256] = int(torch.nonzero(v == val)[0])
    return lut


def signature_case(row, dev="cpu"):
    """d. every K tile of 128 adds its own power of two: A holds a single 1 per K tile (its position inside the tile depends on the row and
    the tile), W[n, k] = sign(n, tile) 2^(tile % 8) for every k of the tile: out[m, n] = sum_t sign(n, t) 2^(t % 8), any partial sum an
    integer below 256.  A dropped, repeated or misplaced K tile changes the sum.  No bias."""
    case = G._case(row, "signature", dev, epi="bias")
    N, K = row.N, row.K
    nk = K // BK8
    lut = _pow2_lut(dev)

    def build(i, wid, M):
        k = torch.arange(K, device=dev)
        t = k // BK8
        n = torch.arange(N, device=dev)[:, None]
        Wv = G._sig_sign(n, t[None, :], wid) * (2 ** (t % 8))[None, :]
        W = lut[Wv + 256].to(torch.uint8)
        m = torch.arange(M, device=dev)
        pos = ((m * 11 + 7)[:, None] + 37 * t[None, :]) % BK8
        A = (((k[None, :] % BK8) == pos).to(torch.uint8) * ONE)
        lin = torch.zeros(M, N, dtype=torch.float64, device=dev)
        for tt in range(nk):
            lin += G._sig_sign(n.t(), tt, wid).double() * 2.0 ** (tt % 8)
        return A, torch.ones(M, device=dev), W, torch.ones(N, device=dev), None, lin + 0.0
    return _finish(case, row, dev, build)


def bound_case(row, family, dev="cpu"):
    """e. the `randn` / `cancel` operands of G.bound_case, quantised: A by the quantiser model above (per row), W per output channel.
    lin = (A8 @ W8^T) ascale wscale + bias in fp64 on the QUANTISED values, S = sum_k |a| |w| ascale wscale."""
    base = G.bound_case(row, family, "cpu")
    case = G._case(row, "bound_" + family, dev, epi="bias")
    made = {}
    for p0 in base.probs:
        A, asc = quantize_rows(p0.A)
        W, ws = made.setdefault(0 if _share(row) else id(p0.W), (p0.W, p0.wscale))
        p = NS(M=p0.M, A=A.to(dev), ascale=asc.to(dev), W=W.to(dev), wscale=ws.to(dev), bias=p0.bias.to(dev), wid=p0.wid, R=p0.M, out_rows=None,
               gate=None, resid=None, out_init=G.sentinel((p0.M + G.XR, row.N + G.XC), dev))
        av, wv = a_values(p), G.w_values(p)
        sc = p.ascale.double()[:, None] * p.wscale.double()[None, :]
        p.lin = av @ wv.t() * sc + p.bias.double()
        p.S = av.abs() @ wv.abs().t() * sc
        case.probs.append(p)
    return case


def bound_ratio(case, outs):
    """worst |out - lin| / (2^-8 |lin| + (K + 2) 2^-22 S + 1e-30): the bound of tests/gemm_model.py with one more bit on the sum term - at
    most K fp32 additions and two scale multiplications each err by at most one ulp of a partial sum <= S, whether the unit rounds or
    truncates.  The sentinel outside the problem must be intact (-> inf)."""
    worst = 0.0
    for p, got in zip(case.probs, outs):
        if p.M == 0:
            continue
        if not G.outside_intact(p, got, case.N):
            return float("inf")
        bound = 2.0 ** -8 * p.lin.abs() + (case.K + 2) * 2.0 ** -22 * p.S + 1e-30
        worst = max(worst, float(((got[:p.M, :case.N].double() - p.lin).abs() / bound).max()))
    return worst


def qkv_case(row, dev="cpu"):
    """f. G.qkv_case restated on fp8 operands: one-hot A as byte codes with unit row scales, W[n, k] = sign(n) 2^(k % 8) as byte codes with
    unit channel scales - the same integer arithmetic, the same expected Q, K slab and V^T slab (G.qkv_expected / G.check_qkv)."""
    case = G.qkv_case(row, dev)
    p = case.probs[0]
    p.W = _pow2_lut(dev)[p.W.long() + 256].to(torch.uint8)
    p.wscale = torch.ones(row.N, device=dev)
    p.A = _onehot(p.M, row.K, dev)
    p.ascale = torch.ones(p.M, device=dev)
    return case


# ---- the emulation -----------------------------------------------------------------------------------------------------------------------
def _a_tile(a, kt, mutant):
    """The 128 values of K tile kt of the A rows as the MFMA pairs them with W's: lane group g = l >> 4 holds k = 32 g + 16 h + j
    (h = which ds_read_b128, j = byte) of the tile.  The mutants move A's bytes only - W keeps its order."""
    t = a[:, kt * BK8:(kt + 1) * BK8].reshape(a.shape[0], 4, 2, 16)
    if mutant == "k_halves_swapped":
        t = t.flip(2)
    if mutant == "lane_groups_permuted":
        t = t.roll(1, dims=1)
    return t.reshape(a.shape[0], BK8)


def emulate(case, row, mutant=None):
    """What the launch of `row` writes for `case`: the destination buffers (Q/K/V: (out, K slab, V^T slab)).  Whole-K tiles only: the
    128 x 128 geometry, the 256 x 256 geometry, or - quarter - the quadrants of 256 x 256 parent tiles."""
    big, quarter = bool(row.plan & G.BIG), bool(row.plan & G.QUARTER)
    PB = 256 if big else 128
    probs = [p for p in case.probs if p.M > 0]
    dev = probs[0].A.device
    tab = G.e4m3fn_table(dev).float()
    for p in probs:
        p.Af, p.Wf, p.out = tab[p.A.long()], tab[p.W.long()], p.out_init.clone()
    if case.qkv is not None:
        case.qkv.ks, case.qkv.vt = case.qkv.k_init.clone(), case.qkv.vt_init.clone()
    nk = case.K // BK8 - (1 if mutant == "last_k_tile_dropped" else 0)
    for p in probs:
        for t in range(((p.M + PB - 1) // PB) * ((case.N + PB - 1) // PB)):
            tm, tn = G.tile_coords(t, p.M, case.N, PB)
            blocks = [(tm * 256 + (q >> 1) * 128, tn * 256 + (q & 1) * 128, 128) for q in range(4)] if quarter else [(tm * PB, tn * PB, PB)]
            for m0, n0, B in blocks:
                if m0 >= p.M or n0 >= case.N:
                    continue
                rows = (m0 + torch.arange(B, device=dev)).clamp(max=p.M - 1)
                a = p.Af[rows]
                w = p.Wf[(n0 + torch.arange(B, device=dev)).clamp(max=case.N - 1)]
                acc = torch.zeros(B, B, device=dev)
                for kt in range(nk):
                    acc = acc + _a_tile(a, kt, mutant) @ w[:, kt * BK8:(kt + 1) * BK8].t()
                asc = p.ascale[torch.arange(B, device=dev).clamp(max=p.M - 1)] if mutant == "row_scale_of_tile_row" else p.ascale[rows]
                if mutant == "scales_after_bias":
                    n = (n0 + torch.arange(B, device=dev)).clamp(max=case.N - 1)
                    bias = p.bias.float()[n] if p.bias is not None else torch.zeros(B, device=dev)
                    c = ((acc + bias) * asc[:, None]) * p.wscale[n]
                    G._epilogue(case, NS(**{**p.__dict__, "bias": None, "wscale": None}), probs[0], c, m0, n0, B, None)
                else:
                    G._epilogue(case, p, probs[0], acc * asc[:, None], m0, n0, B, None)          # then * wscale[n] + bias, as with bf16 A
    if case.qkv is not None:
        return [(probs[0].out, case.qkv.ks, case.qkv.vt)]
    outs = {id(p): p.out for p in probs}
    return [outs.get(id(p), p.out_init) for p in case.probs]
