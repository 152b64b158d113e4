"""A model of the flash-attention tile core (regione_amd/csrc/attn_tile.h) and the probes that pin its three sequence front ends:
rgn_text_attention_bf16 (width 64, T5 bias table, CLIP causal), rgn_lm_attention_bf16 (width 128, causal, grouped-query) and
rgn_vision_attention_bf16 (widths 32 / 64 / 96 / 128, packed segments).  Plain torch, CPU or GPU tensors.

  ref64 / bound      the fp64 softmax of the operation and the element-wise tolerance of the tile arithmetic;
  emulate            the scheme of the header comment (32-key tiles, fp32 scores, online softmax, P rounded to bf16, the row sum taken over
                     the rounded P, fp32 accumulation) with named defects - a model of the scheme, not of any kernel's instruction order;
  *_case             probe inputs whose correct output is known EXACTLY (counting, spike, head map) and the random / stress inputs of the
                     bound check; a case carries q [Hq, L, D], k, v [Hkv, L, D] and what the kernel is told (scale, causal, table, segments);
  check_*            the checks.  tests/test_gpu_attn_tile_probes.py applies them to the kernels, tests/test_attn_tile_model.py applies the
                     same functions to `emulate` and shows that each defect fails at least one of them.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

BQ, BK = 64, 32                                                     # queries per block, keys per tile (ATTN_BQ, ATTN_BK)
BF16 = torch.bfloat16
DEFECTS = ("drop_last_key", "count_one_padded_key", "causal_off_by_one", "bias_offset_plus_one", "bias_edge_wrong",
           "gqa_head_map_wrong", "no_rescale")

# ---- the shapes of the GPU tests (the CPU test walks the same lists) -----------------------------------------------------------------
LENGTHS = [1, 31, 32, 33, 63, 64, 65, 97, 129]                     # around the 32-key tile and the 64-query block
TEXT_LONG, VISION_LONG, LM_LONG = 1000, 1000, 1500
HEADS = [1, 3]
LM_HEADS = [(1, 1), (4, 2), (6, 2), (28, 4)]                        # (28, 4), the real model's, at L = 65 only
SPIKE_LENGTHS = [33, 65, 129]
WINDOWS_18x22 = [64, 64, 48, 64, 64, 48, 16, 16, 12]                # the window list of an 18 x 22 grid, window 112
VISION_SEGS = {"one": [1], "33": [33], "mixed": [31, 1, 64, 65], "crossing": [60, 70, 3], "windows_18x22": WINDOWS_18x22}
VISION_WIDTHS = [32, 64, 96, 128]
FAMILIES = ["randn", "late_max", "first_max"]


def spike_deltas(L, Lmax):
    """The offsets of the spike: the two edges of the window, the tile boundaries, the diagonal.  An offset the table of Lmax does not hold
    is left out; one it holds outside the window of L (|delta| >= L) stays: no row may see it."""
    return sorted({d for d in [-(L - 1), -33, -32, -1, 0, 1, 31, 32, L - 1] if abs(d) <= Lmax - 1})


def spike_lmaxes(L):
    return [L, L + 3, 4096]


def lm_cases_LH():
    """(L, Hq, Hkv) of every LM test."""
    out = [(L, hq, hkv) for L in LENGTHS for hq, hkv in LM_HEADS[:3]]
    return out + [(65, 28, 4), (LM_LONG, 2, 1)]


def text_cases_LH():
    return [(L, H) for L in LENGTHS for H in HEADS] + [(TEXT_LONG, 1)]


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def head_map(Hq, Hkv, wrong=False):
    """KV head of every query head: h // (Hq / Hkv)."""
    h = torch.arange(Hq)
    return h % Hkv if wrong else h // (Hq // Hkv)


# ---- reference and bound --------------------------------------------------------------------------------------------------------------
def ref64(q, k, v, scale, bias=None, mask=None):
    """fp64 softmax(scale q k^T + bias, masked) over q [Hq, Lq, D], k [Hkv, Lk, D], v [Hkv, Lk, Dv] (query head h reads KV head
    h // (Hq / Hkv)); bias [Hq, Lq, Lk] is added, mask [Lq, Lk] is True where a key is allowed.  `scale` is rounded to fp32 first: that is
    the number a kernel receives.  Returns O_ref = P V and A_ref = P |V|."""
    hm = head_map(q.shape[0], k.shape[0]).to(q.device)
    kd, vd = k.double()[hm], v.double()[hm]
    s = _f32(scale) * (q.double() @ kd.transpose(1, 2))
    if bias is not None:
        s = s + bias.double()
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, -1)
    return p @ vd, p @ vd.abs()


def bound(O_ref, A_ref):
    """Element-wise tolerance of the tile arithmetic against ref64: 2^-8 A_ref + 2^-8 |O_ref| + 1e-6.

    The kernel returns bf16(N / l) with N = sum_j p_j v_j and l = sum_j p_j, where p_j = bf16(w_j) is the softmax weight rounded to
    bf16: p_j = w_j (1 + e_j), |e_j| <= 2^-9.  The SAME rounded weights enter numerator and denominator:
      * numerator:   |sum_j w_j e_j v_j| <= 2^-9 sum_j w_j |v_j|; after the division by sum_j w_j that is 2^-9 A;
      * denominator: l = (sum_j w_j)(1 + e), |e| <= 2^-9, moves the quotient by at most 2^-9 |O| <= 2^-9 A (|O| <= A);
        together 2^-8 A;
      * the one rounding of the quotient to bf16: 2^-9 |O|;
      * a second 2^-9 |O| and the 1e-6 cover what is left: fp32 scores and accumulation (relative 2^-24 per operation - a logit of 60
        moves its weight by about 60 * 2^-24 = 4e-6, about 2^-18), the hardware exp2 (about 1 ulp of fp32) and second-order terms.
    The tile emulation with correct arithmetic reaches at most 0.53 of this bound at L in {777, 1000, 1500}, D in {64, 96, 128}, with and
    without an N(0, 2) bias, and at most 0.76 at the short lengths of the tests; the kernels on an MI355X reach the same figures
    (profiles/r13_attn_tile_probes.txt).  The bound is not to be widened to make a case pass: a case over it is a finding."""
    return 2.0 ** -8 * A_ref + 2.0 ** -8 * O_ref.abs() + 1e-6


# ---- the tile arithmetic ---------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, scale, bias=None, mask=None, defect=None):
    """The scheme of attn_tile.h on q [Hq, Lq, D], k, v [Hkv, Lk, D] (bf16), keys in tiles of 32 from key 0: fp32 scores
    s * scale (+ bias), a masked or padded slot exactly -inf; per tile m' = max(m, tile max), alpha = exp2((m - m') log2 e),
    p = bf16(exp2(s log2 e - m' log2 e)), l = l alpha + sum(p) over the ROUNDED p, o = o alpha + p V in fp32; out = bf16(o * (1 / l)).
    Padded keys hold K = V = 0.  Returns bf16 [Hq, Lq, D].

    `defect` names one mistake of the kind such a kernel can make (DEFECTS):
      drop_last_key          the last key is never counted
      count_one_padded_key   the first key past the end (a zero K / V row of the last tile) gets score 0 instead of -inf
      causal_off_by_one      with a mask: key j + 1 is visible wherever key j is (key i + 1 to query i under a causal mask)
      bias_offset_plus_one   the bias of offset j - i + 1 is read for the pair (i, j) (0 past the window)
      bias_edge_wrong        the bias at the two extreme offsets +-(L - 1) is read as 0
      gqa_head_map_wrong     query head h reads KV head h % Hkv
      no_rescale             alpha is forced to 1"""
    assert defect is None or defect in DEFECTS, defect
    Hq, Lq, _ = q.shape
    Hkv, Lk, _ = k.shape
    dev = q.device
    hm = head_map(Hq, Hkv, wrong=defect == "gqa_head_map_wrong").to(dev)
    kf, vf = k.float()[hm], v.float()[hm]
    s = (q.float() @ kf.transpose(1, 2)) * _f32(scale)
    if bias is not None:
        b = bias.float()
        if defect == "bias_offset_plus_one":                        # the table is Toeplitz: offset + 1 is the row above
            b2 = torch.zeros_like(b)
            b2[:, 1:, :] = b[:, :-1, :]
            b2[:, 0, :-1] = b[:, 0, 1:]
            b = b2
        elif defect == "bias_edge_wrong":
            b = b.clone()
            b[:, 0, Lk - 1] = 0.0
            b[:, Lq - 1, 0] = 0.0
        s = s + b
    allowed = torch.ones(Lq, Lk, dtype=torch.bool, device=dev) if mask is None else mask.clone()
    if defect == "causal_off_by_one" and mask is not None:
        allowed[:, 1:] |= mask[:, :-1]
    if defect == "drop_last_key":
        allowed[:, Lk - 1] = False
    s = s.masked_fill(~allowed, float("-inf"))
    pad = (-Lk) % BK
    s = F.pad(s, (0, pad), value=float("-inf"))
    vf = F.pad(vf, (0, 0, 0, pad))
    if defect == "count_one_padded_key" and pad:
        s[:, :, Lk] = 0.0
    L2E = torch.tensor(1.4426950408889634, dtype=torch.float32, device=dev)
    m = torch.full((Hq, Lq), float("-inf"), device=dev)
    l = torch.zeros(Hq, Lq, device=dev)
    o = torch.zeros(Hq, Lq, vf.shape[-1], device=dev)
    for k0 in range(0, Lk + pad, BK):
        sc = s[:, :, k0:k0 + BK]
        m_new = torch.maximum(m, sc.amax(-1))
        alpha = torch.exp2((m - m_new) * L2E)
        if defect == "no_rescale":
            alpha = torch.ones_like(alpha)
        p = torch.exp2(sc * L2E + (-m_new * L2E)[..., None]).to(BF16).float()
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p @ vf[:, k0:k0 + BK]
        m = m_new
    return (o * (1.0 / l)[..., None]).to(BF16)


def defect_applies(case, defect):
    """False where the defect provably cannot change the case's output (no table, no mask, one KV head per query head)."""
    if defect in ("bias_offset_plus_one", "bias_edge_wrong"):
        return case.table is not None
    if defect == "gqa_head_map_wrong":
        return case.q.shape[0] != case.k.shape[0]
    if defect == "causal_off_by_one":
        return case.causal
    return True


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _case(kind, q, k, v, scale, causal=False, table=None, Lmax=0, segs=None, **extra):
    assert kind in ("text", "lm", "vision")
    return SimpleNamespace(kind=kind, q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), scale=scale, causal=causal, table=table, Lmax=Lmax, segs=segs,
                           **extra)


def to_device(case, device):
    c = SimpleNamespace(**vars(case))
    c.q, c.k, c.v = c.q.to(device), c.k.to(device), c.v.to(device)
    c.table = None if c.table is None else c.table.to(device)
    return c


def cu_of(segs):
    cu = [0]
    for n in segs:
        cu.append(cu[-1] + n)
    return cu


def dense_bias(case):
    """fp32 [H, L, L]: table[h, j - i + Lmax - 1], the T5 relative-position window of the case (None without a table)."""
    if case.table is None:
        return None
    L = case.q.shape[1]
    i = torch.arange(L, device=case.q.device)[:, None]
    j = torch.arange(L, device=case.q.device)[None, :]
    return case.table.float()[:, j - i + case.Lmax - 1]


def dense_mask(case):
    """bool [L, L], True where query i may see key j: the causal triangle, the block diagonal of the segments, or None (every key)."""
    L, dev = case.q.shape[1], case.q.device
    if case.segs is not None:
        seg = torch.repeat_interleave(torch.arange(len(case.segs)), torch.tensor(case.segs)).to(dev)
        return seg[:, None] == seg[None, :]
    if case.causal:
        return torch.ones(L, L, dtype=torch.bool, device=dev).tril()
    return None


def run_model(case, defect=None):
    """`emulate` the way the kernel of the case walks its keys: a vision segment is its own key range, tiled from the segment's first
    key; text and LM walk keys 0 .. L - 1 under the causal mask."""
    if case.segs is None:
        return emulate(case.q, case.k, case.v, case.scale, dense_bias(case), dense_mask(case), defect)
    cu = cu_of(case.segs)
    return torch.cat([emulate(case.q[:, a:b], case.k[:, a:b], case.v[:, a:b], case.scale, None, None, defect)
                      for a, b in zip(cu[:-1], cu[1:])], dim=1)


def reference(case):
    return ref64(case.q, case.k, case.v, case.scale, dense_bias(case), dense_mask(case))


def _gen(*seed):
    """A CPU generator seeded by the case's parameters (the same inputs in every process and on every machine)."""
    n = 0
    for s in seed:
        n = (n * 1000003 + int(s) + 4096) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(n)


def _ints(g, shape, nonzero=False):
    """Integers of [-4, 4] (exact in bf16; any sum of at most 4096 of them is exact in fp32, in any order: |sum| <= 4 * 4096 < 2^24)."""
    if nonzero:
        return torch.randint(1, 5, shape, generator=g).float() * (2 * torch.randint(0, 2, shape, generator=g).float() - 1)
    return torch.randint(-4, 5, shape, generator=g).float()


def _dims(kind, L, Hq, Hkv, D, segs):
    if kind == "text":
        assert D == 64 and Hq == Hkv
    if kind == "lm":
        assert D == 128
    if kind == "vision":
        assert Hq == Hkv and sum(segs) == L
    return (Hq, L, D), (Hkv, L, D)


def counting_case(kind, L, Hq, Hkv, D, causal=False, zero_table=False, segs=None, width=None):
    """q = 0: every allowed key has weight exactly 1 and the row sum is exactly the key count.  V holds integers of [-4, 4], so every
    sum is exact in fp32 in any order; K is N(0, 1) and must not matter.  `width` < D: the channels past it are zero in q, k and v (a
    head of that width padded with zero columns)."""
    qs, ks = _dims(kind, L, Hq, Hkv, D, segs)
    g = _gen(1, L, Hq, Hkv, D, causal, zero_table)
    k, v = torch.randn(ks, generator=g), _ints(g, ks)
    if width is not None:
        k[..., width:] = 0
        v[..., width:] = 0
    table = torch.zeros(Hq, 2 * (L + 3) - 1, dtype=BF16) if zero_table else None
    return _case(kind, torch.zeros(qs), k, v, D ** -0.5, causal, table, L + 3 if zero_table else 0, segs, width=width)


def spike_case(L, H, delta, Lmax, causal):
    """The text kernel with a bias table that is zero except +40 at offset delta, q = 0: query i, where key i + delta exists and the mask
    allows it, gives that key weight 1 and every other key e^-40 = 4e-18, and returns V[i + delta].  V holds NONZERO integers of
    [-4, 4]: the e^-40 weights (at most 129 of them) cannot move the fp32 sum off a nonzero integer, let alone its bf16 rounding,
    while next to a zero they would be the whole result."""
    assert abs(delta) <= Lmax - 1 and L <= Lmax
    g = _gen(2, L, H, delta, Lmax, causal)
    k, v = torch.randn(H, L, 64, generator=g), _ints(g, (H, L, 64), nonzero=True)
    table = torch.zeros(H, 2 * Lmax - 1, dtype=BF16)
    table[:, delta + Lmax - 1] = 40.0
    return _case("text", torch.zeros(H, L, 64), k, v, 0.125, causal, table, Lmax, None, delta=delta)


def headmap_case(L, Hq, Hkv):
    """Every element of the V columns of KV head g is g + 1; q and k are N(0, 1): whatever the weights, query head h must return
    h // (Hq / Hkv) + 1 (at most 4: exact in bf16, and the fp32 rounding of sum(p) (g + 1) / sum(p) is far inside a bf16 step)."""
    g = _gen(3, L, Hq, Hkv)
    q, k = torch.randn(Hq, L, 128, generator=g), torch.randn(Hkv, L, 128, generator=g)
    v = (torch.arange(Hkv).float() + 1)[:, None, None].expand(Hkv, L, 128).clone()
    return _case("lm", q, k, v, 128 ** -0.5, True)


STRESS_LOGIT = 60.0


def bound_case(kind, family, L, Hq, Hkv, D, causal=False, bias=False, segs=None, width=None):
    """Inputs of the fp64 bound check.
      randn      q, k, v of N(0, 1).
      late_max   channel 0 steers the logits: scale q.k climbs from about -60 in the first key tile (of the segment) to about +60 in the
                 last, tile by tile, so the running maximum moves in EVERY tile (alpha != 1 each time) and the largest score of every
                 row lies in the last tile the row sees; the other channels are N(0, 0.4^2), a logit noise of sigma 0.16.
      first_max  the mirror image: key 0 (of the segment) at +60, the tiles falling from +56 to -60: the maximum never moves after the
                 first tile and the last tile's weights underflow.
    The steps between tiles are at least 116 / 46 = 2.5, sixteen sigma of the noise, so the tile of the maximum is certain;
    check_stress_shape asserts it and that the fp64 reference is finite.  bias: a 2 N(0, 1) table, Lmax = L + 3 (text only)."""
    assert family in FAMILIES
    qs, ks = _dims(kind, L, Hq, Hkv, D, segs)
    g = _gen(4, L, Hq, Hkv, D, causal, bias, FAMILIES.index(family))
    scale = (width or D) ** -0.5
    if family == "randn":
        q, k = torch.randn(qs, generator=g), torch.randn(ks, generator=g)
    else:
        q, k = 0.4 * torch.randn(qs, generator=g), 0.4 * torch.randn(ks, generator=g)
        t = torch.empty(L)
        cu = cu_of(segs) if segs is not None else [0, L]
        for a, b in zip(cu[:-1], cu[1:]):
            tile = (torch.arange(b - a) // BK).float()
            nt = int(tile[-1]) + 1
            if family == "late_max":
                t[a:b] = -STRESS_LOGIT + 2 * STRESS_LOGIT * tile / (nt - 1) if nt > 1 else STRESS_LOGIT
            else:
                t[a:b] = (STRESS_LOGIT - 4) - (2 * STRESS_LOGIT - 4) * tile / (nt - 1) if nt > 1 else -STRESS_LOGIT
                t[a] = STRESS_LOGIT
        q[..., 0] = 8.0
        k[..., 0] = t / (_f32(scale) * 8.0)
    v = torch.randn(ks, generator=g)
    if width is not None:
        q[..., width:] = 0
        k[..., width:] = 0
        v[..., width:] = 0
    table = (2.0 * torch.randn(Hq, 2 * (L + 3) - 1, generator=g)).to(BF16) if bias else None
    return _case(kind, q, k, v, scale, causal, table, L + 3 if bias else 0, segs, family=family, width=width)


# ---- expected outputs and checks -------------------------------------------------------------------------------------------------------
def counting_allowed(case):
    """The two values an element of the counting probe may take, bf16 [Hq, L, D] each: with sum and count the exact sum of V[:, c] over
    the keys the row may see and their number,  bf16(fp32(sum) * fp32(1 / count))  - the kernel's o * (1 / l) -  and  bf16(sum / count)
    in fp64.  They differ only where the rounded reciprocal moves the product across a bf16 tie.  (fp64 -> bf16 goes through fp32; a
    quotient of integers below 2^15 by a count below 2^12 is an exact bf16 tie or at least 2^-20 relative away from one: no double rounding.)"""
    hm = head_map(case.q.shape[0], case.k.shape[0]).to(case.q.device)
    vh = case.v[hm]
    mask = dense_mask(case)
    if mask is None:                                                # every key, for every query (Sq != Skv: the region kernels)
        mask = torch.ones(case.q.shape[1], vh.shape[1], dtype=torch.bool, device=vh.device)
    total = mask.double() @ vh.double()                             # exact
    count = mask.sum(-1).double()[None, :, None]
    return two_roundings(total, count)


def two_roundings(total, count):
    """The two-value rule of counting_allowed on an exact fp64 sum and count (broadcast against each other)."""
    a = (total.float() * (1.0 / count.float())).to(BF16)
    b = (total / count).float().to(BF16)
    return a, b


def spike_allowed(case):
    """counting_allowed, with V[i + delta] (both values) in the rows whose spike key exists and is visible."""
    a, b = counting_allowed(case)
    L, d = case.q.shape[1], case.delta
    rows = [i for i in range(L) if 0 <= i + d < L and (not case.causal or d <= 0)]
    if rows:
        rows = torch.tensor(rows, device=case.q.device)
        a[:, rows] = case.v[:, rows + d]
        b[:, rows] = case.v[:, rows + d]
    return a, b


def probe_mismatches(out, a, b):
    """Number of elements that equal neither allowed value (torch.equal semantics: values compare, a NaN equals nothing)."""
    return int((~((out == a) | (out == b))).sum())


def check_counting(case, out):
    n = probe_mismatches(out, *counting_allowed(case))
    if case.width is not None:
        n += int((out[..., case.width:] != 0).sum())               # the pad columns stay exactly 0
    return n


def check_spike(case, out):
    return probe_mismatches(out, *spike_allowed(case))


def check_headmap(case, out):
    Hq, Hkv = case.q.shape[0], case.k.shape[0]
    want = (head_map(Hq, Hkv).float() + 1).to(out.device)[:, None, None].expand_as(out)
    return int((out.float() != want).sum())


def bound_ratio(case, out, ref=None):
    """max over the elements of |out - O_ref| / bound (a NaN counts as infinite); <= 1 passes."""
    O_ref, A_ref = reference(case) if ref is None else ref
    assert bool(torch.isfinite(O_ref).all()) and bool(torch.isfinite(A_ref).all()), "the fp64 reference itself must be finite"
    r = (out.double() - O_ref).abs() / bound(O_ref, A_ref)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def check_stress_shape(case):
    """The promises of bound_case for the stress families, on the fp64 logits WITHOUT the bias: they reach 50, and the largest one of
    every row lies in the last key tile the row sees (late_max) / on the first key (first_max)."""
    if case.family == "randn":
        return
    L = case.q.shape[1]
    hm = head_map(case.q.shape[0], case.k.shape[0]).to(case.q.device)
    s = _f32(case.scale) * (case.q.double() @ case.k.double()[hm].transpose(1, 2))
    assert float(s.abs().max()) >= 50.0, float(s.abs().max())
    mask = dense_mask(case)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    arg = s.argmax(-1)                                              # [Hq, L]
    rows = torch.arange(L, device=s.device)
    if case.segs is not None:
        cu = torch.tensor(cu_of(case.segs), device=s.device)
        seg = torch.bucketize(rows, cu[1:], right=True)
        first, last = cu[seg], cu[seg + 1] - 1
    else:
        first, last = torch.zeros_like(rows), rows if case.causal else torch.full_like(rows, L - 1)
    if case.family == "late_max":
        assert bool(((arg - first) // BK == (last - first) // BK).all()), "the largest logit of a row is not in its last key tile"
    else:
        assert bool((arg == first).all()), "the largest logit of a row is not on its first key"


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)
