"""A model of the wide decode step (regione_amd/csrc/decode.hip: lm_gemm_rows_kernel behind rgn_lm_gemm_rows_bf16, rgn_lm_gemm_rows_w8 and
rgn_lm_head_argmax_wide) and the probes that pin the kernel to the mathematics.  Plain torch on the CPU, no GPU import; the number formats
(`e4m3fn_table`) and the `randn` / `cancel` families of the fp64 bound are those of tests/gemm_model.py.  What the model states:

  fragment k map   a block owns 16 weight rows and walks K in chunks of KC = 1024; wave w of 4 owns k in [256 w, 256 w + 256) of a chunk,
                   KW = 256 k = 8 MFMAs of 32 k; element j of lane group g of MFMA m is k = 32 m + 8 g + j for bf16 weights and
                   k = 64 (m // 2) + 16 g + 8 (m % 2) + j for fp8 weights, X under the SAME map (`kmap`);
  K split / fold   the split depends on K alone (uneven when K % 1024 != 0: at K = 2 KW + 64 the waves own 256, 256, 64 and 0 k); the four
                   fp32 partial sums are added in wave order 0, 1, 2, 3;
  scale once       v = fma(folded sum, wscale[n], bias[n]): the per-channel scale of ops.quantize_w8 multiplies the folded sum, once;
  two roundings    y = bf16(v), or with a residual bf16(bf16(v) + resid[b, n]);
  tie rule         lm_head keeps fp32 logits; a block keeps the FIRST maximum of its 16 rows, the finalize the lowest index among equals.

`emulate` / `emulate_head` carry the named defects of MUTANTS; tests/test_lm_rows_mfma_model.py shows that every one of them changes at
least one probe, tests/test_gpu_lm_rows_mfma.py applies the same probes to the kernels.
"""
from types import SimpleNamespace as NS

import torch

import gemm_model as G

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
KW, KC, NWAVE, TILE = 256, 1024, 4, 16
MAX_B = 32
SENT = -7.0                                     # the sentinel of the frames: no probe produces it
MUTANTS = ("k_halves_swapped", "scale_per_partial", "resid_before_rounding", "tail_writes_column_n", "row_b_written", "tie_to_higher_index",
           "fold_order_reads_b")
TINY = [(1, 64), (15, 64), (17, 128), (33, 2 * KW + 64)]                         # the last: an uneven K split (256, 256, 64, 0)
BATCHES = (1, 2, 15, 16, 17, 31, 32)


def gen(seed, dev="cpu"):
    return torch.Generator(device=dev).manual_seed(seed)


def kmap(m, w8):
    """The 32 k (inside a wave's 256) of MFMA m, as [4 lane groups, 8 elements]."""
    g, j = torch.arange(4)[:, None], torch.arange(8)[None, :]
    return 64 * (m // 2) + 16 * g + 8 * (m % 2) + j if w8 else 32 * m + 8 * g + j


def w_values(p):
    """W as fp64 values, without the scale."""
    return G.e4m3fn_table(p.W.device)[p.W.long()] if p.w8 else p.W.double()


def int_codes(dev="cpu"):
    """uint8 [17]: entry v + 8 is the e4m3fn byte code of the integer v in [-8, 8]."""
    t = G.e4m3fn_table()
    return torch.tensor([next(c for c in range(256) if float(t[c]) == float(v) and not (v == 0 and c != 0)) for v in range(-8, 9)],
                        dtype=torch.uint8, device=dev)


# ---- problems -------------------------------------------------------------------------------------------------------------------------------
def problem(W, X, w8=False, wscale=None, bias=None, resid=None, pad=0):
    """One call: W [N, K] (bf16, or uint8 e4m3fn codes with `wscale`), X [32, K] bf16 (a call of B rows reads the first B).  `pad` extra
    columns go behind every row of X, resid and Y (strided calls)."""
    N, K = W.shape
    return NS(W=W, X=X, w8=w8, wscale=wscale, bias=bias, resid=resid, N=N, K=K, pad=pad)


def reference64(p, B):
    """fp64: (sum_k W[n, k] X[b, k]) * scale + bias, [B, N]; and S = sum |w x| * scale."""
    wv, x = w_values(p), p.X[:B].double()
    sc = p.wscale.double()[None, :] if p.w8 else 1.0
    lin = x @ wv.t() * sc + (p.bias.double()[None, :] if p.bias is not None else 0.0)
    return lin, x.abs() @ wv.abs().t() * sc


def expected_exact(p, B):
    """The output of a probe whose sums are exact in fp32 (integers below 2^24; a power-of-two or a single scale product): bf16 [B, N]."""
    lin, _ = reference64(p, B)
    v = lin.float()
    if p.resid is not None:
        return (v.to(BF16).float() + p.resid[:B, :p.N].float()).to(BF16)
    return v.to(BF16)


def integer_case(N, K, w8, seed=0, resid=True, dev="cpu"):
    """X in [-4, 4], W in [-8, 8] (fp8: the codes of those integers, a power-of-two scale per channel), integer bias and resid: every fp32
    sum is exact in any order, so the output is known bit for bit - and a k map that pairs a weight with another x changes it."""
    g = gen(100 + seed + N + K, dev)
    X = torch.randint(-4, 5, (MAX_B, K), generator=g, device=dev).to(BF16)
    Wi = torch.randint(-8, 9, (N, K), generator=g, device=dev, dtype=torch.int32)
    bias = torch.randint(-16, 17, (N,), generator=g, device=dev).to(BF16)
    rs = torch.randint(-64, 65, (MAX_B, N), generator=g, device=dev).to(BF16) if resid else None
    if w8:
        W = int_codes(dev)[(Wi + 8).long()]
        ws = 2.0 ** torch.randint(-2, 3, (N,), generator=g, device=dev).float()
        return problem(W, X, True, ws, bias, rs)
    return problem(Wi.to(BF16), X, False, None, bias, rs)


def index_case(N, K, k0, w8=False, dev="cpu"):
    """One-hot rows: row b of X is 1 at k = k0 + b, so Y[b, n] = W[n, k0 + b] itself (W[n, k] = a value naming (n, k))."""
    X = torch.zeros(MAX_B, K, device=dev)
    for b in range(MAX_B):
        if k0 + b < K:
            X[b, k0 + b] = 1.0
    n, k = torch.arange(N, device=dev)[:, None], torch.arange(K, device=dev)[None, :]
    if w8:
        W = ((n * 7 + k * 13) % 127).to(torch.uint8) + 128 * ((n + k) % 2).to(torch.uint8)       # finite codes, both signs
        return problem(W, X.to(BF16), True, torch.ones(N, device=dev))
    W = (((n * 31 + k) % 251) - 125).float().to(BF16)                            # integers below 256: exact in bf16
    return problem(W, X.to(BF16))


def codes_case():
    """All 254 finite e4m3fn codes as weights against x = 1: Y[b, n] = the value of code n's byte, rounded to bf16 (it is one)."""
    fin = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)
    W = torch.zeros(fin.numel(), 64, dtype=torch.uint8)
    W[:, 0] = fin
    W[:, 37] = fin.flip(0)
    X = torch.zeros(MAX_B, 64)
    X[0::2, 0] = 1.0
    X[1::2, 37] = 1.0
    return problem(W, X.to(BF16), True, torch.ones(fin.numel()))


def scale_case(N=33, K=2 * KW + 64, seed=0):
    """The scale once: wave 0's k hold a sum S0 near 2^22, wave 1's hold -S0 + 1 (exact integers), the scale is a full 24-bit fp32.
    Once: bf16(fl(1 * scale)) = bf16(scale).  Per partial sum, fl(S0 scale) + fl((1 - S0) scale) is a multiple of ulp(S0 scale): off by
    up to half of the result."""
    assert K >= 2 * KW
    g = gen(300 + seed)
    X = torch.zeros(MAX_B, K)
    X[:, :KW] = 128.0
    X[:, KW:2 * KW] = 128.0
    codes = G.e4m3fn_table()
    big = [c for c in range(128) if float(codes[c]) in (96.0, 112.0, 128.0, 160.0)]
    W = torch.zeros(N, K, dtype=torch.uint8)
    W[:, :KW] = torch.tensor(big)[torch.randint(0, len(big), (N, KW), generator=g)].to(torch.uint8)
    W[:, KW:2 * KW] = W[:, :KW] | 0x80                                           # the negatives: S1 = -S0 ...
    one = int(next(c for c in range(128) if float(codes[c]) == 1.0))
    W[:, KW] = one                                                               # ... + (1 + w[0]) * 128: replace -w[0] by +1
    X[:, KW] = 1.0                                                               # x = 1 there: S1 = -S0 + 128 w[0] + 1
    X[:, 0] = 0.0                                                                # and drop w[0] from S0
    ws = (1.0 + torch.rand(N, generator=g)).float() * 2.0 ** -7
    return problem(W, X.to(BF16), True, ws)


def bound_case(N, K, family, w8, seed=0, dev="cpu"):
    """The `randn` / `cancel` operands of gemm_model.bound_case with a bf16 bias (no residual: the bound is on the sum)."""
    g = gen(400 + seed + G.FAMILIES.index(family), dev)
    rn = lambda *shape: torch.randn(*shape, generator=g, device=dev)
    if family == "randn":
        A, Wf = rn(MAX_B, K) * G.SIGMA, rn(N, K) * G.SIGMA
    else:
        A = (rn(MAX_B, K // 2) * 4).repeat_interleave(2, dim=1)
        y = rn(N, K // 2) * 4
        Wf = torch.stack([y, -y * (1 + rn(N, K // 2) * 2.0 ** -8)], dim=2).reshape(N, K)
    bias = rn(N).to(BF16)
    if w8:
        s = Wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0
        return problem((Wf / s[:, None]).to(FP8).view(torch.uint8), A.to(BF16), True, s.float(), bias)
    return problem(Wf.to(BF16), A.to(BF16), False, None, bias)


def bound_ratio(p, B, got):
    """worst |out - ref64| / (2^-8 |ref64| + K 2^-23 S + 1e-30): the bound of the bf16 GEMM probes."""
    lin, S = reference64(p, B)
    return float(((got[:B, :p.N].double() - lin).abs() / (2.0 ** -8 * lin.abs() + p.K * 2.0 ** -23 * S + 1e-30)).max())


def frames(p, B):
    """(X, resid / Y buffer) of a strided call: `pad` columns behind every row and rows up to MAX_B + 1, all holding the sentinel where the
    call may not write.  Y aliases resid when the problem has one."""
    ldy = p.N + p.pad
    Y = torch.full((MAX_B + 1, ldy), SENT, device=p.X.device).to(BF16)
    if p.resid is not None:
        Y[:B, :p.N] = p.resid[:B, :p.N]
    return Y


def frame_intact(p, B, Y):
    want = torch.full_like(Y, SENT)
    want[:B, :p.N] = Y[:B, :p.N]
    return torch.equal(Y.view(torch.int16), want.view(torch.int16))


# ---- the kernel, restated ---------------------------------------------------------------------------------------------------------------------
def partial_sums(p, B, mutant=None):
    """fp32 [4 waves, 16 TM, N]: what each wave's accumulators hold after the K loop.  An MFMA adds the 32 products of its k to the fp32
    accumulator (modelled as one fp64 dot product rounded once: the probes with exact sums do not depend on that)."""
    rows = 16 if B <= 16 else 32
    x = torch.zeros(rows, p.K, dtype=torch.float64)
    x[:B] = p.X[:B].double()                                                     # rows >= B of the tile are zero
    wv = w_values(p)
    acc = torch.zeros(NWAVE, rows, p.N, dtype=torch.float32)
    for kb in range(0, p.K, KC):
        for w in range(NWAVE):
            kw = kb + w * KW
            for m in range(KW // 32):
                if kw + 32 * m >= p.K:
                    continue
                kk = kw + kmap(m, p.w8)                                          # [4, 8]
                kx = kk[[1, 0, 3, 2]] if mutant == "k_halves_swapped" else kk    # X read with adjacent 16-byte vectors swapped
                acc[w] = (acc[w].double() + x[:, kx.flatten()] @ wv[:, kk.flatten()].t()).float()
    return acc


def fold(acc, B, mutant=None):
    order = (3, 2, 1, 0) if mutant == "fold_order_reads_b" and B > 16 else (0, 1, 2, 3)
    s = acc[order[0]].clone()
    for w in order[1:]:
        s = s + acc[w]
    return s


def emulate(p, B, Y, mutant=None):
    """The call on the frame Y (resid is read from it when the problem has one: Y aliases resid); returns Y."""
    acc = partial_sums(p, B, mutant)
    bias = p.bias.float()[None, :] if p.bias is not None else torch.zeros(1, p.N)
    if p.w8 and mutant == "scale_per_partial":
        s = fold(acc * p.wscale[None, None, :], B, mutant)
        v = s + bias
    else:
        s = fold(acc, B, mutant)
        v = (s.double() * p.wscale.double()[None, :] + bias.double()).float() if p.w8 else s + bias     # fma: one rounding
    rows = s.shape[0] if mutant == "row_b_written" else B
    cols = min(p.N + 1, Y.shape[1]) if mutant == "tail_writes_column_n" else p.N
    vv = torch.ones(rows, cols)                                                  # a column past N (a mutant's) gets a value of its own
    vv[:, :p.N] = v[:rows]
    if p.resid is not None:
        r = Y[:rows, :cols].float()
        out = (vv + r).to(BF16) if mutant == "resid_before_rounding" else (vv.to(BF16).float() + r).to(BF16)
    else:
        out = vv.to(BF16)
    Y[:rows, :cols] = out
    return Y


def head_case(V, K, B=MAX_B, seed=0, dev="cpu"):
    """Integer lm_head probe: X in [-4, 4], W in [-2, 2], every logit exact; `plant` puts a row's maximum at chosen indices."""
    g = gen(500 + seed + V, dev)
    X = torch.randint(-4, 5, (MAX_B, K), generator=g, device=dev)
    X[:, 0] = 4                                                                  # no zero row
    W = torch.randint(-2, 3, (V, K), generator=g, device=dev)
    return problem(W.to(BF16), X.to(BF16))


def plant(p, b, rows):
    """Make the weight rows `rows` equal 8 sign(x_b): the logit of row b there is 8 sum |x_b|, above every other logit of row b (|w| <= 2
    elsewhere), and the same value at each planted index."""
    sgn = torch.sign(p.X[b].float())
    for n in rows:
        p.W[n] = (8 * sgn).to(BF16)


def emulate_head(p, B, mutant=None):
    """(tokens [B] int64, fp32 logits [B, V])."""
    z = fold(partial_sums(p, B, mutant), B, mutant)[:B]
    hi = mutant == "tie_to_higher_index"
    tok = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        parts = []
        for n0 in range(0, p.N, TILE):                                           # a block: ascending, strict >
            best, at = z[b, n0], n0
            for n in range(n0 + 1, min(n0 + TILE, p.N)):
                if z[b, n] > best or (hi and z[b, n] == best):
                    best, at = z[b, n], n
            parts.append((best, at))
        best, at = parts[0]
        for v, i in parts[1:]:                                                   # the finalize: the lowest index among equal values
            if v > best or (hi and v == best):
                best, at = v, i
        tok[b] = at
    return tok, z


def head_expected(p, B):
    """Exact integer logits and the first maximum."""
    lin, _ = reference64(p, B)
    return torch.argmax(lin, dim=1), lin.float()                                 # torch.argmax returns the first maximal index


def head_bound(p, B):
    """K 2^-23 S + 2^-24 |ref64| per logit."""
    lin, S = reference64(p, B)
    return lin, p.K * 2.0 ** -23 * S + 2.0 ** -24 * lin.abs()


# ---- the probes: each takes `run(p, B, Y) -> Y` (the entry on a frame) or `run_head(p, B) -> (tokens, logits)` and returns True when met ------
def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def with_pad(p):
    p.pad = 8 - p.N % 8                                                          # ldy = N + pad: a multiple of 8, at least one column behind N
    return p


def check_integer(run, N, K, w8, B, resid=True, dev="cpu"):
    """Integer probe in a sentinel frame, Y aliasing resid: exact bits inside, the frame (rows >= B, columns >= N) intact."""
    p = with_pad(integer_case(N, K, w8, resid=resid, dev=dev))
    Y = run(p, B, frames(p, B))
    return same_bits(Y[:B, :N], expected_exact(p, B)) and frame_intact(p, B, Y)


def check_index(run, N, K, w8, k0s=None, dev="cpu"):
    """One-hot rows return W[n, k] itself for every k: 32 k per call."""
    for k0 in (range(0, K, MAX_B) if k0s is None else k0s):
        p = with_pad(index_case(N, K, k0, w8, dev))
        Y = run(p, MAX_B, frames(p, MAX_B))
        if not (same_bits(Y[:MAX_B, :N], expected_exact(p, MAX_B)) and frame_intact(p, MAX_B, Y)):
            return False
    return True


def check_codes(run):
    p = with_pad(codes_case())
    Y = run(p, MAX_B, frames(p, MAX_B))
    return same_bits(Y[:MAX_B, :p.N], expected_exact(p, MAX_B))


def check_scale(run, B=17):
    p = with_pad(scale_case())
    Y = run(p, B, frames(p, B))
    return same_bits(Y[:B, :p.N], expected_exact(p, B))


HOSTILE = (float("nan"), float("inf"), float("-inf"), 3e38)


def invariance_case(N, K, w8, seed=0, dev="cpu"):
    """Random operands on which the fold order shows in the bf16 output: where K reaches a third wave (K >= 2 KW + 64) the k of wave 1
    mirror those of wave 0 with the opposite sign at magnitude ~2^22, so the first two partial sums cancel exactly and the result is the
    O(10) rest - folded in another order, the rest is rounded to the fp32 grid of 2^22 first (0.5)."""
    g = gen(600 + seed + N + K, dev)
    X = torch.randn(MAX_B, K, generator=g, device=dev)
    big = K >= 2 * KW + 64
    if big:
        X[:, :KW] *= 1024.0
    X = X.to(BF16)
    if big:
        X[:, KW:2 * KW] = X[:, :KW]
    bias = torch.randn(N, generator=g, device=dev).to(BF16)
    if w8:
        sign = (torch.randint(0, 2, (N, K), generator=g, device=dev) * 128).to(torch.uint8)
        W = torch.randint(0x20, 0x38, (N, K), generator=g, device=dev).to(torch.uint8) | sign          # 2^-3 <= |w| < 1
        if big:
            W[:, :KW] = torch.randint(0x70, 0x7f, (N, KW), generator=g, device=dev).to(torch.uint8) | sign[:, :KW]     # 128 <= |w| <= 448
            W[:, KW:2 * KW] = W[:, :KW] ^ 0x80
        return problem(W, X, True, ((1.0 + torch.rand(N, generator=g, device=dev)) * 0.125).float(), bias)
    Wf = torch.randn(N, K, generator=g, device=dev)
    if big:
        Wf[:, :KW] *= 256.0
    W = Wf.to(BF16)
    if big:
        W[:, KW:2 * KW] = -W[:, :KW]
    return problem(W, X, False, None, bias)


def check_invariance(run, N, K, w8, rows=(0, 5, 16, 31), dev="cpu"):
    """Row b of a B = 32 call equals the B = 1 call on row b alone, whatever the other 31 rows hold (NaN, +-inf, 3e38)."""
    base = invariance_case(N, K, w8, dev=dev)
    for b in rows:
        p = with_pad(invariance_case(N, K, w8, dev=dev))
        for i in range(MAX_B):
            if i != b:
                p.X[i] = HOSTILE[i % 4]
        wide = run(p, MAX_B, frames(p, MAX_B))
        one = with_pad(invariance_case(N, K, w8, dev=dev))
        one.X[0] = base.X[b]
        alone = run(one, 1, frames(one, 1))
        if not same_bits(wide[b:b + 1, :N], alone[:1, :N]) or bool(torch.isnan(alone[:1, :N].float()).any()):
            return False
    return True


def check_head_invariance(run_head, V, K, rows=(0, 17, 31), dev="cpu"):
    """The same for lm_head: row b's token and fp32 logits of a B = 32 call are those of the B = 1 call on row b."""
    base = invariance_case(V, K, False, dev=dev)
    base.bias = None
    for b in rows:
        p = invariance_case(V, K, False, dev=dev)
        p.bias = None
        for i in range(MAX_B):
            if i != b:
                p.X[i] = HOSTILE[i % 4]
        tok, z = run_head(p, MAX_B)
        one = invariance_case(V, K, False, dev=dev)
        one.bias = None
        one.X[0] = base.X[b]
        tok1, z1 = run_head(one, 1)
        if not (torch.equal(z[b].cpu().view(torch.int32), z1[0].cpu().view(torch.int32)) and int(tok[b]) == int(tok1[0])):
            return False
    return True


def tie_cases(V):
    """(name, {row: planted indices}) - ties inside one 16-row tile, across blocks, and with another row's maximum in the last partial tile."""
    last = V - 1
    cases = [("inside_a_tile", {0: (3, 9) if V > 9 else (0, V - 1)})]
    if V > 16:
        cases.append(("across_two_blocks", {1: (2, last)}))
    if V > 40:
        cases.append(("across_blocks", {1: (18, 35, last), 30: (last - 1,)}))
        cases.append(("other_rows_maximum_in_the_last_tile", {2: (5, 21), 17: (last,), 31: (last - 17,)}))
    return cases


def check_head_ties(run_head, V, K=64, B=MAX_B, dev="cpu"):
    for name, plants in tie_cases(V):
        p = head_case(V, K, dev=dev)
        plants = {b % B: rows for b, rows in plants.items()}
        for b, rows in plants.items():
            plant(p, b, rows)
        tok, z = run_head(p, B)
        want, zw = head_expected(p, B)
        if not (torch.equal(tok.cpu(), want.cpu()) and torch.equal(z.cpu(), zw.cpu())):
            return False
        for b, rows in plants.items():                                           # the probe is what it says: the lowest planted index wins
            assert int(want[b]) == min(rows), (name, b)
    return True
