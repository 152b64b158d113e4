"""A model of the VAE convolutions (regione_amd/csrc/gemm.hip: rgn_conv_bf16, rgn_conv_s2_bf16, rgn_conv_up2_bf16 on
gemm_bf16_kernel<RGN_EPI_CONV, ...>) and the probes that pin every launch path of the three entries to the mathematics.  Plain torch, CPU
or GPU tensors, no GPU import.

  TABLE        one row per kernel instantiation and feature: image size, channels, pixel group, residual, statistics, the geometry knob
               and the instantiation `dispatch` (a restatement of the entries' rule) must pick;
  *_case       probe inputs whose correct output is known EXACTLY from a closed form that holds no convolution (one-hot taps: a shifted
               image; K-tile signatures: a sum of powers of two; all ones: Cin times the taps inside the image; two-rounding skip on
               halves), and the random / cancelling inputs of the fp64 bound.  A case holds interior images [H, W, C] only;
  expected_* / check_* / bound_ratio   the checks: a count of violating elements (0 = pass) or a ratio (<= 1 = pass);
  emulate      a torch emulation of the scheme - padded pixel-major image with guard rows, the K walk with conv_row_tiles / conv_jump,
               pixel groups, the tile map, an epilogue per tile with mask, then statistics, then store, row tables, four phase problems
               with a running slot index - with the named defects of MUTANTS.  Not a model of any kernel's instruction order.
tests/test_gpu_conv_probes.py applies the checks to the kernels; tests/test_conv_model.py applies the same functions to `emulate`, shows
that each mutant fails at least one of them and that every expectation is bf16-exact.
"""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from gemm_model import BF16, BK, SIG_TILES, _sig_sign, bits, mismatches, sentinel, tile_coords

GUARD = 72                                      # PaddedImage: Wp + 72 guard rows on each side of an image
MUTANTS = ("jump_one_tile_late", "jump_of_wp", "kx_reversed", "origin_off_by_one", "mask_missing_last_column", "mask_missing_last_row",
           "mask_before_skip", "stats_before_mask", "stats_shift_of_wrong_channel_count", "slot_of_neighbour_tile", "up2_slot_base_restarted",
           "group_pixels_swapped", "hanging_row_dropped", "s2_origin_without_offset", "s2_pad_top", "s2_pad_left", "phases_exchanged",
           "up2_border_not_zeroed", "skip_before_rounding", "group_m_tiles_swapped")
# s2_origin_without_offset: A starts at padded pixel (0, 0) instead of (1, 1) - in this scheme that IS "the padding on the top / left"
# (out(yo, xo) = sum in(2 yo + ky - 1, 2 xo + kx - 1)); s2_pad_top / s2_pad_left are the two halves of it.

# ---- the table of launch paths -------------------------------------------------------------------------------------------------------
# gemm_bf16_kernel<RGN_EPI_CONV, BM, BN, WM, WN, MODE_FULL, AV> instantiations the three entries can launch (launch_conv), against the
# rows that are there for them.  use_big = K >= 256 && forced != 128 && (forced == 256 || big >= 100)   (rgn_conv_bf16)
#                                use_big =             forced != 128 && (forced == 256 || big >= 100)   (rgn_conv_s2_bf16: K = 9 Cin >= 576)
#                                use_big = K >= 256 && forced != 128 && (forced == 256 || 4 big >= 100) (rgn_conv_up2_bf16: K = 4 Cin >= 256)
#   <128,128,2,2> AV 0  two-stage loop, stage() jump: !use_big
#        rgn_conv_bf16 3 x 3   a_1x1img a_g1 a_g2 a_rgb a_m33 thr_below
#        rgn_conv_bf16 1 x 1   a_1x1 a_1x1_g2 a_1x1_k128_f256 (K = 128 < 256 under gemm_geometry = 256)
#        rgn_conv_s2_bf16      a_s2_2x2 a_s2 a_s2_tiles
#        rgn_conv_up2_bf16     a_up2_2x2 a_up2 a_up2_tiles up2_thr_below
#   <256,256,2,2> AV 3  hand-scheduled conv ring (RGN_GEMM_LOOP4W_CONV_ASM): use_big, 3 x 3 / stride 2 / phases
#        rgn_conv_bf16 3 x 3   r_c64 (conv_row_tiles 3) r_c128 (6) r_c192 (9, 3/4 N tile, ldy > Cout) r_c512 (24: the ring wraps inside a
#                              kernel row) r_g2 (8) r_g8 (20) r_m33 thr_above
#        rgn_conv_s2_bf16      r_s2_2x2 r_s2
#        rgn_conv_up2_bf16     r_up2_c64 (K = 256, conv_row_tiles 2: the shortest K) r_up2_c64_tiles r_up2_c256 up2_thr_above
#   <256,256,2,2> AV 1  plain ring: use_big, 1 x 1 (conv_row_tiles 0, K >= 256)   p_1x1 p_1x1_g2
# Features: residual on (a_g1 a_g2 r_c64 r_c512 r_g2 p_1x1) and off; gn with 128 (a_g1 a_g2 r_g2 ...), 256 (r_c64 a_m33 r_up2_c256) and
# 512 (r_c128 r_m33 p_1x1) channels per pixel and off; ldy > Cout (a_rgb r_g8: written as 0 by the pixel-group launch; r_c192: untouched).
# Left out: images past 114 x 114 (whole rounds + remainder do not exist for the convolutions: one launch of all tiles, gg.tile_offset = 0).


def _row(name, kind, H, W, cin, cout, geometry, geom, av, group=1, taps=9, ldy=None, resid=False, gn=False, **feat):
    return NS(name=name, kind=kind, H=H, W=W, cin=cin, cout=cout, geometry=geometry, geom=geom, av=av, group=group, taps=taps,
              ldy=ldy or cout, resid=resid, gn=gn, feat=feat)


TABLE = [
    # <128,128,2,2> AV 0
    _row("a_1x1img", "conv", 1, 1, 64, 128, 128, 128, 0, gn=True),                           # Hp = Wp = 3: one interior pixel
    _row("a_g1", "conv", 5, 7, 64, 128, 128, 128, 0, resid=True, gn=True),                   # a single ragged tile
    _row("a_g2", "conv", 9, 11, 128, 128, 128, 128, 0, group=2, resid=True, gn=True),        # Wp = 13, Hp Wp = 143 odd: the last row hangs; two N tiles
    _row("a_rgb", "conv", 13, 10, 128, 3, 128, 128, 0, group=8, ldy=8),                      # Wp = 12, 180 % 8 = 4; N = 64, conv_row_tiles = 20
    _row("a_m33", "conv", 33, 33, 64, 256, 128, 128, 0, gn=True),                            # 10 x 2 tiles: two GROUP_M groups, tiles cut image rows
    _row("a_1x1", "conv", 5, 7, 128, 256, 128, 128, 0, taps=1),
    _row("a_1x1_g2", "conv", 9, 11, 256, 128, 128, 128, 0, taps=1, group=2, gn=True),
    _row("a_1x1_k128_f256", "conv", 17, 20, 128, 128, 256, 128, 0, taps=1, gn=True),         # 418 rows: 4 tiles of 128, not 2 of 256
    _row("a_s2_2x2", "s2", 2, 2, 64, 64, 128, 128, 0),
    _row("a_s2", "s2", 4, 6, 64, 192, 128, 128, 0),
    _row("a_up2_2x2", "up2", 2, 2, 64, 128, 128, 128, 0, gn=True),
    _row("a_up2", "up2", 4, 6, 64, 128, 128, 128, 0, gn=True),
    _row("a_s2_tiles", "s2", 20, 30, 64, 320, 128, 128, 0),                                  # 320 x 320: 3 x 3 ragged tiles
    _row("a_up2_tiles", "up2", 17, 20, 64, 256, 128, 128, 0, gn=True),                       # 418 rows: 4 x 2 tiles per phase, 32 slots
    # <256,256,2,2> AV 3
    _row("r_c64", "conv", 17, 20, 64, 256, 256, 256, 3, resid=True, gn=True),                # 418 rows: the tile boundary cuts image row 11
    _row("r_c128", "conv", 5, 7, 128, 512, 256, 256, 3, gn=True),
    _row("r_c192", "conv", 5, 7, 192, 192, 256, 256, 3, ldy=200),
    _row("r_c512", "conv", 5, 7, 512, 512, 256, 256, 3, resid=True),
    _row("r_g2", "conv", 17, 18, 128, 128, 256, 256, 3, group=2, resid=True, gn=True),       # Wp = 20: guard rows -1 and + 0 reach interior outputs
    _row("r_g8", "conv", 13, 10, 128, 3, 256, 256, 3, group=8, ldy=8),
    _row("r_m33", "conv", 33, 33, 64, 512, 256, 256, 3, gn=True),                            # 5 x 2 tiles: a GROUP_M group of 4 and one of 1
    _row("r_s2_2x2", "s2", 2, 2, 64, 64, 256, 256, 3),
    _row("r_s2", "s2", 20, 30, 64, 320, 256, 256, 3),                                        # 320 rows x 320 columns: 2 x 2 ragged tiles
    _row("r_up2_c64", "up2", 4, 6, 64, 128, 256, 256, 3, gn=True),
    _row("r_up2_c64_tiles", "up2", 17, 20, 64, 512, 256, 256, 3, gn=True),                   # 2 x 2 tiles per phase
    _row("r_up2_c256", "up2", 6, 5, 256, 256, 256, 256, 3, gn=True),
    # <256,256,2,2> AV 1
    _row("p_1x1", "conv", 17, 20, 256, 512, 256, 256, 1, taps=1, resid=True, gn=True),
    _row("p_1x1_g2", "conv", 17, 19, 256, 128, 256, 256, 1, taps=1, group=2, gn=True),
    # geometry left to the library: big = tiles of 256 of the problem
    _row("thr_above", "conv", 112, 112, 64, 512, None, 256, 3, gn=True, huge=True),          # 12996 rows: 51 x 2 = 102 >= 100
    _row("thr_below", "conv", 108, 108, 64, 512, None, 128, 0, gn=True, huge=True),          # 12100 rows: 48 x 2 = 96 -> 95 x 4 = 380 tiles of 128
    _row("up2_thr_above", "up2", 54, 55, 64, 512, None, 256, 3, gn=True, huge=True),         # 3192 rows: 4 x 13 x 2 = 104
    _row("up2_thr_below", "up2", 53, 53, 64, 512, None, 128, 0, gn=True, huge=True),         # 3025 rows: 4 x 24 = 96 -> 4 x 24 x 4 = 384 tiles of 128
]
TABLE_BY_NAME = {r.name: r for r in TABLE}
SMALL_ROWS = [r.name for r in TABLE if not r.feat.get("huge")]
HUGE_ROWS = [r.name for r in TABLE if r.feat.get("huge")]
RESID_ROWS = [r.name for r in TABLE if r.resid]
GN_ROWS = [r.name for r in TABLE if r.gn and not r.feat.get("huge")]
GROUP_ROWS = [r.name for r in TABLE if r.group > 1 and r.taps == 9]


def geo(row):
    """The GEMM the entry builds from the row (elements, not bytes; `origin` relative to row 0 of the padded input image)."""
    g = NS(Hp=row.H + 2, Wp=row.W + 2, group=row.group, ldy=row.ldy, cin=row.cin)
    g.rows = g.Hp * g.Wp
    if row.kind == "conv":
        g.Ho, g.Wo, g.nprob, g.mask, g.table = row.H, row.W, 1, True, False
        g.M = (g.rows + row.group - 1) // row.group
        g.win = row.group + 2 if row.taps == 9 else row.group
        g.K = (3 if row.taps == 9 else 1) * g.win * row.cin
        g.N = row.group * row.ldy if row.group > 1 else row.cout
        g.lda, g.ldc = row.group * row.cin, row.group * row.ldy
        g.origin = [-(g.Wp + 1) * row.cin if row.taps == 9 else 0]
        g.crt = g.win * row.cin // BK if row.taps == 9 else 0
        g.jump = (g.Wp - g.win) * row.cin
        g.cpp = row.ldy if row.group > 1 else 1 << 30
        g.gn_c = row.ldy if row.group > 1 else row.cout
    elif row.kind == "s2":
        g.Ho, g.Wo, g.nprob, g.mask, g.table = row.H // 2, row.W // 2, 1, False, True
        g.M, g.win, g.K, g.N = g.Ho * g.Wp, 3, 9 * row.cin, row.cout
        g.lda, g.ldc, g.origin = 2 * row.cin, row.ldy, [(g.Wp + 1) * row.cin]
        g.crt, g.jump, g.cpp, g.gn_c = 3 * row.cin // BK, (g.Wp - 3) * row.cin, 1 << 30, row.cout
    else:
        g.Ho, g.Wo, g.nprob, g.mask, g.table = 2 * row.H, 2 * row.W, 4, True, True
        g.M, g.win, g.K, g.N = g.rows, 2, 4 * row.cin, row.cout
        g.lda, g.ldc = row.cin, row.ldy
        g.origin = [((a - 1) * g.Wp + (b - 1)) * row.cin for a in range(2) for b in range(2)]
        g.crt, g.jump, g.cpp, g.gn_c = 2 * row.cin // BK, (g.Wp - 2) * row.cin, 1 << 30, row.cout
    g.Hq, g.Wq = g.Ho + 2, g.Wo + 2                       # the padded output image
    g.rows_out = g.Hq * g.Wq
    g.gin, g.gout = g.Wp + GUARD, g.Wq + GUARD           # guard rows of the input / output storage
    return g


def _tiles(M, N, b):
    return ((M + b - 1) // b) * ((N + b - 1) // b)


def dispatch(row):
    """(geometry, AV, tiles per problem, problems): the rule of the three entries restated."""
    g = geo(row)
    big, small, forced = _tiles(g.M, g.N, 256), _tiles(g.M, g.N, 128), row.geometry or 0
    enough = (4 * big if row.kind == "up2" else big) >= 100
    use_big = (row.kind == "s2" or g.K >= 4 * BK) and forced != 128 and (forced == 256 or enough)
    av = 0 if not use_big else (1 if row.kind == "conv" and row.taps == 1 else 3)
    return (256 if use_big else 128), av, (big if use_big else small), g.nprob


def nblk(row):
    _, _, per, nprob = dispatch(row)
    return per * nprob


def row_table(row, dev="cpu"):
    """The row tables restated: [nprob][M] rows of the padded output image, the first row behind it (`scratch`) for what is no output."""
    g = geo(row)
    m = torch.arange(g.M, device=dev)
    py, px = m // g.Wp, m % g.Wp
    scratch = g.rows_out
    if row.kind == "s2":
        return torch.where(px < g.Wo, (py + 1) * g.Wq + px + 1, torch.full_like(m, scratch))[None]
    ok = (py >= 1) & (py <= row.H) & (px >= 1) & (px <= row.W)
    return torch.stack([torch.where(ok, (2 * (py - 1) + a + 1) * g.Wq + 2 * (px - 1) + b + 1, torch.full_like(m, scratch))
                        for a in range(2) for b in range(2)])


def toeplitz(row, w4, bias):
    """(W [N, K], bias [N]) as rgn_conv_bf16 wants them (ConvWeights restated): group = 1 the matrix [Cout, taps Cin]; group > 1 row
    p ldy + c holds w4[c, ky, kx] at window pixel p + kx of kernel row ky."""
    co, kh, kw, ci = w4.shape
    if row.group == 1:
        return w4.reshape(co, -1).to(BF16), bias.to(BF16)
    win = row.group + 2 if kh == 3 else row.group
    t = torch.zeros((row.group, row.ldy, kh, win, ci), dtype=torch.float32, device=w4.device)
    b = torch.zeros((row.group, row.ldy), dtype=torch.float32, device=w4.device)
    for p in range(row.group):
        for kx in range(kw):
            t[p, :co, :, p + kx, :] = w4[:, :, kx, :].float()
    b[:, :co] = bias.float()
    return t.reshape(row.group * row.ldy, -1).to(BF16), b.reshape(-1).to(BF16)


FOLD = ([[0], [1, 2]], [[0, 1], [2]])           # phase 0: window rows (y - 1, y) <- taps (0), (1, 2); phase 1: (y, y + 1) <- (0, 1), (2)


def phase_fold(w4, dtype=torch.float64):
    """[4][Cout, 2, 2, Cin]: the taps a low-resolution pixel is seen through, summed in `dtype` (UpConvWeights restated; fp64 = exact)."""
    co, _, _, ci = w4.shape
    out = []
    for a in range(2):
        for b in range(2):
            t = torch.zeros((co, 2, 2, ci), dtype=dtype, device=w4.device)
            for r in range(2):
                for c in range(2):
                    for ky in FOLD[a][r]:
                        for kx in FOLD[b][c]:
                            t[:, r, c, :] += w4[:, ky, kx, :].to(dtype)
            out.append(t)
    return torch.stack(out)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _gen(row, salt):
    return torch.Generator().manual_seed(1000 * salt + 7 * len(row.name) + row.cin + row.H)


def _case(row, kind, dev, x, w4, bias, resid=None, img=None, lin=None, S=None, exact_stats=False):
    g = geo(row)
    c = NS(kind=kind, x=x.to(dev).to(BF16), w4=w4.to(dev).to(BF16).float(), bias=bias.to(dev).to(BF16).float(),
           resid=None if resid is None else resid.to(dev).to(BF16), img=img, lin=lin, S=S, exact_stats=exact_stats)
    assert c.x.shape == (row.H, row.W, row.cin) and c.w4.shape[0] == row.cout and (c.resid is None or c.resid.shape == (g.Ho, g.Wo, row.cout))
    return c


def perm(row, dev="cpu"):
    """The input channel output channel co selects: a fixed non-trivial map (odd stride: a bijection when Cout = Cin)."""
    return (5 * torch.arange(row.cout, device=dev) + 3) % row.cin


def taps_of(row):
    return [(1, 1)] if row.taps == 1 else [(ky, kx) for ky in range(3) for kx in range(3)]


def _finite_bf16(shape, gen):
    """Arbitrary finite bf16 values: every exponent, both signs, subnormals; no zero (a product -0 would hide behind +0)."""
    b = torch.randint(1, 0x7f80, shape, generator=gen, dtype=torch.int32)                  # magnitude bits below infinity
    b = torch.where(torch.rand(shape, generator=gen) < 0.05, b & 0x7f, b)                  # a share of subnormals
    b = torch.where(b == 0, torch.ones_like(b), b) | (torch.randint(0, 2, shape, generator=gen, dtype=torch.int32) << 15)
    return b.to(torch.int16).view(BF16)


def _source(row, x):
    """The image the 3 x 3 window of an output pixel walks, and its stride: x itself, x with the bottom / right padding, or nearest 2 x."""
    if row.kind == "up2":
        return x.repeat_interleave(2, 0).repeat_interleave(2, 1), 1
    return x, (2 if row.kind == "s2" else 1)


def _shifted(row, x, ky, kx):
    """out(y, x) = src(s y + ky - o, s x + kx - o), zero outside src; o = 1 (padding 1) or 0 (stride 2: F.pad (0, 1, 0, 1))."""
    g = geo(row)
    src, s = _source(row, x)
    o = 0 if row.kind == "s2" else 1
    big = torch.zeros((src.shape[0] + 4, src.shape[1] + 4, src.shape[2]), dtype=src.dtype, device=src.device)
    big[2:2 + src.shape[0], 2:2 + src.shape[1]] = src
    ys = s * torch.arange(g.Ho, device=x.device) + ky - o + 2
    xs = s * torch.arange(g.Wo, device=x.device) + kx - o + 2
    return big[ys][:, xs]


def _inside(row, ky, kx, dev):
    """[Ho, Wo] 1.0 where tap (ky, kx) of the output pixel lies inside the source image."""
    one = torch.ones((row.H, row.W, 1), dtype=torch.float64, device=dev)
    return _shifted(row, one, ky, kx)[..., 0]


def shift_case(row, tap, dev="cpu", ints=False):
    """a. one-hot weights w[co, ky, kx, perm(co)] = 1 for a single tap: the output is the input shifted by (ky - 1, kx - 1) with zero fill,
    channel-mapped, bit for bit.  ints: small integers in x, bias and the skip - every stored value and every tile's sum and sum of squares
    is then exact in fp32 (d)."""
    gen, g = _gen(row, 1 + 3 * tap[0] + tap[1]), geo(row)
    k = 1 if row.taps == 1 else 3
    w4 = torch.zeros(row.cout, k, k, row.cin)
    w4[torch.arange(row.cout), tap[0] if k == 3 else 0, tap[1] if k == 3 else 0, perm(row)] = 1
    resid = None
    if ints:
        x = torch.randint(-4, 5, (row.H, row.W, row.cin), generator=gen).float()
        bias = ((3 * torch.arange(row.cout)) % 5 - 2).float()
        if row.resid:
            resid = torch.randint(-3, 4, (g.Ho, g.Wo, row.cout), generator=gen).float()
    else:
        x, bias = _finite_bf16((row.H, row.W, row.cin), gen), torch.zeros(row.cout)
    c = _case(row, "shift", dev, x, w4, bias, resid, exact_stats=ints)
    img = _shifted(row, c.x, *tap)[..., perm(row, dev)]
    if ints:
        c.lin = img.double() + c.bias.double() + (0 if resid is None else c.resid.double())
        img = (img.float() + c.bias).to(BF16)
        if resid is not None:
            img = (c.resid.float() + img.float()).to(BF16)
    c.img = img
    return c


def signature_passes(row):
    nhs = (len(taps_of(row)) * row.cin) // 32
    return (nhs + 2 * SIG_TILES - 1) // (2 * SIG_TILES)


def signature_case(row, ps, dev="cpu"):
    """b. The signature of gemm_model.py on the (ky, kx, ci) axis: half step hs = ((3 ky + kx) Cin + ci) / 32 of the window [8 ps, 8 ps + 8)
    holds sign(co, hs) 2^(hs - 8 ps) in every weight, each pixel a single 1 per 32 channels: out = the sum of the signed powers of two of
    the window's taps that lie inside the image - an integer below 256 in every order of summation.  The passes cover every K tile, the
    tiles on both sides of every kernel-row jump and of the ring wrap among them.  No bias."""
    taps = taps_of(row)
    k = 1 if row.taps == 1 else 3
    pix = torch.arange(row.H * row.W).reshape(row.H, row.W, 1)
    x = ((torch.arange(row.cin)[None, None, :] % 32) == (11 * pix + 7) % 32).float()
    co = torch.arange(row.cout)[:, None]
    w4 = torch.zeros(row.cout, k, k, row.cin)
    lin = torch.zeros(geo(row).Ho, geo(row).Wo, row.cout, dtype=torch.float64)
    for ti, (ky, kx) in enumerate(taps):
        hs = (ti * row.cin + torch.arange(row.cin)[None, :]) // 32                       # [1, Cin]
        j = hs - 2 * SIG_TILES * ps
        on = (j >= 0) & (j < 2 * SIG_TILES)
        wt = torch.where(on, _sig_sign(co, hs, 0).double() * 2.0 ** j.clamp(0, 7), torch.zeros(1, dtype=torch.float64))
        w4[:, ky if k == 3 else 0, kx if k == 3 else 0, :] = wt.float()
        lin += _inside(row, ky, kx, "cpu")[:, :, None] * wt[:, ::32].sum(1)[None, None, :]
    c = _case(row, "signature", dev, x, w4, torch.zeros(row.cout))
    c.img = lin.to(dev).to(BF16)
    c.lin = lin.to(dev)
    return c


def count_case(row, dev="cpu", with_bias=False):
    """b. image = 1 on the interior, weights = 1: out = Cin x the taps inside the image (9, 6 or 4 of them; 1 x 1: one), plus an integer
    bias j Cin, j = 0 ... 2: (taps + j) Cin has at most four significant bits - a bf16 for every Cin."""
    k = 1 if row.taps == 1 else 3
    n = sum(_inside(row, ky, kx, "cpu") for ky, kx in taps_of(row))
    bias = (torch.arange(row.cout) % 3).float() * row.cin if with_bias else torch.zeros(row.cout)
    lin = row.cin * n[:, :, None] + bias.double()[None, None, :]
    c = _case(row, "count", dev, torch.ones(row.H, row.W, row.cin), torch.ones(row.cout, k, k, row.cin), bias)
    c.img, c.lin = lin.to(dev).to(BF16), lin.to(dev)
    return c


def epilogue_case(row, dev="cpu"):
    """c. the ResNet skip bf16(f32(resid) + f32(bf16(acc + bias))) on pre-activations that are no bf16: the centre tap selects an even
    integer in [256, 512) (ulp 2), the bias adds +-1, +-3 or a half, the skip an integer or a half - rounding once (the sum of all three)
    and rounding twice differ on a good share of the elements (test_conv_model.py counts them)."""
    assert row.resid
    gen, g = _gen(row, 40), geo(row)
    x = (256 + 2 * torch.randint(0, 128, (row.H, row.W, row.cin), generator=gen)).float()
    bias = torch.tensor([1.0, -1.0, 3.0, 0.5, -3.0, 1.5])[torch.arange(row.cout) % 6]
    resid = torch.tensor([1.0, 0.5, -0.5, 2.0, 1.5, -1.0, 3.0])[torch.randint(0, 7, (g.Ho, g.Wo, row.cout), generator=gen)]
    k = 1 if row.taps == 1 else 3
    w4 = torch.zeros(row.cout, k, k, row.cin)
    w4[torch.arange(row.cout), k // 2, k // 2, perm(row)] = 1
    c = _case(row, "epilogue", dev, x, w4, bias, resid)
    pre = _shifted(row, c.x, 1, 1)[..., perm(row, dev)].float() + c.bias                     # exact in fp32
    c.img = (c.resid.float() + pre.to(BF16).float()).to(BF16)
    c.once = (c.resid.float() + pre).to(BF16)                                                # what a single rounding would store
    return c


FAMILIES = ("randn", "cancel")


def ref64(row, x, w4, bias, wph=None):
    """conv2d in float64 of the interior image [H, W, Cin] -> [Ho, Wo, Cout].  up2: the four 2 x 2 phase convolutions with the phase
    weights `wph` [4][Cout, 2, 2, Cin] as stored."""
    xi = x.double().permute(2, 0, 1)[None]
    if row.kind == "up2":
        g = geo(row)
        out = torch.zeros(g.Ho, g.Wo, row.cout, dtype=torch.float64, device=x.device)
        xp = F.pad(xi, (1, 1, 1, 1))
        for ph in range(4):
            a, b = ph >> 1, ph & 1
            y = F.conv2d(xp[:, :, a:a + row.H + 1, b:b + row.W + 1], wph[ph].double().permute(0, 3, 1, 2))
            out[a::2, b::2] = y[0].permute(1, 2, 0)
        return out + bias.double()
    w = w4.double().permute(0, 3, 1, 2)
    if row.kind == "s2":
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), w, stride=2)
    else:
        y = F.conv2d(xi, w, padding=w.shape[-1] // 2)
    return y[0].permute(1, 2, 0) + bias.double()


def bound_case(row, family, dev="cpu"):
    """e. N(0, 1) operands, or `cancel`: products of magnitude ~16 in adjacent channel pairs of opposite sign whose sum is ~2^-8 of them."""
    gen, g = _gen(row, 50 + FAMILIES.index(family)), geo(row)
    k = 1 if row.taps == 1 else 3
    if family == "randn":
        x, w4 = torch.randn(row.H, row.W, row.cin, generator=gen), torch.randn(row.cout, k, k, row.cin, generator=gen)
    else:
        x = (torch.randn(row.H, row.W, row.cin // 2, generator=gen) * 4).repeat_interleave(2, dim=2)
        y = torch.randn(row.cout, k, k, row.cin // 2, generator=gen) * 4
        w4 = torch.stack([y, -y * (1 + torch.randn(y.shape, generator=gen) * 2.0 ** -8)], dim=4).reshape(row.cout, k, k, row.cin)
    bias = torch.randn(row.cout, generator=gen)
    resid = torch.randn(g.Ho, g.Wo, row.cout, generator=gen) * 4 if row.resid else None
    c = _case(row, "bound_" + family, "cpu", x, w4, bias, resid)                             # the float64 reference runs on the CPU
    c.wph = phase_fold(c.w4, torch.float32).to(BF16) if row.kind == "up2" else None          # as UpConvWeights stores them
    c.lin = ref64(row, c.x, c.w4, c.bias, c.wph)
    c.S = ref64(row, c.x.abs(), c.w4.abs(), torch.zeros_like(c.bias), None if c.wph is None else c.wph.abs())
    for k, v in list(c.__dict__.items()):
        if torch.is_tensor(v):
            setattr(c, k, v.to(dev))
    return c


# ---- expected outputs and checks -------------------------------------------------------------------------------------------------------
def gemm_view(row, img):
    """The stored image [Ho, Wo, Cout] as the launch's problems see it: per problem (E [M, N] bf16, care [M] bool) - E the value of every
    GEMM row after mask (zeros on the border, on the pixels a group hangs past the image and in the padding channels of a group), care =
    the row is an output (stride 2: the unused columns of the wide grid are not)."""
    g, dev = geo(row), img.device
    if row.kind == "conv":
        pad = torch.zeros(g.M * row.group, g.N // row.group if row.group > 1 else row.cout, dtype=BF16, device=dev)
        v = pad[:g.rows].view(g.Hp, g.Wp, -1)
        v[1:-1, 1:-1, :row.cout] = img
        return [(pad.view(g.M, g.N), torch.ones(g.M, dtype=torch.bool, device=dev))]
    m = torch.arange(g.M, device=dev)
    py, px = m // g.Wp, m % g.Wp
    if row.kind == "s2":
        care = px < g.Wo
        E = torch.zeros(g.M, g.N, dtype=BF16, device=dev)
        E[care] = img[py[care], px[care]]
        return [(E, care)]
    ok = (py >= 1) & (py <= row.H) & (px >= 1) & (px <= row.W)
    out = []
    for ph in range(4):
        E = torch.zeros(g.M, g.N, dtype=BF16, device=dev)
        E[ok] = img[2 * (py[ok] - 1) + (ph >> 1), 2 * (px[ok] - 1) + (ph & 1)]
        out.append((E, torch.ones_like(ok)))
    return out


def new_output(row, dev="cpu"):
    """The output storage [gout + rows_out + gout, ldy], prefilled with the sentinel."""
    g = geo(row)
    return sentinel((g.rows_out + 2 * g.gout, row.ldy), dev)


def expected_storage(row, img):
    """(Y, care): every bit of the output storage a correct launch leaves, and the rows it is defined on (all but the stride-2 scratch
    row).  identity launches: rows [0, M group) x columns [0, N) of each GEMM row; table launches: the rows the table names."""
    g, dev = geo(row), img.device
    Y = new_output(row, dev)
    care = torch.ones(Y.shape[0], dtype=torch.bool, device=dev)
    views = gemm_view(row, img)
    if not g.table:
        E = views[0][0]
        Y[g.gout:].reshape(-1)[:g.M * g.ldc].view(g.M, g.ldc)[:, :g.N] = E
    else:
        tab = row_table(row, dev)
        for ph, (E, ok) in enumerate(views):
            Y[g.gout + tab[ph][ok], :g.N] = E[ok]
        if row.kind == "up2":
            Y[g.gout + g.rows_out, :g.N] = 0                 # border pixels: zeroed, then stored to the scratch row
        else:
            care[g.gout + g.rows_out] = False
    return Y, care


def check_store(row, case, res):
    """Every bit of the output storage: the image, the border, the sentinel around it.  -> violating elements."""
    want, care = expected_storage(row, case.img)
    return int((bits(res.Y) != bits(want))[care].sum())


def expected_partials(row, img):
    """[nblk, 64] fp32: per tile of the tile map (GROUP_M 8 / 4) [32 groups][sum, sum of squares] of the stored values, in fp64 from the
    expected image, the four problems of up2 in consecutive slot ranges."""
    g, dev = geo(row), img.device
    geom, _, per, nprob = dispatch(row)
    shift = {128: 2, 256: 3, 512: 4}[g.gn_c]
    out = torch.zeros(per * nprob, 64, dtype=torch.float64, device=dev)
    grp = (torch.arange(g.N, device=dev) & (g.gn_c - 1)) >> shift
    for ph, (E, _) in enumerate(gemm_view(row, img)):
        for t in range(per):
            tm, tn = tile_coords(t, g.M, g.N, geom)
            v = E[tm * geom:(tm + 1) * geom, tn * geom:(tn + 1) * geom].double()
            gi = grp[tn * geom:(tn + 1) * geom]
            out[ph * per + t, 0::2].index_add_(0, gi, v.sum(0))
            out[ph * per + t, 1::2].index_add_(0, gi, (v * v).sum(0))
    assert float(out.abs().max()) < 2 ** 24                  # exact in fp32 in every order
    return out.float()


def check_partials(row, case, res):
    """d. the tile count, every slot bit for bit, the sentinel behind the last slot, the image's totals.  -> violating elements."""
    assert case.exact_stats
    want = expected_partials(row, case.img)
    n = want.shape[0]
    bad = int(res.nblk != n)
    ws = res.ws.view(-1)
    got = ws[:n * 64].view(n, 64)
    bad += int((got.view(torch.int32) != want.view(torch.int32)).sum()) if ws.numel() >= n * 64 else 1
    bad += int((ws[n * 64:].view(torch.int32) != WS_SENT).sum())
    tot = case.img.double().reshape(-1, row.cout)
    ch = torch.arange(row.cout, device=tot.device) >> {128: 2, 256: 3, 512: 4}[geo(row).gn_c]
    tw = torch.zeros(32, 2, dtype=torch.float64, device=tot.device)
    tw[:, 0].index_add_(0, ch, tot.sum(0))
    tw[:, 1].index_add_(0, ch, (tot * tot).sum(0))
    bad += int((got.double().sum(0).view(32, 2) != tw).sum())
    return bad


WS_SENT = 0x7f812345                            # fp32 bit pattern the partial workspace is prefilled with (a NaN no sum produces)
WS_EXTRA = 3                                    # slots behind the last one that must keep it


def new_workspace(row, dev="cpu"):
    return torch.full(((nblk(row) + WS_EXTRA) * 64,), WS_SENT, dtype=torch.int32, device=dev).view(torch.float32)


def ulp_bf16(x64):
    """One bf16 ulp at |x| (fp64): 2^(floor(log2 |x|) - 7); the smallest subnormal step below the normal range."""
    e = torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def bound_ratio(row, case, res):
    """e. worst |out - ref64| / (2^-8 |ref64| + K 2^-23 sum|a w| + tiny) over the image, one more bf16 ulp of the result where a skip is
    added (its own rounding); everything outside the interior must be what check_store asks for (-> inf)."""
    g = geo(row)
    lo = expected_storage(row, torch.zeros_like(case.lin).to(BF16))
    got = res.Y[g.gout:g.gout + g.rows_out].view(g.Hq, g.Wq, row.ldy)[1:-1, 1:-1, :row.cout]
    frame = res.Y.clone()
    frame[g.gout:g.gout + g.rows_out].view(g.Hq, g.Wq, row.ldy)[1:-1, 1:-1, :row.cout] = 0
    if int((bits(frame) != bits(lo[0]))[lo[1]].sum()):
        return float("inf")
    ref = case.lin
    bound = 2.0 ** -8 * ref.abs() + g.K * 2.0 ** -23 * case.S + 1e-30
    if case.resid is not None:
        ref = ref + case.resid.double()
        bound = bound + ulp_bf16(ref)
    return float(((got.double() - ref).abs() / bound).max())


# ---- guard rows ----------------------------------------------------------------------------------------------------------------------
def guard_reads(row):
    """Rows of the INPUT storage outside the image (index relative to image row 0: negative in front, >= Hp Wp behind) that a launch reads
    with an effect on an interior output.  group = 1, stride 2 and the phases: none - an interior pixel's window stays inside the image,
    whatever reads a guard row is masked or goes to the scratch row.  A 3 x 3 pixel-group launch multiplies the whole window of group + 2
    pixels per kernel row by the Toeplitz matrix, zeros included: every GEMM row that holds an interior pixel reads rows
    m group - (Wp + 1) + ky Wp + [0, group + 2), and 0 x NaN is NaN.  -> {guard row: GEMM rows that read it}"""
    g, out = geo(row), {}
    if row.kind != "conv" or row.group == 1 or row.taps != 9:
        return out
    for m in range(g.M):
        px = [q for q in range(m * row.group, (m + 1) * row.group) if q < g.rows and 1 <= q // g.Wp <= row.H and 1 <= q % g.Wp <= row.W]
        if not px:
            continue
        for ky in range(3):
            for j in range(g.win):
                r = m * row.group - (g.Wp + 1) + ky * g.Wp + j
                if r < 0 or r >= g.rows:
                    out.setdefault(r, set()).add(m)
    return out


def poison_input(row, storage, keep=()):
    """NaN in every guard row of an input storage [gin + rows + gin, Cin] but the rows `keep` (relative to image row 0)."""
    g = geo(row)
    rel = torch.arange(storage.shape[0], device=storage.device) - g.gin
    bad = (rel < 0) | (rel >= g.rows)
    for r in keep:
        bad &= rel != r
    storage[bad] = float("nan")
    return storage


def build_input(row, x, poison=True, nan_rows=()):
    """The input storage of a case: zero-bordered pixel-major image between guard rows; poison: NaN in every guard row the contract
    (guard_reads) does not name, zeros in those it names; nan_rows: NaN there too."""
    g = geo(row)
    st = torch.zeros((g.rows + 2 * g.gin, row.cin), dtype=BF16, device=x.device)
    st[g.gin:g.gin + g.rows].view(g.Hp, g.Wp, row.cin)[1:-1, 1:-1] = x
    if poison:
        poison_input(row, st, keep=guard_reads(row).keys())
    for r in nan_rows:
        st[g.gin + r] = float("nan")
    return st


def build_resid(row, resid):
    """The skip's storage: the interior, NaN on the border, in the guard rows and in the padding channels."""
    g = geo(row)
    st = torch.full((g.rows_out + 2 * g.gout, row.ldy), float("nan"), dtype=BF16, device=resid.device)
    st[g.gout:g.gout + g.rows_out].view(g.Hq, g.Wq, row.ldy)[1:-1, 1:-1, :row.cout] = resid
    if row.group > 1:
        st[g.gout:g.gout + g.rows_out].view(g.Hq, g.Wq, row.ldy)[1:-1, 1:-1, row.cout:] = 0          # stored as skip + 0: part of the image
    return st


def poisoned_pixels(row, r):
    """[Hp Wp] bool: padded pixels whose stored value turns NaN when guard row r holds NaN (every unmasked pixel of the GEMM rows that read it)."""
    g = geo(row)
    out = torch.zeros(g.rows, dtype=torch.bool)
    for m in guard_reads(row).get(r, ()):
        for q in range(m * row.group, min((m + 1) * row.group, g.rows)):
            out[q] = 1 <= q // g.Wp <= row.H and 1 <= q % g.Wp <= row.W
    return out


# ---- the emulation -------------------------------------------------------------------------------------------------------------------
def emulate(row, case, mutant=None, poison=True, nan_rows=()):
    """-> NS(Y, ws, nblk): what the launch of `row` leaves in the output storage and the partial workspace, computed along the scheme."""
    assert mutant is None or mutant in MUTANTS
    g, dev = geo(row), case.x.device
    geom, _, per, nprob = dispatch(row)
    w4 = case.w4.flip(2) if mutant == "kx_reversed" and case.w4.shape[2] == 3 else case.w4
    if row.kind == "up2":
        Ws = [w.reshape(row.cout, -1) for w in (case.wph if getattr(case, "wph", None) is not None else phase_fold(w4, torch.float32).to(BF16))]
        bias = case.bias.to(BF16)
    else:
        W, bias = toeplitz(row, w4, case.bias)
        Ws = [W]
    flat = build_input(row, case.x, poison, nan_rows).reshape(-1).double()
    rflat = None if case.resid is None else build_resid(row, case.resid)
    Y = new_output(row, dev)
    ws = new_workspace(row, dev)
    tab = row_table(row, dev) if g.table else None
    if mutant == "phases_exchanged" and row.kind == "up2":
        tab = tab[[0, 2, 1, 3]]
    M = g.rows // row.group if mutant == "hanging_row_dropped" else g.M
    shift = {128: 2, 256: 3, 512: 4}.get(g.gn_c, 0) + (mutant == "stats_shift_of_wrong_channel_count")
    k = torch.arange(g.K, device=dev)
    kt = k // BK
    if g.crt:
        jump = g.Wp * row.cin if mutant == "jump_of_wp" else g.jump
        k = k + ((kt - 1).clamp_min(0) if mutant == "jump_one_tile_late" else kt) // g.crt * jump
    m = torch.arange(M, device=dev)
    col = torch.arange(g.N, device=dev)
    pix = m[:, None] * row.group + (col // g.cpp)[None, :]                                   # [M, N] this element's padded pixel
    cpy, cpx = pix // g.Wp, pix % g.Wp
    border = (cpx == 0) | (cpy == 0)
    if mutant != "mask_missing_last_column":
        border |= cpx == g.Wp - 1
    if mutant != "mask_missing_last_row":
        border |= cpy >= g.Hp - 1
    if not g.mask or (mutant == "up2_border_not_zeroed" and row.kind == "up2"):
        border = torch.zeros_like(border)
    for ph in range(nprob):
        origin = g.origin[ph]
        if mutant == "origin_off_by_one":
            origin += row.cin
        if row.kind == "s2":
            origin = {"s2_origin_without_offset": 0, "s2_pad_top": row.cin, "s2_pad_left": g.Wp * row.cin}.get(mutant, origin)
        A = flat[g.gin * row.cin + origin + m[:, None] * g.lda + k[None, :]]
        acc = A @ Ws[ph].double().t()
        if rflat is not None:
            r = rflat[g.gout:].reshape(-1)[:M * g.ldc].view(M, g.ldc)[:, :g.N].float()
            if mutant == "skip_before_rounding":
                v = (acc + bias.double() + r.double()).float().to(BF16)
            else:
                v = (acc + bias.double()).float().to(BF16)
                if mutant == "mask_before_skip":
                    v = torch.where(border, torch.zeros_like(v), v)
                v = (r + v.float()).to(BF16)
        else:
            v = (acc + bias.double()).float().to(BF16)
        stat = v                                                                             # statistics of what is stored
        if mutant != "mask_before_skip":
            v = torch.where(border, torch.zeros_like(v), v)
        if mutant != "stats_before_mask":
            stat = v
        if mutant == "group_pixels_swapped" and row.group > 1:
            v = v.view(M, row.group, -1).flip(1).reshape(M, g.N)
        if row.gn:
            grp = (col & (g.gn_c - 1)) >> shift
            for t in range(per):
                tt = t
                if mutant == "group_m_tiles_swapped" and t < 2 and per >= 2:
                    tt = 1 - t
                tm, tn = tile_coords(tt, g.M, g.N, geom)
                s = stat[tm * geom:(tm + 1) * geom, tn * geom:(tn + 1) * geom].double()
                gi = grp[tn * geom:(tn + 1) * geom]
                slot = torch.zeros(64, dtype=torch.float64, device=dev)
                ok = gi < 32
                slot[0::2].index_add_(0, gi[ok], s.sum(0)[ok])
                slot[1::2].index_add_(0, gi[ok], (s * s).sum(0)[ok])
                at = (t if mutant == "up2_slot_base_restarted" else ph * per + t)
                if mutant == "slot_of_neighbour_tile":
                    at = min(at ^ 1, per * nprob - 1)
                ws[at * 64:(at + 1) * 64] = slot.float()
        if tab is None:
            Y[g.gout:].reshape(-1)[:M * g.ldc].view(M, g.ldc)[:, :g.N] = v
        else:
            Y[g.gout + tab[ph][:M], :g.N] = v
    return NS(Y=Y, ws=ws, nblk=per * nprob if row.gn else 0)
