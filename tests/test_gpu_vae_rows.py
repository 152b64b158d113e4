"""-m gpu: the VAE's row kernels (csrc/vae.hip) and the trunk's small elementwise / row entry points (csrc/norm.hip, csrc/region.hip) pinned
to float64 references computed on the host from the exact bf16 inputs the kernel saw.  tests/test_gpu_vae.py and tests/test_gpu_qwen_vae.py
check these passes only through whole decodes / encodes (PSNR >= 40 dB) or at a few random shapes (PSNR >= 48 dB): a pass that is wrong on
a border column, one row or a special value can clear those bars.  Here: element-wise bars (one bf16 ulp, or bit-exact), border and padding
cells written exactly 0, masked cells poisoned with +1e30 / +inf / NaN, and the shapes where the kernels change path (idle lanes, tail rows,
grid-stride loops, the 24576-column limit).

"<= 1 ulp": |got - ref| <= one bf16 ulp of the float64 reference, with the bf16 ulp of the smallest normal (2^-133) as the floor and an
absolute floor of 2^-126 where a kernel may flush an fp32 denormal intermediate to zero."""
import math

import pytest
import torch

from regione_amd import _lib, ops, vae as V
from tests.test_gpu_vae import _border_is_zero, _padded, _unpadded

pytestmark = pytest.mark.gpu

_TINY = 2.0 ** -126          # smallest normal fp32 / bf16


def _ulp_bf16(ref: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp at each |ref| (float64): 2^(e - 7) for |ref| in [2^e, 2^(e+1)), e >= -126."""
    _, e = torch.frexp(ref.abs().clamp_min(_TINY))
    return torch.ldexp(torch.ones_like(ref), (e - 8).to(torch.int32))


def _assert_within_ulp(got: torch.Tensor, ref: torch.Tensor, what: str, floor: float = 0.0):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    tol = _ulp_bf16(ref).clamp_min(floor)
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values beyond 1 bf16 ulp; first at flat index {i}: "
                             f"got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _bf16_from_bits(bits) -> torch.Tensor:
    return torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


# special bf16 values: +-0, +-1, +-inf, NaN, subnormals (smallest, largest, a middle one, negative), values just inside / outside [-1, 1]
_SPECIAL = _bf16_from_bits([0x0000, 0x8000, 0x3F80, 0xBF80, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x0001, 0x8001, 0x007F, 0x0040, 0x807F,
                            0x3F7F, 0xBF7F, 0x3F81, 0xBF81, 0x7F7F, 0xFF7F, 0x0080, 0x8080])


def _special_fill(n: int, seed: int) -> torch.Tensor:
    """n bf16 values (CPU): every special value at least once, then special / randn * 2 mixed."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g) * 2).bfloat16()
    k = min(n, len(_SPECIAL))
    x[:k] = _SPECIAL[:k]
    pick = torch.rand(n, generator=g) < 0.3
    pick[:k] = False
    x[pick] = _SPECIAL[torch.randint(len(_SPECIAL), (int(pick.sum()),), generator=g)]
    return x[torch.randperm(n, generator=g)] if n > len(_SPECIAL) else x


def _assert_bit_equal_nan_aware(got: torch.Tensor, ref: torch.Tensor, what: str):
    got, ref = got.cpu(), ref.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), f"{what}: NaN at {int((gn != rn).sum())} positions that differ from the reference (got NaN: {int(gn.sum())}, ref: {int(rn.sum())})"
    diff = (_bits(got) != _bits(ref)) & ~rn
    assert not diff.any(), (f"{what}: {int(diff.sum())} values differ bitwise; first: got {got[diff][:4].tolist()}, ref {ref[diff][:4].tolist()}")


# ================================================================================================================================
# 1. rgn_softmax_rows
# ================================================================================================================================
def _key_valid(Hp, Wp, ld, device):
    col = torch.arange(ld, device=device)
    cy, cx = col // Wp, col % Wp
    return (col < Hp * Wp) & (cx != 0) & (cx != Wp - 1) & (cy != 0) & (cy != Hp - 1)


def _softmax_input(Hp, Wp, ld, seed):
    """S [Hp Wp, ld] bf16 on the GPU.  Query row r's regime is r % 4: 0 randn * 3; 1 randn with one dominant logit (+1000 on a valid key);
    2 all equal (0.5); 3 logits around +3e4 or -3e4 (alternating per group of four rows; bf16 spacing 128 there).  Border key columns and
    the padding columns [Hp Wp, ld) hold +1e30, +inf and NaN in turn."""
    dev = "cuda"
    rows = Hp * Wp
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.randn(rows, ld, generator=g, device=dev)
    r = torch.arange(rows, device=dev)[:, None]
    reg = r % 4
    S = torch.where(reg == 0, S * 3.0, S)
    S = torch.where(reg == 2, torch.full_like(S, 0.5), S)
    S = torch.where(reg == 3, torch.where((r // 4) % 2 == 0, 3e4, -3e4) + 300.0 * S, S)
    valid = _key_valid(Hp, Wp, ld, dev)
    vidx = valid.nonzero().reshape(-1)
    dom = vidx[(torch.arange(rows, device=dev) * 7919) % vidx.numel()]           # a valid key column per row
    rr = torch.arange(rows, device=dev)
    S[rr[reg[:, 0] == 1], dom[reg[:, 0] == 1]] = 1000.0
    poison = torch.tensor([1e30, float("inf"), float("nan")], device=dev)[torch.arange(ld, device=dev) % 3]
    S = torch.where(valid[None, :], S, poison[None, :])
    return S.bfloat16().contiguous(), valid


def _softmax_ref(S_rows_bf16: torch.Tensor, valid: torch.Tensor, scale: float) -> torch.Tensor:
    s = S_rows_bf16.double().cpu()[:, valid.cpu()] * scale
    s = s - s.max(dim=1, keepdim=True).values
    e = torch.exp(s)
    return e / e.sum(dim=1, keepdim=True)


@pytest.mark.parametrize("Hp,Wp,ld", [(3, 3, 64), (5, 7, ops.padded(35)), (18, 34, ops.padded(18 * 34) + 64), (130, 130, 16960),
                                      (128, 192, 24576)])
def test_softmax_rows_vs_fp64(Hp, Wp, ld):
    """(3, 3): one valid key; padding columns beyond Hp Wp; the 1024 x 1024 mid block; exactly the 24576-column limit (a seeded sample of
    rows, border query rows included).  Masked columns exactly 0 in every checked row; valid entries <= 1 ulp of softmax(scale S)."""
    rows = Hp * Wp
    scale = 1.0 / math.sqrt(512)
    S, valid = _softmax_input(Hp, Wp, ld, seed=Hp * 1000 + Wp)
    S0 = S.clone()
    _lib.check(_lib.lib().rgn_softmax_rows(ops._p(S), ld, Hp, Wp, scale, ops._stream()), "rgn_softmax_rows")
    torch.cuda.synchronize()
    if rows <= 1024:
        idx = torch.arange(rows)
    else:                                   # border query rows (first / last padded row, left / right columns), then a seeded sample
        g = torch.Generator().manual_seed(rows)
        idx = torch.cat([torch.tensor([0, 1, Wp - 1, Wp, 2 * Wp - 1, rows // 2, rows - Wp, rows - 1]),
                         torch.randint(rows, (184,), generator=g)]).unique()
    got = S[idx.cuda()].cpu()
    vc = valid.cpu()
    masked = got[:, ~vc]
    assert bool((masked == 0).all()), f"{int((masked != 0).sum())} masked (border / padding) columns not 0"
    ref = _softmax_ref(S0[idx.cuda()], valid, scale)
    _assert_within_ulp(got[:, vc], ref, f"softmax_rows {Hp} x {Wp}, ld {ld}", floor=_TINY)
    if int(vc.sum()) == 1:
        assert bool((got[:, vc] == 1).all())
    sel = idx % 4 == 2                                               # all-equal rows: every valid key bf16(1 / N_valid)
    if bool(sel.any()):
        want = torch.tensor(1.0 / int(vc.sum()), dtype=torch.float64).bfloat16()
        assert bool((got[sel][:, vc] == want).all()), "all-equal rows: P != bf16(1 / N_valid)"


def test_softmax_rows_rejects_bad_leading_dimensions_without_a_launch():
    """ld % 8 != 0, ld < Hp Wp, ld > 24576: an error code and the buffer untouched.  Each buffer is large enough for the launch a broken
    check would make (no out-of-range access either way)."""
    L = _lib.lib()
    for Hp, Wp, ld in [(5, 7, 36), (5, 7, 100), (9, 9, 72), (3, 3, 24584)]:
        buf = torch.full((Hp * Wp, max(ld, 8)), 0.25, dtype=torch.bfloat16, device="cuda")
        rc = L.rgn_softmax_rows(ops._p(buf), ld, Hp, Wp, 1.0, ops._stream())
        torch.cuda.synchronize()
        assert rc != 0, (Hp, Wp, ld)
        assert bool((buf == 0.25).all()), (Hp, Wp, ld)


# ================================================================================================================================
# 2. layout conversions, bit-exact
# ================================================================================================================================
@pytest.mark.parametrize("H,W,Co,ld", [(1, 1, 3, 8), (3, 5, 16, 64), (37, 61, 48, 64), (37, 61, 3, 8)])
def test_padded_to_nchw_cvt_bit_exact(H, W, Co, ld):
    """rgn_padded_to_nchw_cvt (bf16 / fp32 output, clamp on / off) and rgn_padded_to_nchw against torch.clamp(x, -1, 1).to(dtype): bit for
    bit, NaN where torch keeps NaN; the first Co of ld channels read, the border never; nothing written past the output."""
    Hp, Wp = H + 2, W + 2
    X = _special_fill(Hp * Wp * ld, seed=H * 100 + W).reshape(Hp * Wp, ld)
    x = X.reshape(Hp, Wp, ld)[1:-1, 1:-1, :Co].permute(2, 0, 1).contiguous()          # [Co, H, W]
    Xg = X.cuda()
    L, n, extra = _lib.lib(), Co * H * W, 64
    for dtype in (torch.bfloat16, torch.float32):
        for clamp in (False, True):
            out = torch.full((n + extra,), 7.0, dtype=dtype, device="cuda")
            _lib.check(L.rgn_padded_to_nchw_cvt(ops._p(Xg), ld, ops._p(out), Co, H, W, int(clamp), int(dtype == torch.float32), ops._stream()),
                       "rgn_padded_to_nchw_cvt")
            torch.cuda.synchronize()
            ref = (torch.clamp(x, -1, 1) if clamp else x).to(dtype)
            _assert_bit_equal_nan_aware(out[:n].reshape(Co, H, W), ref, f"padded_to_nchw_cvt {dtype} clamp={clamp}")
            assert bool((out[n:] == 7.0).all()), "written past the output"
    out = torch.full((n + extra,), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(L.rgn_padded_to_nchw(ops._p(Xg), ld, ops._p(out), Co, H, W, ops._stream()), "rgn_padded_to_nchw")
    torch.cuda.synchronize()
    _assert_bit_equal_nan_aware(out[:n].reshape(Co, H, W), x, "padded_to_nchw")
    assert bool((out[n:] == 7.0).all())


def test_padded_to_nchw_cvt_clamp_keeps_nan():
    """The decoded image of an overflowed decode: NaN must stay NaN (torch.clamp), not become -1 or 1 (fminf / fmaxf drop a NaN operand)."""
    X = torch.zeros((3 * 3, 8), dtype=torch.bfloat16)
    X[4, :3] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    Xg = X.cuda()
    for fp32 in (0, 1):
        out = torch.zeros(3, dtype=torch.float32 if fp32 else torch.bfloat16, device="cuda")
        _lib.check(_lib.lib().rgn_padded_to_nchw_cvt(ops._p(Xg), 8, ops._p(out), 3, 1, 1, 1, fp32, ops._stream()), "rgn_padded_to_nchw_cvt")
        torch.cuda.synchronize()
        assert torch.isnan(out[0]).item() and out[1].item() == 1.0 and out[2].item() == -1.0, out


@pytest.mark.parametrize("Cz,H,W,Cpad", [(3, 1, 1, 8), (16, 3, 5, 64), (3, 37, 61, 64), (13, 37, 61, 16), (16, 128, 128, 512)])
def test_nchw_to_padded_bit_exact(Cz, H, W, Cpad):
    """rgn_nchw_to_padded into a destination pre-filled with a non-zero pattern: the image bit for bit (specials included), border rows and
    channels [Cz, Cpad) exactly +0, nothing written past the image; 130 x 130 x 512 > 8192 x 1024 elements runs the grid-stride loop.  The
    round trip through rgn_padded_to_nchw gives the input back bit for bit."""
    Hp, Wp = H + 2, W + 2
    Z = _special_fill(Cz * H * W, seed=Cz + H * W).reshape(Cz, H, W)
    Zg = Z.cuda()
    total, extra = Hp * Wp * Cpad, 256
    Y = torch.full((total + extra,), 0x5A5A, dtype=torch.int32, device="cuda").to(torch.int16).view(torch.bfloat16)
    _lib.check(_lib.lib().rgn_nchw_to_padded(ops._p(Zg), ops._p(Y), Cz, H, W, Cpad, ops._stream()), "rgn_nchw_to_padded")
    torch.cuda.synchronize()
    assert bool((_bits(Y[total:]) == 0x5A5A).all()), "written past the image"
    y = Y[:total].reshape(Hp, Wp, Cpad).cpu()
    yb = _bits(y)
    interior = y[1:-1, 1:-1]
    _assert_bit_equal_nan_aware(interior[..., :Cz].permute(2, 0, 1).contiguous(), Z, "nchw_to_padded image")
    assert bool((_bits(interior[..., Cz:]) == 0).all()), "padding channels not +0"
    assert bool((yb[0] == 0).all() and (yb[-1] == 0).all() and (yb[:, 0] == 0).all() and (yb[:, -1] == 0).all()), "border not +0"
    back = torch.empty((Cz, H, W), dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_padded_to_nchw(ops._p(Y), Cpad, ops._p(back), Cz, H, W, ops._stream()), "rgn_padded_to_nchw")
    torch.cuda.synchronize()
    _assert_bit_equal_nan_aware(back, Z, "round trip")


# ================================================================================================================================
# 3. rgn_rms_norm_silu at the shapes tests/test_gpu_qwen_vae.py does not reach
# ================================================================================================================================
def _silu64(t):
    return t / (1.0 + torch.exp(-t))


@pytest.mark.parametrize("H,W,c_valid,c_pad", [(13, 17, 64, 64), (9, 31, 300, 320), (5, 7, 512, 512), (21, 11, 100, 128), (6, 5, 8, 64)])
@pytest.mark.parametrize("silu", [False, True])
def test_rms_norm_silu_vs_fp64(H, W, c_valid, c_pad, silu):
    """8 lanes per pixel (C_pad 64), 24 idle lanes (320), 64 lanes (512); C_valid not a multiple of 8 (100 of 128); pixel counts that are
    not a multiple of the rows per block (the tail rows take part in the shuffles); all-zero pixels (0, no NaN); pixel scales from 1e-2 to
    1e2.  Non-zero garbage in the input's border rows, padding channels and gamma past C_valid: the norm covers X[:C_valid] only.  The
    output starts as a non-zero pattern: border rows and padding channels must come out exactly +0; bit-reproducible."""
    Hp, Wp = H + 2, W + 2
    rows = Hp * Wp
    g = torch.Generator().manual_seed(c_pad * 100 + H)
    scale = torch.pow(10.0, torch.empty(rows, 1).uniform_(-2, 2, generator=g))
    X = (torch.randn(rows, c_pad, generator=g) * scale).bfloat16()
    zero = torch.zeros(rows, dtype=torch.bool)
    zero[torch.randperm(rows, generator=g)[: max(2, rows // 10)]] = True
    X[zero, :c_valid] = 0                                              # all-zero pixels (their padding channels keep garbage)
    gamma = (1.0 + 0.2 * torch.randn(c_pad, generator=g)).bfloat16()
    gamma[c_valid:] = 3.0
    Xg, gg = X.cuda(), gamma.cuda()
    outs = []
    for _ in range(2):
        Y = torch.full((rows, c_pad), -5.0, dtype=torch.bfloat16, device="cuda")
        _lib.check(_lib.lib().rgn_rms_norm_silu(ops._p(Xg), ops._p(Y), Hp, Wp, c_valid, c_pad, ops._p(gg), int(silu), ops._stream()),
                   "rgn_rms_norm_silu")
        torch.cuda.synchronize()
        outs.append(Y.cpu())
    Y = outs[0]
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "not bit-reproducible"
    y = Y.reshape(Hp, Wp, c_pad)
    yb = _bits(y)
    assert bool((yb[0] == 0).all() and (yb[-1] == 0).all() and (yb[:, 0] == 0).all() and (yb[:, -1] == 0).all()), "border rows not +0"
    assert bool((yb[..., c_valid:] == 0).all()), "padding channels not +0"
    xv = X.double().reshape(Hp, Wp, c_pad)[1:-1, 1:-1, :c_valid]
    nrm = xv.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    ref = xv / nrm * math.sqrt(c_valid) * gamma[:c_valid].double()
    if silu:
        ref = _silu64(ref)
    got = y[1:-1, 1:-1, :c_valid]
    _assert_within_ulp(got, ref, f"rms_norm_silu C {c_valid}/{c_pad} silu={silu}", floor=_TINY)
    zi = zero.reshape(Hp, Wp)[1:-1, 1:-1]
    assert bool((got[zi] == 0).all()), "all-zero pixels must give 0"


# ================================================================================================================================
# 4. GroupNorm where the mean dwarfs the spread
# ================================================================================================================================
def _gn_input(H, W, C, ratio, seed):
    """x = mu_g + sigma_g N(0, 1) per group, sigma_g in [0.5, 2], |mu_g| = ratio * sigma_g, the sign alternating per group."""
    g = torch.Generator().manual_seed(seed)
    sig = torch.empty(32).uniform_(0.5, 2.0, generator=g)
    mu = ratio * sig * torch.where(torch.arange(32) % 2 == 0, 1.0, -1.0)
    cpg = C // 32
    return torch.randn(1, C, H, W, generator=g) * sig.repeat_interleave(cpg)[None, :, None, None] + mu.repeat_interleave(cpg)[None, :, None, None]


def _gn_bar(got, ref, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    tol = 2.0 ** -7 * ref.abs().clamp_min(1.0)
    assert bool((err <= tol).all()), f"{what}: max |got - ref| = {float(err.max()):.3g} (worst ratio to the bar {float((err / tol).max()):.2f})"


@pytest.mark.parametrize("H,W,C", [(32, 48, 128), (64, 64, 512), (130, 126, 256)])
@pytest.mark.parametrize("ratio", [30.0, 100.0])
def test_groupnorm_standalone_statistics_large_mean(H, W, C, ratio):
    """gn_stats_kernel + gn_finalize_kernel (one-pass E[x^2] - E[x]^2 from fp32 partial sums) at mean / sigma 30 and 100, against float64
    group_norm of the bf16 input: max |got - ref| <= 2^-7 max(|ref|, 1) before SiLU (and after it, against silu(ref))."""
    x = _gn_input(H, W, C, ratio, seed=C + H + int(ratio))
    g = torch.Generator().manual_seed(C)
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g)).bfloat16(), (0.1 * torch.randn(C, generator=g)).bfloat16()
    ref = torch.nn.functional.group_norm(x.bfloat16().double(), 32, gamma.double(), beta.double(), eps=1e-6)
    xi = _padded(x)
    for silu in (False, True):
        out = V.PaddedImage(H, W, C, "cuda")
        out.t.fill_(-3.0)                                              # the border must be written as 0, not left as found
        V.groupnorm_silu(xi, gamma.cuda(), beta.cuda(), out, silu=silu)
        torch.cuda.synchronize()
        assert _border_is_zero(out)
        _gn_bar(_unpadded(out), torch.nn.functional.silu(ref) if silu else ref, f"groupnorm {H} x {W} x {C}, mean/sigma {ratio}, silu={silu}")


@pytest.mark.parametrize("H,W,cin,cout,group", [(32, 48, 128, 128, 2), (64, 64, 256, 512, 1), (130, 126, 128, 256, 1)])
@pytest.mark.parametrize("ratio", [30.0, 100.0])
def test_groupnorm_epilogue_statistics_large_mean(H, W, cin, cout, group, ratio):
    """The precomputed_blocks > 0 path: rgn_conv_bf16(gn=True) leaves per-tile fp32 sums of the image it stores (here conv + bias + a ResNet
    skip carrying the large per-group means), the GroupNorm finalizes them.  Same bar against float64 group_norm of that stored image.
    With the statistics already taken, the input's border rows are then poisoned: the apply pass must still write its border as 0."""
    g = torch.Generator().manual_seed(H + cin + cout + int(ratio))
    x = torch.randn(1, cin, H, W, generator=g)
    r = _gn_input(H, W, cout, ratio, seed=H + cout)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = 0.1 * torch.randn(cout, generator=g)
    gamma, beta = (1.0 + 0.2 * torch.randn(cout, generator=g)).bfloat16(), (0.1 * torch.randn(cout, generator=g)).bfloat16()
    xi, ri = _padded(x), _padded(r)
    cw = V.ConvWeights(w.permute(0, 2, 3, 1).cuda(), b.cuda(), group=group)
    y, n = V.PaddedImage(H, W, cout, "cuda"), V.PaddedImage(H, W, cout, "cuda")
    V.conv(xi, cw, y, resid=ri, gn=True)
    owner, nblk = V.gn_handoff(y.t.device)
    assert owner is y and nblk > 0
    yv = _unpadded(y).double().cpu()
    t = y.t.view(y.Hp, y.Wp, cout)
    t[0], t[-1], t[:, 0], t[:, -1] = 7.0, -7.0, 5.0, float("nan")
    n.t.fill_(-3.0)
    V.groupnorm_silu(y, gamma.cuda(), beta.cuda(), n, silu=False)
    torch.cuda.synchronize()
    assert _border_is_zero(n)
    ref = torch.nn.functional.group_norm(yv, 32, gamma.double(), beta.double(), eps=1e-6)
    _gn_bar(_unpadded(n), ref, f"groupnorm after conv {H} x {W} {cin} -> {cout}, mean/sigma {ratio}")


# ================================================================================================================================
# 6. the trunk's remaining row entry points
# ================================================================================================================================
@pytest.mark.parametrize("M,d,ldx", [(64, 3584, 3584 + 64), (37, 100, 136), (5, 100, 100)])
def test_rms_norm_rows_vs_diffusers_rmsnorm(M, d, ldx):
    """rgn_rms_norm_rows against diffusers RMSNorm's arithmetic: fp32 variance, x rsqrt(var + eps), round to bf16, times the bf16 weight
    (one more bf16 rounding).  The intermediate is rounded from a float64 value here: the output must equal bf16(h w) bit for bit, where h
    may be the neighbouring bf16 value only if the float64 intermediate lies within 2^-16 (relative) of a bf16 rounding boundary - the one
    place an fp32 computation may legitimately round the other way.  Columns past d of the output row stride are not written."""
    g = torch.Generator().manual_seed(d + M)
    ldo = ldx + 8
    scale = torch.pow(10.0, torch.empty(M, 1).uniform_(-2, 2, generator=g))
    x = (torch.randn(M, ldx, generator=g) * scale).bfloat16()
    x[:, d:] = float("nan")                                                # never read
    w = (1.0 + 0.3 * torch.randn(d, generator=g)).bfloat16()
    eps = 1e-6
    xg, wg = x.cuda(), w.cuda()
    out = torch.full((M, ldo), 9.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_rms_norm_rows(ops._p(xg), ldx, ops._p(wg), ops._p(out), ldo, M, d, eps, ops._stream()), "rgn_rms_norm_rows")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[:, d:] == 9.0).all()), "written past d"
    got = out[:, :d]
    xd = x[:, :d].double()
    h64 = xd / torch.sqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    h = h64.bfloat16()
    ref = (h.float() * w.float()).bfloat16()                             # a bf16 x bf16 product is exact in fp32: one rounding, as torch
    ok = _bits(got) == _bits(ref)
    if not bool(ok.all()):
        hb = _bits(h).to(torch.int32)                                    # the two bf16 neighbours of h
        up = (hb + 1).to(torch.int16).view(torch.bfloat16)
        dn = (hb - 1).to(torch.int16).view(torch.bfloat16)
        mid_up = (h.double() + up.double()) / 2
        mid_dn = (h.double() + dn.double()) / 2
        near = torch.minimum((h64 - mid_up).abs(), (h64 - mid_dn).abs()) <= 2.0 ** -16 * h64.abs()
        alt = (_bits((up.float() * w.float()).bfloat16()) == _bits(got)) | (_bits((dn.float() * w.float()).bfloat16()) == _bits(got))
        bad = ~ok & ~(near & alt)
        assert not bool(bad.any()), (f"rms_norm_rows d {d}: {int(bad.sum())} values differ from bf16(bf16(x r) w); first got "
                                     f"{got[bad][:4].tolist()}, ref {ref[bad][:4].tolist()}")
        assert int((~ok).sum()) <= max(8, got.numel() // 1000), "too many rounding-boundary flips"


@pytest.mark.parametrize("n", [1, 1023, 1024 * 256 + 4097])
def test_silu_bf16_vs_fp64(n):
    """rgn_silu_bf16: odd n, n > 1024 x 256 (the grid-stride loop runs), +-inf (silu(+inf) = inf; silu(-inf) is NaN in float64 as in
    torch), inputs in [-80, 80] (below about -88.7 fp32 exp overflows and torch's own fp32 / bf16 SiLU returns -0 as this kernel does).
    <= 1 ulp against float64 SiLU; nothing written past n."""
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=g) * 4).clamp(-80, 80)
    x[torch.rand(n, generator=g) < 0.01] *= 20
    x = x.clamp(-80, 80).bfloat16()
    if n >= 3:
        x[0], x[n // 2], x[-1] = float("inf"), -float("inf"), 0.0
    xg = x.cuda()
    y = torch.full((n + 64,), 3.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_silu_bf16(ops._p(xg), ops._p(y), n, ops._stream()), "rgn_silu_bf16")
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[n:] == 3.0).all()), "written past n"
    got, ref = y[:n], _silu64(x.double())
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref))
    assert bool((got[torch.isinf(ref)] == ref[torch.isinf(ref)].bfloat16()).all())
    _assert_within_ulp(got[fin], ref[fin], f"silu n {n}", floor=_TINY)


@pytest.mark.parametrize("row_bytes", [12, 36, 4096, 4100])
@pytest.mark.parametrize("offset", [0, 4])
def test_scatter_gather_rows_round_trip(row_bytes, offset):
    """rgn_scatter_rows / rgn_gather_rows on the 16-byte path (row_bytes 4096, 16-byte aligned views) and the 4-byte path (12, 36, 4100; or
    any row size on views shifted by 4 bytes): dst[ids[k]] = src[k] bit for bit, rows not named keep their bytes, gather(scatter(x)) = x."""
    g = torch.Generator().manual_seed(row_bytes + offset)
    L_rows, K = 97, 41
    w = row_bytes // 4
    ids = torch.randperm(L_rows, generator=g)[:K].to(torch.int64)
    src_store = torch.randint(-2 ** 31, 2 ** 31 - 1, (K * w + 16,), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    dst_store = torch.randint(-2 ** 31, 2 ** 31 - 1, (L_rows * w + 16,), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    o = offset // 4
    src = src_store[o:o + K * w].view(K, w)
    dst = dst_store[o:o + L_rows * w].view(L_rows, w)
    dst0 = dst_store.clone()
    idg = ids.cuda()
    L = _lib.lib()
    _lib.check(L.rgn_scatter_rows(ops._p(src), ops._p(idg), ops._p(dst), K, row_bytes, ops._stream()), "rgn_scatter_rows")
    back = torch.zeros((K * w + 16,), dtype=torch.int32, device="cuda")
    bv = back[o:o + K * w].view(K, w)
    _lib.check(L.rgn_gather_rows(ops._p(dst), ops._p(idg), ops._p(bv), K, row_bytes, ops._stream()), "rgn_gather_rows")
    torch.cuda.synchronize()
    want = dst0[o:o + L_rows * w].view(L_rows, w).clone()
    want[ids.cuda()] = src
    assert torch.equal(dst, want)
    assert torch.equal(dst_store[:o], dst0[:o]) and torch.equal(dst_store[o + L_rows * w:], dst0[o + L_rows * w:]), "written outside dst"
    assert torch.equal(bv, src)
    assert bool((back[:o] == 0).all() and (back[o + K * w:] == 0).all())
