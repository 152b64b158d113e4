"""-m gpu: the fused mid-block attention of the VAEs (rgn_vae_attention_bf16, csrc/vae.hip) and the decode / encode sizes it opens.

Kernel level: against a float64 reference computed on the device from the exact bf16 inputs, in query chunks.  Element-wise bar, derived
from the kernel's one approximation that matters - P rounded to bf16 (relative error <= 2^-9 per weight, RNE): with weights p_j (1 + e_j),
|O~ - O| = |sum p_j e_j (v_j - O)| / sum p~_j <= 2^-9 / (1 - 2^-9) * max_j |v_j - O| <= 2^-8 * range_c(V), plus one bf16 rounding of the
output (2^-8 |O|, generous) and the fp32 score accumulation (2^-9 range_c(V) at logits of +-100).

Module level: the AutoencoderKL decoder / encoder and the Qwen-Image classes above the materialised path's 24576-row limit (latent 160,
1280 x 1280, and 2048 x 2048) against the fp32 host stand-ins, >= 40 dB; the 2048 x 2048 references compute the attention in query chunks
(subclasses below), since `q @ k^T` there would need 17 GB of fp32."""
import math

import pytest
import torch

from regione_amd import RegionEHelper, _lib, ops, qwen_vae as Q, vae as V
from tests import host_qwen_vae as HQ
from tests import host_standins as HS
from tests import host_vae

pytestmark = pytest.mark.gpu

def _psnr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    peak = float(b.max() - b.min())
    return 10 * math.log10(peak * peak / max(float(((a - b) ** 2).mean()), 1e-30))


def _fp32_on_cpu(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 64))
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.set_num_threads(n)


def _valid_rows(Hp, Wp, device="cuda"):
    y, x = torch.meshgrid(torch.arange(1, Hp - 1, device=device), torch.arange(1, Wp - 1, device=device), indexing="ij")
    return (y * Wp + x).reshape(-1)


def _run(q, k, v, bv, o, Hp, Wp, C):
    rc = _lib.lib().rgn_vae_attention_bf16(ops._p(q), ops._p(k), ops._p(v), None if bv is None else ops._p(bv), ops._p(o), Hp, Wp, C,
                                           1.0 / math.sqrt(C), ops._stream())
    _lib.check(rc, "rgn_vae_attention_bf16")
    torch.cuda.synchronize()
    return o


def _reference(q, k, v, bv, Hp, Wp, C, qrows, chunk=512):
    """float64 O for the padded rows `qrows` over every valid key, on the device, in query chunks."""
    kv = _valid_rows(Hp, Wp)
    K, Vd = k[kv].double(), v[kv].double()
    out = []
    for i in range(0, qrows.numel(), chunk):
        s = (q[qrows[i:i + chunk]].double() @ K.T) / math.sqrt(C)
        out.append(torch.softmax(s, dim=-1) @ Vd)
    o = torch.cat(out)
    if bv is not None:
        o = o + bv.double()
    return o


def _check(got, ref, v, Hp, Wp):
    kv = _valid_rows(Hp, Wp)
    vv = v[kv].double()
    rng = (vv.max(0).values - vv.min(0).values)                   # range_c(V)
    tol = (2.0 ** -8 + 2.0 ** -9) * rng + 2.0 ** -8 * ref.abs() + 1e-6
    err = (got.double() - ref).abs()
    bad = err > tol
    assert not bad.any(), (int(bad.sum()), float((err - tol).max()), float(err.max()))
    assert torch.isfinite(got.float()).all()


def _inputs(Hp, Wp, C, seed, logit=3.0, peak_last=False):
    """Q, K, V [Hp * Wp, C] bf16 with zero borders; scale * q . k has a spread of about `logit`.  peak_last: every query's largest logit is at
    the last valid key (the last key tile), so the running max moves there and the rescale of O is exercised."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = Hp * Wp
    a = math.sqrt(logit)                                         # q, k ~ N(0, a^2) each: scale * q . k = q . k / sqrt C ~ N(0, logit^2)
    q = torch.randn(rows, C, device="cuda", generator=g) * a
    k = torch.randn(rows, C, device="cuda", generator=g) * a
    v = torch.randn(rows, C, device="cuda", generator=g)
    if peak_last:
        u = torch.randn(C, device="cuda", generator=g)
        u = u / u.norm()
        q = q + 8.0 * a * u
        last = int(_valid_rows(Hp, Wp)[-1])
        k[last] = 2.0 * a * C ** 0.5 * u                         # scale * q . k_last ~ 16 logit +- 2 logit; other keys' maximum ~ 4.5 logit
    border = torch.ones(rows, dtype=torch.bool, device="cuda")
    border[_valid_rows(Hp, Wp)] = False
    for t in (q, k, v):
        t[border] = 0
    bv = (0.1 * torch.randn(C, device="cuda", generator=g)).bfloat16()
    return q.bfloat16().contiguous(), k.bfloat16().contiguous(), v.bfloat16().contiguous(), bv, border


@pytest.mark.parametrize("H,W,C", [(1, 1, 512), (1, 1, 384), (7, 11, 512), (37, 53, 384), (61, 3, 512), (128, 128, 512), (128, 128, 384)])
def test_fused_attention_vs_fp64(H, W, C):
    """3 x 3 (one valid key), odd Wp and query / key counts that are no multiple of the 64-query block or the 32-key tile, and the 1024^2
    mid block (130 x 130) at both widths: every valid query row against the fp64 reference; border rows of O are not written."""
    Hp, Wp = H + 2, W + 2
    q, k, v, bv, border = _inputs(Hp, Wp, C, seed=H * 1000 + W + C)
    o = torch.full_like(q, 7.0)
    _run(q, k, v, bv, o, Hp, Wp, C)
    qr = _valid_rows(Hp, Wp)
    _check(o[qr], _reference(q, k, v, bv, Hp, Wp, C, qr), v, Hp, Wp)
    assert bool((o[border] == 7.0).all())                         # the header's promise: border rows are left as they were
    if H * W == 1:
        assert torch.equal(o[qr].float(), (v[qr].float() + bv.float()).bfloat16().float())


@pytest.mark.parametrize("logit,peak_last", [(30.0, False), (30.0, True), (3.0, True)])
def test_fused_attention_stress_logits_and_late_max(logit, peak_last):
    """Logits up to about +-100 (scale * q . k with a spread of 30 over 16384 keys) and the row maximum in the last key tile."""
    Hp = Wp = 130
    C = 512
    q, k, v, bv, _ = _inputs(Hp, Wp, C, seed=int(logit) + 100 * peak_last, logit=logit, peak_last=peak_last)
    qr = _valid_rows(Hp, Wp)
    s = (q[qr[:256]].float() @ k[qr].float().T) / math.sqrt(C)
    if logit >= 30:
        assert float(s.abs().max()) >= 90.0
    if peak_last:
        assert bool((s.argmax(-1) == qr.numel() - 1).all())
    o = torch.empty_like(q)
    _run(q, k, v, bv, o, Hp, Wp, C)
    _check(o[qr], _reference(q, k, v, bv, Hp, Wp, C, qr), v, Hp, Wp)


def test_fused_attention_2048_mid_block_sampled():
    """The 2048^2 mid block (258 x 258, 66564 rows, 65536 keys) at C = 512: a seeded sample of 2048 query rows that includes the first,
    the last and the border-adjacent rows, against all keys."""
    Hp = Wp = 258
    C = 512
    q, k, v, bv, _ = _inputs(Hp, Wp, C, seed=2048)
    o = torch.empty_like(q)
    _run(q, k, v, bv, o, Hp, Wp, C)
    qr = _valid_rows(Hp, Wp)
    H = W = 256
    must = {0, qr.numel() - 1, W - 1, (H - 1) * W}               # first, last, the other two corners
    must |= {W * y for y in range(0, H, 37)} | {W * y + W - 1 for y in range(0, H, 41)} | set(range(0, W, 29)) | set(range((H - 1) * W, H * W, 31))
    g = torch.Generator().manual_seed(7)
    pick = set(must)
    for i in torch.randperm(qr.numel(), generator=g).tolist():
        if len(pick) >= 2048:
            break
        pick.add(i)
    idx = torch.tensor(sorted(pick), device="cuda")
    assert idx.numel() == 2048 and must <= pick
    sel = qr[idx]
    _check(o[sel], _reference(q, k, v, bv, Hp, Wp, C, sel, chunk=256), v, Hp, Wp)


@pytest.mark.parametrize("C", [384, 512])
def test_fused_attention_ignores_border_keys_and_repeats_bit_identically(C):
    """Border keys contribute nothing: K, V (and Q) rows on the border poisoned with NaN / 1e30 leave every valid output bit-identical; two
    calls give bit-identical output; O may be Q itself."""
    Hp, Wp = 45, 67
    q, k, v, bv, border = _inputs(Hp, Wp, C, seed=C)
    o1 = torch.empty_like(q)
    _run(q, k, v, bv, o1, Hp, Wp, C)
    o2 = torch.empty_like(q)
    _run(q, k, v, bv, o2, Hp, Wp, C)
    qr = _valid_rows(Hp, Wp)
    assert torch.equal(o1[qr], o2[qr])
    qp, kp, vp = q.clone(), k.clone(), v.clone()
    qp[border] = float("nan")
    kp[border] = 1e30
    vp[border] = float("nan")
    o3 = torch.empty_like(q)
    _run(qp, kp, vp, bv, o3, Hp, Wp, C)
    assert torch.equal(o3[qr], o1[qr])
    qa = q.clone()
    _run(qa, k, v, bv, qa, Hp, Wp, C)                                # in place: O = Q
    assert torch.equal(qa[qr], o1[qr])
    o4 = torch.empty_like(q)
    _run(q, k, v, None, o4, Hp, Wp, C)                               # no bias
    _check(o4[qr], _reference(q, k, v, None, Hp, Wp, C, qr), v, Hp, Wp)


def test_fused_attention_rejects_bad_arguments_without_a_launch():
    h = _lib.lib()
    t = torch.zeros(9, 512, dtype=torch.bfloat16, device="cuda")
    P = t.data_ptr()
    torch.cuda.synchronize()
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 3, 3, 256, 0.05, None) < 0
    assert h.rgn_vae_attention_bf16(P + 2, P, P, None, P, 3, 3, 512, 0.05, None) < 0
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 2, 3, 512, 0.05, None) < 0
    torch.cuda.synchronize()


# -- the VAEs above the materialised path's limit ------------------------------------------------------------------------------------------

class _ChunkedAttention(host_vae.Attention):
    """host_vae's mid-block attention with the softmax taken in query chunks (same fp32 arithmetic per row, no [hw, hw] matrix)."""

    def forward(self, x):
        b, c, h, w = x.shape
        t = self.group_norm(x).view(b, c, h * w).transpose(1, 2)
        q, k, v = self.to_q(t), self.to_k(t), self.to_v(t)
        o = torch.cat([torch.softmax(q[:, i:i + 2048] @ k.transpose(1, 2) / (c ** 0.5), dim=-1) @ v for i in range(0, h * w, 2048)], dim=1)
        return x + self.to_out[0](o).transpose(1, 2).reshape(b, c, h, w)


def _chunked(m):
    for part in (m.decoder, m.encoder):
        part.mid_block.attentions[0].__class__ = _ChunkedAttention
    return m


@pytest.fixture(scope="module")
def kl():
    return _chunked(host_vae.seeded(11))


@pytest.fixture(scope="module")
def kl_pair(kl):
    return V.HipVaeDecoder(kl.state_dict(), "cuda"), V.HipVaeEncoder(kl.state_dict(), "cuda")


def _pool_bytes(obj):
    return sum(img.storage.numel() * 2 for lst in obj.pool.free.values() for img in lst)


@pytest.mark.parametrize("h", [160, 256])
def test_decoder_above_the_old_limit_vs_fp32_module(kl, kl_pair, h):
    """1280 x 1280 (162^2 = 26244 mid-block rows > 24576: raised before) and 2048 x 2048: >= 40 dB against the fp32 module.  At 2048^2 the
    decode allocates no score matrix: `_attn_buf` stays empty and the peak allocation exceeds the decoder's pooled images by < 1 GB (an S
    would take 8.9 GB)."""
    dec, _ = kl_pair
    z = torch.randn(1, 16, h, h, generator=torch.Generator().manual_seed(h))
    ref = _fp32_on_cpu(lambda: kl.decoder(z.bfloat16().float()))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pooled = _pool_bytes(dec)
    img = dec.decode(z.cuda())
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert img.shape == (1, 3, 8 * h, 8 * h) and torch.isfinite(img.float()).all()
    assert dec._attn_buf == {}
    grown = _pool_bytes(dec) - pooled
    assert peak - grown < 2 ** 30, (peak, grown)
    p = _psnr(img, ref)
    print(f"[vae] decode {8 * h} x {8 * h}: HIP (fused attention) vs fp32 module {p:.1f} dB; peak {peak / 2 ** 30:.2f} GiB, pool {grown / 2 ** 30:.2f} GiB")
    assert p >= 40.0, p


@pytest.mark.parametrize("H", [1280, 2048])
def test_encoder_above_the_old_limit_vs_fp32_module(kl, kl_pair, H):
    _, enc = kl_pair
    x = torch.randn(1, 3, H, H, generator=torch.Generator().manual_seed(H)).clamp(-1, 1)
    ref = _fp32_on_cpu(lambda: kl.encoder(x.bfloat16().float()))
    got = enc.encode(x.cuda())
    torch.cuda.synchronize()
    assert got.shape == (1, 32, H // 8, H // 8) and torch.isfinite(got.float()).all()
    assert enc._attn_buf == {}
    p = _psnr(got, ref)
    print(f"[vae] encode {H} x {H}: HIP (fused attention) vs fp32 module {p:.1f} dB")
    assert p >= 40.0, p


def test_auto_is_the_materialized_path_at_1024_and_fused_is_close():
    """Where the materialised path runs, "auto" keeps it (bit-identical output); "fused" is >= 50 dB against it."""
    m = host_vae.seeded(3)
    dec = V.HipVaeDecoder(m.state_dict(), "cuda")
    z = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    auto = dec.decode(z)
    dec.attention = "materialized"
    mat = dec.decode(z)
    dec.attention = "fused"
    fused = dec.decode(z)
    torch.cuda.synchronize()
    assert torch.equal(auto, mat)
    p = _psnr(fused, mat)
    print(f"[vae] decode 1024 x 1024: fused vs materialised attention {p:.1f} dB")
    assert p >= 50.0, p


def test_a_warm_decode_above_the_old_limit_dispatches_only_libregione_hip_kernels(kl_pair):
    from tests.test_gpu_no_eager_kernels import _foreign, _gpu_activity_names
    dec, _ = kl_pair
    z = torch.randn(1, 16, 160, 160).to("cuda", torch.bfloat16)
    dec.decode(z)
    torch.cuda.synchronize()
    img, names = _gpu_activity_names(lambda: dec.decode(z))
    assert any("vae_attention_kernel" in n for n in names) and not any("softmax_rows" in n for n in names), names
    assert _foreign(names) == [], _foreign(names)
    assert img.shape == (1, 3, 1280, 1280)


def test_qwen_vae_above_the_old_limit_vs_3d_module():
    """HipQwenVaeDecoder / Encoder at latent 160 (1280 x 1280: refused before) against the fp32 stand-in's 2-D form."""
    m = HQ.seeded(4)
    sd = m.state_dict()
    dec, enc = Q.HipQwenVaeDecoder(sd, "cuda"), Q.HipQwenVaeEncoder(sd, "cuda")
    z = torch.randn(1, 16, 1, 160, 160, generator=torch.Generator().manual_seed(160))
    ref = _fp32_on_cpu(lambda: HQ.decode2d(m, z[:, :, 0].bfloat16().float()))
    img = dec.decode(z.cuda())
    torch.cuda.synchronize()
    assert img.shape == (1, 3, 1, 1280, 1280) and dec._attn_buf == {}
    p = _psnr(img[:, :, 0], ref)
    print(f"[qwen vae] decode 1280 x 1280: {p:.1f} dB")
    assert p >= 40.0, p
    x = torch.randn(1, 3, 1, 1280, 1280, generator=torch.Generator().manual_seed(1280)).clamp(-1, 1)
    ref = _fp32_on_cpu(lambda: HQ.encode2d(m, x[:, :, 0].bfloat16().float()))
    got = enc.encode(x.cuda())
    torch.cuda.synchronize()
    assert enc._attn_buf == {}
    p = _psnr(got[:, :, 0], ref)
    print(f"[qwen vae] encode 1280 x 1280: {p:.1f} dB")
    assert p >= 40.0, p


@pytest.mark.parametrize("size", [1280, 2048])
def test_step1x_hosted_edit_above_the_old_limit_runs_on_the_hip_vae(size):
    """A hosted Step1X-Edit pipeline (AutoencoderKL stand-in) with an input image above the old limit: encode and decode run on the HIP
    kernels, the host module's methods are never entered, and the image is >= 40 dB against the host module's fp32 decode of the same
    latents.  2048 x 2048 is what `size_level=2048` hands the VAE (the stand-in's encode_image ignores size_level: the image size carries it)."""
    from regione_amd import vae as V

    class KL(host_vae.AutoencoderKLStandIn):
        dtype = torch.float32
        config = HS.Vae.config
        n = 0

        def decode(self, z, return_dict=True):
            KL.n += 1
            return super().decode(z, return_dict=return_dict)

        def encode(self, x, return_dict=True):
            KL.n += 1
            return super().encode(x, return_dict=return_dict)

    seen = {}

    class Step1XEditPipeline(HS.Step1XEditPipeline):             # RegionEHelper dispatches on the class NAME
        def _latents(self, image, dtype, generator, latents):
            z = self.vae.encode(image).latent_dist.mode()
            image_latents = self._pack_latents(z.float().cpu()).to(dtype)
            if latents is None:
                latents = torch.randn(image_latents.shape, generator=generator).to(dtype)
            return latents, image_latents

    torch.manual_seed(12)
    trunk = HS.stub_trunk("step1x")
    pipe = Step1XEditPipeline(trunk)
    object.__setattr__(trunk, "connector", HS.ToyConnector().to(torch.bfloat16))
    pipe.vae = _chunked(KL().eval())
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    img = torch.rand(1, 3, size, size, generator=torch.Generator().manual_seed(size))
    hv = None
    try:
        from regione_amd import adapters as A
        orig = V.HipVaeDecoder.decode

        def spy(self, z):
            seen["z"] = z.detach().clone()
            return orig(self, z)
        V.HipVaeDecoder.decode = spy
        try:
            out = pipe(image=img, prompt="turn the sky green", generator=torch.Generator().manual_seed(0), output_type="pt", latents=None)
        finally:
            V.HipVaeDecoder.decode = orig
        hv = A.hip_vae_for(pipe, torch.device("cuda", 0))
    finally:
        helper.disable()
    assert tuple(out.images.shape) == (1, 3, size, size) and torch.isfinite(out.images.float()).all()
    assert isinstance(hv, V.HipVaeDecoder) and isinstance(pipe._regione_hip_vae_encoder, V.HipVaeEncoder) and KL.n == 0
    assert hv._attn_buf == {} and pipe._regione_hip_vae_encoder._attn_buf == {}
    z = seen["z"]
    assert z.shape[-1] == size // 8
    ref = _fp32_on_cpu(lambda: pipe.vae.decoder(z.float().cpu()))
    got = hv.decode(z)
    torch.cuda.synchronize()
    p = _psnr(got, ref)
    print(f"[vae] hosted Step1X-Edit {size} x {size}: HIP decode vs host module fp32 {p:.1f} dB")
    assert p >= 40.0, p
