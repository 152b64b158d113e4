"""-m gpu: the FLUX.1-Kontext text encoders on the HIP kernels (regione_amd/text_encoders.py, csrc/text.hip).

  * rgn_text_attention_bf16 against an fp32 torch softmax(s Q K^T + bias, causal) V, L in {1, 7, 77, 129, 512, 1000}, H in {1, 12, 64},
    bias and causal each on and off; a repeated call is bit-identical;
  * the row kernels against torch (bit-equal where the op sequence allows it);
  * whole encoders against the genuine transformers modules in fp32: tiny configs and full-size CLIP-L / T5-XXL (seeded init on the
    device) - HIP's PSNR is at most 1 dB below the eager bf16 module's, and at least 35 dB;
  * a warm call dispatches only rgn:: kernels;
  * a hosted FLUX-Kontext edit runs encode_prompt on the HIP encoders (tests/host_text_pipeline.py).
"""
import copy
import math
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel  # noqa: E402

from regione_amd import _lib, ops  # noqa: E402
from regione_amd import text_encoders as TE  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


# ---- attention --------------------------------------------------------------------------------------------------------------------
def _attention_ref(qkv, L, H, scale, causal, table, Lmax):
    x = qkv.float().view(L, 3, H, 64).permute(1, 2, 0, 3)                   # [3, H, L, 64]
    s = scale * x[0] @ x[1].transpose(1, 2)
    if table is not None:
        i = torch.arange(L, device=qkv.device)[:, None]
        j = torch.arange(L, device=qkv.device)[None, :]
        s = s + table.float()[:, j - i + Lmax - 1]
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ x[2]).permute(1, 0, 2).reshape(L, H * 64)


def _attention(qkv, L, H, scale, causal, table, Lmax):
    o = torch.empty(L, H * 64, dtype=torch.bfloat16, device=qkv.device)
    rc = _lib.lib().rgn_text_attention_bf16(_p(qkv), _p(o), L, H, scale, int(causal), _p(table), Lmax, _stream())
    _lib.check(rc, "rgn_text_attention_bf16")
    return o


@pytest.mark.parametrize("H", [1, 12, 64])
@pytest.mark.parametrize("L", [1, 7, 77, 129, 512, 1000])
def test_text_attention_matches_fp32_softmax(L, H):
    g = torch.Generator(device="cuda").manual_seed(L * 131 + H)
    qkv = torch.randn(L, 3 * H * 64, device="cuda", generator=g).bfloat16()
    Lmax = max(L, 512) + 3
    table = (2.0 * torch.randn(H, 2 * Lmax - 1, device="cuda", generator=g)).bfloat16()
    for bias in (False, True):
        for causal in (False, True):
            scale = 0.125 if causal else 0.35
            tb = table if bias else None
            got = _attention(qkv, L, H, scale, causal, tb, Lmax)
            ref = _attention_ref(qkv, L, H, scale, causal, tb, Lmax)
            err = float((got.float() - ref).abs().max())
            assert err <= 2e-2, (L, H, bias, causal, err)
            assert psnr(got, ref) >= 40.0, (L, H, bias, causal, psnr(got, ref))
            again = _attention(qkv, L, H, scale, causal, tb, Lmax)
            assert torch.equal(got, again), "a repeated call must be bit-identical"


# ---- row kernels ------------------------------------------------------------------------------------------------------------------
def _ulp_close(got, want, frac=0.999):
    """Equal to torch's bf16 result except, rarely, by one bf16 ulp (an fp32 reduction order / transcendental of another library)."""
    a, b = got.view(torch.int16).int(), want.view(torch.int16).int()
    d = (a - b).abs()
    assert int(d.max()) <= 1, int(d.max())
    assert float((d == 0).float().mean()) >= frac


def test_row_kernels_follow_the_eager_bf16_ops():
    """Against torch's eager ops on the same device.  The independent check - every bf16 input, fp64 intervals, exact probes, the second
    pass of the grid-stride loops - is tests/test_gpu_encoder_rows.py."""
    from transformers.activations import ACT2FN
    g = torch.Generator(device="cuda").manual_seed(7)
    lib = _lib.lib()
    # geglu: bf16(gelu_half * linear_half) - one rounding, bit-equal
    M, F = 37, 264
    x = torch.randn(M, 2 * F + 8, device="cuda", generator=g).bfloat16()
    y = torch.empty(M, F, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.rgn_geglu_bf16(_p(x), x.stride(0), _p(y), F, M, F, _stream()), "geglu")
    assert torch.equal(y, x[:, F:2 * F] * x[:, :F])
    # quick_gelu: the module of transformers on bf16
    x = (3 * torch.randn(4099, device="cuda", generator=g)).bfloat16()
    y = torch.empty_like(x)
    _lib.check(lib.rgn_quick_gelu_bf16(_p(x), _p(y), x.numel(), _stream()), "quick_gelu")
    _ulp_close(y, ACT2FN["quick_gelu"](x))
    # affine LayerNorm: nn.LayerNorm on bf16
    for d in (64, 768, 1000):
        x = (torch.randn(50, d, device="cuda", generator=g) * 3 + 1).bfloat16()
        ln = torch.nn.LayerNorm(d, eps=1e-5).cuda().bfloat16()
        with torch.no_grad():
            ln.weight.copy_(1 + 0.3 * torch.randn(d, device="cuda", generator=g))
            ln.bias.copy_(0.3 * torch.randn(d, device="cuda", generator=g))
            want = ln(x)
        y = torch.empty_like(x)
        _lib.check(lib.rgn_layer_norm_rows(_p(x), d, _p(ln.weight), _p(ln.bias), _p(y), d, 50, d, 1e-5, _stream()), "layer_norm_rows")
        _ulp_close(y, want, 0.99)
    # embedding gather (+ position row); ids out of range give zero rows
    vocab, d, L = 300, 128, 77
    tok = torch.randn(vocab, d, device="cuda", generator=g).bfloat16()
    pos = torch.randn(L, d, device="cuda", generator=g).bfloat16()
    ids = torch.randint(0, vocab, (L,), device="cuda", generator=g)
    ids[3], ids[10], ids[20] = -1, vocab, 1 << 40
    for P in (None, pos):
        y = torch.full((L, d), 7.0, dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.rgn_text_embed(_p(ids), L, _p(tok), vocab, _p(P), 0 if P is None else L, _p(y), d, _stream()), "text_embed")
        ok = (ids >= 0) & (ids < vocab)
        want = tok[ids.clamp(0, vocab - 1)]
        if P is not None:
            want = want + P
        want = torch.where(ok[:, None], want, torch.zeros_like(want))
        assert torch.equal(y, want)
    # pooled row
    x = torch.randn(L, d, device="cuda", generator=g).bfloat16()
    for eos in (2, 299, 5000):
        ids = torch.randint(3, 290, (L,), device="cuda", generator=g)
        ids[30], ids[40], ids[50] = 299, 299, 295
        out = torch.empty(d, dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.rgn_text_pool_row(_p(ids), L, eos, _p(x), d, d, _p(out), _stream()), "text_pool_row")
        assert torch.equal(out, x[TE.pooled_index(ids[None], eos)[0]])


# ---- whole encoders ---------------------------------------------------------------------------------------------------------------
def _parity(make_fp32, ids, run_keys):
    """fp32 module on the device, its bf16 copy, the HIP adoption of that copy: PSNR of bf16 eager and of HIP against fp32."""
    torch.manual_seed(0)
    with torch.device("cuda"):
        ref = make_fp32().eval()
    bf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = TE.HipClipTextModel(bf) if isinstance(ref, CLIPTextModel) else TE.HipT5EncoderModel(bf, max_length=max(512, ids.shape[1]))
    with torch.no_grad():
        r, e = ref(ids), bf(ids)
    h = hip(ids, output_hidden_states=False)
    res = {}
    for k in run_keys:
        pe, ph = psnr(getattr(e, k), getattr(r, k)), psnr(getattr(h, k), getattr(r, k))
        print(f"{type(ref).__name__} {k}: HIP {ph:.2f} dB, eager bf16 {pe:.2f} dB against fp32")
        assert ph >= 35.0 and ph >= pe - 1.0, (k, ph, pe)
        res[k] = (ph, pe)
    del ref, bf, hip
    torch.cuda.empty_cache()
    return res


def _clip_ids(L, vocab, eos_id, n_words, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((1, L), eos_id, dtype=torch.int64)
    ids[0, 0] = eos_id - 1
    ids[0, 1:1 + n_words] = torch.randint(3, eos_id - 2, (n_words,), generator=g)
    return ids.cuda()


@pytest.mark.parametrize("eos", [2, 999])
def test_tiny_clip_matches_the_genuine_module(eos):
    cfg = CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                         max_position_embeddings=77, bos_token_id=998, eos_token_id=eos, pad_token_id=999)
    _parity(lambda: CLIPTextModel(cfg), _clip_ids(77, 1000, 999, 11, 1), ("last_hidden_state", "pooler_output"))


@pytest.mark.parametrize("L", [1, 40, 129])
def test_tiny_t5_matches_the_genuine_module(L):
    cfg = T5Config(vocab_size=500, d_model=256, d_kv=64, d_ff=640, num_layers=3, num_heads=4, feed_forward_proj="gated-gelu",
                   is_encoder_decoder=False)
    ids = torch.randint(0, 500, (1, L), generator=torch.Generator().manual_seed(L)).cuda()
    _parity(lambda: T5EncoderModel(cfg), ids, ("last_hidden_state",))


def test_full_size_clip_l_matches_the_genuine_module():
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                         max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=49406, eos_token_id=2,
                         pad_token_id=1, projection_dim=768)
    _parity(lambda: CLIPTextModel(cfg), _clip_ids(77, 49408, 49407, 14, 2), ("last_hidden_state", "pooler_output"))


def test_full_size_t5_xxl_matches_the_genuine_module():
    cfg = T5Config(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu",
                   relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6,
                   is_encoder_decoder=False)
    g = torch.Generator().manual_seed(4)
    ids = torch.zeros(1, 512, dtype=torch.int64)
    ids[0, :40] = torch.randint(3, 32100, (40,), generator=g)
    ids[0, 40] = 1                                                            # </s>, then padding 0 as the T5 tokenizer writes it
    _parity(lambda: T5EncoderModel(cfg), ids.cuda(), ("last_hidden_state",))


# ---- kernel-only dispatch ---------------------------------------------------------------------------------------------------------
def test_a_warm_call_dispatches_only_libregione_hip_kernels():
    from torch.profiler import ProfilerActivity, profile
    import host_text_pipeline as HT
    clip, t5 = HT.tiny_text_encoders()
    hc, ht = TE.HipClipTextModel(clip, "cuda"), TE.HipT5EncoderModel(t5, "cuda")
    ids_c = torch.randint(3, 990, (1, 77), device="cuda")
    ids_t = torch.randint(3, 990, (1, 512), device="cuda")
    hc(ids_c), ht(ids_t)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        a, b = hc(ids_c), ht(ids_t)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    assert any("text_attention_kernel" in n for n in names) and any("gemm" in n for n in names)
    assert torch.isfinite(a.pooler_output.float()).all() and torch.isfinite(b.last_hidden_state.float()).all()


def test_buffers_are_kept_for_the_last_length_only():
    import host_text_pipeline as HT
    _, t5 = HT.tiny_text_encoders()
    ht = TE.HipT5EncoderModel(t5, "cuda")
    ids = torch.randint(3, 990, (1, 100), device="cuda")
    first = ht(ids).last_hidden_state
    for L in (30, 60, 512, 100):
        ht(torch.randint(3, 990, (1, L), device="cuda"))
        assert ht.buf.L == L and all(t.shape[0] == L for t in ht.buf.t.values())
    assert torch.equal(ht(ids).last_hidden_state, first)                      # a new length does not disturb the result of another
    assert first.data_ptr() != ht(ids).last_hidden_state.data_ptr()           # outputs are fresh tensors (the caller keeps them)


# ---- the hosted pipeline ----------------------------------------------------------------------------------------------------------
def _picture(h=256, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g)


def _fallback_warnings(rec):
    return [str(r.message) for r in rec if "kept on the host module" in str(r.message)]


def test_hosted_flux_edit_encodes_prompts_on_the_hip_encoders():
    import host_standins as HS
    import host_text_pipeline as HT
    from regione_amd import RegionEHelper
    clip, t5 = HT.tiny_text_encoders()
    fired = []
    for m in (clip, t5):
        m.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe = HT.FluxKontextPipeline(HS.stub_trunk("flux"), clip, t5)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
    assert _fallback_warnings(rec) == []
    hc, ht = pipe._regione_hip_text
    assert isinstance(hc, TE.HipClipTextModel) and isinstance(ht, TE.HipT5EncoderModel)
    kw = dict(image=_picture(), prompt="make the square red", negative_prompt="blurry", true_cfg_scale=2.0, guidance_scale=2.5,
              preferred_resolutions=[(256, 256)], max_sequence_length=32, output_type="latent")
    lat = pipe(generator=torch.Generator().manual_seed(1), **kw).images
    assert fired == [] and torch.isfinite(lat.float()).all()
    assert pipe.text_encoder is clip and pipe.text_encoder_2 is t5                # bindings restored
    assert len(pipe.encoded) == 2                                                  # positive and negative prompt
    for (pe, pooled), prompt in zip(pipe.encoded, ("make the square red", "blurry")):
        he, hp, _ = pipe.encode_prompt(prompt=prompt, device=torch.device("cpu"), max_sequence_length=32)
        assert pe.shape == he.shape == (1, 32, 256) and pooled.shape == hp.shape == (1, 64) and pe.dtype == torch.bfloat16
        print(f"hosted encode_prompt {prompt!r}: prompt_embeds {psnr(pe, he):.1f} dB, pooled {psnr(pooled, hp):.1f} dB")
        assert psnr(pe, he) >= 40.0 and psnr(pooled, hp) >= 40.0
    assert len(fired) == 4                                                         # the host-encoded references ran on the modules
    helper.disable()


def test_hosted_flux_fallbacks_keep_the_host_module_and_warn_once():
    import host_standins as HS
    import host_text_pipeline as HT
    from regione_amd import RegionEHelper
    clip, t5 = HT.tiny_text_encoders(clip_kw=dict(hidden_act="gelu"))
    fired = []
    for m in (clip, t5):
        m.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe = HT.FluxKontextPipeline(HS.stub_trunk("flux"), clip, t5)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with pytest.warns(RuntimeWarning, match="text_encoder kept on the host module: hidden_act 'gelu'"):
        helper.enable()
    kw = dict(image=_picture(), prompt="make the square red", guidance_scale=2.5, preferred_resolutions=[(256, 256)],
              max_sequence_length=32, output_type="latent")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(2):
            pipe(generator=torch.Generator().manual_seed(1), **kw)
    assert _fallback_warnings(rec) == []                                          # decided once, at enable()
    assert fired == ["CLIPTextModel", "CLIPTextModel"]                              # CLIP on the host, T5 on the HIP kernels
    helper.disable()
    # switched off on purpose: both host modules, no warning
    clip2, t52 = HT.tiny_text_encoders()
    fired.clear()
    for m in (clip2, t52):
        m.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe2 = HT.FluxKontextPipeline(HS.stub_trunk("flux"), clip2, t52)
    pipe2._regione_hip_text = False
    helper2 = RegionEHelper(pipe2)
    helper2.set_params(threshold=0.5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper2.enable()
        pipe2(generator=torch.Generator().manual_seed(1), **kw)
    assert _fallback_warnings(rec) == []
    assert sorted(fired) == ["CLIPTextModel", "T5EncoderModel"]
    helper2.disable()
