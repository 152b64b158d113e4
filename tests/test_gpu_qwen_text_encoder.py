"""-m gpu: the language model of the Qwen2.5-VL prompt encoder on the HIP kernels (regione_amd/qwen_text_encoder.py, csrc/text.hip; SURVEY.md
section 8 row f4).

  * rgn_lm_attention_bf16 against an fp32 torch softmax(causal(s Q K^T)) V with the KV heads repeated, L in {1, 7, 129, 512, 1500, 4096},
    (Hq, Hkv) in {(2, 1), (4, 4), (28, 4)}: max abs error 2e-2 and PSNR >= 40 dB on N(0, 1) inputs (the bounds of the head-64 kernel's
    test, same arithmetic); a repeated call is bit-identical; a changed key j > i leaves row i bit-identical;
  * rgn_mrope_bf16 bit-equal to torch's bf16 op sequence, V columns untouched; rgn_swiglu_bf16 within one bf16 ulp, rarely (the
    quick_gelu check of test_gpu_text_encoders.py, fraction 0.999);
  * the whole model against the genuine transformers module in fp32 (the `_parity` protocol of test_gpu_text_encoders.py): HIP's PSNR at
    most 1 dB below the eager bf16 module's; tiny configs also >= 35 dB; one full-size language model at L = 1500;
  * a warm text-only call dispatches only rgn:: kernels; the hosted Edit / Edit-Plus pipelines encode both prompts on the HIP class.
"""
import copy
import math
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


# ---- attention --------------------------------------------------------------------------------------------------------------------
def _attention_ref(qkv, L, Hq, Hkv, scale):
    x = qkv.float()
    q = x[:, :Hq * 128].view(L, Hq, 128).transpose(0, 1)
    k = x[:, Hq * 128:(Hq + Hkv) * 128].view(L, Hkv, 128).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    v = x[:, (Hq + Hkv) * 128:].view(L, Hkv, 128).transpose(0, 1).repeat_interleave(Hq // Hkv, dim=0)
    out = torch.empty(Hq, L, 128, device=qkv.device)
    mask = torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1)
    for h in range(Hq):                                                       # per head: [L, L] fp32 scores, not [Hq, L, L]
        s = (scale * q[h] @ k[h].T).masked_fill(mask, float("-inf"))
        out[h] = torch.softmax(s, -1) @ v[h]
    return out.transpose(0, 1).reshape(L, Hq * 128)


def _attention(qkv, L, Hq, Hkv, scale):
    o = torch.empty(L, Hq * 128, dtype=torch.bfloat16, device=qkv.device)
    _lib.check(_lib.lib().rgn_lm_attention_bf16(_p(qkv), _p(o), L, Hq, Hkv, scale, _stream()), "rgn_lm_attention_bf16")
    return o


@pytest.mark.parametrize("heads", [(2, 1), (4, 4), (28, 4)])
@pytest.mark.parametrize("L", [1, 7, 129, 512, 1500, 4096])
def test_lm_attention_matches_fp32_softmax(L, heads):
    Hq, Hkv = heads
    g = torch.Generator(device="cuda").manual_seed(L * 131 + Hq)
    qkv = torch.randn(L, (Hq + 2 * Hkv) * 128, device="cuda", generator=g).bfloat16()
    scale = 128 ** -0.5
    got = _attention(qkv, L, Hq, Hkv, scale)
    ref = _attention_ref(qkv, L, Hq, Hkv, scale)
    err, p = float((got.float() - ref).abs().max()), psnr(got, ref)
    print(f"lm_attention L={L} Hq={Hq} Hkv={Hkv}: max abs err {err:.3e}, PSNR {p:.2f} dB")
    assert err <= 2e-2, (L, heads, err)
    assert p >= 40.0, (L, heads, p)
    assert torch.equal(got, _attention(qkv, L, Hq, Hkv, scale)), "a repeated call must be bit-identical"


@pytest.mark.parametrize("L,i", [(7, 3), (129, 63), (129, 64), (512, 31), (1500, 1000)])
def test_lm_attention_is_causal_bit_for_bit(L, i):
    """Keys and values after position i are replaced: rows <= i of the output must not change by a bit."""
    Hq, Hkv = 4, 2
    g = torch.Generator(device="cuda").manual_seed(L + i)
    qkv = torch.randn(L, (Hq + 2 * Hkv) * 128, device="cuda", generator=g).bfloat16()
    base = _attention(qkv, L, Hq, Hkv, 0.09)
    other = qkv.clone()
    other[i + 1:, Hq * 128:] = (5 * torch.randn(L - i - 1, 2 * Hkv * 128, device="cuda", generator=g)).bfloat16()
    got = _attention(other, L, Hq, Hkv, 0.09)
    assert torch.equal(got[:i + 1], base[:i + 1])
    assert not torch.equal(got[i + 1:], base[i + 1:])


# ---- row kernels ------------------------------------------------------------------------------------------------------------------
def _ulp_close(got, want, frac=0.999):
    """Equal to torch's bf16 result except, rarely, by one bf16 ulp (a transcendental of another library)."""
    a, b = got.view(torch.int16).int(), want.view(torch.int16).int()
    d = (a - b).abs()
    assert int(d.max()) <= 1, int(d.max())
    assert float((d == 0).float().mean()) >= frac, float((d == 0).float().mean())


@pytest.mark.parametrize("L,Hq,Hkv", [(1, 2, 1), (77, 4, 4), (300, 28, 4)])
def test_mrope_is_bit_equal_to_the_eager_bf16_ops(L, Hq, Hkv):
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import apply_multimodal_rotary_pos_emb
    g = torch.Generator(device="cuda").manual_seed(L)
    ld = (Hq + 2 * Hkv) * 128
    qkv = (2 * torch.randn(L, ld, device="cuda", generator=g)).bfloat16()
    pos = torch.randint(0, 3000, (3, 1, L))
    inv = QT.default_inv_freq(HQ.tiny_qwen25vl().config)
    tab = QT.mrope_tables(inv, pos, [16, 24, 24]).cuda()                       # [2, 1, L, 128], the selection already applied
    # the eager call with UNSELECTED tables [3, 1, L, 128] of which every position axis carries the selected one: the same values
    cos3, sin3 = tab[0].expand(3, -1, -1, -1), tab[1].expand(3, -1, -1, -1)
    q = qkv[:, :Hq * 128].view(1, L, Hq, 128).transpose(1, 2)
    k = qkv[:, Hq * 128:(Hq + Hkv) * 128].view(1, L, Hkv, 128).transpose(1, 2)
    qe, ke = apply_multimodal_rotary_pos_emb(q, k, cos3, sin3, [16, 24, 24])
    want = torch.cat([qe.transpose(1, 2).reshape(L, -1), ke.transpose(1, 2).reshape(L, -1), qkv[:, (Hq + Hkv) * 128:]], dim=1)
    got = qkv.clone()
    rc = _lib.lib().rgn_mrope_bf16(_p(got), ld, _p(tab[0, 0]), _p(tab[1, 0]), L, Hq, Hkv, _stream())
    _lib.check(rc, "rgn_mrope_bf16")
    assert torch.equal(got[:, (Hq + Hkv) * 128:], qkv[:, (Hq + Hkv) * 128:]), "V columns must be untouched"
    assert torch.equal(got, want)
    assert not torch.equal(got[:, :Hq * 128], qkv[:, :Hq * 128]) or L == 1


def test_swiglu_follows_the_eager_bf16_ops():
    from transformers.activations import ACT2FN
    g = torch.Generator(device="cuda").manual_seed(9)
    M, F = 131, 1096
    x = (3 * torch.randn(M, 2 * F + 8, device="cuda", generator=g)).bfloat16()
    y = torch.empty(M, F + 8, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_swiglu_bf16(_p(x), x.stride(0), _p(y), y.stride(0), M, F, _stream()), "rgn_swiglu_bf16")
    _ulp_close(y[:, :F], ACT2FN["silu"](x[:, :F]) * x[:, F:2 * F])


# ---- whole model ------------------------------------------------------------------------------------------------------------------
def _parity(ref, inputs, floor=35.0, max_length=4096):
    """`_parity` of test_gpu_text_encoders.py: the fp32 module on the device, its bf16 copy, the HIP adoption of that copy; PSNR of
    eager bf16 and of HIP against fp32 over the valid positions of `hidden_states[-1]`."""
    bf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = QT.HipQwen25VLTextEncoder(bf, max_length=max_length)
    with torch.no_grad():
        r = ref(**inputs, output_hidden_states=True).hidden_states[-1]
        e = bf(**inputs, output_hidden_states=True).hidden_states[-1]
    out = hip(**inputs, output_hidden_states=True)
    h = out.hidden_states[-1]
    assert h.dtype == torch.bfloat16 and h.shape == r.shape and out.last_hidden_state is h
    mask = inputs.get("attention_mask")
    valid = torch.ones(r.shape[:2], dtype=torch.bool, device=r.device) if mask is None else mask.bool()
    if not bool(valid.all()):
        assert float(h[~valid].float().abs().max()) == 0.0                    # padded positions are zero rows
    pe, ph = psnr(e[valid], r[valid]), psnr(h[valid], r[valid])
    print(f"Qwen2.5-VL language model {tuple(r.shape)}: HIP {ph:.2f} dB, eager bf16 {pe:.2f} dB against fp32")
    assert ph >= pe - 1.0, (ph, pe)
    if floor is not None:
        assert ph >= floor, ph
    del bf, hip
    torch.cuda.empty_cache()
    return ph, pe


def _tiny_fp32(layers=3):
    torch.manual_seed(0)
    return HQ.tiny_qwen25vl(dtype=torch.float32, layers=layers).cuda()


def _tiny_inputs(n_images, prompts, with_types):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    plus = n_images > 1
    base = "".join(f"Picture {i + 1}: <image> " if plus else "<image> " for i in range(n_images))
    mi = HQ.ToyProcessor()(text=[base + p for p in prompts], images=images or None).to("cuda")
    kw = dict(input_ids=mi.input_ids, attention_mask=mi.attention_mask)
    if n_images:
        kw.update(pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw)
    if with_types:
        kw["mm_token_type_ids"] = (mi.input_ids == HQ.IMAGE).int()
    return kw


@pytest.mark.parametrize("with_types", [False, True])
@pytest.mark.parametrize("case", ["text", "one_image", "two_images", "batch_of_two"])
def test_tiny_model_matches_the_genuine_module(case, with_types):
    one = ("make the square red and keep the rest of the picture as it is",)
    two = ("make the square red", "replace the sky of the picture with a much darker one and add three birds to it")
    n_images, prompts = {"text": (0, one), "one_image": (1, one), "two_images": (2, one), "batch_of_two": (1, two)}[case]
    kw = _tiny_inputs(n_images, prompts, with_types)
    if case == "batch_of_two":
        assert not bool(kw["attention_mask"].bool().all())                    # right padding in the shorter row
    _parity(_tiny_fp32(), kw)


def test_tiny_model_with_precomputed_image_embeds_and_position_ids():
    """`image_embeds=` instead of `pixel_values` and the caller's own `position_ids`: the same result as the module-driven call."""
    m = HQ.tiny_qwen25vl().cuda()
    hip = QT.HipQwen25VLTextEncoder(m)
    kw = _tiny_inputs(1, ("make the square red",), True)
    want = hip(**kw).last_hidden_state
    with torch.no_grad():
        emb = torch.cat(m.get_image_features(kw["pixel_values"], kw["image_grid_thw"]).pooler_output)
    pos = hip.position_ids_for(kw["input_ids"], kw["attention_mask"], kw["image_grid_thw"], None, kw["mm_token_type_ids"])
    sd_hip = QT.HipQwen25VLTextEncoder(dict(m.state_dict()), "cuda", config=m.config)
    sd_hip.inv_freq = hip.inv_freq                                            # the bf16-rounded buffer of the `.to(bfloat16)` module
    got = sd_hip(kw["input_ids"], attention_mask=kw["attention_mask"], image_embeds=emb, position_ids=pos).last_hidden_state
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="do not match"):
        sd_hip(kw["input_ids"], attention_mask=kw["attention_mask"], image_embeds=emb[:-1], position_ids=pos)


def test_buffers_are_kept_for_the_last_length_only():
    m = HQ.tiny_qwen25vl().cuda()
    hip = QT.HipQwen25VLTextEncoder(m)
    ids = torch.randint(3, 990, (1, 100), device="cuda")
    first = hip(ids).last_hidden_state
    for L in (30, 60, 512, 100):
        hip(torch.randint(3, 990, (1, L), device="cuda"))
        assert hip.buf.L == L and all(t.shape[0] == L for t in hip.buf.t.values())
    again = hip(ids).last_hidden_state
    assert torch.equal(again, first) and again.data_ptr() != first.data_ptr()  # bit-identical, and outputs are fresh tensors


def test_full_size_language_model_matches_the_genuine_module():
    """Qwen2.5-VL-7B's language model (28 layers, d 3584, 28 / 4 heads, intermediate 18944, vocab 152064) with a tiny vision tower, seeded
    init on the device, L = 1500 text-only ids.  No floor is fixed in advance for this depth: HIP must be within 1 dB of eager bf16;
    both values are printed (profiles/r08_qwen_text_encoder_bench.json records those of the bench tool's own `--parity` run)."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    cfg = full_size_config()
    torch.manual_seed(0)
    with torch.device("cuda"):
        ref = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    ids = torch.randint(0, 151000, (1, 1500), generator=torch.Generator().manual_seed(5)).cuda()
    _parity(ref, dict(input_ids=ids, attention_mask=torch.ones_like(ids)), floor=None)


def full_size_config():
    from transformers import Qwen2_5_VLConfig
    t = dict(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28, num_key_value_heads=4,
             rms_norm_eps=1e-6, max_position_embeddings=128000, rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[16, 24, 24]),
             tie_word_embeddings=False)
    v = dict(depth=2, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=3584, patch_size=14, spatial_merge_size=2,
             temporal_patch_size=2, window_size=56, fullatt_block_indexes=[1], in_channels=3)
    return Qwen2_5_VLConfig(text_config=t, vision_config=v)


# ---- kernel-only dispatch ---------------------------------------------------------------------------------------------------------
def test_a_warm_text_only_call_dispatches_only_libregione_hip_kernels():
    from torch.profiler import ProfilerActivity, profile
    m = HQ.tiny_qwen25vl().cuda()
    hip = QT.HipQwen25VLTextEncoder(m)
    kw = _tiny_inputs(0, ("make the square red", "a longer instruction than the first one by some words"), False)
    hip(**kw, output_hidden_states=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        a = hip(**kw, output_hidden_states=True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    assert any("text_attention_kernel" in n for n in names) and any("gemm" in n for n in names)
    assert any("mrope_kernel" in n for n in names) and any("swiglu_kernel" in n for n in names)
    assert torch.isfinite(a.hidden_states[-1].float()).all()


# ---- the hosted pipelines ---------------------------------------------------------------------------------------------------------
def _picture(h=256, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g)


def _fallback_warnings(rec):
    return [str(r.message) for r in rec if "kept on the host module" in str(r.message)]


@pytest.mark.parametrize("plus", [False, True])
def test_hosted_qwen_edit_encodes_both_prompts_on_the_hip_language_model(plus):
    import host_standins as HS
    from regione_amd import RegionEHelper
    m = HQ.tiny_qwen25vl()
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    cls = HQ.QwenImageEditPlusPipeline if plus else HQ.QwenImageEditPipeline
    pipe = cls(HS.stub_trunk("qwen"), m)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
    assert _fallback_warnings(rec) == []
    assert isinstance(pipe._regione_hip_qwen_text, QT.HipQwen25VLTextEncoder)
    image = [_picture(192, 384, seed=2), _picture(256, 256, seed=3)] if plus else _picture()
    prompts = ("put the object of image 1 into image 2" if plus else "add a red hat", "blurry")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        lat = pipe(image=image, prompt=prompts[0], negative_prompt=prompts[1], true_cfg_scale=4.0, generator=torch.Generator().manual_seed(1),
                   output_type="latent").images
    assert _fallback_warnings(rec) == []
    assert fired == [] and torch.isfinite(lat.float()).all()
    assert pipe.text_encoder is m and "text_encoder" in pipe.__dict__               # the binding is undone
    assert len(pipe.encoded) == 2                                                  # positive and negative prompt (true CFG)
    prompt_image = pipe.last_image
    assert (isinstance(prompt_image, list) and len(prompt_image) == 2) if plus else isinstance(prompt_image, torch.Tensor)
    for (pe, pm), prompt in zip(list(pipe.encoded), prompts):
        he, hm = pipe.encode_prompt(image=prompt_image, prompt=prompt, device=torch.device("cpu"))     # the host module, on the CPU
        assert pe.shape == he.shape and pe.shape[2] == 256 and pe.dtype == torch.bfloat16 and torch.equal(pm.cpu(), hm)
        print(f"hosted encode_prompt {prompt!r}: prompt_embeds {tuple(pe.shape)} {psnr(pe.cpu(), he):.1f} dB against the host module")
        assert psnr(pe.cpu(), he) >= 40.0
    assert len(fired) == 2 * len(m.model.language_model.layers)                     # the host-encoded references ran on the module
    helper.disable()


def test_hosted_qwen_with_sliding_window_layers_stays_on_the_host_with_one_warning():
    import host_standins as HS
    from regione_amd import RegionEHelper
    m = HQ.tiny_qwen25vl(text_kw=dict(use_sliding_window=True, sliding_window=4096, max_window_layers=1))
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with pytest.warns(RuntimeWarning, match="text_encoder kept on the host module: sliding-window"):
        helper.enable()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        lat = pipe(image=_picture(), prompt="add a red hat", negative_prompt="blurry", true_cfg_scale=4.0,
                   generator=torch.Generator().manual_seed(1), output_type="latent").images
    assert _fallback_warnings(rec) == []                                          # decided once, at enable()
    assert len(fired) == 2 * len(m.model.language_model.layers) and torch.isfinite(lat.float()).all()
    helper.disable()
