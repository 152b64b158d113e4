"""-m gpu: the vision tower of the Qwen2.5-VL prompt encoder on the HIP kernels (regione_amd/qwen_vision.py, csrc/vision.hip; SURVEY.md
section 8 row f4).

  * rgn_vision_attention_bf16 against an fp32 block-diagonal softmax(s Q K^T) V, Dp in {32, 64, 96, 128}, H in {2, 16}, segment lists with
    one-row, four-row and 64-row-crossing segments: max abs error 2e-2 and PSNR >= 40 dB on N(0, 1) inputs (the bounds of
    test_lm_attention_matches_fp32_softmax, same tile arithmetic); a repeated call is bit-identical; replacing one segment's K and V rows
    changes that segment's output rows only; head width 80 inside Dp = 96 leaves the pad columns exactly 0;
  * rgn_vision_rope_bf16 bit-equal to apply_rotary_pos_emb_vision, V and pad columns untouched; rgn_gelu_erf_bf16 within one bf16 ulp,
    rarely; rgn_cast_pad_rows bit-equal to `.to(bfloat16)` + zero pad;
  * the whole tower against the genuine transformers module in fp32 (the `_parity` protocol of the text-encoder tests): HIP's PSNR at most
    1 dB below the eager bf16 module's; tiny towers also >= 35 dB; one full-size tower at a 28 x 28 grid;
  * the prompt encoder with the tower meets the same bars, and a warm call with an image dispatches only rgn:: kernels; the hosted Edit /
    Edit-Plus pipelines run neither the module's vision blocks nor its language-model layers.
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
from regione_amd import qwen_vision as QV  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream

WINDOWS_18x22 = [64, 64, 48, 64, 64, 48, 16, 16, 12]                              # the window list of an 18 x 22 grid, window 112
SEGMENTS = {"one": [1], "small": [4, 16, 64, 64, 12], "crossing": [60, 70, 3], "long": [777], "windows": None,   # None: of a 28 x 28 grid
            "windows_18x22": WINDOWS_18x22}


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def _segments(name):
    if name != "windows":
        return SEGMENTS[name]
    cfg = _vision_config(**HEAD80)
    cu = QV.vision_tables(cfg, QV.default_inv_freq(cfg), torch.tensor([[1, 28, 28]]))["cu_window_seqlens"].tolist()
    return [b - a for a, b in zip(cu[:-1], cu[1:])]


def _cu(segs):
    cu = [0]
    for s in segs:
        cu.append(cu[-1] + s)
    return cu


# ---- attention --------------------------------------------------------------------------------------------------------------------
def _attention_ref(qkv, cu, H, Dp, D, scale):
    """fp32 block-diagonal softmax(scale Q K^T) V over the first D columns of every head: [L, H, D]."""
    L = qkv.shape[0]
    x = qkv.float().view(L, 3, H, Dp)[..., :D]
    out = torch.empty(L, H, D, device=qkv.device)
    for a, b in zip(cu[:-1], cu[1:]):
        q, k, v = (x[a:b, i].transpose(0, 1) for i in range(3))                   # [H, n, D]
        out[a:b] = (torch.softmax(scale * q @ k.transpose(1, 2), -1) @ v).transpose(0, 1)
    return out


def _attention(qkv, cu, H, Dp, scale, out=None):
    L = qkv.shape[0]
    items = QV.attention_items(cu).cuda()
    o = torch.full((L, H * Dp), float("nan"), dtype=torch.bfloat16, device=qkv.device) if out is None else out
    rc = _lib.lib().rgn_vision_attention_bf16(_p(qkv), _p(o), L, H, Dp, scale, _p(items), items.shape[0], _stream())
    _lib.check(rc, "rgn_vision_attention_bf16")
    return o


@pytest.mark.parametrize("H", [2, 16])
@pytest.mark.parametrize("Dp", [32, 64, 96, 128])
@pytest.mark.parametrize("segs", list(SEGMENTS))
def test_vision_attention_matches_fp32_block_diagonal_softmax(segs, Dp, H):
    cu = _cu(_segments(segs))
    L = cu[-1]
    g = torch.Generator(device="cuda").manual_seed(L * 131 + Dp + H)
    qkv = torch.randn(L, 3 * H * Dp, device="cuda", generator=g).bfloat16()
    scale = Dp ** -0.5
    got = _attention(qkv, cu, H, Dp, scale)
    ref = _attention_ref(qkv, cu, H, Dp, Dp, scale).reshape(L, H * Dp)
    assert torch.isfinite(got.float()).all(), "every row lies in an item and is written"
    err, p = float((got.float() - ref).abs().max()), psnr(got, ref)
    print(f"vision_attention {segs} L={L} Dp={Dp} H={H}: max abs err {err:.3e}, PSNR {p:.2f} dB")
    assert err <= 2e-2, (segs, Dp, H, err)
    assert p >= 40.0, (segs, Dp, H, p)
    assert torch.equal(got, _attention(qkv, cu, H, Dp, scale)), "a repeated call must be bit-identical"


@pytest.mark.parametrize("segs,which", [("small", 0), ("small", 2), ("crossing", 1), ("crossing", 2), ("windows", 5)])
def test_vision_attention_keeps_segments_apart_bit_for_bit(segs, which):
    """K and V rows of one segment are replaced: that segment's output rows change, no other row changes by a bit."""
    H, Dp = 4, 96
    cu = _cu(_segments(segs))
    L, a, b = cu[-1], cu[which], cu[which + 1]
    g = torch.Generator(device="cuda").manual_seed(L + which)
    qkv = torch.randn(L, 3 * H * Dp, device="cuda", generator=g).bfloat16()
    base = _attention(qkv, cu, H, Dp, 0.11)
    other = qkv.clone()
    other[a:b, H * Dp:] = (3 * torch.randn(b - a, 2 * H * Dp, device="cuda", generator=g)).bfloat16()
    got = _attention(other, cu, H, Dp, 0.11)
    assert torch.equal(got[:a], base[:a]) and torch.equal(got[b:], base[b:])
    assert not torch.equal(got[a:b], base[a:b])


@pytest.mark.parametrize("segs", ["small", "crossing", "windows"])
def test_head_width_80_runs_in_96_with_exact_zero_pad_columns(segs):
    H, D, Dp = 16, 80, 96
    cu = _cu(_segments(segs))
    L = cu[-1]
    g = torch.Generator(device="cuda").manual_seed(L + 80)
    x = torch.randn(L, 3, H, Dp, device="cuda", generator=g).bfloat16()
    x[..., D:] = 0                                                                # what zero weight rows and bias entries give
    qkv = x.reshape(L, 3 * H * Dp)
    scale = D ** -0.5
    got = _attention(qkv, cu, H, Dp, scale).view(L, H, Dp)
    assert float(got[..., D:].float().abs().max()) == 0.0
    ref = _attention_ref(qkv, cu, H, Dp, D, scale)
    err, p = float((got[..., :D].float() - ref).abs().max()), psnr(got[..., :D], ref)
    print(f"vision_attention head 80 in 96, {segs}: max abs err {err:.3e}, PSNR {p:.2f} dB")
    assert err <= 2e-2 and p >= 40.0, (err, p)


def test_vision_attention_skips_items_outside_the_buffer():
    """The item table is device data: an item that does not lie inside [0, L) is skipped, the rows of the others are written."""
    H, Dp, L = 2, 32, 40
    qkv = torch.randn(L, 3 * H * Dp, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).bfloat16()
    items = torch.tensor([[0, 20, 0, 20], [20, 64, 20, 84], [-4, 8, 0, 20], [20, 20, 20, 40], [30, 0, 20, 40], [20, 10, 30, 20]],
                         dtype=torch.int32, device="cuda")
    o = torch.zeros(L, H * Dp, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_vision_attention_bf16(_p(qkv), _p(o), L, H, Dp, 0.2, _p(items), items.shape[0], _stream()), "vision_attention")
    assert torch.equal(o, _attention(qkv, [0, 20, 40], H, Dp, 0.2))


# ---- row kernels ------------------------------------------------------------------------------------------------------------------
def _ulp_close(got, want, frac=0.999):
    """Equal to torch's bf16 result except, rarely, by one bf16 ulp (a transcendental of another library)."""
    a, b = got.view(torch.int16).int(), want.view(torch.int16).int()
    d = (a - b).abs()
    assert int(d.max()) <= 1, int(d.max())
    assert float((d == 0).float().mean()) >= frac, float((d == 0).float().mean())


@pytest.mark.parametrize("origin", [torch.bfloat16, torch.float32], ids=["bf16_tables", "fp32_tables"])
@pytest.mark.parametrize("L", [1, 76, 396])
@pytest.mark.parametrize("D", [32, 80])
def test_vision_rope_is_bit_equal_to_the_eager_op(D, L, origin):
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import apply_rotary_pos_emb_vision
    H, Dp = 4, QV.padded_to(D, 32)
    g = torch.Generator(device="cuda").manual_seed(L + D)
    qkv = (2 * torch.randn(L, 3 * H * Dp, device="cuda", generator=g)).bfloat16()
    ang = (torch.rand(L, D // 2, generator=torch.Generator().manual_seed(L)) * 40).to(origin)
    emb = torch.cat((ang, ang), dim=-1)
    cos, sin = emb.cos().cuda(), emb.sin().cuda()                                  # in the tables' own dtype, as the module builds them
    x = qkv.view(L, 3, H, Dp)
    qe, ke = apply_rotary_pos_emb_vision(x[:, 0, :, :D], x[:, 1, :, :D], cos, sin)
    want = x.clone()
    want[:, 0, :, :D], want[:, 1, :, :D] = qe, ke
    got = qkv.clone()
    cf, sf = cos.float().contiguous(), sin.float().contiguous()
    _lib.check(_lib.lib().rgn_vision_rope_bf16(_p(got), got.stride(0), _p(cf), _p(sf), L, H, D, Dp, _stream()), "rgn_vision_rope_bf16")
    gv = got.view(L, 3, H, Dp)
    assert torch.equal(gv[:, 2], x[:, 2]), "V columns must be untouched"
    assert torch.equal(gv[..., D:], x[..., D:]), "pad columns must be untouched"
    assert torch.equal(gv, want)
    assert not torch.equal(gv[:, :2, :, :D], x[:, :2, :, :D])


def test_gelu_erf_follows_nn_gelu():
    g = torch.Generator(device="cuda").manual_seed(4)
    x = (3 * torch.randn(131 * 1096 + 5, device="cuda", generator=g)).bfloat16()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().rgn_gelu_erf_bf16(_p(x), _p(y), x.numel(), _stream()), "rgn_gelu_erf_bf16")
    _ulp_close(y, torch.nn.GELU()(x))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,K,Kp", [(1, 8, 8), (37, 1176, 1216), (300, 27, 64)])
def test_cast_pad_rows_is_the_cast_plus_zero_columns(M, K, Kp, dtype):
    g = torch.Generator(device="cuda").manual_seed(M + K)
    x = (5 * torch.randn(M, K, device="cuda", generator=g)).to(dtype)
    y = torch.full((M, Kp), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_cast_pad_rows(_p(x), ops._dt(x), x.stride(0), _p(y), M, K, Kp, _stream()), "rgn_cast_pad_rows")
    assert torch.equal(y[:, :K], x.to(torch.bfloat16)) and not y[:, K:].any()


# ---- whole tower ------------------------------------------------------------------------------------------------------------------
HEAD80 = dict(depth=4, hidden_size=320, intermediate_size=856, num_heads=4, out_hidden_size=256, window_size=112, fullatt_block_indexes=[1, 3])
FULL = dict(depth=32, hidden_size=1280, intermediate_size=3420, num_heads=16, out_hidden_size=3584, window_size=112,
            fullatt_block_indexes=[7, 15, 23, 31])


def _vision_config(**kw):
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLVisionConfig
    v = dict(depth=2, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=256, patch_size=14, spatial_merge_size=2,
             temporal_patch_size=2, window_size=56, fullatt_block_indexes=[1], in_channels=3)
    v.update(kw)
    return Qwen2_5_VLVisionConfig(**v)


def _tower_fp32(kw, seed=0):
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel
    torch.manual_seed(seed)
    with torch.device("cuda"):
        return Qwen2_5_VisionTransformerPretrainedModel(_vision_config(**kw)).eval()


def _pixels(grid, seed=2):
    N = sum(h * w for _, h, w in grid)
    return torch.randn(N, 1176, generator=torch.Generator().manual_seed(seed)).cuda(), torch.tensor(grid, device="cuda")


def _tower_parity(ref, grid, floor=35.0):
    """The `_parity` protocol: the fp32 module on the device, its bf16 copy, the HIP adoption of that copy; PSNR of eager bf16 and of HIP
    against fp32 on `pooler_output`."""
    bf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = QV.HipQwen25VLVisionTower(bf)
    px, g = _pixels(grid)
    with torch.no_grad():
        r = ref(px, g).pooler_output
        e = bf(px, g).pooler_output
    out = hip(px, g)
    h = out.pooler_output
    assert h.dtype == torch.bfloat16 and h.shape == r.shape and out.last_hidden_state.shape == (px.shape[0], ref.config.hidden_size)
    pe, ph = psnr(e, r), psnr(h, r)
    print(f"Qwen2.5-VL vision tower d={ref.config.hidden_size} grid {grid}: HIP {ph:.2f} dB, eager bf16 {pe:.2f} dB against fp32")
    assert ph >= pe - 1.0, (ph, pe)
    if floor is not None:
        assert ph >= floor, ph
    del bf, hip
    torch.cuda.empty_cache()
    return ph, pe


@pytest.mark.parametrize("grid", [[[1, 4, 4]], [[1, 4, 4], [1, 6, 10]], [[1, 18, 22]]], ids=["4x4", "4x4+6x10", "18x22"])
@pytest.mark.parametrize("kw", [{}, HEAD80], ids=["tiny", "head80"])
def test_tiny_tower_matches_the_genuine_module(kw, grid):
    _tower_parity(_tower_fp32(kw), grid)


def test_full_size_tower_matches_the_genuine_module():
    """Qwen2.5-VL's vision tower (32 blocks, d 1280, 16 heads of 80, MLP 3420, out 3584, window 112, full attention in 7 / 15 / 23 / 31),
    seeded init on the device, a 28 x 28 grid.  No floor is fixed in advance for this depth: HIP must be within 1 dB of eager bf16; both
    values are printed (profiles/r11_qwen_vision_bench.json records those of the bench tool's own `--parity` run)."""
    _tower_parity(_tower_fp32(FULL), [[1, 28, 28]], floor=None)


def test_tables_and_buffers_are_kept_for_the_last_grid_only():
    m = _tower_fp32(HEAD80).to(torch.bfloat16)
    hip = QV.HipQwen25VLVisionTower(m)
    px, g = _pixels([[1, 18, 22]])
    first = hip(px, g)
    px2, g2 = _pixels([[1, 4, 4], [1, 6, 10]], seed=3)
    hip(px2, g2)
    assert hip.buf.L == ((1, 4, 4), (1, 6, 10)) and all(t.shape[0] in (76, 19) for t in hip.buf.t.values())
    assert hip._tab["cos"].shape[0] == 76
    again = hip(px, g)
    for a, b in ((again.pooler_output, first.pooler_output), (again.last_hidden_state, first.last_hidden_state)):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()                  # bit-identical, and outputs are fresh tensors


# ---- the prompt encoder with the tower ------------------------------------------------------------------------------------------------
def _tiny_inputs(n_images, prompts):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    plus = n_images > 1
    base = "".join(f"Picture {i + 1}: <image> " if plus else "<image> " for i in range(n_images))
    mi = HQ.ToyProcessor()(text=[base + p for p in prompts], images=images or None).to("cuda")
    return dict(input_ids=mi.input_ids, attention_mask=mi.attention_mask, pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw)


@pytest.mark.parametrize("case", ["one_image", "two_images", "batch_of_two"])
def test_text_encoder_with_the_hip_tower_matches_the_genuine_module(case):
    one = ("make the square red and keep the rest of the picture as it is",)
    two = ("make the square red", "replace the sky of the picture with a much darker one and add three birds to it")
    n_images, prompts = {"one_image": (1, one), "two_images": (2, one), "batch_of_two": (1, two)}[case]
    kw = _tiny_inputs(n_images, prompts)
    torch.manual_seed(0)
    ref = HQ.tiny_qwen25vl(dtype=torch.float32, layers=3).cuda()
    bf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = QT.HipQwen25VLTextEncoder(bf, vision=QV.HipQwen25VLVisionTower(bf))
    with torch.no_grad():
        r = ref(**kw, output_hidden_states=True).hidden_states[-1]
        e = bf(**kw, output_hidden_states=True).hidden_states[-1]
    h = hip(**kw, output_hidden_states=True).hidden_states[-1]
    valid = kw["attention_mask"].bool()
    if not bool(valid.all()):
        assert float(h[~valid].float().abs().max()) == 0.0
    pe, ph = psnr(e[valid], r[valid]), psnr(h[valid], r[valid])
    print(f"Qwen2.5-VL prompt encoder with the HIP tower, {case}: HIP {ph:.2f} dB, eager bf16 {pe:.2f} dB against fp32")
    assert ph >= pe - 1.0 and ph >= 35.0, (ph, pe)


def test_a_warm_call_with_an_image_dispatches_only_libregione_hip_kernels():
    from torch.profiler import ProfilerActivity, profile
    m = HQ.tiny_qwen25vl().cuda()
    hip = QT.HipQwen25VLTextEncoder(m, vision=QV.HipQwen25VLVisionTower(m))
    kw = _tiny_inputs(2, ("make the square red",))
    hip(**kw, output_hidden_states=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        a = hip(**kw, output_hidden_states=True)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    assert any("vision_attention" in n for n in names) and any("vision_rope" in n for n in names)
    assert any("gelu_erf" in n for n in names) and any("cast_pad_rows" in n for n in names)
    assert any("text_attention_kernel" in n for n in names) and any("gemm" in n for n in names)
    assert torch.isfinite(a.hidden_states[-1].float()).all()


# ---- the hosted pipelines ---------------------------------------------------------------------------------------------------------
def _picture(h=256, w=256, seed=5):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(seed))


def _fallback_warnings(rec):
    return [str(r.message) for r in rec if "kept on the host module" in str(r.message)]


def _hooked(m):
    vis, lm = [], []
    for blk in m.model.visual.blocks:
        blk.register_forward_hook(lambda mod, i, o: vis.append(type(mod).__name__))
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: lm.append(type(mod).__name__))
    return vis, lm


def _hosted(m, plus=False):
    import host_standins as HS
    from regione_amd import RegionEHelper
    cls = HQ.QwenImageEditPlusPipeline if plus else HQ.QwenImageEditPipeline
    pipe = cls(HS.stub_trunk("qwen"), m)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    return pipe, helper


def _run(pipe, plus=False):
    image = [_picture(192, 384, seed=2), _picture(256, 256, seed=3)] if plus else _picture()
    prompts = ("put the object of image 1 into image 2" if plus else "add a red hat", "blurry")
    lat = pipe(image=image, prompt=prompts[0], negative_prompt=prompts[1], true_cfg_scale=4.0, generator=torch.Generator().manual_seed(1),
               output_type="latent").images
    assert torch.isfinite(lat.float()).all()
    return prompts


@pytest.mark.parametrize("plus", [False, True])
def test_hosted_qwen_edit_runs_neither_the_eager_tower_nor_the_eager_language_model(plus):
    m = HQ.tiny_qwen25vl()
    vis, lm = _hooked(m)
    pipe, helper = _hosted(m, plus)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
        prompts = _run(pipe, plus)
    assert _fallback_warnings(rec) == []
    assert vis == [] and lm == []
    assert isinstance(pipe._regione_hip_qwen_text, QT.HipQwen25VLTextEncoder)
    assert isinstance(pipe._regione_hip_qwen_text.vision, QV.HipQwen25VLVisionTower)
    assert len(pipe.encoded) == 2
    prompt_image = pipe.last_image
    for (pe, pm), prompt in zip(list(pipe.encoded), prompts):
        he, hm = pipe.encode_prompt(image=prompt_image, prompt=prompt, device=torch.device("cpu"))     # the host module, on the CPU
        assert pe.shape == he.shape and pe.dtype == torch.bfloat16 and torch.equal(pm.cpu(), hm)
        print(f"hosted encode_prompt {prompt!r} with the HIP tower: {psnr(pe.cpu(), he):.1f} dB against the host module")
        assert psnr(pe.cpu(), he) >= 40.0
    assert len(vis) == 2 * len(m.model.visual.blocks)                              # the host-encoded references ran on the module
    helper.disable()


def test_hosted_qwen_keeps_the_host_tower_on_request():
    m = HQ.tiny_qwen25vl()
    vis, lm = _hooked(m)
    pipe, helper = _hosted(m)
    pipe._regione_hip_vision = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
        _run(pipe)
    assert _fallback_warnings(rec) == []
    assert len(vis) == 2 * len(m.model.visual.blocks) and lm == []
    assert pipe._regione_hip_qwen_text.vision is None
    helper.disable()


def test_hosted_qwen_with_a_gelu_tower_keeps_it_on_the_host_with_one_warning():
    from transformers import Qwen2_5_VLForConditionalGeneration
    cfg = copy.deepcopy(HQ.tiny_qwen25vl().config)
    cfg.vision_config.hidden_act = "gelu"
    torch.manual_seed(31)
    m = Qwen2_5_VLForConditionalGeneration(cfg).eval().to(torch.bfloat16)
    vis, lm = _hooked(m)
    pipe, helper = _hosted(m)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
    assert len(_fallback_warnings(rec)) == 1 and "vision tower kept on the host module: hidden_act 'gelu'" in _fallback_warnings(rec)[0]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _run(pipe)
    assert _fallback_warnings(rec) == []                                          # decided once, at enable()
    assert isinstance(pipe._regione_hip_qwen_text, QT.HipQwen25VLTextEncoder) and pipe._regione_hip_qwen_text.vision is None
    assert len(vis) == 2 * len(m.model.visual.blocks) and lm == []
    helper.disable()
