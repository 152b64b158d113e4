"""CPU: the host side of HipQwen25VLTextEncoder.generate (regione_amd/qwen_text_encoder.py) - the decode positions against the genuine
transformers module, every refusal before any library call, lm_head adoption, and the argument checks of the four decode entries of
csrc/decode.hip (no GPU is touched)."""
import ctypes

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

PROMPT = "make the square red and keep the rest of the picture as it is"


def _inputs(n_images):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    base = "".join(f"Picture {i + 1}: <image> " if n_images > 1 else "<image> " for i in range(n_images))
    extra = " with three birds" if n_images > 1 else ""                          # L = 46 with two images (31 with one)
    return HQ.ToyProcessor()(text=[base + PROMPT + extra], images=images or None)


# ---- decode positions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_images,L,top", [(0, None, None), (1, 31, 28), (2, 46, 40)])
def test_decode_positions_equal_the_modules_positions_of_the_extended_sequence(n_images, L, top):
    """The positions of 16 appended tokens: `compute_3d_position_ids` of the genuine module over the extended sequence, exactly."""
    m = HQ.tiny_qwen25vl()
    enc = QT.HipQwen25VLTextEncoder(m, device="cpu")
    mi = _inputs(n_images)
    ids = mi.input_ids
    if L is not None:
        assert ids.shape[1] == L
    types = (ids == HQ.IMAGE).int()
    prompt_pos = enc.position_ids_for(ids, mi.attention_mask, mi.image_grid_thw, None, types)
    if top is not None:
        assert int(prompt_pos.max()) == top
    got = QT.decode_position_ids(prompt_pos, 16)
    ext = torch.cat([ids, torch.randint(3, 990, (1, 16), generator=torch.Generator().manual_seed(1))], dim=1)
    want = m.model.compute_3d_position_ids(input_ids=ext, image_grid_thw=mi.image_grid_thw, video_grid_thw=None, inputs_embeds=None,
                                           attention_mask=torch.ones_like(ext), past_key_values=None, mm_token_type_ids=(ext == HQ.IMAGE).int())
    if n_images == 0 and want is None:                                           # no image: the arange of Qwen2_5_VLTextModel.forward
        want = torch.arange(ext.shape[1]).view(1, 1, -1).expand(3, 1, -1)
    assert want is not None and want.shape[0] == 3
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 1, 16)
    assert torch.equal(got, want[:, :, ids.shape[1]:])
    first = int(prompt_pos.max()) + 1
    assert got[0, 0].tolist() == list(range(first, first + 16))
    if n_images:
        assert first < ids.shape[1]                                              # image tokens share positions: not the text-only arange


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def enc(monkeypatch):
    m = HQ.tiny_qwen25vl()
    e = QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=64)

    def boom():
        raise AssertionError("a refusal must come before any library call")
    monkeypatch.setattr(_lib, "lib", boom)
    return e


IDS = torch.randint(3, 990, (1, 12), generator=torch.Generator().manual_seed(0))


@pytest.mark.parametrize("kw,match", [
    (dict(do_sample=True), "do_sample"),
    (dict(num_beams=4), "num_beams"),
    (dict(temperature=0.7), "temperature"),
    (dict(top_k=50), "top_k"),
    (dict(top_p=0.9), "top_p"),
    (dict(repetition_penalty=1.1), "repetition_penalty"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
    (dict(past_key_values=object()), "past_key_values"),
    (dict(streamer=object()), "streamer"),
    (dict(pixel_values_videos=torch.zeros(1)), "pixel_values_videos"),
    (dict(video_grid_thw=torch.zeros(1, 3)), "video_grid_thw"),
    (dict(some_new_argument=1), "some_new_argument"),
    (dict(generation_config=None), "generation_config"),
    (dict(max_new_tokens=None), "max_new_tokens"),
    (dict(max_new_tokens=0), "max_new_tokens"),
    (dict(max_new_tokens=2.0), "max_new_tokens"),
    (dict(max_new_tokens=True), "max_new_tokens"),
    (dict(max_new_tokens=53), "max_length"),
    (dict(sync_every=0), "sync_every"),
    (dict(eos_token_id="7"), "eos_token_id"),
    (dict(attention_mask=torch.tensor([[1] * 11 + [0]])), "attention_mask"),
    (dict(input_ids=torch.cat([IDS, IDS])), "B = 2"),
    (dict(input_ids=torch.tensor([[3, 4, HQ.VIDEO, 5]])), "video"),
])
def test_generate_refuses_before_any_library_call(enc, kw, match):
    args = dict(input_ids=IDS, max_new_tokens=4)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        enc.generate(**args)


def test_generate_does_not_deviate_silently_from_the_modules_generation_config(enc):
    enc.module.generation_config.do_sample = True
    with pytest.raises(_lib.RegionEHipError, match="generation_config.do_sample"):
        enc.generate(IDS, max_new_tokens=4)
    enc.module.generation_config.do_sample = False
    enc.module.generation_config.num_beams = 3
    with pytest.raises(_lib.RegionEHipError, match="num_beams"):
        enc.generate(IDS, max_new_tokens=4)


def test_an_empty_eos_list_asks_for_no_eos_and_none_takes_the_modules(enc):
    enc.module.generation_config.eos_token_id = 7
    assert enc._generate_args(IDS, None, 4, None, None, 8, {}) == [7]
    assert enc._generate_args(IDS, None, 4, [], None, 8, {}) == []
    assert enc._generate_args(IDS, None, 4, [5, 6], None, 8, {}) == [5, 6]


def test_an_accepted_call_reaches_the_library(enc):
    """The fixture's library raises: arguments generate accepts get past every refusal (so the refusals above are not vacuous)."""
    with pytest.raises(AssertionError, match="before any library call"):
        enc.generate(IDS, attention_mask=torch.ones_like(IDS), max_new_tokens=52, do_sample=False, num_beams=1, use_cache=True,
                     eos_token_id=[5, 6], temperature=None, sync_every=3)


def test_lm_head_is_adopted_lazily_and_a_state_dict_without_it_is_refused(monkeypatch):
    m = HQ.tiny_qwen25vl()
    e = QT.HipQwen25VLTextEncoder(m, device="cpu")
    assert e.lm_head is None                                                     # encode-only users do not pay for it
    assert e._adopt_lm_head().data_ptr() == m.lm_head.weight.data_ptr() and e.lm_head is not None
    sd = {k: v for k, v in m.state_dict().items() if not k.startswith("lm_head.")}
    e = QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("library call")))
    pos = torch.arange(12).view(1, 1, -1).expand(3, 1, -1)
    with pytest.raises(_lib.RegionEHipError, match="lm_head.weight is missing"):
        e.generate(IDS, max_new_tokens=4, position_ids=pos)
    sd["lm_head.weight"] = m.lm_head.weight.float()
    e = QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    with pytest.raises(_lib.RegionEHipError, match="lm_head.weight is torch.float32"):
        e.generate(IDS, max_new_tokens=4, position_ids=pos)
    tied = HQ.tiny_qwen25vl(text_kw=dict(tie_word_embeddings=True))
    tied.config.tie_word_embeddings = True
    e = QT.HipQwen25VLTextEncoder(tied, device="cpu")
    assert e._adopt_lm_head() is e.tok


# ---- the four entries validate before they launch ---------------------------------------------------------------------------------------
def test_decode_entries_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address

    def msg():
        return h.rgn_last_error().decode()
    # rgn_lm_gemv_bf16(W, x, bias, resid, y, N, K, stream)
    assert h.rgn_lm_gemv_bf16(None, P, None, None, P, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_bf16(P, None, None, None, P, 8, 64, None) < 0
    assert h.rgn_lm_gemv_bf16(P, P, None, None, None, 8, 64, None) < 0
    assert h.rgn_lm_gemv_bf16(P, P, None, None, P, 0, 64, None) < 0
    assert h.rgn_lm_gemv_bf16(P, P, None, None, P, 8, 96, None) < 0 and "multiple of 64" in msg()
    assert h.rgn_lm_gemv_bf16(P, P, None, None, P, 8, 0, None) < 0
    assert h.rgn_lm_gemv_bf16(P + 8, P, None, None, P, 8, 64, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_gemv_bf16(P, P + 2, None, None, P, 8, 64, None) < 0 and "aligned" in msg()
    # rgn_lm_kv_append_bf16(QKV, ld, cache, cap, row0, L, Hq, Hkv, stream)
    assert h.rgn_lm_kv_append_bf16(None, 512, P, 64, 0, 1, 2, 1, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_kv_append_bf16(P, 512, None, 64, 0, 1, 2, 1, None) < 0
    assert h.rgn_lm_kv_append_bf16(P, 504, P, 64, 0, 1, 2, 1, None) < 0                       # ld < (Hq + 2 Hkv) 128
    assert h.rgn_lm_kv_append_bf16(P, 512, P, 64, 60, 5, 2, 1, None) < 0 and "cap" in msg()   # rows past the cache
    assert h.rgn_lm_kv_append_bf16(P, 512, P, 4097, 0, 1, 2, 1, None) < 0 and "4096" in msg()
    assert h.rgn_lm_kv_append_bf16(P, 512, P, 64, -1, 1, 2, 1, None) < 0
    assert h.rgn_lm_kv_append_bf16(P + 4, 512, P, 64, 0, 1, 2, 1, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_kv_append_bf16(P, 512, P, 64, 0, 0, 2, 1, None) == 0                      # nothing to append
    # rgn_lm_decode_attention_bf16(q, cache, O, n, Hq, Hkv, scale, workspace, workspace_bytes, stream)
    big = 1 << 30
    assert h.rgn_lm_decode_attention_workspace_bytes(28, 1500) == 28 * 24 * 130 * 4
    assert h.rgn_lm_decode_attention_workspace_bytes(2, 64) == 2 * 130 * 4 and h.rgn_lm_decode_attention_workspace_bytes(2, 65) == 4 * 130 * 4
    assert h.rgn_lm_decode_attention_bf16(None, P, P, 8, 2, 1, 0.1, P, big, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 8, 2, 1, 0.1, None, big, None) < 0
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 0, 2, 1, 0.1, P, big, None) < 0 and "4096" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 4097, 2, 1, 0.1, P, big, None) < 0 and "4096" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 8, 3, 2, 0.1, P, big, None) < 0 and "Hq % Hkv" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 8, 16, 1, 0.1, P, big, None) < 0 and "Hq / Hkv > 8" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 8, 2, 1, 0.0, P, big, None) < 0
    assert h.rgn_lm_decode_attention_bf16(P, P + 8, P, 8, 2, 1, 0.1, P, big, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_decode_attention_bf16(P, P, P, 65, 2, 1, 0.1, P, 4 * 130 * 4 - 1, None) < 0 and "workspace" in msg()
    # rgn_lm_head_argmax(W, x, V, K, token_out, logits_out, workspace, workspace_bytes, stream)
    assert h.rgn_lm_head_workspace_bytes(1) == 8 and h.rgn_lm_head_workspace_bytes(152064) == 38016 * 8
    assert h.rgn_lm_head_argmax(None, P, 8, 64, P, None, P, big, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_head_argmax(P, P, 8, 64, None, None, P, big, None) < 0
    assert h.rgn_lm_head_argmax(P, P, 8, 64, P, None, None, big, None) < 0
    assert h.rgn_lm_head_argmax(P, P, 0, 64, P, None, P, big, None) < 0
    assert h.rgn_lm_head_argmax(P, P, 8, 72, P, None, P, big, None) < 0 and "multiple of 64" in msg()
    assert h.rgn_lm_head_argmax(P + 2, P, 8, 64, P, None, P, big, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_head_argmax(P, P, 8, 64, P + 4, None, P, big, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_head_argmax(P, P, 1000, 64, P, None, P, 250 * 8 - 1, None) < 0 and "workspace" in msg()
    assert isinstance(ctypes.c_size_t(h.rgn_lm_head_workspace_bytes(0)).value, int) and h.rgn_lm_head_workspace_bytes(0) == 0
