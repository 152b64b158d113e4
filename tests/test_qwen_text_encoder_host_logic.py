"""CPU: the host side of the HIP Qwen2.5-VL language model (regione_amd/qwen_text_encoder.py) against the genuine transformers module -
adoption, refusals with their reasons, the cos / sin tables and position ids (bit-equal to the module's), the image rows, the mask rule,
the adapter's binding, and the argument checks of the three new C entries (no GPU is touched)."""
import re
import warnings
from pathlib import Path

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib, adapters  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
LM = "model.language_model."


def _inputs(n_images, prompts=("make the square red",), plus=None):
    plus = n_images > 1 if plus is None else plus
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    base = "".join(f"Picture {i + 1}: <image> " if plus else "<image> " for i in range(n_images))
    return HQ.ToyProcessor()(text=[base + p for p in prompts], images=images or None)


# ---- adoption ---------------------------------------------------------------------------------------------------------------------
def test_adoption_from_the_genuine_module_concatenates_and_shares_the_embedding():
    m = HQ.tiny_qwen25vl(layers=3)
    assert len(m.state_dict()) == 2 + 12 * 3 + 1 + len([k for k in m.state_dict() if k.startswith("model.visual.")])
    enc = QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=64)
    assert enc.dtype == torch.bfloat16 and enc.config is m.config and enc.device == torch.device("cpu") and enc.max_length == 64
    assert (enc.d, enc.F, enc.Hq, enc.Hkv, enc.qkv_cols) == (256, 512, 2, 1, 512) and len(enc.layers) == 3
    lm = m.model.language_model
    assert enc.tok.data_ptr() == lm.embed_tokens.weight.data_ptr()                # used in place, not copied
    a, mlp, p = lm.layers[1].self_attn, lm.layers[1].mlp, enc.layers[1]
    assert torch.equal(p["wqkv"], torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]))
    assert torch.equal(p["bqkv"], torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]))
    assert torch.equal(p["wgu"], torch.cat([mlp.gate_proj.weight, mlp.up_proj.weight]))
    assert torch.equal(p["wo"], a.o_proj.weight) and torch.equal(p["wdown"], mlp.down_proj.weight)
    assert torch.equal(p["ln1"], lm.layers[1].input_layernorm.weight) and torch.equal(enc.final_ln, lm.norm.weight)
    assert torch.equal(enc.inv_freq, lm.rotary_emb.inv_freq.float())


def test_adoption_from_a_state_dict_ignores_lm_head_and_the_vision_tower():
    m = HQ.tiny_qwen25vl()
    sd = dict(m.state_dict())
    assert any(k.startswith("lm_head.") for k in sd) and any(k.startswith("model.visual.") for k in sd)
    enc = QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    assert enc.module is None and torch.equal(enc.layers[0]["wo"], m.model.language_model.layers[0].self_attn.o_proj.weight)
    only_lm = {k: v for k, v in sd.items() if k.startswith(LM)}
    assert QT.HipQwen25VLTextEncoder(only_lm, device="cpu", config=m.config).tok.data_ptr() == enc.tok.data_ptr()
    sd["model.visual.blocks.0.attn.qkv.weight"] = sd["model.visual.blocks.0.attn.qkv.weight"].float()     # not adopted: any dtype
    QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    assert torch.equal(enc.inv_freq, QT.default_inv_freq(m.config))
    with pytest.raises(_lib.RegionEHipError, match="needs its config"):
        QT.HipQwen25VLTextEncoder(sd, device="cpu")


def test_adoption_refusals_name_the_reason():
    m = HQ.tiny_qwen25vl()
    with pytest.raises(_lib.RegionEHipError, match="non-bf16 weights"):
        QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(dtype=torch.float32), device="cpu")
    sd = dict(m.state_dict())
    del sd[LM + "layers.1.self_attn.k_proj.bias"]
    with pytest.raises(_lib.RegionEHipError, match="missing"):
        QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    sd = dict(m.state_dict())
    sd[LM + "layers.0.self_attn.q_proj.lora_A.weight"] = torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="LoRA"):
        QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    sd = dict(m.state_dict())
    sd[LM + "layers.0.self_attn.q_norm.weight"] = torch.zeros(128, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="does not know"):
        QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    sd = dict(m.state_dict())
    sd[LM + "layers.0.mlp.up_proj.weight"] = torch.zeros(256, 256, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="has shape"):
        QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    with pytest.raises(_lib.RegionEHipError, match="max_length"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=5000)


@pytest.mark.parametrize("kw,why", [
    (dict(num_attention_heads=4, num_key_value_heads=2), "head dim 64"),
    (dict(hidden_size=384, num_attention_heads=3, num_key_value_heads=2), "Hq % Hkv"),
    (dict(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=1e6, mrope_section=[16, 24, 24])), "rope_type 'linear'"),
    (dict(use_sliding_window=True, sliding_window=8, max_window_layers=1), "sliding-window"),
    (dict(hidden_act="gelu"), "hidden_act 'gelu'"),
    (dict(intermediate_size=480), "not multiples of 64"),
    (dict(rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[8, 28, 28])), None),
    (dict(rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[16, 16, 16])), "mrope_section"),
])
def test_qwen25vl_refusal_names_every_uncovered_config(kw, why):
    from transformers import Qwen2_5_VLTextConfig
    base = dict(vocab_size=64, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[16, 24, 24]))
    base.update(kw)
    got = QT.qwen25vl_refusal(Qwen2_5_VLTextConfig(**base))
    if why is None:
        assert got is None
    else:
        assert got is not None and why in got, got


def test_refusal_of_a_whole_config_and_of_another_model():
    m = HQ.tiny_qwen25vl()
    assert QT.qwen25vl_refusal(m.config) is None and QT.qwen25vl_refusal(m.config.text_config) is None
    from transformers import T5Config
    assert "model_type 't5'" in QT.qwen25vl_refusal(T5Config())
    sw = HQ.tiny_qwen25vl(text_kw=dict(use_sliding_window=True, sliding_window=8, max_window_layers=1))
    with pytest.raises(_lib.RegionEHipError, match="sliding-window"):
        QT.HipQwen25VLTextEncoder(sw, device="cpu")


# ---- call refusals: before any kernel (a CPU adoption cannot launch one) ----------------------------------------------------------
def test_call_refusals_come_before_any_kernel_and_name_the_reason():
    m = HQ.tiny_qwen25vl()
    enc = QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=32)
    ids = torch.randint(3, 900, (1, 8))
    cases = [
        (dict(pixel_values_videos=torch.zeros(4, 1176)), "videos"), (dict(video_grid_thw=torch.tensor([[1, 2, 2]])), "videos"),
        (dict(past_key_values=object()), "past_key_values"), (dict(use_cache=True), "use_cache"),
        (dict(inputs_embeds=torch.zeros(1, 8, 256)), "inputs_embeds"), (dict(output_attentions=True), "output_attentions"),
        (dict(labels=ids), "labels"), (dict(logits_to_keep=1), "logits_to_keep"),
        (dict(attention_mask=torch.tensor([[0, 0, 1, 1, 1, 1, 1, 1]])), "run of ones followed by zeros"),
        (dict(attention_mask=torch.tensor([[1, 1, 1, 0, 1, 1, 0, 0]])), "run of ones followed by zeros"),
        (dict(attention_mask=torch.zeros(1, 8)), "empty row"),
        (dict(attention_mask=torch.ones(1, 7)), "attention_mask of shape"),
        (dict(position_ids=torch.zeros(3, 1, 9, dtype=torch.int64)), "position_ids of shape"),
        (dict(pixel_values=torch.zeros(4, 1176), image_embeds=torch.zeros(1, 256)), "not both"),
    ]
    for kw, why in cases:
        with pytest.raises(_lib.RegionEHipError, match=why):
            enc(ids, **kw)
    with pytest.raises(_lib.RegionEHipError, match="sequence length 33"):
        enc(torch.zeros(1, 33, dtype=torch.int64))
    with pytest.raises(_lib.RegionEHipError, match=r"\[B, L\]"):
        enc(torch.zeros(8, dtype=torch.int64))
    vid = ids.clone()
    vid[0, 3] = HQ.VIDEO
    with pytest.raises(_lib.RegionEHipError, match="video tokens"):
        enc(vid)
    sd_enc = QT.HipQwen25VLTextEncoder(dict(m.state_dict()), device="cpu", config=m.config)
    with pytest.raises(_lib.RegionEHipError, match="pass position_ids"):
        sd_enc(ids)
    with pytest.raises(_lib.RegionEHipError, match="pass image_embeds"):
        sd_enc(ids, pixel_values=torch.zeros(4, 1176), image_grid_thw=torch.tensor([[1, 2, 2]]), position_ids=torch.arange(8)[None])
    # accepted arguments reach the kernels: on a CPU adoption that is the library's own "no CPU fallback" error
    with pytest.raises(_lib.RegionEHipError, match="no CPU fallback"):
        enc(ids, attention_mask=torch.tensor([[1, 1, 1, 1, 1, 0, 0, 0]]), use_cache=False, output_hidden_states=True)


# ---- positions and tables ---------------------------------------------------------------------------------------------------------
def _module_tables(m, pos):
    """cos / sin as Qwen2_5_VLTextModel.forward + apply_multimodal_rotary_pos_emb see them (bf16, after the mrope_section selection)."""
    cos, sin = m.model.language_model.rotary_emb(torch.zeros(1, dtype=torch.bfloat16), pos)
    sec = m.config.text_config.rope_parameters["mrope_section"] * 2
    pick = lambda t: torch.cat([c[i % 3] for i, c in enumerate(t.split(sec, dim=-1))], dim=-1)
    return pick(cos), pick(sin)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n_images", [0, 1, 2])
@pytest.mark.parametrize("with_types", [False, True])
def test_positions_and_tables_are_the_modules_own(n_images, with_types, dtype):
    m = HQ.tiny_qwen25vl(dtype=dtype)                   # `.to(bfloat16)` rounds the inv_freq buffer: the tables follow the module's
    sd = {k: v.to(torch.bfloat16) for k, v in m.state_dict().items()}
    enc = QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config)
    enc.module = m
    enc.inv_freq = m.model.language_model.rotary_emb.inv_freq.detach().float().cpu()
    mi = _inputs(n_images, prompts=("make the square red", "a much longer instruction than the other one is"))
    ids, mask = mi.input_ids, mi.attention_mask
    B, L = ids.shape
    mm = (ids == HQ.IMAGE).int() if with_types else None
    want = m.model.compute_3d_position_ids(input_ids=ids, image_grid_thw=mi.image_grid_thw, video_grid_thw=None, inputs_embeds=None,
                                           attention_mask=mask, past_key_values=None, mm_token_type_ids=mm)
    if with_types and n_images:
        assert want is not None and not torch.equal(want[1], want[2])              # genuine 3-D positions
    else:
        assert want is None                                                        # transformers 5.15: the module falls back to arange
        want = torch.arange(L).view(1, 1, -1).expand(3, B, -1)
    got = enc.position_ids_for(ids, mask, mi.image_grid_thw, None, mm)
    assert torch.equal(got, want)
    tab = QT.mrope_tables(enc.inv_freq, got, enc.mrope_section)
    cos, sin = _module_tables(m, want)
    assert tab.dtype == torch.bfloat16 and tuple(tab.shape) == (2, B, L, 128)
    assert torch.equal(tab[0], cos) and torch.equal(tab[1], sin)


def test_caller_position_ids_are_used_as_the_text_model_uses_them():
    m = HQ.tiny_qwen25vl()
    enc = QT.HipQwen25VLTextEncoder(m, device="cpu")
    ids = torch.randint(3, 900, (2, 6))
    p2 = torch.arange(6)[None].expand(2, -1) + 5
    assert torch.equal(enc.position_ids_for(ids, position_ids=p2), p2[None].expand(3, -1, -1))
    p4 = torch.randint(0, 50, (4, 2, 6))
    assert torch.equal(enc.position_ids_for(ids, position_ids=p4), p4[1:])
    p3 = torch.randint(0, 50, (3, 2, 6))
    assert torch.equal(enc.position_ids_for(ids, position_ids=p3), p3)


def test_hidden_states_last_entry_is_the_normed_final_state_in_transformers():
    """What the HIP class returns as `hidden_states[-1]` is what the genuine module returns there."""
    m = HQ.tiny_qwen25vl(dtype=torch.float32)
    mi = _inputs(1)
    with torch.no_grad():
        o = m(input_ids=mi.input_ids, attention_mask=mi.attention_mask, pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw,
              output_hidden_states=True)
        last = m.model(input_ids=mi.input_ids, attention_mask=mi.attention_mask, pixel_values=mi.pixel_values,
                       image_grid_thw=mi.image_grid_thw).last_hidden_state
    assert torch.equal(o.hidden_states[-1], last)
    out = QT.QwenTextEncoderOutput(last, True)
    assert out.hidden_states[-1] is last and len(out.hidden_states) == 1 and out[0] is last and out["last_hidden_state"] is last
    assert QT.QwenTextEncoderOutput(last, False).hidden_states is None
    assert "absent" in QT.HipQwen25VLTextEncoder.__doc__ and "ABSENT" in QT.QwenTextEncoderOutput.__doc__


# ---- image rows and the mask rule -------------------------------------------------------------------------------------------------
def test_image_rows_and_the_placeholder_count_error():
    mi = _inputs(2, prompts=("red", "a longer instruction here"))
    ids = mi.input_ids
    lengths = QT.valid_lengths(mi.attention_mask, *ids.shape)
    assert lengths == [int(v) for v in mi.attention_mask.sum(1)] and lengths[0] < lengths[1] == ids.shape[1]
    rows = QT.image_rows(ids, lengths, HQ.IMAGE, 2 * (4 + 6))
    for b in range(2):
        assert torch.equal(rows[b], torch.nonzero(ids[b] == HQ.IMAGE).flatten()) and rows[b].numel() == 10
    with pytest.raises(ValueError, match="Image features and image tokens do not match, tokens: 20, features: 19"):
        QT.image_rows(ids, lengths, HQ.IMAGE, 19)
    bad = ids.clone()
    bad[0, -1] = HQ.IMAGE                                   # a placeholder in the padding of row 0
    with pytest.raises(_lib.RegionEHipError, match="padded part"):
        QT.image_rows(bad, lengths, HQ.IMAGE, 21)
    # the module agrees about the count
    m = HQ.tiny_qwen25vl()
    with torch.no_grad(), pytest.raises(ValueError, match="do not match"):
        m(input_ids=ids[1:, :-12], pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw)


def test_mask_rule_accepts_right_padding_only():
    ok = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]])
    assert QT.valid_lengths(ok, 3, 5) == [3, 5, 1] and QT.valid_lengths(None, 2, 7) == [7, 7]
    assert QT.valid_lengths(ok.bool(), 3, 5) == [3, 5, 1] and QT.valid_lengths(ok.float(), 3, 5) == [3, 5, 1]
    for bad in ([[0, 1, 1, 1, 1]], [[1, 0, 1, 0, 0]], [[0, 0, 0, 0, 1]]):
        with pytest.raises(_lib.RegionEHipError, match="left padding and holes"):
            QT.valid_lengths(torch.tensor(bad), 1, 5)


# ---- the adapter ------------------------------------------------------------------------------------------------------------------
class _Host:
    pass


def test_adapter_binds_and_restores_even_on_an_exception():
    h = _Host()
    m = HQ.tiny_qwen25vl()
    h.text_encoder = m
    enc = adapters.hip_qwen_text_encoder_for(h, "cpu")
    assert isinstance(enc, QT.HipQwen25VLTextEncoder) and h._regione_hip_qwen_text is enc
    assert adapters.hip_qwen_text_encoder_for(h, "cpu") is enc                     # adopted once
    assert enc.dtype == torch.bfloat16 and enc.device == torch.device("cpu") and enc.config is m.config
    with pytest.raises(ValueError):
        with adapters._hip_qwen_text_encoder(h, "cpu"):
            assert h.text_encoder is enc
            raise ValueError("boom")
    assert h.text_encoder is m
    with adapters._hip_qwen_text_encoder(h, "cpu"):
        assert h.text_encoder is enc
    assert h.text_encoder is m


def test_adapter_keeps_an_uncovered_module_with_one_warning():
    h = _Host()
    h.text_encoder = HQ.tiny_qwen25vl(text_kw=dict(use_sliding_window=True, sliding_window=8, max_window_layers=1))
    with pytest.warns(RuntimeWarning, match="text_encoder kept on the host module: sliding-window") as rec:
        assert adapters.hip_qwen_text_encoder_for(h, "cpu") is None
    assert len([r for r in rec if "kept on the host module" in str(r.message)]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                            # decided once: no second warning
        assert adapters.hip_qwen_text_encoder_for(h, "cpu") is None
        with adapters._hip_qwen_text_encoder(h, "cpu"):
            assert h.text_encoder.__class__.__name__ == "Qwen2_5_VLForConditionalGeneration"
    h2 = _Host()
    h2.text_encoder = HQ.tiny_qwen25vl(dtype=torch.float32)
    with pytest.warns(RuntimeWarning, match="non-bf16"):
        assert adapters.hip_qwen_text_encoder_for(h2, "cpu") is None
    h3 = _Host()
    h3.text_encoder = HQ.tiny_qwen25vl()
    h3.text_encoder.model.language_model.layers[0].self_attn.lora_A = torch.nn.Linear(256, 4, bias=False).to(torch.bfloat16)
    with pytest.warns(RuntimeWarning, match="LoRA"):
        assert adapters.hip_qwen_text_encoder_for(h3, "cpu") is None


def test_adapter_opt_out_and_other_text_encoders_are_silent():
    import host_standins as HS
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h = _Host()
        h.text_encoder = HQ.tiny_qwen25vl()
        h._regione_hip_text = False
        assert adapters.hip_qwen_text_encoder_for(h, "cpu") is None and "_regione_hip_qwen_text" not in h.__dict__
        assert adapters.hip_qwen_text_encoder_for(_Host(), "cpu") is None          # no text_encoder at all
        h = _Host()
        h.text_encoder = torch.nn.Linear(4, 4)                                     # some other module
        assert adapters.hip_qwen_text_encoder_for(h, "cpu") is None
        old = HS.QwenImageEditPipeline.__new__(HS.QwenImageEditPipeline)           # the hash-seeded stand-in: no text_encoder attribute
        assert adapters.hip_qwen_text_encoder_for(old, "cpu") is None
        with adapters._hip_qwen_text_encoder(old, "cpu"):
            assert "text_encoder" not in old.__dict__
        assert "text_encoder" not in old.__dict__


def test_the_standin_pipeline_encodes_like_diffusers_on_the_cpu():
    """The restated `_get_qwen_prompt_embeds`: template prefix dropped, rows padded to the longest, mask of ones then zeros."""
    m = HQ.tiny_qwen25vl(dtype=torch.float32)
    pipe = HQ.QwenImageEditPlusPipeline.__new__(HQ.QwenImageEditPlusPipeline)
    pipe.calls, pipe.encoded, pipe.text_encoder, pipe.processor = [], [], m, HQ.ToyProcessor()
    g = torch.Generator().manual_seed(1)
    imgs = [torch.rand(1, 3, 64, 64, generator=g), torch.rand(1, 3, 64, 96, generator=g)]
    with torch.no_grad():
        e, mask = pipe.encode_prompt(prompt=["red", "make it much more blue"], image=imgs, device=torch.device("cpu"))
    n_img = 2 * 2 + (1 + 4 + 1) + (1 + 6 + 1)                                      # "Picture k:" words + the two vision runs
    assert tuple(e.shape) == (2, n_img + 5 + 3, 256) and mask.tolist() == [[1] * (n_img + 4) + [0] * 4, [1] * (n_img + 8)]
    assert float(e[0, n_img + 4:].abs().max()) == 0.0 and torch.isfinite(e).all()


# ---- the new C entries: argument checks without a GPU -------------------------------------------------------------------------------
def test_new_c_entries_validate_arguments_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()
    assert h.rgn_lm_attention_bf16(None, P, 8, 2, 1, 0.1, None) == -1 and "bad argument" in msg()
    assert h.rgn_lm_attention_bf16(P, None, 8, 2, 1, 0.1, None) == -1
    assert h.rgn_lm_attention_bf16(P, P, 0, 2, 1, 0.1, None) == -1 and "L >= 1" in msg()
    assert h.rgn_lm_attention_bf16(P, P, 8, 3, 2, 0.1, None) == -1 and "Hq % Hkv" in msg()
    assert h.rgn_lm_attention_bf16(P, P, 8, 2, 0, 0.1, None) == -1
    assert h.rgn_lm_attention_bf16(P, P, 8, 1, 2, 0.1, None) == -1
    assert h.rgn_lm_attention_bf16(P, P, 8, 2, 1, 0.0, None) == -1 and "scale" in msg()
    assert h.rgn_lm_attention_bf16(P, P, 8, 2, 1, float("inf"), None) == -1
    assert h.rgn_lm_attention_bf16(P, P, 8, 2, 1, float("nan"), None) == -1
    assert h.rgn_lm_attention_bf16(P, P, 4097, 2, 1, 0.1, None) == -1 and "4096" in msg()
    assert h.rgn_lm_attention_bf16(P + 2, P, 8, 2, 1, 0.1, None) == -1 and "aligned" in msg()
    assert h.rgn_mrope_bf16(None, 512, P, P, 8, 2, 1, None) == -1 and "bad argument" in msg()
    assert h.rgn_mrope_bf16(P, 512, None, P, 8, 2, 1, None) == -1 and h.rgn_mrope_bf16(P, 512, P, None, 8, 2, 1, None) == -1
    assert h.rgn_mrope_bf16(P, 504, P, P, 8, 2, 1, None) == -1 and "ld >=" in msg()
    assert h.rgn_mrope_bf16(P, 516, P, P, 8, 2, 1, None) == -1
    assert h.rgn_mrope_bf16(P, 512, P, P, 0, 2, 1, None) == -1 and h.rgn_mrope_bf16(P, 512, P, P, 8, 0, 1, None) == -1
    assert h.rgn_mrope_bf16(P, 512, P + 4, P, 8, 2, 1, None) == -1 and "aligned" in msg()
    assert h.rgn_swiglu_bf16(P, 100, P, 64, 4, 64, None) == -1 and "ldx >= 2 F" in msg()
    assert h.rgn_swiglu_bf16(P, 128, P, 64, 4, 60, None) == -1 and h.rgn_swiglu_bf16(P, 128, P, 32, 4, 64, None) == -1
    assert h.rgn_swiglu_bf16(None, 128, P, 64, 4, 64, None) == -1 and h.rgn_swiglu_bf16(P, 128, P, 64, -1, 64, None) == -1
    assert h.rgn_swiglu_bf16(P + 2, 128, P, 64, 4, 64, None) == -1 and "aligned" in msg()
    assert h.rgn_swiglu_bf16(None, 128, P, 64, 0, 64, None) == 0                      # M = 0: nothing to do


def test_header_signatures_and_library_agree_on_the_new_entries():
    text = (ROOT / "include" / "regione_hip.h").read_text()
    h = _lib.lib()
    for name, nargs in (("rgn_lm_attention_bf16", 7), ("rgn_mrope_bf16", 8), ("rgn_swiglu_bf16", 7)):
        decl = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name])
        assert getattr(h, name).argtypes == _lib.SIGNATURES[name]
    assert h.rgn_version() == int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 108
    assert "apply_multimodal_rotary_pos_emb" in text and "Qwen2MLP" in text and "Qwen2_5_VLAttention" in text
