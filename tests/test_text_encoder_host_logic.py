"""CPU: the host side of the HIP text encoders (regione_amd/text_encoders.py) against the genuine transformers modules - the T5 bias
table, adoption (tied embeddings, an fp32 `wo`, the concatenated weights), refusals with their reasons, the CLIP pooled-row rule, the
adapter's fallbacks, and the argument checks of the new C entries (no GPU is touched)."""
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")
from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel  # noqa: E402

from regione_amd import _lib, adapters  # noqa: E402
from regione_amd import text_encoders as TE  # noqa: E402


def tiny_t5(**kw):
    c = dict(vocab_size=96, d_model=128, d_kv=64, d_ff=192, num_layers=2, num_heads=2, feed_forward_proj="gated-gelu",
             relative_attention_num_buckets=32, relative_attention_max_distance=128, is_encoder_decoder=False)
    c.update(kw)
    torch.manual_seed(0)
    return T5EncoderModel(T5Config(**c)).eval()


def tiny_clip(**kw):
    c = dict(vocab_size=96, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
             bos_token_id=0, eos_token_id=2, pad_token_id=1)
    c.update(kw)
    torch.manual_seed(0)
    return CLIPTextModel(CLIPTextConfig(**c)).eval()


# ---- T5 relative-position bias table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 77, 128, 129, 512])
def test_t5_bias_table_is_bit_equal_to_compute_bias(L):
    m = tiny_t5(num_heads=3).to(torch.bfloat16)
    attn = m.encoder.block[0].layer[0].SelfAttention
    w = attn.relative_attention_bias.weight
    Lmax = 512
    for table in (TE.t5_bias_table(w, Lmax, 32, 128, attention=attn), TE.t5_bias_table(w, Lmax, 32, 128)):
        assert table.shape == (3, 2 * Lmax - 1) and table.dtype == torch.bfloat16
        want = attn.compute_bias(L, L)[0]                                         # [H, L, L]
        i = torch.arange(L)[:, None]
        j = torch.arange(L)[None, :]
        got = table[:, (j - i + Lmax - 1)]                                        # [H, L, L]
        assert torch.equal(got, want)


def test_t5_bias_table_covers_the_bucket_edges():
    """Distances 16, 32 and 64 sit exactly on an integer of the float32 log expression: the table must hold what compute_bias gives."""
    m = tiny_t5(num_heads=2).to(torch.bfloat16)
    attn = m.encoder.block[0].layer[0].SelfAttention
    with torch.no_grad():
        attn.relative_attention_bias.weight.copy_(torch.arange(64, dtype=torch.bfloat16).view(32, 2))   # value = 2 * bucket + head
    table = TE.t5_bias_table(attn.relative_attention_bias.weight, 512, 32, 128, attention=attn)
    ref = attn.compute_bias(512, 512)[0]
    for r in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 300):
        for s in (r, -r):
            i, j = (0, s) if s > 0 else (-s, 0)
            assert table[0, s + 511] == ref[0, i, j], (s, table[0, s + 511], ref[0, i, j])


# ---- adoption ---------------------------------------------------------------------------------------------------------------------
def test_t5_adoption_from_the_genuine_module_ties_embeddings_and_concatenates():
    m = tiny_t5().to(torch.bfloat16)
    assert m.shared.weight.data_ptr() == m.encoder.embed_tokens.weight.data_ptr()
    enc = TE.HipT5EncoderModel(m, device="cpu", max_length=64)
    assert enc.dtype == torch.bfloat16 and enc.config is m.config and enc.device == torch.device("cpu")
    assert torch.equal(enc.tok, m.shared.weight)
    a = m.encoder.block[1].layer[0].SelfAttention
    ff = m.encoder.block[1].layer[1].DenseReluDense
    p = enc.layers[1]
    assert torch.equal(p["wqkv"], torch.cat([a.q.weight, a.k.weight, a.v.weight]))
    assert torch.equal(p["wi"], torch.cat([ff.wi_1.weight, ff.wi_0.weight]))
    assert torch.equal(p["wo_ff"], ff.wo.weight) and enc.bias_table.shape == (2, 127)


def test_t5_adoption_casts_an_fp32_wo_once_and_says_so():
    m = tiny_t5().to(torch.bfloat16)
    for blk in m.encoder.block:
        blk.layer[1].DenseReluDense.wo.float()
    with pytest.warns(RuntimeWarning, match="fp32"):
        enc = TE.HipT5EncoderModel(m, device="cpu", max_length=16)
    assert enc.layers[0]["wo_ff"].dtype == torch.bfloat16
    assert torch.equal(enc.layers[0]["wo_ff"], m.encoder.block[0].layer[1].DenseReluDense.wo.weight.to(torch.bfloat16))


def test_t5_adoption_from_a_state_dict_with_only_one_embedding_key():
    m = tiny_t5().to(torch.bfloat16)
    sd = {k: v for k, v in m.state_dict().items() if k != "encoder.embed_tokens.weight"}
    enc = TE.HipT5EncoderModel(sd, device="cpu", config=m.config, max_length=32)
    assert torch.equal(enc.tok, m.shared.weight)
    ref = TE.t5_bias_table(m.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight, 32, 32, 128,
                           attention=m.encoder.block[0].layer[0].SelfAttention)
    assert torch.equal(enc.bias_table, ref)


def test_clip_adoption_from_the_genuine_module():
    m = tiny_clip().to(torch.bfloat16)
    assert not any(k.startswith("text_model.") for k in m.state_dict())
    enc = TE.HipClipTextModel(m, device="cpu")
    a = m.encoder.layers[0].self_attn
    assert torch.equal(enc.layers[0]["wqkv"], torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight]))
    assert torch.equal(enc.layers[0]["bqkv"], torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias]))
    assert enc.max_length == 77 and enc.eos == 2 and enc.scale == 0.125
    # the older layout with the `text_model.` prefix is the same module
    sd = {"text_model." + k: v for k, v in m.state_dict().items()}
    enc2 = TE.HipClipTextModel(sd, device="cpu", config=m.config)
    assert torch.equal(enc2.layers[1]["w2"], m.encoder.layers[1].mlp.fc2.weight)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,why", [
    (dict(feed_forward_proj="relu"), "non-gated or ReLU"),
    (dict(feed_forward_proj="gated-silu"), "gated-GELU"),
    (dict(d_kv=32), "head dim 32"),
])
def test_t5_refuses_what_it_does_not_implement(kw, why):
    m = tiny_t5(**kw).to(torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match=why):
        TE.HipT5EncoderModel(m, device="cpu")


def test_refusals_name_the_reason():
    t5 = tiny_t5()                                                            # fp32 weights
    with pytest.raises(_lib.RegionEHipError, match="non-bf16 weights"):
        TE.HipT5EncoderModel(t5, device="cpu")
    clip = tiny_clip(hidden_act="gelu").to(torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="quick_gelu"):
        TE.HipClipTextModel(clip, device="cpu")
    clip = tiny_clip(num_attention_heads=4).to(torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="head dim 32"):
        TE.HipClipTextModel(clip, device="cpu")
    m = tiny_clip().to(torch.bfloat16)
    sd = dict(m.state_dict())
    sd["encoder.layers.0.self_attn.q_proj.lora_A.weight"] = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="LoRA"):
        TE.HipClipTextModel(sd, device="cpu", config=m.config)
    sd = dict(m.state_dict())
    del sd["encoder.layers.1.mlp.fc1.bias"]
    with pytest.raises(_lib.RegionEHipError, match="missing"):
        TE.HipClipTextModel(sd, device="cpu", config=m.config)
    t5 = tiny_t5().to(torch.bfloat16)
    sd = dict(t5.state_dict())
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"].clone() + 1
    with pytest.raises(_lib.RegionEHipError, match="differ"):
        TE.HipT5EncoderModel(sd, device="cpu", config=t5.config)


def test_call_refusals_come_before_any_kernel():
    m = tiny_t5().to(torch.bfloat16)
    enc = TE.HipT5EncoderModel(m, device="cpu", max_length=16)
    ids = torch.zeros(1, 8, dtype=torch.int64)
    for kw, why in ((dict(attention_mask=torch.ones(1, 8)), "attention_mask"), (dict(output_hidden_states=True), "output_hidden_states"),
                    (dict(position_ids=ids), "position_ids")):
        with pytest.raises(_lib.RegionEHipError, match=why):
            enc(ids, **kw)
    with pytest.raises(_lib.RegionEHipError, match="sequence length 17"):
        enc(torch.zeros(1, 17, dtype=torch.int64))


# ---- the CLIP pooled row ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eos", [2, 49])
def test_pooled_index_matches_transformers(eos):
    m = tiny_clip(eos_token_id=eos)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(3, 90, (4, 20), generator=g)
    ids[0, 7] = eos
    ids[1, 3] = eos
    ids[1, 12] = eos                                   # a repeated eos: the first one
    ids[2, 5] = 95                                     # the largest id (eos 2: argmax picks it)
    ids[2, 9] = 95
    ids[3] = torch.where(ids[3] == eos, torch.full_like(ids[3], 4), ids[3])   # no eos at all
    with torch.no_grad():
        out = m(ids)
    idx = TE.pooled_index(ids, eos)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(4), idx])


# ---- the adapter ------------------------------------------------------------------------------------------------------------------
class _Host:
    pass


def test_adapter_keeps_host_modules_it_does_not_cover_with_one_warning_each():
    h = _Host()
    h.text_encoder = tiny_clip(hidden_act="gelu").to(torch.bfloat16)
    h.text_encoder_2 = tiny_t5()                                              # fp32
    with pytest.warns(RuntimeWarning) as rec:
        got = adapters.hip_text_encoders_for(h, "cpu")
    msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert got == (None, None)
    assert len(msgs) == 2 and "text_encoder kept on the host module" in msgs[0] and "quick_gelu" in msgs[0]
    assert "text_encoder_2 kept on the host module" in msgs[1] and "non-bf16" in msgs[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert adapters.hip_text_encoders_for(h, "cpu") == (None, None)          # decided once: no second warning


def test_adapter_without_modules_or_switched_off_is_silent():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert adapters.hip_text_encoders_for(_Host(), "cpu") == (None, None)
        h = _Host()
        h.text_encoder = tiny_clip().to(torch.bfloat16)
        h._regione_hip_text = False
        assert adapters.hip_text_encoders_for(h, "cpu") == (None, None)


def test_adapter_binds_and_restores_even_on_an_exception():
    h = _Host()
    clip, t5 = tiny_clip().to(torch.bfloat16), tiny_t5().to(torch.bfloat16)
    h.text_encoder, h.text_encoder_2 = clip, t5
    hc, ht = adapters.hip_text_encoders_for(h, "cpu")
    assert isinstance(hc, TE.HipClipTextModel) and isinstance(ht, TE.HipT5EncoderModel)
    with pytest.raises(ValueError):
        with adapters._hip_text_encoders(h, "cpu"):
            assert h.text_encoder is hc and h.text_encoder_2 is ht
            raise ValueError("boom")
    assert h.text_encoder is clip and h.text_encoder_2 is t5


def test_adapter_refuses_another_layout_and_peft_layers():
    from transformers import CLIPTextModelWithProjection
    h = _Host()
    torch.manual_seed(0)
    h.text_encoder = CLIPTextModelWithProjection(tiny_clip().config).to(torch.bfloat16)
    clip = tiny_clip().to(torch.bfloat16)
    clip.encoder.layers[0].self_attn.lora_A = torch.nn.Linear(128, 4, bias=False).to(torch.bfloat16)
    h.text_encoder_2 = None
    with pytest.warns(RuntimeWarning, match="another layout"):
        assert adapters.hip_text_encoders_for(h, "cpu") == (None, None)
    h2 = _Host()
    h2.text_encoder = clip
    with pytest.warns(RuntimeWarning, match="LoRA"):
        assert adapters.hip_text_encoders_for(h2, "cpu") == (None, None)


# ---- the new C entries: argument checks without a GPU -------------------------------------------------------------------------------
def test_new_c_entries_validate_arguments_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()
    assert h.rgn_text_attention_bf16(None, P, 8, 2, 1.0, 0, None, 8, None) < 0 and "bad argument" in msg()
    assert h.rgn_text_attention_bf16(P, P, 0, 2, 1.0, 0, None, 8, None) < 0
    assert h.rgn_text_attention_bf16(P, P, 8, 2, 0.0, 0, None, 8, None) < 0 and "scale" in msg()
    assert h.rgn_text_attention_bf16(P, P, 4097, 2, 1.0, 0, None, 4097, None) == -2 and "4096" in msg()
    assert h.rgn_text_attention_bf16(P, P, 100, 2, 1.0, 0, P, 77, None) < 0 and "Lmax" in msg()
    assert h.rgn_text_attention_bf16(P + 2, P, 8, 2, 1.0, 0, None, 8, None) < 0 and "aligned" in msg()
    assert h.rgn_text_embed(None, 8, P, 10, None, 0, P, 64, None) < 0 and "bad argument" in msg()
    assert h.rgn_text_embed(P, 8, P, 10, None, 0, P, 60, None) < 0 and "multiple of 8" in msg()
    assert h.rgn_text_embed(P, 78, P, 10, P, 77, P, 64, None) < 0 and "position table" in msg()
    assert h.rgn_geglu_bf16(P, 100, P, 64, 4, 64, None) < 0 and "ldx >= 2 F" in msg()
    assert h.rgn_geglu_bf16(P, 128, P, 64, 4, 60, None) < 0
    assert h.rgn_geglu_bf16(None, 128, P, 64, 0, 64, None) == 0                       # M = 0: nothing to do
    assert h.rgn_quick_gelu_bf16(None, P, 8, None) < 0 and h.rgn_quick_gelu_bf16(P, P, 0, None) == 0
    assert h.rgn_layer_norm_rows(P, 64, None, P, P, 64, 4, 64, 1e-5, None) < 0 and "layer_norm_rows" in msg()
    assert h.rgn_layer_norm_rows(P, 32, P, P, P, 64, 4, 64, 1e-5, None) < 0
    assert h.rgn_text_pool_row(None, 8, 2, P, 64, 64, P, None) < 0 and "text_pool_row" in msg()
    assert h.rgn_text_pool_row(P, 0, 2, P, 64, 64, P, None) < 0
