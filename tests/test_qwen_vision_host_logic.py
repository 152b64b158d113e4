"""CPU: the host side of the HIP Qwen2.5-VL vision tower (regione_amd/qwen_vision.py) against the genuine transformers module - the
parameter table, the zero padding and its inverse, the rotary table and the segment lists (bit-equal to what the module hands its
blocks), the attention item tables, the refusals with their reasons, and the argument checks of the four new C entries (no GPU is touched)."""
import copy
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib, adapters  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402
from regione_amd import qwen_vision as QV  # noqa: E402

GRIDS = ([[1, 18, 22]], [[1, 4, 4], [1, 6, 10]], [[1, 28, 28]])


def vision_config(**kw):
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLVisionConfig
    v = dict(depth=2, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=256, patch_size=14, spatial_merge_size=2,
             temporal_patch_size=2, window_size=56, fullatt_block_indexes=[1], in_channels=3)
    v.update(kw)
    return Qwen2_5_VLVisionConfig(**v)


HEAD80 = dict(depth=4, hidden_size=320, intermediate_size=856, num_heads=4, out_hidden_size=256, window_size=112, fullatt_block_indexes=[1, 3])
FULL = dict(depth=32, hidden_size=1280, intermediate_size=3420, num_heads=16, out_hidden_size=3584, window_size=112,
            fullatt_block_indexes=[7, 15, 23, 31])


def tower(cfg, dtype=torch.bfloat16, seed=7):
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel
    torch.manual_seed(seed)
    return Qwen2_5_VisionTransformerPretrainedModel(cfg).eval().to(dtype)


# ---- parameter shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, HEAD80], ids=["tiny", "head80"])
def test_param_shapes_equal_the_genuine_state_dict(kw):
    cfg = vision_config(**kw)
    m = tower(cfg)
    assert QV.vision_param_shapes(cfg) == {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_param_shapes_of_the_composite_model_carry_the_visual_prefix():
    m = HQ.tiny_qwen25vl()
    want = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("model.visual.")}
    assert QV.vision_param_shapes(m.config, "model.visual.") == want


# ---- padding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, HEAD80], ids=["tiny", "head80"])
def test_padding_is_zero_and_unpadding_returns_the_original_bits(kw):
    cfg = vision_config(**kw)
    m = tower(cfg)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    pw = QV.pad_weights(sd, cfg)
    back = QV.unpad_weights(pw, cfg)
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    d, H, F = cfg.hidden_size, cfg.num_heads, cfg.intermediate_size
    hd, K = d // H, 3 * 2 * 14 * 14
    Dp, Fp, Kp = QV.padded_widths(cfg)
    assert Dp % 32 == 0 and Fp % 64 == 0 and Kp % 64 == 0 and 0 <= Dp - hd < 32 and 0 <= Fp - F < 64 and 0 <= Kp - K < 64
    if kw:
        assert (Dp, Fp, Kp) == (96, 896, 1216)
    assert pw["patch"].shape == (d, Kp) and not pw["patch"][:, K:].any()
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        assert pw[b + "wqkv"].shape == (3 * H * Dp, d) and pw[b + "bqkv"].shape == (3 * H * Dp,) and pw[b + "wproj"].shape == (d, H * Dp)
        assert not pw[b + "wqkv"].reshape(3, H, Dp, d)[:, :, hd:].any() and not pw[b + "bqkv"].reshape(3, H, Dp)[:, :, hd:].any()
        assert not pw[b + "wproj"].reshape(d, H, Dp)[:, :, hd:].any()
        assert pw[b + "wgu"].shape == (2 * Fp, d) and pw[b + "bgu"].shape == (2 * Fp,) and pw[b + "wdown"].shape == (d, Fp)
        assert not pw[b + "wgu"].reshape(2, Fp, d)[:, F:].any() and not pw[b + "bgu"].reshape(2, Fp)[:, F:].any()
        assert not pw[b + "wdown"][:, F:].any()
    assert all(v.dtype == torch.bfloat16 and v.is_contiguous() for v in pw.values())


def test_the_full_size_widths():
    assert QV.padded_widths(vision_config(**FULL)) == (96, 3456, 1216)


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _captured(m, grid):
    """What the genuine forward hands a window block and a full-attention block."""
    seen = {}

    def hook(i):
        def f(mod, args, kwargs):
            seen[i] = (kwargs["cu_seqlens"].clone(), tuple(t.clone() for t in kwargs["position_embeddings"]))
        return f
    handles = [blk.register_forward_pre_hook(hook(i), with_kwargs=True) for i, blk in enumerate(m.blocks)]
    g = torch.tensor(grid)
    N = int((g[:, 1] * g[:, 2]).sum())
    with torch.no_grad():
        m(torch.zeros(N, 1176, dtype=next(m.parameters()).dtype), g)
    for h in handles:
        h.remove()
    return seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("grid", GRIDS, ids=["18x22", "4x4+6x10", "28x28"])
@pytest.mark.parametrize("kw", [{}, HEAD80], ids=["tiny", "head80"])
def test_tables_equal_what_the_module_hands_its_blocks(kw, grid, dtype):
    cfg = vision_config(**kw)
    m = tower(cfg, dtype)
    seen = _captured(m, grid)
    tab = QV.vision_tables(cfg, m.rotary_pos_emb.inv_freq.detach(), torch.tensor(grid))
    full, win = cfg.fullatt_block_indexes[0], 0
    cos, sin = seen[win][1]
    assert cos.dtype == dtype and tab["cos"].dtype == torch.float32 and tab["cos"].shape == cos.shape
    assert torch.equal(tab["cos"], cos.float()) and torch.equal(tab["sin"], sin.float())          # bit for bit
    assert torch.equal(seen[full][1][0], cos)                                                       # every block gets the same table
    assert tab["cu_window_seqlens"].tolist() == seen[win][0].tolist()
    assert tab["cu_seqlens"].tolist() == seen[full][0].tolist()
    N = cos.shape[0]
    assert sorted(tab["patch_rows"].tolist()) == list(range(N)) and sorted(tab["window_index"].tolist()) == list(range(N // 4))
    x = torch.arange(N)                                                            # `hidden_states[window_index]` on rows of merge^2
    want = x.reshape(N // 4, 4)[tab["window_index"]].reshape(N)
    got = torch.empty(N, dtype=torch.int64)
    got[tab["patch_rows"]] = x
    assert torch.equal(got, want)


def test_the_window_list_of_an_18_by_22_grid():
    cfg = vision_config(**HEAD80)
    tab = QV.vision_tables(cfg, QV.default_inv_freq(cfg), torch.tensor([[1, 18, 22]]))
    assert tab["cu_window_seqlens"].tolist() == [0, 64, 128, 176, 240, 304, 352, 368, 384, 396]
    assert tab["cu_seqlens"].tolist() == [0, 396]
    assert torch.equal(QV.default_inv_freq(cfg), tower(cfg, torch.float32).rotary_pos_emb.inv_freq)


# ---- item tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cu", [[0, 1], [0, 4, 20, 84, 148, 160], [0, 60, 130, 133], [0, 777], [0, 64, 128, 176, 240, 304, 352, 368, 384, 396]])
def test_items_cover_every_row_once_inside_one_segment(cu):
    items = QV.attention_items(cu)
    assert items.dtype == torch.int32 and items.shape[1] == 4 and items.is_contiguous()
    owner = torch.zeros(cu[-1], dtype=torch.int64)
    for q0, nq, lo, hi in items.tolist():
        assert 1 <= nq <= 64
        seg = [(a, b) for a, b in zip(cu[:-1], cu[1:]) if a <= q0 < b]
        assert seg == [(lo, hi)] and q0 + nq <= hi                                # no item crosses a segment; its keys are the segment
        owner[q0:q0 + nq] += 1
    assert bool((owner == 1).all())


def test_items_of_a_grid_follow_its_segment_lists():
    cfg = vision_config(**HEAD80)
    tab = QV.vision_tables(cfg, QV.default_inv_freq(cfg), torch.tensor([[1, 4, 4], [1, 6, 10]]))
    assert tab["items_full"].tolist() == [[0, 16, 0, 16], [16, 60, 16, 76]]
    assert torch.equal(tab["items_window"], QV.attention_items(tab["cu_window_seqlens"].tolist()))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_vision_refusal_names_each_config_it_does_not_cover():
    assert QV.vision_refusal(vision_config()) is None and QV.vision_refusal(vision_config(**FULL)) is None
    assert QV.vision_refusal(vision_config(**HEAD80)) is None and QV.vision_refusal(HQ.tiny_qwen25vl().config) is None
    assert "hidden_act 'gelu'" in QV.vision_refusal(vision_config(hidden_act="gelu"))
    assert "not a multiple of 64" in QV.vision_refusal(vision_config(hidden_size=96, num_heads=2))
    assert "not divisible by num_heads" in QV.vision_refusal(vision_config(hidden_size=128, num_heads=3))
    assert "head width 12" in QV.vision_refusal(vision_config(hidden_size=192, num_heads=16))
    assert "head width 256" in QV.vision_refusal(vision_config(hidden_size=512, num_heads=2))
    assert "out_hidden_size 100" in QV.vision_refusal(vision_config(out_hidden_size=100))


def test_adoption_and_call_refusals_name_the_reason():
    cfg = vision_config()
    m = tower(cfg)
    t = QV.HipQwen25VLVisionTower(m, device="cpu")
    assert t.dtype == torch.bfloat16 and (t.d, t.H, t.hd, t.Dp, t.Fp, t.Kp, t.K) == (64, 2, 32, 32, 128, 1216, 1176)
    assert t.inv_freq.dtype == torch.bfloat16 and torch.equal(t.inv_freq, m.rotary_pos_emb.inv_freq)
    whole = HQ.tiny_qwen25vl()
    t2 = QV.HipQwen25VLVisionTower(whole, device="cpu")                           # `model.visual.*` of the composite module
    assert torch.equal(t2.w["blocks.1.wproj"], whole.model.visual.blocks[1].attn.proj.weight)
    t3 = QV.HipQwen25VLVisionTower(dict(whole.state_dict()), device="cpu", config=whole.config)
    assert torch.equal(t3.w["merger.w2"], t2.w["merger.w2"]) and torch.equal(t3.inv_freq, QV.default_inv_freq(whole.config))
    with pytest.raises(_lib.RegionEHipError, match="non-bf16 weights"):
        QV.HipQwen25VLVisionTower(tower(cfg, torch.float32), device="cpu")
    with pytest.raises(_lib.RegionEHipError, match="hidden_act"):
        QV.HipQwen25VLVisionTower(tower(vision_config(hidden_act="gelu")), device="cpu")
    sd = dict(m.state_dict())
    sd["blocks.0.attn.qkv.lora_A.weight"] = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_lib.RegionEHipError, match="LoRA"):
        QV.HipQwen25VLVisionTower(sd, device="cpu", config=cfg)
    sd = dict(m.state_dict())
    del sd["merger.mlp.2.bias"]
    with pytest.raises(_lib.RegionEHipError, match="missing"):
        QV.HipQwen25VLVisionTower(sd, device="cpu", config=cfg)
    px = torch.zeros(16, 1176)
    with pytest.raises(_lib.RegionEHipError, match="videos"):
        t(torch.zeros(32, 1176), torch.tensor([[2, 4, 4]]))
    with pytest.raises(_lib.RegionEHipError, match="pixel_values of shape"):
        t(px[:15], torch.tensor([[1, 4, 4]]))
    with pytest.raises(_lib.RegionEHipError, match="multiples of spatial_merge_size"):
        t(px[:12], torch.tensor([[1, 4, 3]]))
    with pytest.raises(_lib.RegionEHipError, match="exceed max_patches"):
        QV.HipQwen25VLVisionTower(m, device="cpu", max_patches=8)(px, torch.tensor([[1, 4, 4]]))
    with pytest.raises(_lib.RegionEHipError, match="not implemented"):
        t(px, torch.tensor([[1, 4, 4]]), output_hidden_states=True)


# ---- the adapter ------------------------------------------------------------------------------------------------------------------
class _Host:
    def __init__(self, m):
        self.text_encoder = m


def test_the_adapter_adopts_the_tower_with_the_language_model():
    m = HQ.tiny_qwen25vl()
    host = _Host(m)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        enc = adapters.hip_qwen_text_encoder_for(host, "cpu")
    assert [str(r.message) for r in rec if "kept on the host module" in str(r.message)] == []
    assert isinstance(enc, QT.HipQwen25VLTextEncoder) and isinstance(enc.vision, QV.HipQwen25VLVisionTower)
    assert adapters.hip_qwen_text_encoder_for(host, "cpu") is enc                 # once per host
    assert QT.HipQwen25VLTextEncoder(m, device="cpu").vision is None              # the default keeps the module's eager tower


def test_the_adapter_keeps_the_host_tower_on_request_or_with_one_warning():
    host = _Host(HQ.tiny_qwen25vl())
    host._regione_hip_vision = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        enc = adapters.hip_qwen_text_encoder_for(host, "cpu")
    assert rec == [] and isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.vision is None
    m = HQ.tiny_qwen25vl()
    cfg = copy.deepcopy(m.config)
    cfg.vision_config.hidden_act = "gelu"
    m.config = cfg
    host = _Host(m)
    with pytest.warns(RuntimeWarning, match="vision tower kept on the host module: hidden_act 'gelu'") as rec:
        enc = adapters.hip_qwen_text_encoder_for(host, "cpu")
    assert len([r for r in rec if "kept on the host module" in str(r.message)]) == 1
    assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.vision is None      # the language model is still adopted
    host = _Host(HQ.tiny_qwen25vl())
    host._regione_hip_text = False                                                # "all host"
    assert adapters.hip_qwen_text_encoder_for(host, "cpu") is None


# ---- argument checks of the C entries: a bad argument returns a code and a message, nothing is launched ------------------------------
def test_the_new_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    keep = torch.zeros(64, dtype=torch.int32)
    buf = (keep.data_ptr() + 15) // 16 * 16                                         # host memory: never dereferenced on a refusal
    cases = [
        (lib.rgn_vision_attention_bf16(None, buf, 4, 2, 32, 0.1, buf, 1, None), "vision_attention: bad argument"),
        (lib.rgn_vision_attention_bf16(buf, buf, 4, 2, 32, 0.0, buf, 1, None), "vision_attention: bad argument"),
        (lib.rgn_vision_attention_bf16(buf, buf, 4, 2, 80, 0.1, buf, 1, None), "Dp must be 32, 64, 96 or 128"),
        (lib.rgn_vision_attention_bf16(buf, buf + 2, 4, 2, 32, 0.1, buf, 1, None), "16-byte aligned"),
        (lib.rgn_vision_rope_bf16(buf, 192, buf, buf, 4, 2, 20, 32, None), "vision_rope: bad argument"),
        (lib.rgn_vision_rope_bf16(buf, 100, buf, buf, 4, 2, 32, 32, None), "vision_rope: bad argument"),
        (lib.rgn_vision_rope_bf16(buf, 192, buf + 4, buf, 4, 2, 32, 32, None), "16-byte aligned"),
        (lib.rgn_gelu_erf_bf16(None, buf, 8, None), "gelu_erf: null pointer"),
        (lib.rgn_cast_pad_rows(buf, 0, 8, buf, 2, 8, 12, None), "cast_pad_rows: bad argument"),
        (lib.rgn_cast_pad_rows(buf, 7, 8, buf, 2, 8, 16, None), "cast_pad_rows: bad argument"),
        (lib.rgn_cast_pad_rows(buf, 0, 4, buf, 2, 8, 16, None), "cast_pad_rows: bad argument"),
    ]
    for rc, msg in cases:
        assert rc != 0
    for call, msg in [(lambda: lib.rgn_vision_attention_bf16(buf, buf, 4, 2, 80, 0.1, buf, 1, None), "Dp must be 32, 64, 96 or 128"),
                      (lambda: lib.rgn_cast_pad_rows(buf, 0, 8, buf, 2, 8, 12, None), "cast_pad_rows: bad argument")]:
        assert call() != 0 and msg in lib.rgn_last_error().decode()
    assert lib.rgn_vision_attention_bf16(buf, buf, 4, 2, 32, 0.1, buf, 0, None) == 0          # nothing to do
    assert lib.rgn_gelu_erf_bf16(buf, buf, 0, None) == 0 and lib.rgn_cast_pad_rows(buf, 0, 8, buf, 0, 8, 16, None) == 0
