"""CPU: the host side of a batched HipQwen25VLTextEncoder.generate (`max_batch=`; regione_amd/qwen_text_encoder.py) - every new refusal
before any library call, the default adoption's refusals unchanged, left-padded positions against the genuine transformers module,
the pad-token resolution, the sequence assembly against transformers' greedy-search rule, and the argument checks of the five `_rows`
entries of csrc/decode.hip (no GPU is touched)."""
import ctypes
import os
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_ENTRIES = ("rgn_lm_gemv_bf16_rows", "rgn_lm_gemv_w8_rows", "rgn_lm_head_argmax_rows", "rgn_lm_kv_append_bf16_rows",
                "rgn_lm_decode_attention_bf16_rows")


def _boom():
    raise AssertionError("a refusal must come before any library call")


@pytest.fixture
def enc(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, max_batch=4)
    monkeypatch.setattr(_lib, "lib", _boom)
    return e


G = torch.Generator().manual_seed(0)
IDS = torch.randint(3, 990, (3, 12), generator=G)
LEFT = torch.tensor([[1] * 12, [0] * 5 + [1] * 7, [0] * 11 + [1]])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(attention_mask=torch.tensor([[1] * 12, [1] * 7 + [0] * 5, [1] * 12])), "right padding"),
    (dict(attention_mask=torch.tensor([[1] * 12, [0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1], [1] * 12])), "holes"),
    (dict(attention_mask=torch.tensor([[1] * 12, [0] * 12, [1] * 12])), "empty row"),
    (dict(attention_mask=torch.ones(3, 11, dtype=torch.int64)), "attention_mask of shape"),
    (dict(input_ids=torch.cat([IDS, IDS[:2]])), "max_batch = 4"),
    (dict(max_new_tokens=53), "row 0: n \\+ max_new_tokens = 65"),               # rows of 12, 7 and 1 valid tokens; max_length 64
    (dict(max_new_tokens=58, attention_mask=LEFT[[2, 1, 0]]), "row 1: n \\+ max_new_tokens = 65"),      # rows of 1, 7 and 12
    (dict(max_new_tokens=0), "max_new_tokens"),
    (dict(do_sample=True), "do_sample"),
    (dict(top_k=5), "top_k"),
    (dict(some_new_argument=1), "some_new_argument"),
    (dict(pad_token_id=7, sync_every=0), "sync_every"),                         # pad_token_id itself is accepted by such an adoption
])
def test_a_batched_generate_refuses_before_any_library_call(enc, kw, match):
    args = dict(input_ids=IDS, attention_mask=LEFT, max_new_tokens=4)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        enc.generate(**args)


def test_sampling_over_a_batch_is_refused_by_name(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, max_batch=4, sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="rgn_lm_pick is one sequence"):
        e.generate(IDS, attention_mask=LEFT, max_new_tokens=4, do_sample=True, temperature=0.7)
    with pytest.raises(_lib.RegionEHipError, match="rgn_lm_pick is one sequence"):
        e.generate(IDS, attention_mask=LEFT, max_new_tokens=4)


def test_image_tokens_in_the_padding_are_refused_and_embeddings_go_to_the_rows_in_order(enc):
    ids = IDS.clone()
    ids[0, 3:5] = HQ.IMAGE
    ids[1, 6] = HQ.IMAGE
    rows = QT.image_rows_left(ids, [12, 7, 1], HQ.IMAGE, 3)
    assert [r.tolist() for r in rows] == [[3, 4], [1], []]                       # counted from each row's first valid token
    with pytest.raises(ValueError, match="tokens: 3, features: 2"):
        QT.image_rows_left(ids, [12, 7, 1], HQ.IMAGE, 2)
    ids[1, 2] = HQ.IMAGE                                                         # in the padded part of row 1
    with pytest.raises(_lib.RegionEHipError, match="padded part"):
        QT.image_rows_left(ids, [12, 7, 1], HQ.IMAGE, 4)
    pos = torch.arange(12).view(1, 1, -1).expand(3, 3, -1)
    with pytest.raises(_lib.RegionEHipError, match="padded part"):
        enc.generate(ids, attention_mask=LEFT, max_new_tokens=4, image_embeds=torch.zeros(4, 256, dtype=torch.bfloat16), position_ids=pos)
    # the existing function keeps its right-padding behaviour
    assert [r.tolist() for r in QT.image_rows(ids, [12, 7, 3], HQ.IMAGE, 4)] == [[3, 4], [2, 6], []]


@pytest.mark.parametrize("bad", [0, 9, -1, True, 2.0, "2", None])
def test_max_batch_is_an_int_in_1_to_8(bad):
    with pytest.raises(_lib.RegionEHipError, match="max_batch"):
        QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_batch=bad)


def test_the_default_adoption_refuses_what_it_refused_word_for_word(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64)
    assert e.max_batch == 1
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="input_ids with B = 2: generate is implemented for B == 1"):
        e.generate(IDS[:2], max_new_tokens=4)
    with pytest.raises(_lib.RegionEHipError, match="attention_mask must be all ones for generate \\(no padding inside a KV cache\\)"):
        e.generate(IDS[1:2], attention_mask=LEFT[1:2], max_new_tokens=4)
    with pytest.raises(_lib.RegionEHipError, match="arguments \\['pad_token_id'\\] are not implemented"):
        e.generate(IDS[:1], max_new_tokens=4, pad_token_id=7)


def test_one_row_under_max_batch_keeps_the_one_row_rules(enc):
    with pytest.raises(_lib.RegionEHipError, match="attention_mask must be all ones"):
        enc.generate(IDS[1:2], attention_mask=LEFT[1:2], max_new_tokens=4)
    with pytest.raises(_lib.RegionEHipError, match="L \\+ max_new_tokens = 65"):
        enc.generate(IDS[:1], max_new_tokens=53)


def test_an_accepted_batch_reaches_the_library(enc):
    """The fixture's library raises: a batch generate accepts gets past every refusal (so the refusals above are not vacuous)."""
    with pytest.raises(AssertionError, match="before any library call"):
        enc.generate(IDS, attention_mask=LEFT, max_new_tokens=52, eos_token_id=[5, 6], pad_token_id=0, sync_every=3)
    with pytest.raises(AssertionError, match="before any library call"):
        enc.generate(IDS, max_new_tokens=4)                                      # no mask: every row is whole


def test_the_adapter_hands_the_pipelines_batch_switch_to_the_constructor(monkeypatch):
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl()
    seen = []

    class Recorder:
        def __init__(self, module, device=None, weights="bf16", **kw):
            seen.append((weights, kw))
    monkeypatch.setattr(QT, "HipQwen25VLTextEncoder", Recorder)

    def pipe(**attrs):
        p = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
        p._regione_hip_vision = False                                            # the language model alone
        for k, v in attrs.items():
            setattr(p, k, v)
        return p
    p = pipe(_regione_hip_text_batch=8, _regione_hip_text_weights="fp8")
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [("fp8", {"max_batch": 8})] and p._regione_hip_qwen_text is enc
    adapters.hip_qwen_text_encoder_for(pipe(), torch.device("cpu"))
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_batch=1), torch.device("cpu"))
    assert seen[1:] == [("bf16", {})] * 2                                        # the default adoption is constructed as before
    for bad in (0, 9, True, 2.0, "4", None):
        p = pipe(_regione_hip_text_batch=bad)
        with pytest.raises(ValueError, match="_regione_hip_text_batch = .*1\\.\\.8"):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 3     # nothing adopted, nothing cached


# ---- positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_image", [True, False])
def test_left_padded_positions_equal_the_modules_and_the_unpadded_rows(with_image):
    m = HQ.tiny_qwen25vl()
    e = QT.HipQwen25VLTextEncoder(m, device="cpu", max_batch=4)
    singles = QB.rows(QB.PROMPTS if with_image else QB.PROMPTS[1:])
    ids, mask, grids, _ = QB.left_padded(singles)
    L = ids.shape[1]
    assert len({s.input_ids.shape[1] for s in singles}) == len(singles) and int(mask.sum()) < mask.numel()
    types = (ids == HQ.IMAGE).int() if with_image else None
    pos = e.position_ids_for(ids, mask, grids, None, types, text_from_mask=True)
    kw = dict(attention_mask=mask, input_ids=ids)
    if with_image:
        kw.update(mm_token_type_ids=types, image_grid_thw=grids)
    want = m._prepare_position_ids_for_generation(ids, kw)                       # [4, B, L]: the text positions, then the three axes
    assert tuple(pos.shape) == (3, len(singles), L) and torch.equal(pos, want[1:])
    new = QT.decode_position_ids(pos, 6)
    for b, s in enumerate(singles):
        n = s.input_ids.shape[1]
        alone = e.position_ids_for(s.input_ids, s.attention_mask, s.image_grid_thw, None,
                                   (s.input_ids == HQ.IMAGE).int() if s.image_grid_thw is not None else None)
        assert torch.equal(pos[:, b, L - n:], alone[:, 0]), b
        assert torch.equal(new[:, b], QT.decode_position_ids(alone, 6)[:, 0]), b
        assert new[0, b].tolist() == list(range(int(alone.max()) + 1, int(alone.max()) + 7))
    if with_image:
        assert int(pos[:, 0].max()) + 1 < singles[0].input_ids.shape[1]          # image tokens share positions: not the text-only arange


def test_left_valid_lengths():
    assert QT.left_valid_lengths(None, 2, 5) == [5, 5]
    assert QT.left_valid_lengths(LEFT, 3, 12) == [12, 7, 1]
    assert QT.left_valid_lengths(LEFT.bool(), 3, 12) == [12, 7, 1]


# ---- pad token and assembly ---------------------------------------------------------------------------------------------------------------
def test_the_pad_token_is_the_argument_then_the_config_then_the_first_eos():
    class GC:
        pad_token_id = 11
    assert QT.resolve_pad_token_id(4, GC, [7, 8]) == 4
    assert QT.resolve_pad_token_id(0, GC, [7, 8]) == 0                           # 0 is an id, not "absent"
    assert QT.resolve_pad_token_id(None, GC, [7, 8]) == 11
    GC.pad_token_id = None
    assert QT.resolve_pad_token_id(None, GC, [7, 8]) == 7
    assert QT.resolve_pad_token_id(None, None, [8]) == 8
    assert QT.resolve_pad_token_id(None, None, []) is None                       # no EOS: no row finishes, nothing is padded
    assert QT.resolve_pad_token_id(torch.tensor(5), None, []) == 5


def _table(seed, T=9, B=4):
    return torch.randint(20, 900, (T, B), generator=torch.Generator().manual_seed(seed))


def _cases():
    prompt = torch.randint(20, 900, (4, 5), generator=torch.Generator().manual_seed(9))
    t = _table(1)
    t[0, :] = 7                                                                  # every row ends at step 0
    yield "eos at step 0", prompt, t, [7], 3, 1
    yield "no row finishes", prompt, _table(2), [7, 8], 3, 9
    t = _table(3)
    t[2, 0], t[5, 2], t[6, 2] = 7, 8, 7                                          # rows 0 and 2 finish, rows 1 and 3 never do
    yield "only some rows finish", prompt, t, [7, 8], 3, 9
    t = _table(4)
    t[1, 0], t[4, 1], t[4, 2], t[6, 3] = 7, 7, 7, 7                              # the pad id IS the eos id
    t[3, 0] = 555                                                                # what the device went on decoding is overwritten
    yield "eos id equal to the pad id", prompt, t, [7], 7, 7
    t = _table(5)
    t[3, :] = 8
    t[1, 1] = 7
    yield "all finish at different steps, two eos ids", prompt, t, [7, 8], 0, 4
    yield "no eos at all", prompt, _table(6), [], None, 9


@pytest.mark.parametrize("name,prompt,table,eos,pad,n_new", list(_cases()), ids=[c[0] for c in _cases()])
def test_the_assembly_is_transformers_greedy_search_rule(name, prompt, table, eos, pad, n_new):
    want = QB.greedy_search_rule(prompt, table, eos, pad)
    got, n = QT.assemble_sequences(prompt, table, eos, pad)
    assert n == n_new and got.dtype == torch.int64 and tuple(got.shape) == (4, 5 + n_new)
    assert torch.equal(got, want), name
    # the cut does not depend on how many further steps the device has already decoded
    for k in range(n_new, table.shape[0] + 1):
        if eos and n_new < table.shape[0]:
            assert torch.equal(QT.assemble_sequences(prompt, table[:k], eos, pad)[0], want), (name, k)
    assert torch.equal(got[:, :5], prompt)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "regione_hip.h")).read()
    assert re.search(r"#define RGN_LM_MAX_BATCH 8\b", text) and QT.MAX_BATCH == 8
    assert int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 121
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = _lib.lib()
    for name in ROWS_ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name


def test_the_rows_entries_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address

    def msg():
        return h.rgn_last_error().decode()

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)
    # rgn_lm_gemv_bf16_rows(W, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream)
    for B in (0, 9, -1):
        assert h.rgn_lm_gemv_bf16_rows(P, P, 64, None, None, 0, P, 8, B, 8, 64, None) < 0 and "B outside [1, 8]" in msg()
    assert h.rgn_lm_gemv_bf16_rows(None, P, 64, None, None, 0, P, 8, 2, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_bf16_rows(P, P, 64, None, None, 0, P, 8, 2, 8, 96, None) < 0 and "multiple of 64" in msg()
    assert h.rgn_lm_gemv_bf16_rows(P, P, 68, None, None, 0, P, 8, 2, 8, 64, None) < 0 and "strides" in msg()      # ldx % 8
    assert h.rgn_lm_gemv_bf16_rows(P, P, 56, None, None, 0, P, 8, 2, 8, 64, None) < 0 and "strides" in msg()      # ldx < K
    assert h.rgn_lm_gemv_bf16_rows(P, P, 64, None, None, 0, P, 12, 2, 8, 64, None) < 0 and "strides" in msg()     # ldy % 8
    assert h.rgn_lm_gemv_bf16_rows(P, P, 64, None, None, 0, P, 8, 2, 16, 64, None) < 0 and "strides" in msg()     # ldy < N
    assert h.rgn_lm_gemv_bf16_rows(P, P, 64, None, P, 4, P, 8, 2, 8, 64, None) < 0 and "strides" in msg()         # ldr with resid
    assert h.rgn_lm_gemv_bf16_rows(P, P + 8, 64, None, None, 0, P, 8, 2, 8, 64, None) < 0 and "aligned" in msg()
    # rgn_lm_gemv_w8_rows(W8, wscale, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream)
    assert h.rgn_lm_gemv_w8_rows(P, P, P, 64, None, None, 0, P, 8, 9, 8, 64, None) < 0 and "B outside [1, 8]" in msg()
    assert h.rgn_lm_gemv_w8_rows(P, None, P, 64, None, None, 0, P, 8, 2, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_w8_rows(P, P, P, 72, None, None, 0, P, 8, 2, 8, 72, None) < 0 and "multiple of 16" in msg()
    assert h.rgn_lm_gemv_w8_rows(P, P, P, 84, None, None, 0, P, 8, 2, 8, 80, None) < 0 and "strides" in msg()
    assert h.rgn_lm_gemv_w8_rows(P, P, P, 64, None, None, 0, P + 2, 8, 2, 8, 64, None) < 0 and "aligned" in msg()
    # rgn_lm_head_argmax_rows(W, X, ldx, B, V, K, token_out, token_stride, logits_out, ldl, workspace, workspace_bytes, stream)
    big = 1 << 30
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 0, 8, 64, P, 1, None, 0, P, big, None) < 0 and "B outside [1, 8]" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 2, 8, 64, None, 1, None, 0, P, big, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 2, 8, 64, P, 0, None, 0, P, big, None) < 0 and "token_stride" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 2, 8, 64, P, 1, P, 7, P, big, None) < 0 and "ldl" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 60, 2, 8, 64, P, 1, None, 0, P, big, None) < 0 and "ldx" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 2, 8, 64, P + 4, 1, None, 0, P, big, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_head_argmax_rows(P, P, 64, 3, 1000, 64, P, 1, None, 0, P, 3 * 250 * 8 - 1, None) < 0 and "workspace" in msg()
    # rgn_lm_kv_append_bf16_rows(QKV, ld, cache, cache_stride, cap, row0_host, B, Hq, Hkv, stream)
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 64 * 256, 64, ints(0, 1), 9, 2, 1, None) < 0 and "B outside [1, 8]" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 64 * 256, 64, None, 2, 2, 1, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 504, P, 64 * 256, 64, ints(0, 1), 2, 2, 1, None) < 0
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 64 * 256, 64, ints(0, 64), 2, 2, 1, None) < 0 and "row0[b]" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 64 * 256, 64, ints(-1, 3), 2, 2, 1, None) < 0 and "row0[b]" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 63 * 256, 64, ints(0, 1), 2, 2, 1, None) < 0 and "cache_stride" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 64 * 256 + 4, 64, ints(0, 1), 2, 2, 1, None) < 0 and "cache_stride" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P, 512, P, 4097 * 256, 4097, ints(0, 1), 2, 2, 1, None) < 0 and "4096" in msg()
    assert h.rgn_lm_kv_append_bf16_rows(P + 4, 512, P, 64 * 256, 64, ints(0, 1), 2, 2, 1, None) < 0 and "aligned" in msg()
    # rgn_lm_decode_attention_bf16_rows(Q, ldq, cache, cache_stride, O, ldo, n_host, B, Hq, Hkv, scale, workspace, workspace_bytes, stream)
    cs = 4096 * 256
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, ints(8, 9), 0, 2, 1, 0.1, P, big, None) < 0 and "B outside [1, 8]" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, None, 2, 2, 1, 0.1, P, big, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, ints(8, 0), 2, 2, 1, 0.1, P, big, None) < 0 and "n[b] outside [1, 4096]" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, ints(4097, 8), 2, 2, 1, 0.1, P, big, None) < 0 and "n[b] outside [1, 4096]" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 508, P, cs, P, 256, ints(8, 9), 2, 2, 1, 0.1, P, big, None) < 0 and "strides" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 128, ints(8, 9), 2, 2, 1, 0.1, P, big, None) < 0 and "strides" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, 8 * 256, P, 256, ints(8, 9), 2, 2, 1, 0.1, P, big, None) < 0 and "cache_stride" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, ints(8, 9), 2, 3, 2, 0.1, P, big, None) < 0 and "Hq % Hkv" in msg()
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P + 8, cs, P, 256, ints(8, 9), 2, 2, 1, 0.1, P, big, None) < 0 and "aligned" in msg()
    one = h.rgn_lm_decode_attention_workspace_bytes(2, 65)
    assert h.rgn_lm_decode_attention_bf16_rows(P, 512, P, cs, P, 256, ints(8, 65), 2, 2, 1, 0.1, P, 2 * one - 1, None) < 0 and "workspace" in msg()
