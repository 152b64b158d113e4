"""CPU: the host side of HipQwen25VLTextEncoder(weights="fp8") (regione_amd/qwen_text_encoder.py) - what is quantised and what stays bf16,
the per-channel scale of a concatenation, the dequantisation error of the format, the refusal of an unknown format before any library
call, the adapter's `_regione_hip_text_weights` switch - and the argument checks of rgn_lm_gemv_w8 (csrc/decode.hip; no GPU is touched)."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

FP8 = torch.float8_e4m3fn
MATS = ("wqkv", "wo", "wgu", "wdown")


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("adoption and its refusals make no library call")
    monkeypatch.setattr(_lib, "lib", boom)


def _tensors(obj, seen=None):
    """Every tensor reachable from `obj` through attributes, dicts, lists and tuples (the adopted host module aside: it is the caller's)."""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        yield obj
        s = getattr(obj, "_rgn_scale", None)
        if s is not None:
            yield s
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v, seen)
    elif hasattr(obj, "__dict__") and not isinstance(obj, (torch.nn.Module, type)):
        yield from _tensors(vars(obj), seen)


def test_an_unknown_format_is_refused_by_name_before_anything_is_moved(no_library):
    m = HQ.tiny_qwen25vl()
    with pytest.raises(_lib.RegionEHipError, match="int4"):
        QT.HipQwen25VLTextEncoder(m, device="meta", weights="int4")              # a device nothing could be moved to: never reached
    with pytest.raises(_lib.RegionEHipError, match=r"bf16.*fp8"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", weights="FP8")


def test_fp8_adoption_quantises_the_four_matrices_of_every_layer_and_nothing_else(no_library):
    m = HQ.tiny_qwen25vl()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    e8 = QT.HipQwen25VLTextEncoder(sd, device="cpu", config=m.config, weights="fp8")
    e16 = QT.HipQwen25VLTextEncoder(m, device="cpu")
    assert e8.weights == "fp8" and e16.weights == "bf16" and len(e8.layers) == 2
    b8 = b16 = 0
    for i, (p8, p16) in enumerate(zip(e8.layers, e16.layers)):
        for k in MATS:
            q, s = p8[k], p8[k]._rgn_scale
            N = p16[k].shape[0]
            assert q.dtype == FP8 and q.shape == p16[k].shape and q.is_contiguous()
            assert s.dtype == torch.float32 and s.shape == (N,) and s.is_contiguous() and bool((s > 0).all())
            b8 += q.numel() * q.element_size() + s.numel() * s.element_size()
            b16 += p16[k].numel() * p16[k].element_size()
            assert 2 * q.numel() * q.element_size() == p16[k].numel() * p16[k].element_size()
        for k in ("ln1", "ln2", "bqkv"):
            assert p8[k].dtype == torch.bfloat16 and torch.equal(p8[k], p16[k])
        # the scale is per output channel: the concatenation quantises as its parts do
        att = m.model.language_model.layers[i].self_attn
        parts = [ops.quantize_w8(getattr(att, n).weight.data) for n in ("q_proj", "k_proj", "v_proj")]
        assert torch.equal(p8["wqkv"]._rgn_scale, torch.cat([t._rgn_scale for t in parts]))
        assert torch.equal(p8["wqkv"].view(torch.uint8), torch.cat([t.view(torch.uint8) for t in parts]))
    n_rows = sum(p[k].shape[0] for p in e16.layers for k in MATS)
    assert b8 == b16 // 2 + 4 * n_rows                                           # half the bytes, plus one fp32 per output channel
    for e in (e8, e16):
        assert e.tok.dtype == e.final_ln.dtype == torch.bfloat16
        assert e.lm_head is None and e._adopt_lm_head().dtype == torch.bfloat16 and e.lm_head.dtype == torch.bfloat16
    # no bf16 form of a layer matrix is left on the object (the state dict it was adopted from is the caller's, not kept)
    shapes = {tuple(p[k].shape) for p in e16.layers for k in MATS}
    kept = {id(e8.tok), id(e8.lm_head), id(e8._lm_head_src)}                     # [V, d] has the shape of gate|up on the tiny model
    own = [t for t in _tensors(e8) if id(t) not in kept]
    assert sum(t.dtype == FP8 for t in own) == 4 * len(e8.layers)
    assert [tuple(t.shape) for t in own if t.dtype != FP8 and t.dim() == 2 and tuple(t.shape) in shapes] == []
    assert sum(t.numel() * t.element_size() for t in own if t.dtype == FP8) == b16 // 2


def test_dequantisation_error_is_within_the_formats_bound(no_library):
    m = HQ.tiny_qwen25vl()
    e8 = QT.HipQwen25VLTextEncoder(m, device="cpu", weights="fp8")
    e16 = QT.HipQwen25VLTextEncoder(m, device="cpu")
    for p8, p16 in zip(e8.layers, e16.layers):
        for k in MATS:
            w, s = p16[k].double(), p8[k]._rgn_scale.double()[:, None]
            err = (p8[k].float().double() * s - w).abs()
            # 3 mantissa bits: relative 2^-4; below the smallest normal the spacing is 2^-9 (in units of the scale)
            assert bool((err <= 2.0 ** -4 * w.abs() + s * 2.0 ** -9).all()), k
            assert float(p8[k].float().abs().max()) == 448.0                    # every row with a nonzero entry uses the full range


def test_the_default_and_bf16_build_identical_tensors(no_library):
    m = HQ.tiny_qwen25vl()
    a, b = QT.HipQwen25VLTextEncoder(m, device="cpu"), QT.HipQwen25VLTextEncoder(m, device="cpu", weights="bf16")
    assert a.weights == b.weights == "bf16" and torch.equal(a.tok, b.tok) and torch.equal(a.final_ln, b.final_ln)
    for pa, pb in zip(a.layers, b.layers):
        assert set(pa) == set(pb)
        for k in pa:
            assert pa[k].dtype == pb[k].dtype == torch.bfloat16 and torch.equal(pa[k], pb[k]) and not hasattr(pa[k], "_rgn_scale")
    lay = m.model.language_model.layers[0]
    assert a.layers[0]["wo"].data_ptr() == lay.self_attn.o_proj.weight.data_ptr()      # in place, as before: no copy of a single matrix


def test_the_adapter_hands_the_pipelines_format_to_the_constructor(monkeypatch):
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl()
    seen = []

    class Recorder:
        def __init__(self, module, device=None, weights="bf16", **kw):
            seen.append((module, weights))
    monkeypatch.setattr(QT, "HipQwen25VLTextEncoder", Recorder)

    def pipe(**attrs):
        p = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
        p._regione_hip_vision = False                                            # the language model alone
        for k, v in attrs.items():
            setattr(p, k, v)
        return p
    p = pipe(_regione_hip_text_weights="fp8")
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [(m, "fp8")] and p._regione_hip_qwen_text is enc
    assert isinstance(adapters.hip_qwen_text_encoder_for(pipe(), torch.device("cpu")), Recorder) and seen[-1] == (m, "bf16")
    for bad in ("int4", "FP8", None, True):
        p = pipe(_regione_hip_text_weights=bad)
        with pytest.raises(ValueError, match=r"bf16.*fp8"):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 2     # nothing adopted, nothing cached


# ---- rgn_lm_gemv_w8 validates before it launches ---------------------------------------------------------------------------------------
def test_lm_gemv_w8_returns_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address

    def msg():
        return h.rgn_last_error().decode()
    # rgn_lm_gemv_w8(W8, wscale, x, bias, resid, y, N, K, stream)
    assert h.rgn_lm_gemv_w8(None, P, P, None, None, P, 8, 64, None) < 0 and "non-null" in msg() and "lm_gemv_w8" in msg()
    assert h.rgn_lm_gemv_w8(P, None, P, None, None, P, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_w8(P, P, None, None, None, P, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, None, 8, 64, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, 0, 64, None) < 0                          # the ranges of rgn_lm_gemv_bf16
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, -3, 64, None) < 0
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, 8, 0, None) < 0
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, 8, 48, None) < 0
    assert h.rgn_lm_gemv_bf16(P, P, None, None, P, 0, 64, None) < 0 and h.rgn_lm_gemv_bf16(P, P, None, None, P, 8, 48, None) < 0
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, 8, 72, None) < 0 and "multiple of 16" in msg()
    assert h.rgn_lm_gemv_w8(P, P, P, None, None, P, 8, 3592, None) < 0 and "multiple of 16" in msg()
    for bad in ((P + 8, P, P, P), (P, P + 4, P, P), (P, P, P + 2, P), (P, P, P, P + 2)):
        W, s, x, y = bad
        assert h.rgn_lm_gemv_w8(W, s, x, None, None, y, 8, 64, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_gemv_w8(P, P, P, P + 1, None, P, 8, 64, None) < 0 and "aligned" in msg()
