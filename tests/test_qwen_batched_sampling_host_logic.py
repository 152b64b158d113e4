"""CPU: the host side of sampling and repetition penalty over a batch (`batch_sampling=True`; regione_amd/qwen_text_encoder.py) - the
constructor's rules, the unchanged refusal without the opt-in, every new refusal before any library call, the argument checks of
rgn_lm_pick_rows (csrc/decode.hip; no GPU is touched) and the hosted `_regione_hip_text_batch_sampling` switch."""
import math
import os
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = torch.Generator().manual_seed(0)
IDS = torch.randint(3, 990, (3, 12), generator=G)
LEFT = torch.tensor([[1] * 12, [0] * 5 + [1] * 7, [0] * 11 + [1]])
T, B = 4, 3


def _boom():
    raise AssertionError("a refusal must come before any library call")


def _enc(monkeypatch, **gc):
    m = HQ.tiny_qwen25vl()
    for k, v in gc.items():
        setattr(m.generation_config, k, v)
    e = QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=64, sampling=True, max_batch=4, batch_sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    return e


# ---- the constructor --------------------------------------------------------------------------------------------------------------------
def test_batch_sampling_is_a_bool_that_defaults_to_false_and_needs_sampling_and_a_batch():
    m = HQ.tiny_qwen25vl()
    assert QT.HipQwen25VLTextEncoder(m, device="cpu").batch_sampling is False
    assert QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True, max_batch=4).batch_sampling is False
    assert QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True, max_batch=2, batch_sampling=True).batch_sampling is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(_lib.RegionEHipError, match="batch_sampling=.*True or False"):
            QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True, max_batch=4, batch_sampling=bad)
    with pytest.raises(_lib.RegionEHipError, match="batch_sampling=True without sampling=True"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", max_batch=4, batch_sampling=True)
    with pytest.raises(_lib.RegionEHipError, match="batch_sampling=True with max_batch=1"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True, batch_sampling=True)
    with pytest.raises(_lib.RegionEHipError, match="batch_sampling=True with max_batch=1"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True, max_batch=1, batch_sampling=True)


def test_without_the_opt_in_sampling_over_a_batch_is_refused_as_before(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, max_batch=4, sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="sampling=True with B = 3: rgn_lm_pick is one sequence \\(batched picking is not implemented\\)"):
        e.generate(IDS, attention_mask=LEFT, max_new_tokens=T, do_sample=True, temperature=0.7)
    with pytest.raises(_lib.RegionEHipError, match="rgn_lm_pick is one sequence"):
        e.generate(IDS, attention_mask=LEFT, max_new_tokens=T)


# ---- refusals of a batch under the opt-in -------------------------------------------------------------------------------------------------
def _strided():
    u = torch.rand(T, 2 * B)[:, ::2]
    assert tuple(u.shape) == (T, B) and not u.is_contiguous()
    return u


@pytest.mark.parametrize("kw,match", [
    (dict(uniforms=torch.rand(T)), "uniforms must be a contiguous float32 tensor of shape \\(4, 3\\)"),
    (dict(uniforms=torch.rand(T, B + 1)), "shape \\(4, 3\\)"),
    (dict(uniforms=torch.rand(T, B - 1)), "shape \\(4, 3\\)"),
    (dict(uniforms=torch.rand(B, T)), "shape \\(4, 3\\)"),
    (dict(uniforms=_strided()), "contiguous float32 tensor of shape \\(4, 3\\)"),
    (dict(uniforms=torch.rand(T, B, device="meta")), "shape \\(4, 3\\) on cpu"),
    (dict(uniforms=torch.rand(T, B, dtype=torch.float64)), "float32 tensor of shape \\(4, 3\\)"),
    (dict(uniforms=torch.rand(T, B), generator=torch.Generator()), "generator= and uniforms="),
    (dict(generator=7), "generator"),
    (dict(top_k=0), "top_k"),
    (dict(top_p=1.5), "top_p"),
    (dict(temperature=0.0), "temperature"),
    (dict(repetition_penalty=-1.0), "repetition_penalty"),
    (dict(min_p=0.1), "min_p"),
    (dict(num_return_sequences=2), "num_return_sequences"),
    (dict(num_beams=2), "num_beams"),
    (dict(output_scores="yes"), "output_scores"),
    (dict(attention_mask=torch.tensor([[1] * 12, [1] * 7 + [0] * 5, [1] * 12])), "right padding"),
    (dict(input_ids=torch.cat([IDS, IDS[:2]]), attention_mask=None), "max_batch = 4"),
])
def test_a_sampled_batch_refuses_before_any_library_call(monkeypatch, kw, match):
    e = _enc(monkeypatch)
    args = dict(input_ids=IDS, attention_mask=LEFT, max_new_tokens=T, do_sample=True)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        e.generate(**args)


@pytest.mark.parametrize("field,value", [("min_p", 0.05), ("typical_p", 0.9), ("no_repeat_ngram_size", 3), ("num_return_sequences", 2),
                                         ("renormalize_logits", True)])
def test_a_generation_config_field_the_one_sequence_path_refuses_is_refused_for_a_batch(monkeypatch, field, value):
    e = _enc(monkeypatch, **{field: value})
    with pytest.raises(_lib.RegionEHipError, match=f"generation_config.{field}"):
        e.generate(IDS, attention_mask=LEFT, max_new_tokens=T, do_sample=True)
    with pytest.raises(_lib.RegionEHipError, match=f"generation_config.{field}"):
        e.generate(IDS[:1], max_new_tokens=T, do_sample=True)                    # one row of the same adoption: uniforms [T]   


def test_one_row_under_the_opt_in_keeps_the_one_sequence_uniforms(monkeypatch):
    e = _enc(monkeypatch)
    with pytest.raises(_lib.RegionEHipError, match="shape \\(4,\\)"):
        e.generate(IDS[:1], max_new_tokens=T, do_sample=True, uniforms=torch.rand(T, 1))
    with pytest.raises(AssertionError, match="before any library call"):
        e.generate(IDS[:1], max_new_tokens=T, do_sample=True, uniforms=torch.rand(T))


def test_an_accepted_sampled_batch_reaches_the_library(monkeypatch):
    """The library of `_enc` raises: what a batch accepts gets past every refusal (so the refusals above are not vacuous)."""
    e = _enc(monkeypatch, do_sample=True, temperature=0.7, repetition_penalty=1.05)
    for kw in (dict(), dict(uniforms=torch.rand(T, B)), dict(generator=torch.Generator().manual_seed(1)), dict(do_sample=False),
               dict(do_sample=False, repetition_penalty=1.0),
               dict(top_k=20, top_p=0.8, uniforms=torch.rand(T, B), output_scores=True, output_logits=True, return_dict_in_generate=True,
                    eos_token_id=[5, 6], pad_token_id=0, sync_every=3)):
        with pytest.raises(AssertionError, match="before any library call"):
            e.generate(IDS, attention_mask=LEFT, max_new_tokens=T, **kw)
    p = e._pick_plan(None, T, dict(uniforms=torch.rand(T, B)), B)
    assert (p.sample, p.penalty, p.temperature) == (True, 1.05, 0.7) and tuple(p.uniforms.shape) == (T, B)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_pick_is_declared_exported_and_bound_and_the_abi_version_moved():
    text = open(os.path.join(ROOT, "include", "regione_hip.h")).read()
    assert int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 122
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint rgn_lm_pick_rows\s*\(", code)
    assert "rgn_lm_pick_rows" in _lib.SIGNATURES and hasattr(_lib.lib(), "rgn_lm_pick_rows")
    assert len(_lib.SIGNATURES["rgn_lm_pick_rows"]) == 19


def test_the_rows_pick_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address
    big = 1 << 30

    def msg():
        return h.rgn_last_error().decode()

    def pick(z=P, ldl=8, B=2, V=8, seen=P, ss=8, pen=1.05, sample=1, T=0.7, k=20, p=0.8, u=P, tok=P, ts=1, scores=None, lds=0, ws=P, nb=big):
        rc = h.rgn_lm_pick_rows(z, ldl, B, V, seen, ss, pen, sample, T, k, p, u, tok, ts, scores, lds, ws, nb, None)
        assert rc == 0 or (rc == -1 and msg().startswith("lm_pick_rows:")), (rc, msg())
        return rc
    for name in ("z", "seen", "tok", "ws"):
        assert pick(**{name: None}) < 0 and "non-null" in msg(), name
    assert pick(V=0) < 0 and pick(V=-3) < 0
    assert pick(V=(1 << 20) + 1, ldl=1 << 21, ss=1 << 21) < 0 and "1048576" in msg()
    for bad in (0, 9, -1):
        assert pick(B=bad) < 0 and "B outside [1, 8]" in msg(), bad
    assert pick(ldl=7) < 0 and "ldl >= V" in msg()
    assert pick(ss=7) < 0 and "seen_stride >= V" in msg()
    assert pick(ts=0) < 0 and "token_stride >= 1" in msg()
    assert pick(scores=P + 4096, lds=7) < 0 and "lds >= V" in msg()
    assert pick(k=-1) < 0 and "top_k" in msg()
    for bad in (0.0, -0.5, 1.0 + 2.0 ** -40, 1.5, math.nan):
        assert pick(p=bad) < 0 and "top_p" in msg(), bad
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert pick(T=bad) < 0 and "temperature" in msg(), bad
        assert pick(T=bad, sample=0, u=None) < 0 and "temperature" in msg(), bad             # validated whatever `sample` is
        assert pick(pen=bad) < 0 and "penalty" in msg(), bad
    assert pick(u=None) < 0 and "uniform" in msg()
    assert pick(tok=P + 4) < 0 and "aligned" in msg()
    assert pick(z=P + 2) < 0 and "aligned" in msg()
    assert pick(u=P + 1) < 0 and "aligned" in msg()
    assert pick(scores=P + 4096 + 2, lds=8) < 0 and "aligned" in msg()
    # scores_out may not overlap the logits: rows [P, P + 4 (ldl + V)) against [S, S + 4 (lds + V)) at B = 2
    assert pick(scores=P, lds=8) < 0 and "scores_out may not overlap" in msg()
    assert pick(scores=P + 4 * 15, lds=8) < 0 and "overlap" in msg()                          # the last logit of row 1
    assert pick(scores=P - 4 * 15, lds=8) < 0 and "overlap" in msg()                          # the last score of row 1 is the first logit
    assert pick(scores=P + 4 * 8, lds=16, ldl=16) < 0 and "overlap" in msg()                  # interleaved rows are refused too
    assert pick(V=1000, ldl=1000, ss=1000, B=3, nb=3 * 4000 - 1) < 0 and "workspace" in msg() and "B rgn_lm_pick_workspace_bytes" in msg()


# ---- the hosted switch ----------------------------------------------------------------------------------------------------------------------
def test_the_adapter_hands_the_pipelines_batch_sampling_switch_to_the_constructor(monkeypatch):
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
    both = dict(_regione_hip_text_sampling=True, _regione_hip_text_batch=4)
    p = pipe(**both, _regione_hip_text_batch_sampling=True)
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [("bf16", {"sampling": True, "max_batch": 4, "batch_sampling": True})]
    assert p._regione_hip_qwen_text is enc
    adapters.hip_qwen_text_encoder_for(pipe(**both), torch.device("cpu"))
    adapters.hip_qwen_text_encoder_for(pipe(**both, _regione_hip_text_batch_sampling=False), torch.device("cpu"))
    assert seen[1:] == [("bf16", {"sampling": True, "max_batch": 4})] * 2        # absent or False: constructed as before
    adapters.hip_qwen_text_encoder_for(pipe(), torch.device("cpu"))
    assert seen[3:] == [("bf16", {})]
    for bad in (1, 0, "yes", None, 1.0):
        p = pipe(**both, _regione_hip_text_batch_sampling=bad)
        with pytest.raises(ValueError, match="_regione_hip_text_batch_sampling = .*True and False"):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 4     # nothing adopted, nothing cached
    for attrs, missing in ((dict(_regione_hip_text_batch=4), "_regione_hip_text_sampling"),
                           (dict(_regione_hip_text_sampling=True), "_regione_hip_text_batch "),
                           (dict(_regione_hip_text_sampling=True, _regione_hip_text_batch=1), "_regione_hip_text_batch "),
                           (dict(), "_regione_hip_text_sampling")):
        p = pipe(**attrs, _regione_hip_text_batch_sampling=True)
        with pytest.raises(ValueError, match="_regione_hip_text_batch_sampling = True needs pipe\\." + missing):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 4
