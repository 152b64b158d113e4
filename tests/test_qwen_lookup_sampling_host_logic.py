"""CPU: the host side of `HipQwen25VLTextEncoder(lookup=True, sampling=True, lookup_sampling=True)` (regione_amd/qwen_text_encoder.py) -
the switch's validation, the refusals that stay word for word without it, the calls that reach the library with it, the module's
generation_config.prompt_lookup_num_tokens honoured under it alone, the hosted pipeline's switch, and the two new entries of
csrc/decode.hip declared, exported, bound and refusing bad arguments (no GPU is touched)."""
import os
import re

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = torch.randint(3, 990, (2, 12), generator=torch.Generator().manual_seed(0))
REACHED = "before any library call"


def _boom():
    raise AssertionError("a refusal must come before any library call")


def _enc(module=None, **kw):
    return QT.HipQwen25VLTextEncoder(module if module is not None else HQ.tiny_qwen25vl(), device="cpu", max_length=64, **kw)


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 1, "yes", None])
def test_lookup_sampling_is_a_bool(bad):
    with pytest.raises(_lib.RegionEHipError, match="lookup_sampling=.*\\(True or False\\)"):
        _enc(lookup=True, sampling=True, lookup_sampling=bad)


def test_lookup_sampling_needs_both_other_switches():
    with pytest.raises(_lib.RegionEHipError, match="lookup_sampling=True without lookup=True"):
        _enc(sampling=True, lookup_sampling=True)
    with pytest.raises(_lib.RegionEHipError, match="lookup_sampling=True without sampling=True"):
        _enc(lookup=True, lookup_sampling=True)
    with pytest.raises(_lib.RegionEHipError, match="lookup_sampling=True without lookup=True"):
        _enc(lookup_sampling=True)
    e = _enc(lookup=True, sampling=True, lookup_sampling=True)
    assert e.lookup_sampling is True and _enc(lookup=True, sampling=True).lookup_sampling is False and _enc().lookup_sampling is False


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
SAMPLED = (dict(do_sample=True), dict(repetition_penalty=1.3), dict(output_scores=True))


def test_without_the_switch_the_three_refusals_stay_word_for_word(monkeypatch):
    e = _enc(lookup=True, sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    want = ("HipQwen25VLTextEncoder: prompt_lookup_num_tokens / draft_tokens with sampling, a repetition penalty or output_scores: drafts are "
            "verified against greedy search only")
    for kw in SAMPLED:
        with pytest.raises(_lib.RegionEHipError) as info:
            e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, **kw)
        assert want in str(info.value), str(info.value)


def test_with_the_switch_those_calls_reach_the_library(monkeypatch):
    e = _enc(lookup=True, sampling=True, lookup_sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    u = torch.rand(4)
    for kw in SAMPLED + (dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05, uniforms=u, output_scores=True),
                         dict(do_sample=True, generator=torch.Generator().manual_seed(1)),
                         dict(do_sample=False, repetition_penalty=1.0)):        # greedy as before: the greedy lookup path
        with pytest.raises(AssertionError, match=REACHED):
            e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, **kw)
        with pytest.raises(AssertionError, match=REACHED):
            e.generate(IDS[:1], max_new_tokens=4, draft_tokens=torch.zeros(3, dtype=torch.int64), **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(input_ids=IDS), "B = 2"),
    (dict(prompt_lookup_num_tokens=0), "prompt_lookup_num_tokens=0 \\(an int in \\[1, 7\\] under batch_kernels=\"fma\""),
    (dict(prompt_lookup_num_tokens=8), "prompt_lookup_num_tokens=8 \\(an int in \\[1, 7\\]"),
    (dict(assistant_model=object()), "assistant_model"),
    (dict(top_k=0), "top_k=0 \\(an int >= 1\\)"),
    (dict(temperature=0.0), "temperature=0.0 \\(a number > 0\\)"),
    (dict(uniforms=torch.rand(5)), "uniforms must be a contiguous float32 tensor of shape \\(4,\\)"),
    (dict(uniforms=torch.rand(4), generator=torch.Generator()), "generator= and uniforms= together"),
    (dict(min_p=0.1), "min_p"),
])
def test_with_the_switch_everything_else_is_still_refused_by_name(monkeypatch, kw, match):
    e = _enc(lookup=True, sampling=True, lookup_sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    args = dict(input_ids=IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        e.generate(**args)


def test_a_batch_is_refused_under_every_adoption_that_has_the_switch(monkeypatch):
    b = _enc(lookup=True, sampling=True, lookup_sampling=True, max_batch=4, batch_sampling=True)
    w = _enc(lookup=True, sampling=True, lookup_sampling=True, batch_kernels="mfma")
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="B = 2: drafts are verified for one sequence"):
        b.generate(IDS, max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(_lib.RegionEHipError, match="B = 2"):
        w.generate(IDS, max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True)
    with pytest.raises(_lib.RegionEHipError, match="an int in \\[1, 31\\] under batch_kernels=\"mfma\""):
        w.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=32, do_sample=True)
    with pytest.raises(AssertionError, match=REACHED):
        w.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=31, do_sample=True)


# ---- the module's generation_config ---------------------------------------------------------------------------------------------------
def test_the_configs_prompt_lookup_num_tokens_is_honoured_under_the_switch_and_ignored_without_it(monkeypatch):
    m = HQ.tiny_qwen25vl()
    m.generation_config.prompt_lookup_num_tokens, m.generation_config.max_matching_ngram_size = 3, 4
    on, off = _enc(m, lookup=True, sampling=True, lookup_sampling=True), _enc(m, lookup=True, sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    for e, want in ((on, [dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=4)]), (off, [])):
        called = []
        monkeypatch.setattr(e, "_generate_lookup", lambda look, *a, **k: called.append(look))
        if want:
            e.generate(IDS[:1], max_new_tokens=4, do_sample=True)
        else:
            with pytest.raises(AssertionError, match=REACHED):                   # the plain loop, as before
                e.generate(IDS[:1], max_new_tokens=4, do_sample=True)
        assert called == want, (e.lookup_sampling, called)
    called = []
    monkeypatch.setattr(on, "_generate_lookup", lambda look, *a, **k: called.append(look))
    on.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=5)           # an argument beats the config's field
    assert called == [dict(prompt_lookup_num_tokens=5, max_matching_ngram_size=4)]
    m.generation_config.prompt_lookup_num_tokens = 9                             # a config the kernels do not take is refused by name
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="prompt_lookup_num_tokens=9 \\(an int in \\[1, 7\\]"):
        on.generate(IDS[:1], max_new_tokens=4, do_sample=True)


# ---- the hosted switch ----------------------------------------------------------------------------------------------------------------
def test_the_adapter_hands_the_pipelines_switch_to_the_constructor(monkeypatch):
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
    p = pipe(_regione_hip_text_lookup=True, _regione_hip_text_sampling=True, _regione_hip_text_lookup_sampling=True)
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [("bf16", {"sampling": True, "lookup": True, "lookup_sampling": True})]
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_lookup=True, _regione_hip_text_sampling=True), torch.device("cpu"))
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_lookup=True, _regione_hip_text_sampling=True,
                                            _regione_hip_text_lookup_sampling=False), torch.device("cpu"))
    assert seen[1:] == [("bf16", {"sampling": True, "lookup": True})] * 2        # absent or False: constructed as before
    # the sampling switch may come from the host's default (what the hosted Step1X-Edit v1p2 call passes)
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_lookup=True, _regione_hip_text_lookup_sampling=True), torch.device("cpu"),
                                       sampling_default=True)
    assert seen[3] == ("bf16", {"sampling": True, "lookup": True, "lookup_sampling": True})
    bad = [(dict(_regione_hip_text_lookup_sampling=v, _regione_hip_text_lookup=True, _regione_hip_text_sampling=True),
            "_regione_hip_text_lookup_sampling = .*True and False are accepted") for v in (0, 1, "yes", None)]
    bad += [(dict(_regione_hip_text_lookup_sampling=True, _regione_hip_text_sampling=True),
             "_regione_hip_text_lookup_sampling = True needs pipe._regione_hip_text_lookup = True"),
            (dict(_regione_hip_text_lookup_sampling=True, _regione_hip_text_lookup=True),
             "_regione_hip_text_lookup_sampling = True needs pipe._regione_hip_text_sampling = True")]
    for attrs, match in bad:
        p = pipe(**attrs)
        with pytest.raises(ValueError, match=match):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 4     # nothing adopted, nothing cached


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "regione_hip.h")).read()
    assert int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 124
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = _lib.lib()
    assert h.rgn_version() >= 124
    for name in ("rgn_lm_pick_verify", "rgn_lm_lookup_step_mark"):
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert len(_lib.SIGNATURES["rgn_lm_lookup_step_mark"]) == len(_lib.SIGNATURES["rgn_lm_lookup_step"]) + 2
    assert len(_lib.SIGNATURES["rgn_lm_pick_verify"]) == 19


def test_the_two_entries_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address
    big = 1 << 30

    def msg():
        return h.rgn_last_error().decode()

    # rgn_lm_pick_verify(logits, ldl, R, V, seen, drafts, penalty, sample, temperature, top_k, top_p, uniform, token_out, token_stride,
    #                    scores_out, lds, workspace, workspace_bytes, stream)
    def verify(z=P, ldl=1000, R=3, V=1000, seen=P, drafts=P, pen=1.1, sample=1, T=0.7, k=20, p=0.8, u=P, tok=P, ts=1, s=None, lds=1000,
               ws=P, wsb=big):
        return h.rgn_lm_pick_verify(z, ldl, R, V, seen, drafts, pen, sample, T, k, p, u, tok, ts, s, lds, ws, wsb, None)
    for k in ("z", "seen", "tok", "ws"):
        assert verify(**{k: None}) == -1 and "non-null" in msg()
    for R in (0, 33, -1):
        assert verify(R=R) == -1 and "outside [1, 32]" in msg()
    assert verify(V=0) == -1 and verify(V=(1 << 20) + 1) == -1 and "1 <= V <= 1048576" in msg()
    assert verify(ldl=999) == -1 and "ldl >= V" in msg()
    assert verify(s=P + (1 << 24), lds=999) == -1 and "lds >= V" in msg()
    assert verify(ts=0) == -1 and "token_stride >= 1" in msg()
    assert verify(pen=0.0) == -1 and "repetition penalty" in msg()
    assert verify(T=0.0) == -1 and "temperature" in msg()
    assert verify(k=-1) == -1 and "top_k" in msg()
    assert verify(p=0.0) == -1 and verify(p=1.5) == -1 and "top_p" in msg()
    assert verify(u=None) == -1 and "uniform non-null" in msg()
    assert verify(tok=P + 4) == -1 and "8-byte" in msg()
    assert verify(z=P + 2) == -1 and "4-byte aligned" in msg()
    assert verify(s=P + 4000, lds=1000) == -1 and "scores_out may not overlap the logits" in msg()
    assert verify(s=P) == -1 and "scores_out may not" in msg()
    assert verify(wsb=3 * h.rgn_lm_pick_workspace_bytes(1000) - 1) == -1 and "workspace smaller" in msg()
    assert verify(drafts=None) == -1 and "drafts must be non-null and 8-byte aligned when R > 1" in msg()
    assert verify(drafts=P + 4) == -1 and "drafts must be non-null and 8-byte aligned when R > 1" in msg()

    # rgn_lm_lookup_step_mark(seq, n, R, head, head_stride, limit, K, max_ngram, guess, guess_len, L, result, seen, V, stream)
    def look(seq=P, n=10, R=2, head=P, hs=1, limit=20, K=3, ngram=2, guess=None, glen=0, L=4, result=P, seen=P, V=1000):
        return h.rgn_lm_lookup_step_mark(seq, n, R, head, hs, limit, K, ngram, guess, glen, L, result, seen, V, None)
    for k in ("seq", "head", "result"):
        assert look(**{k: None}) == -1 and "lm_lookup_step_mark" in msg() and "non-null" in msg()
    for R in (0, 33):
        assert look(R=R, limit=100) == -1 and "R outside [1, 32]" in msg()
    assert look(K=32) == -1 and "K outside [0, 31]" in msg()
    assert look(ngram=9) == -1 and "max_ngram outside [1, 8]" in msg()
    assert look(limit=11) == -1 and "n + R <= limit" in msg()
    assert look(glen=3) == -1 and "guess_len" in msg()
    assert look(seq=P + 4) == -1 and "8-byte aligned" in msg()
    for V in (0, (1 << 20) + 1):
        assert look(V=V) == -1 and "1 <= V <= 1048576 with a byte map" in msg()
