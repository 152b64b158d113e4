"""CPU: the host side of `HipQwen25VLTextEncoder(sampling=True).generate` (regione_amd/qwen_text_encoder.py) - how the decoding
configuration is resolved against the module's generation_config, every new refusal before any library call, the adapter's
`_regione_hip_text_sampling` switch - the argument checks of rgn_lm_seen_mark / rgn_lm_pick (csrc/decode.hip; no GPU is touched), and
the fp64 model of the pick (tests/lm_pick_model.py) against the installed transformers processors on the same fp32 logits."""
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import lm_pick_model as PM  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

IDS = torch.randint(3, 990, (1, 12), generator=torch.Generator().manual_seed(0))
CONFIGS = [(1.05, 1e-6, 0, 1.0), (1.05, 0.1, 1, 0.001), (1.0, 0.7, 20, 0.8), (1.1, 1.0, 0, 0.9), (1.0, 1.3, 50, 1.0), (1.2, 0.7, 0, 0.95)]


# ---- the entries validate before they launch ------------------------------------------------------------------------------------------
def test_pick_entries_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address
    big = 1 << 30

    def msg():
        return h.rgn_last_error().decode()
    # rgn_lm_seen_mark(ids, n, seen, V, stream)
    assert h.rgn_lm_seen_mark(None, 4, P, 8, None) < 0 and "non-null" in msg() and "lm_seen_mark" in msg()
    assert h.rgn_lm_seen_mark(P, 4, None, 8, None) < 0 and "non-null" in msg()
    assert h.rgn_lm_seen_mark(P, -1, P, 8, None) < 0
    assert h.rgn_lm_seen_mark(P, 4, P, 0, None) < 0
    assert h.rgn_lm_seen_mark(P + 4, 4, P, 8, None) < 0 and "aligned" in msg()
    assert h.rgn_lm_seen_mark(None, 0, None, 8, None) == 0                                    # nothing to mark
    # rgn_lm_pick(logits, V, seen, penalty, sample, temperature, top_k, top_p, uniform, token_out, scores_out, workspace, bytes, stream)
    assert h.rgn_lm_pick_workspace_bytes(1) == 4 and h.rgn_lm_pick_workspace_bytes(152064) == 152064 * 4
    assert h.rgn_lm_pick_workspace_bytes(0) == 0 and h.rgn_lm_pick_workspace_bytes(-5) == 0

    def pick(z=P, V=8, seen=P, pen=1.05, sample=1, T=0.7, k=20, p=0.8, u=P, tok=P, scores=None, ws=P, nb=big):
        return h.rgn_lm_pick(z, V, seen, pen, sample, T, k, p, u, tok, scores, ws, nb, None)
    assert pick(z=None) < 0 and "non-null" in msg() and "lm_pick" in msg()
    assert pick(seen=None) < 0 and "non-null" in msg()
    assert pick(tok=None) < 0 and "non-null" in msg()
    assert pick(ws=None) < 0 and "non-null" in msg()
    assert pick(u=None) < 0 and "uniform" in msg()
    assert pick(V=0) < 0 and pick(V=-3) < 0 and pick(V=(1 << 20) + 1) < 0
    assert pick(k=-1) < 0 and "top_k" in msg()
    for bad in (0.0, -0.5, 1.0 + 2.0 ** -40, 1.5, math.nan):
        assert pick(p=bad) < 0 and "top_p" in msg(), bad
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert pick(T=bad) < 0 and "temperature" in msg(), bad
        assert pick(T=bad, sample=0, u=None) < 0 and "temperature" in msg(), bad             # validated whatever `sample` is
        assert pick(pen=bad) < 0 and "penalty" in msg(), bad
    assert pick(V=1000, nb=3999) < 0 and "workspace" in msg()
    assert pick(tok=P + 4) < 0 and "aligned" in msg()
    assert pick(z=P + 2) < 0 and "aligned" in msg()
    assert pick(scores=P) < 0 and "scores_out" in msg()                                      # scores_out may not be the logits


# ---- argument resolution ----------------------------------------------------------------------------------------------------------------
def _enc(monkeypatch, sampling, **gc):
    m = HQ.tiny_qwen25vl()
    for k, v in gc.items():
        setattr(m.generation_config, k, v)
    e = QT.HipQwen25VLTextEncoder(m, device="cpu", max_length=64, **({"sampling": True} if sampling else {}))

    def boom():
        raise AssertionError("a refusal must come before any library call")
    monkeypatch.setattr(_lib, "lib", boom)
    return e


def test_explicit_arguments_win_and_none_takes_the_modules_generation_config(monkeypatch):
    e = _enc(monkeypatch, True, do_sample=True, temperature=1e-6, repetition_penalty=1.05, top_k=20, top_p=0.8)
    p = e._pick_plan(None, 4, {})
    assert (p.sample, p.penalty, p.temperature, p.top_k, p.top_p) == (True, 1.05, 1e-6, 20, 0.8) and not p.greedy_as_before
    p = e._pick_plan(None, 4, dict(temperature=0.7, top_k=5, top_p=None, repetition_penalty=1.2))
    assert (p.sample, p.penalty, p.temperature, p.top_k, p.top_p) == (True, 1.2, 0.7, 5, 0.8)
    p = e._pick_plan(False, 4, {})
    assert p.sample is False and p.penalty == 1.05 and not p.greedy_as_before               # the penalty applies to greedy search too
    p = e._pick_plan(False, 4, dict(repetition_penalty=1.0))
    assert p.greedy_as_before
    p = e._pick_plan(False, 4, dict(repetition_penalty=1.0, output_scores=True))
    assert not p.greedy_as_before and p.output_scores


def test_a_none_or_absent_config_field_means_the_stage_is_off(monkeypatch):
    e = _enc(monkeypatch, True)
    p = e._pick_plan(None, 4, {})
    assert (p.sample, p.penalty, p.temperature, p.top_k, p.top_p) == (False, 1.0, 1.0, 0, 1.0) and p.greedy_as_before
    p = e._pick_plan(True, 4, {})
    assert (p.sample, p.penalty, p.temperature, p.top_k, p.top_p) == (True, 1.0, 1.0, 0, 1.0) and not p.greedy_as_before
    e.module = None                                                              # adopted from a state dict: no config at all
    p = e._pick_plan(True, 4, dict(top_k=3))
    assert (p.sample, p.penalty, p.top_k) == (True, 1.0, 3)


def test_the_checkpoints_own_settings_reach_the_library_under_sampling_and_are_refused_as_before_without(monkeypatch):
    cfg = dict(do_sample=True, temperature=1e-6, repetition_penalty=1.05)
    e = _enc(monkeypatch, True, **cfg)
    with pytest.raises(AssertionError, match="before any library call"):
        e.generate(IDS, max_new_tokens=4)
    with pytest.raises(AssertionError, match="before any library call"):         # every accepted argument at once
        e.generate(IDS, max_new_tokens=4, do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.1,
                   uniforms=torch.rand(4), return_dict_in_generate=True, output_scores=True, output_logits=True)
    with pytest.raises(AssertionError, match="before any library call"):
        e.generate(IDS, max_new_tokens=4, generator=torch.Generator().manual_seed(1))
    e = _enc(monkeypatch, False, **cfg)
    with pytest.raises(_lib.RegionEHipError, match="generation_config.do_sample is true, pass do_sample=False"):
        e.generate(IDS, max_new_tokens=4)
    for kw, match in ((dict(do_sample=True), "do_sample"), (dict(do_sample=False, temperature=0.7), "temperature"),
                      (dict(do_sample=False, top_k=5), "top_k"), (dict(do_sample=False, top_p=0.5), "top_p"),
                      (dict(do_sample=False, repetition_penalty=1.1), "repetition_penalty: sampling and penalty arguments are not implemented"),
                      (dict(do_sample=False, uniforms=torch.rand(4)), "uniforms"), (dict(do_sample=False, generator=torch.Generator()), "generator"),
                      (dict(do_sample=False, output_scores=True), "output_scores")):
        with pytest.raises(_lib.RegionEHipError, match=match):
            e.generate(IDS, max_new_tokens=4, **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(top_k=0), "top_k"),
    (dict(top_k=-2), "top_k"),
    (dict(top_k=2.0), "top_k"),
    (dict(top_k=True), "top_k"),
    (dict(top_p=0.0), "top_p"),
    (dict(top_p=1.01), "top_p"),
    (dict(top_p=-0.1), "top_p"),
    (dict(temperature=0.0), "temperature"),
    (dict(temperature=-1.0), "temperature"),
    (dict(temperature="hot"), "temperature"),
    (dict(repetition_penalty=0.0), "repetition_penalty"),
    (dict(repetition_penalty=-1.3), "repetition_penalty"),
    (dict(uniforms=torch.rand(5)), "uniforms"),
    (dict(uniforms=torch.rand(1, 4)), "uniforms"),
    (dict(uniforms=torch.rand(4, dtype=torch.float64)), "uniforms"),
    (dict(uniforms=torch.rand(4, device="meta")), "uniforms"),
    (dict(uniforms=[0.1, 0.2, 0.3, 0.4]), "uniforms"),
    (dict(uniforms=torch.rand(4), generator=torch.Generator()), "generator= and uniforms="),
    (dict(generator=7), "generator"),
    (dict(output_scores="yes"), "output_scores"),
    (dict(do_sample="yes"), "do_sample"),
    (dict(min_p=0.1), "min_p"),
    (dict(typical_p=0.9), "typical_p"),
    (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
    (dict(num_beams=4), "num_beams"),
    (dict(logits_processor=[]), "logits_processor"),
    (dict(renormalize_logits=True), "renormalize_logits"),
    (dict(some_new_argument=1), "some_new_argument"),
    (dict(max_new_tokens=0), "max_new_tokens"),
    (dict(streamer=object()), "streamer"),
])
def test_a_sampling_adoption_refuses_before_any_library_call(monkeypatch, kw, match):
    e = _enc(monkeypatch, True)
    args = dict(input_ids=IDS, max_new_tokens=4, do_sample=True)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        e.generate(**args)


@pytest.mark.parametrize("field,value", [("min_p", 0.05), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 3e-4),
                                         ("encoder_repetition_penalty", 1.2), ("no_repeat_ngram_size", 3), ("bad_words_ids", [[5]]),
                                         ("suppress_tokens", [7]), ("min_new_tokens", 2), ("renormalize_logits", True),
                                         ("num_return_sequences", 2), ("penalty_alpha", 0.6), ("num_beams", 3),
                                         ("temperature", 0.0), ("top_k", 0), ("top_p", 1.5), ("repetition_penalty", -1.0)])
def test_a_sampling_adoption_does_not_deviate_silently_from_the_modules_generation_config(monkeypatch, field, value):
    e = _enc(monkeypatch, True, **{field: value})
    with pytest.raises(_lib.RegionEHipError, match=field):
        e.generate(IDS, max_new_tokens=4)


def test_config_values_that_switch_a_stage_off_are_accepted(monkeypatch):
    e = _enc(monkeypatch, True, typical_p=1.0, no_repeat_ngram_size=0, num_return_sequences=1, renormalize_logits=False, min_new_tokens=0,
             num_beams=1, length_penalty=1.0)
    with pytest.raises(AssertionError, match="before any library call"):
        e.generate(IDS, max_new_tokens=4)


def test_sampling_must_be_a_bool_and_defaults_to_false():
    m = HQ.tiny_qwen25vl()
    assert QT.HipQwen25VLTextEncoder(m, device="cpu").sampling is False
    assert QT.HipQwen25VLTextEncoder(m, device="cpu", sampling=True).sampling is True
    with pytest.raises(_lib.RegionEHipError, match="sampling"):
        QT.HipQwen25VLTextEncoder(m, device="cpu", sampling="yes")


def test_the_adapter_hands_the_pipelines_sampling_switch_to_the_constructor(monkeypatch):
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl()
    seen = []

    class Recorder:
        def __init__(self, module, device=None, weights="bf16", sampling=False, **kw):
            seen.append((module, weights, sampling))
    monkeypatch.setattr(QT, "HipQwen25VLTextEncoder", Recorder)

    def pipe(**attrs):
        p = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
        p._regione_hip_vision = False                                            # the language model alone
        for k, v in attrs.items():
            setattr(p, k, v)
        return p
    p = pipe(_regione_hip_text_sampling=True, _regione_hip_text_weights="fp8")
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [(m, "fp8", True)] and p._regione_hip_qwen_text is enc
    adapters.hip_qwen_text_encoder_for(pipe(), torch.device("cpu"))
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_sampling=False), torch.device("cpu"))
    assert seen[1:] == [(m, "bf16", False)] * 2
    for bad in (1, "yes", None, 0):
        p = pipe(_regione_hip_text_sampling=bad)
        with pytest.raises(ValueError, match="_regione_hip_text_sampling"):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 3     # nothing adopted, nothing cached


# ---- the fp64 model against the installed processors -------------------------------------------------------------------------------------
def _cases(V, n=8):
    g = torch.Generator().manual_seed(1000 + V)
    for _ in range(n):
        z = (4 * torch.randn(V, generator=g)).float()
        seen = torch.randint(0, V, (40,), generator=g)
        yield z, seen


def _transformers_scores(z, seen_ids, pen, T, k, top_p=None):
    from transformers.generation import logits_process as LP
    ids, s = seen_ids[None], z[None].clone()
    if pen != 1.0:
        s = LP.RepetitionPenaltyLogitsProcessor(penalty=pen)(ids, s)
    s = LP.TemperatureLogitsWarper(T)(ids, s)
    if k:
        s = LP.TopKLogitsWarper(top_k=k, min_tokens_to_keep=1)(ids, s)
    if top_p is not None and top_p < 1.0:
        s = LP.TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=1)(ids, s)
    return s[0]


@pytest.mark.parametrize("V", [1, 1000, 1024, 152064])
def test_the_model_reproduces_the_penalty_temperature_and_top_k_processors_bit_for_bit(V):
    for pen, T, k, _ in CONFIGS:
        for z, seen in _cases(V):
            got = PM.scores_before_top_p(z, PM.seen_mask(V, seen), pen, True, T, k)
            assert torch.equal(got, _transformers_scores(z, seen, pen, T, k)), (V, pen, T, k)
            if pen != 1.0:                                                       # greedy search: the penalty alone
                from transformers.generation import logits_process as LP
                want = LP.RepetitionPenaltyLogitsProcessor(penalty=pen)(seen[None], z[None].clone())[0]
                assert torch.equal(PM.scores_before_top_p(z, PM.seen_mask(V, seen), pen), want)


@pytest.mark.parametrize("V", [1, 1000, 1024, 152064])
def test_the_model_keeps_what_the_top_p_processor_keeps(V):
    for pen, T, k, top_p in CONFIGS:
        for z, seen in _cases(V):
            m = PM.pick(z, PM.seen_mask(V, seen), pen, True, T, k, top_p)
            want = _transformers_scores(z, seen, pen, T, k, top_p)
            assert torch.equal(m["keep"], want > -math.inf), (V, pen, T, k, top_p)
            assert torch.equal(m["scores"], want)
            assert bool(m["keep"][int(torch.argmax(m["before_top_p"]))])


def test_the_model_takes_equal_scores_together_and_draws_the_lowest_index_past_u():
    s = torch.tensor([0.0, 1.0, 1.0, -math.inf, 3.0])
    p = torch.softmax(s.double(), 0)
    gm = PM.group_mass(s)
    assert gm[1] == gm[2] and abs(float(gm[1]) - float(p[0] + p[1] + p[2])) < 1e-15 and float(gm[3]) == 0.0
    assert PM.top_p_keep(s, 1.0 - float(p[0] + p[1]) - 1e-9).tolist() == [False, True, True, False, True]      # the pair straddles: kept whole
    assert PM.top_p_keep(s, 1.0 - float(p[0] + p[1] + p[2]) - 1e-9).tolist() == [False, False, False, False, True]
    assert PM.top_p_keep(s, 1e-9).tolist() == [False, False, False, False, True]                              # never the largest
    idx, C = PM.cdf(s, PM.top_p_keep(s, 1.0))
    assert idx.tolist() == [0, 1, 2, 4]
    mid = torch.cat([C[:1] / 2, (C[1:] + C[:-1]) / 2])
    assert PM.draw(idx, C, mid).tolist() == [0, 1, 2, 4]
    assert PM.draw(idx, C, torch.tensor([0.0, float(C[0]), 1.0])).tolist() == [0, 1, 4]
