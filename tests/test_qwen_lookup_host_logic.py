"""CPU: the host side of prompt-lookup drafts in HipQwen25VLTextEncoder.generate (`lookup=True`; regione_amd/qwen_text_encoder.py) - the
numpy model of rgn_lm_lookup_step (tests/qwen_lookup_model.py) against transformers' PromptLookupCandidateGenerator, the defects the
model's hand-computed cases catch, every new refusal before any library call, the default adoption's refusal unchanged, the hosted
pipeline's switch, and the argument checks of the two new entries of csrc/decode.hip (no GPU is touched)."""
import os
import re

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import qwen_lookup_model as LM  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = torch.randint(3, 990, (2, 12), generator=torch.Generator().manual_seed(0))


def _boom():
    raise AssertionError("a refusal must come before any library call")


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_the_model_proposes_what_transformers_prompt_lookup_proposes():
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    rng = np.random.default_rng(31)
    hits = 0
    for i in range(3000):
        vocab, n = int(rng.integers(3, 6)), int(rng.integers(1, 201))
        max_ngram, K = int(rng.integers(1, 5)), int(rng.integers(1, 32))
        seq = rng.integers(0, vocab, n)
        gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=K, max_matching_ngram_size=max_ngram, max_length=1 << 20)
        cand, _ = gen.get_candidates(torch.from_numpy(seq)[None])
        want = cand[0, n:].tolist()
        # the model through its step: seq[0, n - 1) settled, one row, its argmax is the last id - so n' = n
        buf = np.concatenate([seq[:n - 1], np.full(40, 777)])
        a, drafts, toks, after = LM.step(buf, n - 1, [int(seq[-1])], 1 << 20, K, max_ngram) if n > 1 else \
            (0, LM.propose(seq, n, K, max_ngram), [int(seq[0])], seq)
        assert a == 0 and drafts == want, (i, seq.tolist(), max_ngram, K, drafts, want)
        hits += bool(want)
    assert hits > 2000                                                           # matches are common over 3 to 5 ids


def test_the_hand_computed_cases_hold_and_each_defect_breaks_one():
    for c in LM.CASES:
        assert LM.case_holds(c), c["name"]
    for d in LM.DEFECTS:
        broken = [c["name"] for c in LM.CASES if not LM.case_holds(c, d)]
        assert broken, f"no case catches the defect {d!r}"


def test_the_simulated_loop_counts_steps_and_accepted_drafts():
    G = list(range(100, 110))                                                    # T = 10 greedy tokens
    assert LM.simulate_guess(G, G, 3, 10) == dict(steps=3, drafted=6, accepted=6, tokens=10)      # 1, then 4 + 4, then the last token alone: no room for a draft before the end
    assert LM.simulate_guess(G, [0] * 10, 3, 10) == dict(steps=9, drafted=3 * 6 + 2 + 1 + 0, accepted=0, tokens=10)
    assert LM.simulate_guess(G, G, 7, 1) == dict(steps=0, drafted=0, accepted=0, tokens=1)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def enc(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, lookup=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    return e


@pytest.mark.parametrize("kw,match", [
    (dict(prompt_lookup_num_tokens=0), "prompt_lookup_num_tokens=0 \\(an int in \\[1, 7\\] under batch_kernels=\"fma\""),
    (dict(prompt_lookup_num_tokens=8), "prompt_lookup_num_tokens=8 \\(an int in \\[1, 7\\]"),
    (dict(prompt_lookup_num_tokens=True), "prompt_lookup_num_tokens=True"),
    (dict(prompt_lookup_num_tokens=2.0), "prompt_lookup_num_tokens=2.0"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0), "max_matching_ngram_size=0 \\(an int in \\[1, 8\\]\\)"),
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=9), "max_matching_ngram_size=9"),
    (dict(max_matching_ngram_size=2), "max_matching_ngram_size without prompt_lookup_num_tokens"),
    (dict(draft_tokens=torch.zeros(4, dtype=torch.int32)), "draft_tokens must be a 1-D int64 tensor"),
    (dict(draft_tokens=torch.zeros(1, 4, dtype=torch.int64)), "draft_tokens must be a 1-D int64 tensor"),
    (dict(draft_tokens=torch.zeros(0, dtype=torch.int64)), "draft_tokens must be a 1-D int64 tensor"),
    (dict(draft_tokens=[1, 2, 3]), "draft_tokens must be a 1-D int64 tensor"),
    (dict(prompt_lookup_num_tokens=3, input_ids=IDS), "B = 2"),
    (dict(prompt_lookup_num_tokens=3, do_sample=True), "do_sample"),
    (dict(prompt_lookup_num_tokens=3, repetition_penalty=1.2), "repetition_penalty"),
    (dict(prompt_lookup_num_tokens=3, output_scores=True), "output_scores"),
    (dict(prompt_lookup_num_tokens=3, assistant_model=object()), "assistant_model"),
    (dict(prompt_lookup_num_tokens=3, max_new_tokens=53), "L \\+ max_new_tokens = 65"),
])
def test_a_lookup_generate_refuses_before_any_library_call(enc, kw, match):
    args = dict(input_ids=IDS[:1], max_new_tokens=4)
    args.update(kw)
    with pytest.raises(_lib.RegionEHipError, match=match):
        enc.generate(**args)


def test_the_range_of_k_follows_the_kernel_family(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, lookup=True, batch_kernels="mfma")
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="an int in \\[1, 31\\] under batch_kernels=\"mfma\""):
        e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=32)
    with pytest.raises(AssertionError, match="before any library call"):         # 31 is accepted: the call gets to the library
        e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=31)


def test_drafts_over_a_batch_or_a_sampled_pick_are_refused_by_name(monkeypatch):
    b = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, lookup=True, max_batch=4)
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64, lookup=True, sampling=True)
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="B = 2: drafts are verified for one sequence"):
        b.generate(IDS, max_new_tokens=4, prompt_lookup_num_tokens=3)
    for kw in (dict(do_sample=True), dict(repetition_penalty=1.3), dict(output_scores=True)):
        with pytest.raises(_lib.RegionEHipError, match="drafts are verified against greedy search only"):
            e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, **kw)
    with pytest.raises(_lib.RegionEHipError, match="assistant_model"):
        e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, assistant_model=object())
    with pytest.raises(AssertionError, match="before any library call"):         # a configuration that is greedy as before is accepted
        e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=False, repetition_penalty=1.0)


def test_an_accepted_lookup_generate_reaches_the_library_and_none_runs_the_plain_loop(enc, monkeypatch):
    for kw in (dict(prompt_lookup_num_tokens=7), dict(prompt_lookup_num_tokens=1, max_matching_ngram_size=8),
               dict(draft_tokens=torch.zeros(3, dtype=torch.int64)), dict(draft_tokens=torch.zeros(3, dtype=torch.int64), prompt_lookup_num_tokens=2)):
        with pytest.raises(AssertionError, match="before any library call"):
            enc.generate(IDS[:1], max_new_tokens=4, **kw)
    called = []
    monkeypatch.setattr(enc, "_generate_lookup", lambda *a, **k: called.append(1))
    with pytest.raises(AssertionError, match="before any library call"):         # no K, no guess: today's loop
        enc.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=None, draft_tokens=None)
    assert not called


@pytest.mark.parametrize("bad", [0, 1, "yes", None])
def test_lookup_is_a_bool(bad):
    with pytest.raises(_lib.RegionEHipError, match="lookup="):
        QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", lookup=bad)


def test_the_default_adoption_refuses_the_lookup_arguments_word_for_word(monkeypatch):
    e = QT.HipQwen25VLTextEncoder(HQ.tiny_qwen25vl(), device="cpu", max_length=64)
    assert e.lookup is False
    monkeypatch.setattr(_lib, "lib", _boom)
    with pytest.raises(_lib.RegionEHipError, match="arguments \\['prompt_lookup_num_tokens'\\] are not implemented"):
        e.generate(IDS[:1], max_new_tokens=4, prompt_lookup_num_tokens=3)
    with pytest.raises(_lib.RegionEHipError, match="arguments \\['draft_tokens', 'max_matching_ngram_size'\\] are not implemented"):
        e.generate(IDS[:1], max_new_tokens=4, max_matching_ngram_size=2, draft_tokens=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.RegionEHipError, match="assistant_model: sampling and penalty arguments are not implemented"):
        e.generate(IDS[:1], max_new_tokens=4, assistant_model=object())


def test_the_adapter_hands_the_pipelines_lookup_switch_to_the_constructor(monkeypatch):
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
    p = pipe(_regione_hip_text_lookup=True, _regione_hip_text_batch_kernels="mfma")
    enc = adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
    assert isinstance(enc, Recorder) and seen == [("bf16", {"batch_kernels": "mfma", "lookup": True})] and p._regione_hip_qwen_text is enc
    adapters.hip_qwen_text_encoder_for(pipe(), torch.device("cpu"))
    adapters.hip_qwen_text_encoder_for(pipe(_regione_hip_text_lookup=False), torch.device("cpu"))
    assert seen[1:] == [("bf16", {})] * 2                                        # the default adoption is constructed as before
    for bad in (0, 1, "yes", None):
        p = pipe(_regione_hip_text_lookup=bad)
        with pytest.raises(ValueError, match="_regione_hip_text_lookup = .*True and False are accepted"):
            adapters.hip_qwen_text_encoder_for(p, torch.device("cpu"))
        assert "_regione_hip_qwen_text" not in p.__dict__ and len(seen) == 3     # nothing adopted, nothing cached


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_lookup_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "regione_hip.h")).read()
    assert int(re.search(r"#define RGN_ABI_VERSION (\d+)", text).group(1)) >= 123
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    h = _lib.lib()
    for name in ("rgn_lm_verify_attention_bf16", "rgn_lm_lookup_step"):
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert QT.MAX_NGRAM == 8


def test_the_lookup_entries_return_codes_and_messages_without_touching_the_gpu():
    h = _lib.lib()
    P = 0x10000                                          # a plausible, 16-byte aligned, never dereferenced address
    big = 1 << 30

    def msg():
        return h.rgn_last_error().decode()
    # rgn_lm_verify_attention_bf16(Q, ldq, cache, O, ldo, n0, R, Hq, Hkv, scale, workspace, workspace_bytes, stream)
    def verify(Q=P, ldq=512, cache=P, O=P, ldo=512, n0=5, R=3, Hq=4, Hkv=2, scale=0.1, ws=P, wsb=big):
        return h.rgn_lm_verify_attention_bf16(Q, ldq, cache, O, ldo, n0, R, Hq, Hkv, scale, ws, wsb, None)
    for k in ("Q", "cache", "O", "ws"):
        assert verify(**{k: None}) == -1 and "non-null" in msg()
    assert verify(scale=0.0) == -1 and "0 < scale < inf" in msg()
    assert verify(Hq=3) == -1 and "Hq % Hkv" in msg()
    assert verify(Hq=18, Hkv=2, ldq=18 * 128, ldo=18 * 128) == -1 and "Hq / Hkv > 8" in msg()
    for R in (0, 9, -1):
        assert verify(R=R) == -1 and "R outside [1, 8]" in msg()
    assert verify(n0=0) == -1 and "n0 + r cache rows" in msg()
    assert verify(n0=4095, R=3) == -1 and "[1, 4096]" in msg()                   # the last row would see 4097
    assert verify(n0=4096, R=2) == -1 and "[1, 4096]" in msg()
    assert verify(ldq=511 * 1) == -1 and "ldq and ldo" in msg()
    assert verify(ldq=504) == -1 and "ldq and ldo" in msg()
    assert verify(ldo=516) == -1 and "ldq and ldo" in msg()
    assert verify(Q=P + 8) == -1 and "16-byte aligned" in msg()
    assert verify(ws=P + 4) == -1 and "16-byte aligned" in msg()
    one = h.rgn_lm_decode_attention_workspace_bytes(4, 7)
    assert verify(wsb=3 * one - 1) == -1 and "workspace smaller than R" in msg()
    # rgn_lm_lookup_step(seq, n, R, head, head_stride, limit, K, max_ngram, guess, guess_len, L, result, stream)
    def look(seq=P, n=10, R=2, head=P, hs=1, limit=20, K=3, ngram=2, guess=None, glen=0, L=4, result=P):
        return h.rgn_lm_lookup_step(seq, n, R, head, hs, limit, K, ngram, guess, glen, L, result, None)
    for k in ("seq", "head", "result"):
        assert look(**{k: None}) == -1 and "non-null" in msg()
    assert look(hs=0) == -1 and "head_stride >= 1" in msg()
    for R in (0, 33):
        assert look(R=R, limit=100) == -1 and "R outside [1, 32]" in msg()
    for K in (-1, 32):
        assert look(K=K) == -1 and "K outside [0, 31]" in msg()
    for g in (0, 9):
        assert look(ngram=g) == -1 and "max_ngram outside [1, 8]" in msg()
    assert look(n=0, L=0) == -1 and "n + R <= limit" in msg()
    assert look(L=11) == -1 and "n + R <= limit" in msg()
    assert look(limit=11) == -1 and "n + R <= limit" in msg()                    # n + R = 12: the step's last token would lie past the run
    assert look(guess=P, glen=-1) == -1 and "guess_len" in msg()
    assert look(glen=3) == -1 and "guess_len" in msg()
    assert look(seq=P + 4) == -1 and "8-byte aligned" in msg()
    assert look(guess=P + 4, glen=3) == -1 and "8-byte aligned" in msg()
