"""`HipQwen25VLTextEncoder(lookup=True, sampling=True, lookup_sampling=True)` on the GPU: drafted tokens verified in one step under
sampling and a repetition penalty.  Every comparison is torch.equal: the sequences, fp32 logits and processed scores of a drafted generate
against the SAME adoption's plain sampled generate with the same uniforms - for the n-gram lookup's own drafts and for forced drafts
(all right, every 3rd wrong, all wrong), with the step counts of the host simulation - and the hosted Step1X-Edit v1p2 thinker."""
import functools
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402
import host_step1x_text_pipeline as H1  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
import qwen_lookup_model as LM  # noqa: E402
from regione_amd import RegionEHelper, _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu

NEW = 12
KS = {"fma": (1, 3, 7), "mfma": (1, 3, 7, 15, 31)}
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.05)
PENALISED = dict(do_sample=False, repetition_penalty=1.3)
ADOPTIONS = [(w, k) for w in ("bf16", "fp8") for k in ("fma", "mfma")]
_module, _prompts, _corrupt = QB.module, QB.prompts, QB.corrupt


@functools.lru_cache(maxsize=None)
def _uniforms(T=NEW):
    return torch.rand(T, generator=torch.Generator().manual_seed(7)).cuda()


@functools.lru_cache(maxsize=None)
def _adoption(weights, kernels, max_length=4096):
    return QT.HipQwen25VLTextEncoder(_module(), weights=weights, batch_kernels=kernels, lookup=True, sampling=True, lookup_sampling=True,
                                     max_length=max_length)


def _full(T, **kw):
    return dict(max_new_tokens=T, return_dict_in_generate=True, output_logits=True, output_scores=True, eos_token_id=[], **kw)


def _bits(ts):
    return torch.cat(ts).view(torch.int32)


def _same(got, want, what):
    assert torch.equal(got.sequences, want.sequences), (what, "sequences")
    assert len(got.logits) == len(want.logits) and len(got.scores) == len(want.scores), (what, "n_new")
    assert torch.equal(_bits(got.logits), _bits(want.logits)), (what, "logits")
    assert torch.equal(_bits(got.scores), _bits(want.scores)), (what, "scores")


@functools.lru_cache(maxsize=None)
def _plain(weights, kernels, pi, mode):
    """The baseline, computed once per adoption and prompt: the plain sampled (or penalised greedy) generate."""
    hip, kw = _adoption(weights, kernels), _prompts()[pi]
    pick = dict(SAMPLED, uniforms=_uniforms()) if mode == "sampled" else PENALISED
    out = hip.generate(**kw, **_full(NEW, **pick))
    assert hip.last_lookup_stats is None and out.sequences.shape[1] == kw["input_ids"].shape[1] + NEW
    return out, pick


@pytest.mark.parametrize("pi", [0, 1], ids=["image", "text"])
@pytest.mark.parametrize("weights,kernels", ADOPTIONS)
def test_drafted_sampled_generates_equal_the_plain_sampled_generate_bit_for_bit(weights, kernels, pi):
    hip, kw = _adoption(weights, kernels), _prompts()[pi]
    L = kw["input_ids"].shape[1]
    plain, pick = _plain(weights, kernels, pi, "sampled")
    assert any(bool(torch.isinf(s).any()) for s in plain.scores)                 # top-k / top-p did filter: these are processed scores
    G = plain.sequences[0, L:].cpu()
    for K in KS[kernels]:
        got = hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, **pick))
        _same(got, plain, (pi, K, "lookup"))
        st = hip.last_lookup_stats
        assert st["tokens"] == NEW == 1 + st["steps"] + st["accepted"] and st["accepted"] <= st["drafted"], st
        for name, guess in (("all accepted", G), ("every 3rd wrong", _corrupt(G, 3)), ("all wrong", _corrupt(G, 1))):
            got = hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, draft_tokens=guess.cuda() if K % 2 else guess, **pick))
            _same(got, plain, (pi, K, name))
            assert hip.last_lookup_stats == LM.simulate_guess(G, guess, K, NEW), (pi, K, name, hip.last_lookup_stats)
    seq = hip.generate(**kw, max_new_tokens=NEW, eos_token_id=[], prompt_lookup_num_tokens=3, draft_tokens=G, **pick)
    assert torch.equal(seq, plain.sequences)                                     # no logits, no scores: the rows in the loop's own buffers


@pytest.mark.parametrize("weights,kernels", ADOPTIONS)
def test_a_penalised_greedy_generate_and_a_seeded_generator_draft_the_same_way(weights, kernels):
    hip, kw = _adoption(weights, kernels), _prompts()[1]
    L = kw["input_ids"].shape[1]
    plain, pick = _plain(weights, kernels, 1, "penalised")
    G = plain.sequences[0, L:].cpu()
    top = KS[kernels][-1]
    for K in (3, top):
        _same(hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, **pick)), plain, (K, "penalised lookup"))
        for name, guess in (("all accepted", G), ("every 3rd wrong", _corrupt(G, 3)), ("all wrong", _corrupt(G, 1))):
            _same(hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, draft_tokens=guess, **pick)), plain, (K, "penalised", name))
            assert hip.last_lookup_stats == LM.simulate_guess(G, guess, K, NEW), (K, name)
    for gdev in ("cpu", "cuda"):
        want = hip.generate(**kw, **_full(NEW, generator=torch.Generator(device=gdev).manual_seed(3), **SAMPLED))
        Gs = want.sequences[0, L:].cpu()
        for guess in (Gs, _corrupt(Gs, 3)):
            got = hip.generate(**kw, **_full(NEW, generator=torch.Generator(device=gdev).manual_seed(3), prompt_lookup_num_tokens=top,
                                             draft_tokens=guess, **SAMPLED))
            _same(got, want, (gdev, "generator"))
            assert hip.last_lookup_stats == LM.simulate_guess(Gs, guess, top, NEW)


@pytest.mark.parametrize("kernels", ["fma", "mfma"])
def test_an_eos_inside_an_accepted_run_cuts_the_sequence_as_the_plain_loop_does(kernels):
    hip = _adoption("bf16", kernels)
    for pi, kw in enumerate(_prompts()):
        L = kw["input_ids"].shape[1]
        pick = dict(SAMPLED, uniforms=_uniforms())
        G = _plain("bf16", kernels, pi, "sampled")[0].sequences[0, L:].cpu()
        eos = int(G[4])                                                          # new token 4 (or an earlier equal one): inside the first run of 7
        cut = G.tolist().index(eos) + 1
        args = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, output_scores=True, eos_token_id=[eos], **pick)
        want = hip.generate(**kw, **args)
        assert want.sequences.shape[1] == L + cut and len(want.logits) == cut == len(want.scores)
        _same(hip.generate(**kw, **args, prompt_lookup_num_tokens=7, draft_tokens=G), want, "eos in a forced run")
        st = hip.last_lookup_stats               # the prefill's token, then ONE step of 8 rows (7 drafts and the token after them), then the cut
        assert (st["steps"], st["accepted"], st["tokens"]) == ((1, 7, 9) if cut > 1 else (0, 0, 1)), st
        _same(hip.generate(**kw, **args, prompt_lookup_num_tokens=7), want, "eos with lookup drafts")
        _same(hip.generate(**kw, **args, prompt_lookup_num_tokens=7, draft_tokens=_corrupt(G, 1)), want, "eos with wrong drafts")


@pytest.mark.parametrize("kernels", ["fma", "mfma"])
def test_the_last_token_lands_on_max_length_exactly(kernels):
    """max_new_tokens in {1, 2, K, K + 1} under an adoption whose max_length is L + max_new_tokens: no cache row, logits row, scores row,
    uniform or id past the end, with every draft right (the longest steps) and with the lookup's own drafts."""
    kw = _prompts()[1]
    L = kw["input_ids"].shape[1]
    u = _uniforms(33)
    G = _adoption("bf16", kernels).generate(**kw, **_full(33, uniforms=u, **SAMPLED)).sequences[0, L:].cpu()
    for K in KS[kernels]:
        for T in sorted({1, 2, K, K + 1}):
            hip = _adoption("bf16", kernels, L + T)
            pick = dict(SAMPLED, uniforms=u[:T].clone())
            want = hip.generate(**kw, **_full(T, **pick))
            assert torch.equal(want.sequences[0, L:].cpu(), G[:T])               # position-indexed uniforms: a prefix of the long run
            _same(hip.generate(**kw, **_full(T, prompt_lookup_num_tokens=K, draft_tokens=G, **pick)), want, (K, T, "guess"))
            assert hip.last_lookup_stats == LM.simulate_guess(G[:T], G, K, T), (K, T)
            _same(hip.generate(**kw, **_full(T, prompt_lookup_num_tokens=K, **pick)), want, (K, T, "lookup"))
            with pytest.raises(_lib.RegionEHipError, match="exceeds max_length"):
                hip.generate(**kw, **_full(T + 1, prompt_lookup_num_tokens=K, **dict(SAMPLED, uniforms=u[:T + 1].clone())))


@pytest.mark.parametrize("kernels", ["fma", "mfma"])
def test_a_greedy_call_under_the_switch_is_the_greedy_lookup_adoptions_call(kernels):
    kw = _prompts()[1]
    greedy = QT.HipQwen25VLTextEncoder(_module(), batch_kernels=kernels, lookup=True)
    args = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, eos_token_id=[], prompt_lookup_num_tokens=3)
    want = greedy.generate(**kw, **args)
    got = _adoption("bf16", kernels).generate(**kw, **args, do_sample=False)
    assert torch.equal(got.sequences, want.sequences) and torch.equal(_bits(got.logits), _bits(want.logits)) and got.scores is None
    assert _adoption("bf16", kernels).last_lookup_stats == greedy.last_lookup_stats


def test_a_module_whose_generation_config_asks_for_prompt_lookup_drafts_without_the_argument():
    torch.manual_seed(0)
    m = HQ.tiny_qwen25vl(layers=2).cuda()
    m.generation_config.prompt_lookup_num_tokens = 3
    kw = _prompts()[1]
    on = QT.HipQwen25VLTextEncoder(m, lookup=True, sampling=True, lookup_sampling=True)
    off = QT.HipQwen25VLTextEncoder(m, lookup=True, sampling=True)
    pick = dict(SAMPLED, uniforms=_uniforms())
    want = off.generate(**kw, **_full(NEW, **pick))
    assert off.last_lookup_stats is None                                         # without the switch the config's field is not read
    _same(on.generate(**kw, **_full(NEW, **pick)), want, "the config's K")
    assert on.last_lookup_stats is not None and on.last_lookup_stats["tokens"] == NEW
    with pytest.raises(_lib.RegionEHipError, match="drafts are verified against greedy search only"):
        off.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=3, **pick))     # and the refusal is what it was


# ---- hosted Step1X-Edit v1p2: the thinker's generate drafts under the module's sampling generation_config ---------------------------------
def _enabled(text_encoder, **attrs):
    pipe = H1.Step1XEditPipelineV1P2(HS.stub_trunk("step1x"), text_encoder)
    for k, v in attrs.items():
        setattr(pipe, k, v)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
    assert [str(r.message) for r in rec if "kept on the host module" in str(r.message)] == []
    return pipe, helper


class _SeededThinker(H1.ToyThinker):
    """A ToyThinker whose generate is handed fixed uniforms: the same draws with and without drafts."""

    def _say(self, images, text):
        images = [i.detach().float().cpu() for i in images]
        mi = self.processor(text=[text], images=images, padding=True, return_tensors="pt").to(self.model.device)
        u = torch.rand(self.new_tokens, generator=torch.Generator().manual_seed(9)).to(self.model.device)
        ids = self.model.generate(**mi, max_new_tokens=self.new_tokens, uniforms=u)
        words = " ".join(f"w{int(i)}" for i in ids[0, mi.input_ids.shape[1]:])
        self.said.append((mi, ids, words, self.model.last_lookup_stats))
        return words


def test_the_hosted_thinker_says_the_same_words_with_the_lookup_switches_on():
    said = {}
    for on in (False, True):
        m = HQ.tiny_qwen25vl()
        gc = m.generation_config
        gc.do_sample, gc.temperature, gc.top_k, gc.top_p, gc.repetition_penalty = True, 0.7, 20, 0.8, 1.05
        gc.prompt_lookup_num_tokens = 3
        attrs = dict(_regione_hip_text_lookup=True, _regione_hip_text_lookup_sampling=True) if on else {}
        pipe, helper = _enabled(m, **attrs)
        enc = pipe._regione_hip_qwen_text
        assert enc.sampling is True and enc.lookup is on and enc.lookup_sampling is on
        pipe._regione_thinker = _SeededThinker(enc, pipe.processor)
        out = pipe(image=torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(5)), prompt="turn the sky deep green",
                   generator=torch.Generator().manual_seed(1), output_type="latent", enable_thinking_mode=True, enable_reflection_mode=False)
        (mi, ids, words, stats), = pipe._regione_thinker.said
        assert out.reformat_prompt == words and len(words.split()) == H1.THINK_TOKENS
        assert (stats is not None) is on, stats
        said[on] = (ids.cpu(), words)
        helper.disable()
    assert torch.equal(said[True][0], said[False][0]) and said[True][1] == said[False][1]
