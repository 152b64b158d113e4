"""`HipQwen25VLTextEncoder(lookup=True)` on the GPU: drafted tokens verified in one step.  Every comparison is torch.equal.
  rgn_lm_verify_attention_bf16   every row against the one-row entry rgn_lm_decode_attention_bf16 at n0 + r (bf16 bits), NaN bit patterns
                                 in every cache row no query may see, sentinels beside Q and O, and an exact probe
  rgn_lm_lookup_step             against the numpy model of tests/qwen_lookup_model.py: the hand-computed cases, every accept pattern for
                                 R <= 8, both propose modes, the clamp, sentinels around `seq` and the result buffer
  generate                       sequences and fp32 logits against the SAME adoption's plain greedy generate, for lookup drafts and forced
                                 drafts (all right, every 3rd wrong, all wrong), with the step counts of the host simulation"""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_qwen_text_pipeline as HQ  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
import qwen_lookup_model as LM  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = (0x7FC0, 0xFFFF, 0x7F81)                                              # quiet, negative all-ones and signalling bf16 NaNs
SENT = 0x1234


def _bits(t):
    return t.view(torch.int16)


def _st():
    return ops._stream()


# ---- verify attention -------------------------------------------------------------------------------------------------------------------
CAP = 4100                                                                       # four rows past the longest legal cache


@functools.lru_cache(maxsize=None)
def _base_cache(Hkv):
    g = torch.Generator(device="cuda").manual_seed(5 + Hkv)
    return torch.randn(CAP, 2 * Hkv * 128, device="cuda", generator=g).bfloat16()


def _poisoned(Hkv, nmax):
    """The seeded cache with NaN bit patterns in every row from nmax on."""
    c = _base_cache(Hkv).clone()
    nan = torch.tensor(NAN_BITS, dtype=torch.int32, device="cuda").to(torch.int16)
    rows = CAP - nmax
    _bits(c)[nmax:] = nan[torch.arange(rows * c.shape[1], device="cuda") % 3].view(rows, -1)
    return c


def _verify(Q, cache, n0, R, Hq, Hkv, ldo):
    h = _lib.lib()
    scale = 128 ** -0.5
    O = torch.empty(R, ldo, dtype=torch.bfloat16, device="cuda")
    _bits(O).fill_(SENT)
    wsb = R * h.rgn_lm_decode_attention_workspace_bytes(Hq, n0 + R - 1)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device="cuda")
    _lib.check(h.rgn_lm_verify_attention_bf16(Q.data_ptr(), Q.stride(0), cache.data_ptr(), O.data_ptr(), ldo, n0, R, Hq, Hkv, scale,
                                              ws.data_ptr(), wsb, _st()), "rgn_lm_verify_attention_bf16")
    return O


def _one_row(q, cache, n, Hq, Hkv):
    h = _lib.lib()
    O = torch.empty(Hq * 128, dtype=torch.bfloat16, device="cuda")
    wsb = h.rgn_lm_decode_attention_workspace_bytes(Hq, n)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device="cuda")
    _lib.check(h.rgn_lm_decode_attention_bf16(q.data_ptr(), cache.data_ptr(), O.data_ptr(), n, Hq, Hkv, 128 ** -0.5, ws.data_ptr(), wsb, _st()),
               "rgn_lm_decode_attention_bf16")
    return O


@pytest.mark.parametrize("Hq,Hkv", [(28, 4), (8, 1), (2, 2)])
def test_every_verified_row_has_the_bits_of_the_one_row_entry(Hq, Hkv):
    g = torch.Generator(device="cuda").manual_seed(Hq)
    w = Hq * 128
    ldq, ldo = w + 8, w + 16
    for R in range(1, 9):
        for n0 in (1, 2, 57, 63, 64, 65, 127, 128, 4096 - R + 1):
            nmax = n0 + R - 1
            cache = _poisoned(Hkv, nmax)
            Q = torch.randn(R, ldq, device="cuda", generator=g).bfloat16()
            _bits(Q)[:, w:] = 0x7FC0                                             # beside the queries: never read
            O = _verify(Q, cache, n0, R, Hq, Hkv, ldo)
            assert bool((_bits(O)[:, w:] == SENT).all()), (R, n0, "columns past Hq 128 of O were written")
            for r in range(R):
                want = _one_row(Q[r, :w].clone(), cache, n0 + r, Hq, Hkv)
                assert torch.equal(_bits(O[r, :w]), _bits(want)), (R, n0, r)
            assert not bool(torch.isnan(O[:, :w].float()).any()), (R, n0)
            if (R, n0) in ((8, 63), (3, 4094)):                                  # a second call on the same inputs
                assert torch.equal(_bits(_verify(Q, cache, n0, R, Hq, Hkv, ldo)), _bits(O)), (R, n0)


@pytest.mark.parametrize("base", [0, 64])
def test_a_key_far_above_the_rest_returns_its_value_row_to_the_queries_that_see_it(base):
    """Key base + 60 scores 128 x 4 x 4 / sqrt(128) = 181 above the others' 0: p = 1 and exp(-181) = 0 in fp32, so a query that sees it
    returns V[base + 60] bit for bit; n0 = base + 58 and R = 5: queries 3 and 4 see it, queries 0..2 average the rows they see."""
    Hq, Hkv, R, key = 8, 2, 5, base + 60
    n0 = key - 2
    cache = _poisoned(Hkv, n0 + R - 1)
    cache[:n0 + R - 1, :Hkv * 128] = 0
    cache[key, :Hkv * 128] = 4.0
    Q = torch.full((R, Hq * 128), 4.0, dtype=torch.bfloat16, device="cuda")
    O = _verify(Q, cache, n0, R, Hq, Hkv, Hq * 128)
    G = Hq // Hkv
    for r in range(R):
        for hq in range(Hq):
            v = cache[key, (Hkv + hq // G) * 128:(Hkv + hq // G + 1) * 128]
            same = torch.equal(_bits(O[r, hq * 128:(hq + 1) * 128]), _bits(v))
            assert same == (n0 + r > key), (r, hq)


# ---- the lookup step --------------------------------------------------------------------------------------------------------------------
def _run_step(seq, n, head, limit, K, ngram, guess=None, L=0, hs=1):
    """The kernel on seq (a list; the run ends at `limit`, what follows is kept as it is), with sentinels around seq and the result."""
    h = _lib.lib()
    R = len(head)
    sb = torch.tensor([-7] * 8 + list(seq) + [-7] * 8, dtype=torch.int64).cuda()
    hb = torch.full((R * hs + 1,), -5, dtype=torch.int64)
    hb[:R * hs:hs] = torch.tensor(head, dtype=torch.int64)
    hb = hb.cuda()
    rb = torch.full((4 + 2 + R + 4,), -9, dtype=torch.int64).cuda()
    gb = torch.tensor(list(guess), dtype=torch.int64).cuda() if guess is not None else None
    _lib.check(h.rgn_lm_lookup_step(sb.data_ptr() + 64, n, R, hb.data_ptr(), hs, limit, K, ngram, None if gb is None else gb.data_ptr(),
                                    0 if gb is None else gb.numel(), L, rb.data_ptr() + 32, _st()), "rgn_lm_lookup_step")
    sb, rb = sb.cpu().tolist(), rb.cpu().tolist()
    assert sb[:8] == [-7] * 8 and sb[-8:] == [-7] * 8 and rb[:4] == [-9] * 4 and rb[-4:] == [-9] * 4, "a sentinel was overwritten"
    return sb[8:-8], rb[4:-4]


def _check_step(seq, n, head, limit, K, ngram, guess=None, L=0, hs=1, tag=None):
    a, drafts, toks, after = LM.step(seq, n, head, limit, K, ngram, guess, L)
    got_seq, got_res = _run_step(seq, n, head, limit, K, ngram, guess, L, hs)
    R = len(head)
    assert got_res == [a, len(drafts)] + toks + [-9] * (R - a - 1), (tag, got_res, a, drafts, toks)
    assert got_seq == [int(v) for v in after], (tag, "seq")
    assert got_seq[limit:] == list(seq[limit:]), (tag, "written past the run")
    return a, drafts


def test_the_step_kernel_gives_the_hand_computed_cases():
    for c in LM.CASES:
        a, drafts = _check_step(c["seq"], c["n"], c["head"], c["limit"], c["K"], c["max_ngram"], c["guess"], c["L"], tag=c["name"])
        assert a == c["want_a"] and drafts == c["want_drafts"], c["name"]


BIG = [152063, 7, 151000, 152062, 0]                                             # the ids of a 5-word vocabulary: up to V - 1 of Qwen2.5-VL


def _random_run(rng, n, vocab):
    return [BIG[i] for i in rng.integers(0, vocab, n)]


def test_every_accept_pattern_up_to_8_rows_in_both_modes():
    rng = np.random.default_rng(8)
    for R in range(1, 9):
        for mask in itertools.product((0, 1), repeat=R - 1):                     # which drafts coincide with the argmax before them
            n = int(rng.integers(3, 70))
            settled = _random_run(rng, n, 4)
            head = _random_run(rng, R, 4)
            drafts = [head[i] if m else head[i] ^ 1 for i, m in enumerate(mask)]
            limit = n + R + int(rng.integers(0, 12))
            seq = settled + drafts + [777] * (limit - n - (R - 1))
            want_a = mask.index(0) if 0 in mask else R - 1
            a, _ = _check_step(seq, n, head, limit, 7, int(rng.integers(1, 9)), tag=(R, mask))
            assert a == want_a, (R, mask)
            L = int(rng.integers(0, n + 1))
            guess = _random_run(rng, int(rng.integers(1, 30)), 5)
            a, _ = _check_step(seq, n, head, limit, int(rng.integers(0, 8)), 2, guess, L, hs=3, tag=(R, mask, "guess"))
            assert a == want_a, (R, mask, "guess")


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 4095])
def test_the_proposals_at_every_length_equal_the_model(n):
    rng = np.random.default_rng(n)
    found = 0
    for trial in range(10 if n < 1000 else 4):
        vocab = 2 + trial % 4
        R = 1 if n == 4095 or trial % 2 == 0 else int(rng.integers(2, 9))
        settled = _random_run(rng, n, vocab)
        head = _random_run(rng, R, vocab)
        drafts = [h if rng.random() < 0.7 else h ^ 1 for h in head[:-1]]
        K, ngram = int(rng.integers(1, 32)), int(rng.integers(1, 9))
        for room in (0, 1, 2, 40):                                               # limit - n' for the pattern where every draft is accepted
            limit = n + R + room
            seq = settled + drafts + [777] * (limit - n - (R - 1)) + [555] * 4
            _, d = _check_step(seq, n, head, limit, K, ngram, tag=(n, trial, room))
            found += bool(d)
            guess = _random_run(rng, int(rng.integers(1, 60)), 5)
            _check_step(seq, n, head, limit, K, ngram, guess, int(rng.integers(0, n + 1)), tag=(n, trial, room, "guess"))
    assert found or n < 3                                                        # the lookup did find continuations


def test_the_clamp_leaves_room_for_the_steps_own_token():
    """limit - n' in {0, 1, 2} with a run full of matches: 0, 0 and 1 drafts, in both modes."""
    for R in (1, 4):
        n = 20
        settled, head = [BIG[0]] * n, [BIG[0]] * R
        for room, want in ((0, 0), (1, 0), (2, 1), (3, 2)):
            limit = n + R + room
            seq = settled + head[:-1] + [777] * (limit - n - (R - 1)) + [555] * 3
            a, d = _check_step(seq, n, head, limit, 5, 2, tag=("clamp", R, room))
            assert a == R - 1 and len(d) == want
            a, d = _check_step(seq, n, head, limit, 5, 2, [9] * 64, 3, tag=("clamp", R, room, "guess"))
            assert a == R - 1 and d == [9] * want


# ---- generate ---------------------------------------------------------------------------------------------------------------------------
NEW = 12
KS = {"fma": (1, 3, 7), "mfma": (1, 3, 7, 15, 31)}
_module, _prompts, _corrupt = QB.module, QB.prompts, QB.corrupt


def _full(T, **kw):
    return dict(max_new_tokens=T, return_dict_in_generate=True, output_logits=True, eos_token_id=[], **kw)


def _same(got, want, what):
    assert torch.equal(got.sequences, want.sequences), (what, "sequences")
    assert len(got.logits) == len(want.logits), (what, "n_new")
    assert torch.equal(torch.cat(got.logits), torch.cat(want.logits)), (what, "logits")


@functools.lru_cache(maxsize=None)
def _adoption(weights, kernels):
    return QT.HipQwen25VLTextEncoder(_module(), weights=weights, batch_kernels=kernels, lookup=True)


@pytest.mark.parametrize("pi", [0, 1], ids=["image", "text"])
@pytest.mark.parametrize("kernels", ["fma", "mfma"])
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_drafted_generates_equal_the_plain_greedy_generate_bit_for_bit(weights, kernels, pi):
    hip = _adoption(weights, kernels)
    drafted = 0
    for kw in _prompts()[pi:pi + 1]:
        L = kw["input_ids"].shape[1]
        plain = hip.generate(**kw, **_full(NEW))
        assert hip.last_lookup_stats is None and plain.sequences.shape[1] == L + NEW
        G = plain.sequences[0, L:].cpu()
        for K in KS[kernels]:
            got = hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K))
            _same(got, plain, (pi, K, "lookup"))
            st = hip.last_lookup_stats
            assert st["tokens"] == NEW == 1 + st["steps"] + st["accepted"] and st["accepted"] <= st["drafted"], st
            drafted += st["drafted"]
            _same(hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, max_matching_ngram_size=4)), plain, (pi, K, "4-grams"))
            for name, guess in (("all accepted", G), ("every 3rd wrong", _corrupt(G, 3)), ("all wrong", _corrupt(G, 1))):
                got = hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=K, draft_tokens=guess.cuda() if K % 2 else guess))
                _same(got, plain, (pi, K, name))
                assert hip.last_lookup_stats == LM.simulate_guess(G, guess, K, NEW), (pi, K, name, hip.last_lookup_stats)
            if K >= 7:
                assert hip.last_lookup_stats["accepted"] == 0 and hip.last_lookup_stats["steps"] == NEW - 1      # the "all wrong" run
        top = KS[kernels][-1]
        again = hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=top))
        _same(again, hip.generate(**kw, **_full(NEW, prompt_lookup_num_tokens=top)), (pi, "two identical calls"))
        got = hip.generate(**kw, **_full(NEW, draft_tokens=G))                   # a guess alone: the family's largest K
        _same(got, plain, (pi, "guess alone"))
        assert hip.last_lookup_stats == LM.simulate_guess(G, G, top, NEW)
        seq = hip.generate(**kw, max_new_tokens=NEW, eos_token_id=[], prompt_lookup_num_tokens=3)
        assert torch.equal(seq, plain.sequences)                                 # without return_dict_in_generate: the tensor
    assert drafted > 0 or pi == 0                                                # in the repetitive prompt the n-gram lookup does find drafts


@pytest.mark.parametrize("kernels", ["fma", "mfma"])
def test_the_last_token_lands_on_max_length_exactly(kernels):
    """max_new_tokens in {1, 2, K, K + 1} under an adoption whose max_length is L + max_new_tokens: no cache row, logits row or id past
    the end, with every draft right (the longest steps) and with the lookup's own drafts."""
    kw = _prompts()[1]
    L = kw["input_ids"].shape[1]
    plain = QT.HipQwen25VLTextEncoder(_module(), batch_kernels=kernels, lookup=True).generate(**kw, **_full(33))
    G = plain.sequences[0, L:].cpu()
    for K in KS[kernels]:
        for T in sorted({1, 2, K, K + 1}):
            hip = QT.HipQwen25VLTextEncoder(_module(), batch_kernels=kernels, lookup=True, max_length=L + T)
            want = hip.generate(**kw, **_full(T))
            assert torch.equal(want.sequences, plain.sequences[:, :L + T])
            _same(hip.generate(**kw, **_full(T, prompt_lookup_num_tokens=K, draft_tokens=G)), want, (K, T, "guess"))
            assert hip.last_lookup_stats == LM.simulate_guess(G[:T], G, K, T), (K, T)
            _same(hip.generate(**kw, **_full(T, prompt_lookup_num_tokens=K)), want, (K, T, "lookup"))
            with pytest.raises(_lib.RegionEHipError, match="exceeds max_length"):
                hip.generate(**kw, **_full(T + 1, prompt_lookup_num_tokens=K))


@pytest.mark.parametrize("kernels", ["fma", "mfma"])
def test_an_eos_inside_an_accepted_run_cuts_the_sequence_as_greedy_does(kernels):
    hip = QT.HipQwen25VLTextEncoder(_module(), batch_kernels=kernels, lookup=True)
    for kw in _prompts():
        L = kw["input_ids"].shape[1]
        G = hip.generate(**kw, max_new_tokens=NEW, eos_token_id=[])[0, L:].cpu()
        eos = int(G[4])                                                          # new token 4 (or an earlier equal one): inside the first run of 7
        cut = G.tolist().index(eos) + 1
        args = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True, eos_token_id=[eos])
        want = hip.generate(**kw, **args)
        assert want.sequences.shape[1] == L + cut and len(want.logits) == cut
        got = hip.generate(**kw, **args, prompt_lookup_num_tokens=7, draft_tokens=G)
        _same(got, want, "eos in a forced run")
        st = hip.last_lookup_stats                                               # the whole run of 1 + 7 was decoded, then cut
        assert (st["steps"], st["tokens"]) == ((1, 8) if cut > 1 else (0, 1)), st
        _same(hip.generate(**kw, **args, prompt_lookup_num_tokens=7), want, "eos with lookup drafts")
        _same(hip.generate(**kw, **args, prompt_lookup_num_tokens=7, draft_tokens=_corrupt(G, 1)), want, "eos with wrong drafts")


def test_a_default_adoption_still_refuses_the_argument():
    hip = QT.HipQwen25VLTextEncoder(_module())
    with pytest.raises(_lib.RegionEHipError, match="arguments \\['prompt_lookup_num_tokens'\\] are not implemented"):
        hip.generate(**_prompts()[1], max_new_tokens=4, prompt_lookup_num_tokens=3)
