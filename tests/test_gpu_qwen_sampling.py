"""-m gpu: repetition penalty and sampling for generate() of the Qwen2.5-VL prompt encoder (csrc/decode.hip: rgn_lm_seen_mark, rgn_lm_pick;
regione_amd/qwen_text_encoder.py: HipQwen25VLTextEncoder(sampling=True)).

Kernel level, V in {1, 1000, 1024, 152064}, 8 seeded cases per configuration (penalty, temperature, top_k, top_p) with z = 4 randn(V) in
fp32, 40 random seen ids and 256 uniforms per case:
  * the stages transformers computes in fp32 (penalty, temperature, top-k) are compared with the installed processors run on the CPU on
    the same values with torch.equal, the -inf positions included; `seen` changes at the picked token only, the bytes around token_out
    and around `seen` keep a sentinel;
  * the top-p kept set and every draw are compared with the fp64 model (tests/lm_pick_model.py) outside a rounding bound DELTA.

DELTA.  The kernel's mass of a token is e = expf(x) in fp32 with x = fl32(s - max) <= 0, summed in fp64.  The subtraction is one rounding,
|dx| <= 2^-24 |x|, which changes exp(x) by the relative amount 2^-24 |x|; expf is taken at the 3 ulp OpenCL allows, a relative 3 * 2^-23.
With p the exact softmax, sum_v p_v |x_v| = H(p) - ln Z <= ln V (Z = sum exp(x) >= 1, H <= ln V), so every partial sum A and the total Z
of the masses carry a relative-to-Z error of at most b = 2^-24 (ln V + 6), and a cumulative mass A / Z one of 2 b / (1 - b).  The fp64
sums add at most V 2^-52 in any order.  DELTA = 2^-23 (ln V + 6) + V 2^-50 is 2.2e-6 at V = 152064, below the 1e-5 the check allows: a
kept-set comparison may skip tokens whose model mass lies within DELTA of 1 - top_p, a draw is skipped when u lies within DELTA of a boundary
of the model's CDF.  On the CPU the model finds no token within 1e-5 of the threshold in any case below, so the kept sets are compared whole, and at most
1.6 % of the 2048 draws of a configuration (V = 152064 at (1.1, 1.0, 0, 0.9), about 1000 kept tokens) lie within 1e-5 of a boundary;
both are asserted.

Model level, the tiny seeded module in both weight formats, a text-only and a one-image prompt: penalised greedy tokens are the argmax of
the transformers processor over that step's own raw logits and differ from the unpenalised run; sampled tokens and scores equal the fp64
model's from that step's own logits; repeated calls, `generator=` and `sync_every` change nothing; only library kernels are dispatched; a
default adoption returns the same bits before and after."""
import copy
import functools
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import lm_pick_model as PM  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream
_kernels = QB.kernels

VS = [1, 1000, 1024, 152064]
CONFIGS = [(1.05, 1e-6, 0, 1.0), (1.05, 0.1, 1, 0.001), (1.0, 0.7, 20, 0.8), (1.1, 1.0, 0, 0.9), (1.0, 1.3, 50, 1.0), (1.2, 0.7, 0, 0.95)]
NCASE, NU, GUARD = 8, 256, 64


def delta(V):
    d = 2.0 ** -23 * (math.log(V) + 6) + V * 2.0 ** -50
    assert d <= 1e-5                                                             # a condition, not a measurement
    return d


@functools.lru_cache(maxsize=None)
def _inputs_of_every_case():
    """(V, ci) -> 8 x (z, seen ids, uniforms): ONE seeded CPU generator walked over V = 1000, 1024, 152064, the configurations and the
    cases in this order (the order matters: these are the inputs for which the claims of the module docstring were checked), V = 1 from a
    generator of its own."""
    out = {}
    for seed, vs in ((5, (1000, 1024, 152064)), (6, (1,))):
        g = torch.Generator().manual_seed(seed)
        for V in vs:
            for ci in range(len(CONFIGS)):
                rows = out[(V, ci)] = []
                for _ in range(NCASE):
                    z = (4 * torch.randn(V, generator=g)).float()
                    ids = torch.randint(0, V, (40,), generator=g)
                    rows.append((z, ids, torch.rand(NU, generator=g)))
    return out


@functools.lru_cache(maxsize=None)
def _cases(V, ci):
    """The seeded inputs of configuration `ci` at vocabulary V with the fp64 model's answer, computed once and left unchanged."""
    pen, T, k, top_p = CONFIGS[ci]
    return [dict(z=z, ids=ids, us=us, m=PM.pick(z, PM.seen_mask(V, ids), pen, True, T, k, top_p, us)) for z, ids, us in _inputs_of_every_case()[(V, ci)]]


def _gap(C, us):
    """Per uniform the distance to the nearest boundary of the CDF `C` (ascending fp64)."""
    u = us.double()
    j = torch.searchsorted(C, u).clamp(max=C.numel() - 1)
    return torch.minimum((C[j] - u).abs(), (u - C[(j - 1).clamp(min=0)]).abs())


class Pick:
    """One vocabulary's device buffers around rgn_lm_pick, sentinels on both sides of `seen` and of the token slot."""

    def __init__(self, V):
        self.V, self.lib = V, _lib.lib()
        self.nb = self.lib.rgn_lm_pick_workspace_bytes(V)
        self.ws = torch.empty(self.nb // 4, dtype=torch.float32, device="cuda")
        self.seen_buf = torch.full((V + 2 * GUARD,), 7, dtype=torch.uint8, device="cuda")
        self.seen = self.seen_buf[GUARD:GUARD + V]
        self.tok = torch.full((3,), -5, dtype=torch.int64, device="cuda")
        self.scores = torch.empty(V, dtype=torch.float32, device="cuda")

    def mark(self, ids):
        _lib.check(self.lib.rgn_fill_zero(_p(self.seen), self.V, _stream()), "rgn_fill_zero")
        ids = ids.cuda()
        _lib.check(self.lib.rgn_lm_seen_mark(_p(ids), ids.numel(), _p(self.seen), self.V, _stream()), "rgn_lm_seen_mark")
        return self.seen.clone()

    def __call__(self, z, seen0, pen, sample, T, k, top_p, us, scores=True):
        """tokens [len(us)] on the CPU (one launch per uniform, `seen` restored before each), the scores and `seen` of the last launch."""
        toks = torch.empty(max(len(us), 1), dtype=torch.int64, device="cuda")
        us = us.float().cuda().contiguous()
        for j in range(toks.numel()):
            self.seen.copy_(seen0)
            self.scores.fill_(float("nan"))
            rc = self.lib.rgn_lm_pick(_p(z), self.V, _p(self.seen), pen, int(sample), T, k, top_p, us.data_ptr() + 4 * j if sample else None,
                                      self.tok.data_ptr() + 8, _p(self.scores) if scores else None, _p(self.ws), self.nb, _stream())
            _lib.check(rc, "rgn_lm_pick")
            toks[j] = self.tok[1]
        assert self.tok[0] == -5 and self.tok[2] == -5, "the bytes around token_out"
        assert bool((self.seen_buf[:GUARD] == 7).all()) and bool((self.seen_buf[GUARD + self.V:] == 7).all()), "the bytes around seen"
        return toks.cpu(), self.scores.cpu(), self.seen.cpu()


@functools.lru_cache(maxsize=None)
def _picker(V):
    return Pick(V)


# ---- rgn_lm_seen_mark ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_seen_mark_sets_exactly_the_ids_bytes_and_ignores_ids_outside_the_vocabulary(V):
    pk = _picker(V)
    g = torch.Generator().manual_seed(V)
    good = torch.randint(0, V, (300,), generator=g)                              # duplicates included, more than one block
    ids = torch.cat([good, torch.tensor([-1, V, V + 5, 2 ** 40, -2 ** 40]), good[:7]])
    got = pk.mark(ids).cpu()
    assert torch.equal(got.bool(), PM.seen_mask(V, good)) and int(got.max()) == 1
    assert bool((pk.seen_buf[:GUARD] == 7).all()) and bool((pk.seen_buf[GUARD + V:] == 7).all())
    assert torch.equal(pk.mark(ids).cpu(), got)


# ---- the stages transformers computes in fp32 ------------------------------------------------------------------------------------------------
def _transformers_scores(z, ids, pen, T, k):
    from transformers.generation import logits_process as LP
    s = z[None].clone()
    if pen != 1.0:
        s = LP.RepetitionPenaltyLogitsProcessor(penalty=pen)(ids[None], s)
    if T is not None:
        s = LP.TemperatureLogitsWarper(T)(ids[None], s)
    if k:
        s = LP.TopKLogitsWarper(top_k=k, min_tokens_to_keep=1)(ids[None], s)
    return s[0]


@pytest.mark.parametrize("V", VS)
def test_penalty_temperature_and_top_k_equal_the_transformers_processors_bit_for_bit(V):
    pk = _picker(V)
    extra = [(1.3, 0.05, 7, 1.0), (0.8, 2.5, V, 1.0), (1.0, 1.0, 0, 1.0)]         # a penalty below 1, k = V, every stage off
    for ci, (pen, T, k, top_p) in enumerate(CONFIGS + extra):
        for c in _cases(V, min(ci, len(CONFIGS) - 1))[:4]:
            z, seen0 = c["z"].cuda(), pk.mark(c["ids"])
            toks, got, seen1 = pk(z, seen0, pen, True, T, k, 1.0, c["us"][:1])
            want = _transformers_scores(c["z"], c["ids"], pen, T, k)
            assert torch.equal(got, want), (V, pen, T, k, int((got != want).sum()))
            t = int(toks[0])
            assert got[t] > -math.inf
            changed = torch.nonzero(seen1 != seen0.cpu()).flatten().tolist()
            assert changed in ([], [t]) and int(seen1[t]) == 1, "seen changes at the picked token only"
            assert torch.equal(z.cpu(), c["z"]), "the logits are read, never written"
            # greedy: the penalty alone, the first maximum, and the same token without scores_out
            toks, got, _ = pk(z, seen0, pen, False, T, k, top_p, c["us"][:1])
            want = _transformers_scores(c["z"], c["ids"], pen, None, 0)
            assert torch.equal(got, want) and int(toks[0]) == int(torch.nonzero(want == want.max())[0])
            assert int(pk(z, seen0, pen, False, T, k, top_p, c["us"][:1], scores=False)[0][0]) == int(toks[0])


@pytest.mark.parametrize("V", [1000, 1024, 152064])
def test_a_planted_exact_tie_in_greedy_mode_goes_to_the_lower_index(V):
    pk = _picker(V)
    z0 = _cases(V, 0)[0]["z"]
    for a, b in [(0, 1), (63, 64), (5, V - 3), (V - 2, V - 1), (V // 2 - 7, V // 2 + 300), (17, 1024 * (V // 2048) + 17 if V > 2048 else 900)]:
        assert 0 <= a < b < V
        z = z0.clone()
        z[a] = z[b] = 2.0 * float(z0.max()) + 1.0                                # the largest still after a division by 1.3
        ids = torch.tensor([a, b, 3])                                            # both penalised alike: still a tie
        for pen in (1.0, 1.3):
            toks, s, _ = pk(z.cuda(), pk.mark(ids), pen, False, 1.0, 0, 1.0, torch.zeros(1))
            assert float(s[a]) == float(s[b]) == float(s.max()) and int(toks[0]) == a, (V, a, b, pen)


# ---- top-p and the draw against the fp64 model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("V", VS)
def test_the_kept_set_and_every_draw_equal_the_fp64_models_outside_the_rounding_bound(V, ci):
    pen, T, k, top_p = CONFIGS[ci]
    pk, d = _picker(V), delta(V)
    excluded = wrong = 0
    for c in _cases(V, ci):
        m, z, seen0 = c["m"], c["z"].cuda(), pk.mark(c["ids"])
        toks, got, _ = pk(z, seen0, pen, True, T, k, top_p, c["us"])
        # the kept set: what the model keeps, except tokens whose group mass lies within d of the threshold (asserted: there are none)
        sure = torch.ones(V, dtype=torch.bool)
        if top_p < 1.0:
            sure = (PM.group_mass(m["before_top_p"]) - (1.0 - top_p)).abs() > 1e-5
            sure |= m["before_top_p"] == m["before_top_p"].max()
            sure |= m["before_top_p"] == -math.inf
        assert bool(sure.all()), "a seeded case has a token within 1e-5 of the top-p threshold: choose another seed"
        assert torch.equal(got > -math.inf, m["keep"]) and torch.equal(got, m["scores"]), (V, ci)
        # the draws
        gap = _gap(m["C"], c["us"])
        excluded += int((gap <= 1e-5).sum())
        clear = gap > d
        wrong += int((toks[clear] != m["tokens"][clear]).sum())
        assert bool(m["keep"][toks].all()), "a filtered token was drawn"
        again, _, _ = pk(z, seen0, pen, True, T, k, top_p, c["us"][:16])
        assert torch.equal(again, toks[:16]), "a repeated call must be bit-identical"
    print(f"lm_pick V={V} {CONFIGS[ci]}: {excluded} of {NCASE * NU} draws within 1e-5 of a CDF boundary, delta {d:.2e}, wrong {wrong}")
    assert excluded <= 0.03 * NCASE * NU
    assert wrong == 0


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
@pytest.mark.parametrize("V", VS)
def test_planted_uniforms_return_the_token_whose_interval_they_lie_in(V, ci):
    pen, T, k, top_p = CONFIGS[ci]
    pk, d = _picker(V), delta(V)
    c = _cases(V, ci)[0]
    m, z, seen0 = c["m"], c["z"].cuda(), pk.mark(c["ids"])
    idx, C = m["idx"], m["C"]
    lo = torch.cat([torch.zeros(1, dtype=torch.float64), C[:-1]])
    wide = torch.nonzero(C - lo > 8 * d + 2.0 ** -22).flatten()                  # the fp32 midpoint stays d inside the interval
    wide = wide[torch.linspace(0, wide.numel() - 1, min(wide.numel(), 48)).long()]
    assert wide.numel() >= 1
    mid = ((lo[wide] + C[wide]) / 2).float()
    assert bool(((mid.double() - lo[wide]) > d).all()) and bool(((C[wide] - mid.double()) > d).all())
    toks, _, _ = pk(z, seen0, pen, True, T, k, top_p, mid)
    assert torch.equal(toks, idx[wide]), (V, ci)
    # u = 0: the lowest kept index, up to kept tokens in front of it that together hold less than d of the mass
    t0 = int(pk(z, seen0, pen, True, T, k, top_p, torch.zeros(1))[0][0])
    j0 = int(torch.nonzero(idx == t0)[0])
    assert bool(m["keep"][t0]) and float(lo[j0]) <= d
    if float(C[0]) > d:
        assert t0 == int(idx[0])
    # u just below 1: a kept token, never a filtered one
    top = torch.nextafter(torch.ones(1), torch.zeros(1))
    assert top.dtype == torch.float32 and float(top) < 1.0
    t1, s1, _ = pk(z, seen0, pen, True, T, k, top_p, top)
    assert bool(m["keep"][int(t1[0])]) and s1[int(t1[0])] > -math.inf


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
ONE = "make the square red and keep the rest of the picture as it is"
LONG = " ".join([ONE] * 3)
PROMPTS = {"text": (0, LONG, 53), "one_image": (1, ONE, 31)}
NEW = 16
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.1)


def _inputs(n_images, prompt):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    mi = HQ.ToyProcessor()(text=[("<image> " if n_images else "") + prompt], images=images or None).to("cuda")
    kw = dict(input_ids=mi.input_ids, attention_mask=mi.attention_mask)
    if n_images:
        kw.update(pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw, mm_token_type_ids=(mi.input_ids == HQ.IMAGE).int())
    return kw


@functools.lru_cache(maxsize=None)
def _run(fmt, case):
    """Per weight format and prompt, once: a default adoption's call and greedy generate, then everything a `sampling=True` adoption of
    the same module is asked below, then the default adoption again."""
    n_images, prompt, L = PROMPTS[case]
    torch.manual_seed(0)
    bf = HQ.tiny_qwen25vl(layers=2).cuda()
    plain = QT.HipQwen25VLTextEncoder(bf, weights=fmt)
    hip = QT.HipQwen25VLTextEncoder(copy.deepcopy(bf), weights=fmt, sampling=True)
    kw = _inputs(n_images, prompt)
    assert kw["input_ids"].shape == (1, L)
    full = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    call0, greedy0 = plain(**kw).last_hidden_state, plain.generate(**kw, **full)
    uni = torch.rand(NEW, generator=torch.Generator().manual_seed(11)).cuda()
    s = dict(hip=hip, plain=plain, kw=kw, L=L, uni=uni, call0=call0, greedy0=greedy0)
    s["unpenalised"] = hip.generate(**kw, **full, do_sample=False)
    s["penalised"] = hip.generate(**kw, **full, do_sample=False, repetition_penalty=1.3, output_scores=True)
    s["sampled"] = hip.generate(**kw, **full, **SAMPLED, uniforms=uni, output_scores=True)
    s["sampled2"] = hip.generate(**kw, **full, **SAMPLED, uniforms=uni, output_scores=True)
    s["call1"], s["greedy1"] = plain(**kw).last_hidden_state, plain.generate(**kw, **full)
    return s


RUNS = [(f, c) for f in ("bf16", "fp8") for c in PROMPTS]


@pytest.mark.parametrize("fmt,case", RUNS)
def test_penalised_greedy_tokens_are_the_argmax_of_the_transformers_processor_over_the_steps_own_logits(fmt, case):
    from transformers.generation import logits_process as LP
    s = _run(fmt, case)
    out, L = s["penalised"], s["L"]
    seq = out.sequences.cpu()
    assert seq.shape == (1, L + NEW) and len(out.logits) == len(out.scores) == NEW
    proc = LP.RepetitionPenaltyLogitsProcessor(penalty=1.3)
    for k in range(NEW):
        want = proc(seq[:, :L + k], out.logits[k].cpu().clone())[0]
        assert torch.equal(out.scores[k][0].cpu(), want), k
        assert int(seq[0, L + k]) == int(torch.nonzero(want == want.max())[0]), k
    assert torch.equal(s["unpenalised"].sequences, s["greedy0"].sequences)       # penalty 1, greedy: the path of a default adoption
    assert not torch.equal(seq, s["greedy0"].sequences.cpu()), "the penalty changed no token: the comparison above shows nothing"


@pytest.mark.parametrize("fmt,case", RUNS)
def test_sampled_tokens_and_scores_equal_the_fp64_models_pick_from_the_steps_own_logits(fmt, case):
    s = _run(fmt, case)
    out, L, uni = s["sampled"], s["L"], s["uni"].cpu()
    seq = out.sequences.cpu()
    assert seq.shape == (1, L + NEW) and seq.dtype == torch.int64 and torch.equal(seq[:, :L], s["kw"]["input_ids"].cpu())
    for k in range(NEW):
        m = PM.pick(out.logits[k][0].cpu(), PM.seen_mask(HQ.VOCAB, seq[0, :L + k]), SAMPLED["repetition_penalty"], True, SAMPLED["temperature"],
                    SAMPLED["top_k"], SAMPLED["top_p"], uni[k:k + 1])
        assert torch.equal(out.scores[k][0].cpu(), m["scores"]), k
        assert int(seq[0, L + k]) == int(m["tokens"][0]), k
    assert not torch.equal(seq, s["greedy0"].sequences.cpu())


@pytest.mark.parametrize("fmt,case", RUNS)
def test_a_sampled_generate_is_reproducible(fmt, case):
    s = _run(fmt, case)
    a, b = s["sampled"], s["sampled2"]
    assert torch.equal(a.sequences, b.sequences)
    assert all(torch.equal(x, y) for x, y in zip(a.logits, b.logits)) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    if case == "text":
        g = [s["hip"].generate(**s["kw"], max_new_tokens=NEW, **SAMPLED, generator=torch.Generator(device="cuda").manual_seed(5)) for _ in range(2)]
        assert torch.equal(g[0], g[1])
        cpu = [s["hip"].generate(**s["kw"], max_new_tokens=NEW, **SAMPLED, generator=torch.Generator().manual_seed(5)) for _ in range(2)]
        assert torch.equal(cpu[0], cpu[1])
        want = torch.rand(NEW, generator=torch.Generator().manual_seed(5)).cuda()
        assert torch.equal(cpu[0], s["hip"].generate(**s["kw"], max_new_tokens=NEW, **SAMPLED, uniforms=want))


@pytest.mark.parametrize("fmt,case", RUNS)
def test_the_encoder_call_and_a_default_greedy_generate_keep_their_bits_around_a_sampled_generate(fmt, case):
    s = _run(fmt, case)
    assert torch.equal(s["call0"], s["call1"])
    assert torch.equal(s["greedy0"].sequences, s["greedy1"].sequences)
    assert all(torch.equal(x, y) for x, y in zip(s["greedy0"].logits, s["greedy1"].logits))
    assert s["greedy0"].scores is None


def test_the_eos_cut_of_a_sampled_generate_does_not_depend_on_sync_every():
    tried = 0
    for fmt, case in RUNS[:2]:
        s = _run(fmt, case)
        L, seq = s["L"], s["sampled"].sequences
        new = seq[0, L:].tolist()
        js = [j for j in range(2, NEW) if new[j] not in new[:j]]
        if not js:
            continue
        j = js[len(js) // 2]
        tried += 1
        for every in (1, 4, 8):
            got = s["hip"].generate(**s["kw"], max_new_tokens=NEW, **SAMPLED, uniforms=s["uni"], eos_token_id=new[j], sync_every=every)
            assert torch.equal(got, seq[:, :L + j + 1]), (case, j, every)
        res = s["hip"].generate(**s["kw"], max_new_tokens=NEW, **SAMPLED, uniforms=s["uni"], eos_token_id=new[j], return_dict_in_generate=True,
                                output_scores=True)
        assert len(res.scores) == j + 1 and res.logits is None
        assert all(torch.equal(x, y) for x, y in zip(res.scores, s["sampled"].scores))
    assert tried >= 1, "no run produced a token that first occurs at a new index >= 2"


def test_a_warm_sampled_generate_dispatches_only_libregione_hip_kernels_and_the_default_path_launches_no_pick():
    s = _run("bf16", "text")
    hip, plain, kw, T = s["hip"], s["plain"], s["kw"], 4
    seq, names = _kernels(lambda: hip.generate(**kw, max_new_tokens=T, **SAMPLED, uniforms=s["uni"][:T].contiguous()))
    ok = lambda n: ("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset"))
    foreign = sorted({n[:120] for n in names if not ok(n)})
    assert foreign == [], foreign
    for k in ("lm_gemv_kernel", "lm_kv_append_kernel", "lm_decode_attention_kernel", "lm_decode_merge_kernel", "lm_seen_mark_kernel"):
        assert any(k in n for n in names), k
    assert sum("lm_pick_kernel" in n for n in names) == T and sum("lm_seen_mark_kernel" in n for n in names) == 1
    assert torch.equal(seq, s["sampled"].sequences[:, :s["L"] + T])
    # the default adoption, and a sampling adoption asked for plain greedy search: the kernels of the greedy path, no pick, no byte map
    _, base = _kernels(lambda: plain.generate(**kw, max_new_tokens=T))
    _, same = _kernels(lambda: hip.generate(**kw, max_new_tokens=T, do_sample=False))
    rgn = lambda ns: sorted(n for n in ns if "rgn::" in n)
    assert not any("lm_pick" in n or "lm_seen_mark" in n for n in base) and sum("lm_head_finalize_kernel" in n for n in base) == T
    assert rgn(base) == rgn(same)
    assert len(rgn(names)) == len(rgn(base)) + T + 1                             # one pick per token and one mark, nothing else


def test_the_hosted_switch_answers_a_sampled_generate_on_the_hip_path_and_its_absence_refuses_as_before():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    kw = _inputs(1, ONE)
    uni = torch.rand(4, generator=torch.Generator().manual_seed(2)).cuda()
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_sampling = True
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        assert isinstance(pipe.text_encoder, QT.HipQwen25VLTextEncoder) and pipe.text_encoder.sampling is True
        got = pipe.text_encoder.generate(**kw, max_new_tokens=4, do_sample=True, top_k=5, uniforms=uni)
    assert pipe.text_encoder is m and fired == []
    assert got.shape == (1, 31 + 4) and torch.equal(got[:, :31], kw["input_ids"]) and int(got.max()) < HQ.VOCAB
    assert torch.equal(pipe._regione_hip_qwen_text.generate(**kw, max_new_tokens=4, do_sample=True, top_k=5, uniforms=uni), got)
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        assert pipe.text_encoder.sampling is False
        with pytest.raises(_lib.RegionEHipError, match="do_sample: sampling is not implemented"):
            pipe.text_encoder.generate(**kw, max_new_tokens=4, do_sample=True, uniforms=uni)
    assert fired == []
