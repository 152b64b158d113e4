"""-m gpu: repetition penalty and sampling for generate() of the Qwen2.5-VL prompt encoder over a batch (csrc/decode.hip: rgn_lm_pick_rows;
regione_amd/qwen_text_encoder.py: HipQwen25VLTextEncoder(sampling=True, max_batch=N, batch_sampling=True)).

Nothing here has a tolerance.  The one-sequence entry rgn_lm_pick and the B = 1 sampled `generate` are pinned to the transformers
processors and to the fp64 model by test_gpu_qwen_sampling.py; the batch is invariant, so every comparison below is torch.equal with them.

Kernel level: V in {1, 1000, 1024, 1025, 16385, 152064} (a lone token, less than one 1024-thread round, exactly one, one element alone in
the second round, one element past a batch of 16 loads, the real vocabulary), B in (1, 2, 3, 5, 8), the six sampled configurations of
test_gpu_qwen_sampling.py and penalised greedy.  Every row has its own seeded z = 4 randn, 40 seen ids and uniform; row 0's maximum is
planted at index 0 and the last row's at V - 1 (B = 1: the one row is the last row), so a block that read another row or stopped short
of the tail would pick another token.  ldl, lds, seen_stride > V, token_stride = 3; NaN logits in the padding columns and in rows >= B;
sentinels in the padding columns, in rows >= B and around every buffer written.
Model level, the tiny seeded module, bf16 and fp8, 12 new tokens: a left-padded batch of three prompts (one with image placeholders)
against the B = 1 sampled generate of a plain `sampling=True` adoption on each unpadded prompt."""
import functools

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream

VS = [1, 1000, 1024, 1025, 16385, 152064]
BATCHES = (1, 2, 3, 5, 8)
# (penalty, temperature, top_k, top_p, sample): the configurations of test_gpu_qwen_sampling.py, then penalised greedy
CONFIGS = [(1.05, 1e-6, 0, 1.0, 1), (1.05, 0.1, 1, 0.001, 1), (1.0, 0.7, 20, 0.8, 1), (1.1, 1.0, 0, 0.9, 1), (1.0, 1.3, 50, 1.0, 1),
           (1.2, 0.7, 0, 0.95, 1), (1.3, 1.0, 0, 1.0, 0)]
ROWS, GUARD, TSTRIDE = 8, 64, 3
SCORE_SENT, BYTE_SENT, TOK_SENT = -7.0, 7, -5


@functools.lru_cache(maxsize=None)
def _inputs(V):
    """8 rows of seeded logits, 40 seen ids and one uniform per row (CPU), every row different."""
    g = torch.Generator().manual_seed(1000 + V)
    z = (4 * torch.randn(ROWS, V, generator=g)).float()
    ids = torch.randint(0, V, (ROWS, 40), generator=g)
    us = torch.rand(ROWS, generator=g)
    assert all(not torch.equal(z[0], z[b]) for b in range(1, ROWS)) or V == 1
    return z, ids, us


def _planted(V, B):
    """The logits of a launch over B rows: row 0's maximum at index 0, the last row's at V - 1, each above whatever a penalty leaves."""
    z = _inputs(V)[0][:B].clone()
    top = 2.0 * float(z.abs().max()) + 1.0                                        # the largest still after a division by 1.3
    if B > 1:                                                                     # B = 1: the one row is the last row
        z[0, 0] = top
    z[B - 1, V - 1] = top
    return z


class Rows:
    """The strided device buffers of rgn_lm_pick_rows at one vocabulary, with sentinels, and the one-row entry's buffers beside them."""

    def __init__(self, V):
        self.V, self.lib = V, _lib.lib()
        self.ldl, self.lds, self.ss = V + 5, V + 3, V + 7
        self.nb1 = self.lib.rgn_lm_pick_workspace_bytes(V)
        assert self.nb1 == 4 * V
        self.z = torch.full((ROWS, self.ldl), float("nan"), dtype=torch.float32, device="cuda")
        self.scores_buf = torch.empty(2 * GUARD + ROWS * self.lds, dtype=torch.float32, device="cuda")
        self.scores = self.scores_buf[GUARD:GUARD + ROWS * self.lds].view(ROWS, self.lds)
        self.seen_buf = torch.empty(2 * GUARD + ROWS * self.ss, dtype=torch.uint8, device="cuda")
        self.seen = self.seen_buf[GUARD:GUARD + ROWS * self.ss].view(ROWS, self.ss)
        self.tok_buf = torch.empty(2 * GUARD + ROWS * TSTRIDE, dtype=torch.int64, device="cuda")
        self.tok = self.tok_buf[GUARD:GUARD + ROWS * TSTRIDE].view(ROWS, TSTRIDE)
        self.ws = torch.empty(ROWS * V + GUARD, dtype=torch.float32, device="cuda")
        # the one-row entry's
        self.z1 = torch.empty(V, dtype=torch.float32, device="cuda")
        self.seen1 = torch.empty(V, dtype=torch.uint8, device="cuda")
        self.tok1 = torch.empty(1, dtype=torch.int64, device="cuda")
        self.scores1 = torch.empty(V, dtype=torch.float32, device="cuda")
        self.ws1 = torch.empty(V, dtype=torch.float32, device="cuda")

    def one(self, z, ids, u, cfg):
        """rgn_lm_pick on one row alone: (token, scores, seen) on the CPU."""
        pen, T, k, top_p, sample = cfg
        V, lib = self.V, self.lib
        self.z1.copy_(z)
        ids, u = ids.cuda(), u.reshape(1).float().cuda()
        self.scores1.fill_(float("nan"))
        _lib.check(lib.rgn_fill_zero(_p(self.seen1), V, _stream()), "rgn_fill_zero")
        _lib.check(lib.rgn_lm_seen_mark(_p(ids), ids.numel(), _p(self.seen1), V, _stream()), "rgn_lm_seen_mark")
        rc = lib.rgn_lm_pick(_p(self.z1), V, _p(self.seen1), pen, sample, T, k, top_p, _p(u) if sample else None, _p(self.tok1), _p(self.scores1),
                             _p(self.ws1), self.nb1, _stream())
        _lib.check(rc, "rgn_lm_pick")
        return int(self.tok1[0]), self.scores1.cpu(), self.seen1.cpu()

    def reset(self, z, ids, B):
        """Sentinels everywhere, the B rows of logits in place, `seen` rows zeroed and marked the way generate marks them."""
        V, lib = self.V, self.lib
        self.z.fill_(float("nan"))
        self.z[:B, :V] = z.cuda()
        self.scores_buf.fill_(SCORE_SENT)
        self.seen_buf.fill_(BYTE_SENT)
        self.tok_buf.fill_(TOK_SENT)
        self.ws.fill_(SCORE_SENT)
        self.seen[:B, :V] = 0
        ids = ids.cuda()
        for b in range(B):
            _lib.check(lib.rgn_lm_seen_mark(_p(ids[b]), ids.shape[1], self.seen.data_ptr() + b * self.ss, V, _stream()), "rgn_lm_seen_mark")

    def launch(self, B, us, cfg, scores=True):
        pen, T, k, top_p, sample = cfg
        rc = self.lib.rgn_lm_pick_rows(_p(self.z), self.ldl, B, self.V, _p(self.seen), self.ss, pen, sample, T, k, top_p, _p(us) if sample else None,
                                       _p(self.tok), TSTRIDE, _p(self.scores) if scores else None, self.lds, _p(self.ws), B * self.nb1, _stream())
        _lib.check(rc, "rgn_lm_pick_rows")
        return self.tok[:B, 0].cpu(), self.scores[:B, :self.V].cpu(), self.seen[:B, :self.V].cpu()

    def untouched(self, B, scores=True):
        """What the entry may never write: rows >= B, columns >= V, the guards, the logits."""
        V = self.V
        g = lambda buf, n, s: bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all())
        assert g(self.scores_buf, ROWS * self.lds, SCORE_SENT) and g(self.seen_buf, ROWS * self.ss, BYTE_SENT)
        assert g(self.tok_buf, ROWS * TSTRIDE, TOK_SENT), "the bytes around a buffer"
        assert bool((self.scores[B:] == SCORE_SENT).all()) and bool((self.scores[:, V:] == SCORE_SENT).all()), "scores: rows >= B, columns >= V"
        assert bool((self.seen[B:] == BYTE_SENT).all()) and bool((self.seen[:, V:] == BYTE_SENT).all()), "seen: rows >= B, columns >= V"
        assert bool((self.tok[B:] == TOK_SENT).all()) and bool((self.tok[:, 1:] == TOK_SENT).all()), "tokens: rows >= B, between the strides"
        assert bool((self.ws[B * V:] == SCORE_SENT).all()), "the workspace past B rows"
        if scores:
            assert bool((self.ws == SCORE_SENT).all()), "with scores_out the workspace is not needed"
        else:
            assert bool((self.scores == SCORE_SENT).all()), "scores_out = NULL writes no scores"
        assert bool(self.z[B:].isnan().all()) and bool(self.z[:, V:].isnan().all())


@pytest.mark.parametrize("V", VS)
def test_every_row_of_a_rows_pick_equals_the_one_row_entry_on_that_row_alone(V):
    bufs = Rows(V)
    _, ids, us = _inputs(V)
    us_dev = us.cuda()
    for B in BATCHES:
        z = _planted(V, B)
        for cfg in CONFIGS:
            want = [bufs.one(z[b], ids[b], us[b], cfg) for b in range(B)]
            bufs.reset(z, ids, B)
            tok, scores, seen = bufs.launch(B, us_dev, cfg)
            for b in range(B):
                assert int(tok[b]) == want[b][0], (V, B, cfg, b)
                assert torch.equal(scores[b], want[b][1]), (V, B, cfg, b, "scores, -inf positions included")
                assert torch.equal(seen[b], want[b][2]) and int(seen[b, int(tok[b])]) == 1, (V, B, cfg, b, "seen")
            bufs.untouched(B)
            assert torch.equal(bufs.z[:B, :V].cpu(), z), "the logits are read, never written"
            if not cfg[4] or cfg[1] == 1e-6 or cfg[2] == 1:                        # the pick is the maximum: the planted one
                assert int(tok[0]) == (0 if B > 1 else V - 1) and int(tok[B - 1]) == V - 1, (V, B, cfg)
            # a repeated launch, and the same tokens and seen bytes without scores_out (the scores then live in the workspace rows)
            bufs.reset(z, ids, B)
            again = bufs.launch(B, us_dev, cfg)
            assert all(torch.equal(a, b) for a, b in zip(again, (tok, scores, seen))), "a repeated launch must be bit-identical"
            bufs.reset(z, ids, B)
            tok2, _, seen2 = bufs.launch(B, us_dev, cfg, scores=False)
            assert torch.equal(tok2, tok) and torch.equal(seen2, seen)
            bufs.untouched(B, scores=False)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
NEW = 12
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.1)
PENALISED = dict(do_sample=False, repetition_penalty=1.1)
FULL = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)


_gen, _cuda, _kernels = QB.gen, QB.cuda, QB.kernels


@functools.lru_cache(maxsize=None)
def _run(weights):
    """Per weight format, once: a default adoption's greedy generate, every batched call the tests below look at, the B = 1 calls of a
    plain `sampling=True` adoption on the unpadded prompts, then the default adoption again."""
    torch.manual_seed(0)
    m = HQ.tiny_qwen25vl(layers=2).cuda()
    hip = QT.HipQwen25VLTextEncoder(m, weights=weights, sampling=True, max_batch=8, batch_sampling=True)
    one = QT.HipQwen25VLTextEncoder(m, weights=weights, sampling=True)           # the oracle: the one-sequence pick
    greedy = QT.HipQwen25VLTextEncoder(m, weights=weights, max_batch=8)
    default = QT.HipQwen25VLTextEncoder(m, weights=weights)
    singles = QB.rows()
    ids, mask, grids, _ = QB.left_padded(singles)                               # padded with HQ.PAD
    lens = [s.input_ids.shape[1] for s in singles]
    assert len(set(lens)) == 3 and int((ids[0] == HQ.IMAGE).sum()) == 4 and int((mask == 0).sum()) > 0
    assert not bool((ids[mask == 1] == HQ.PAD).any()), "the pad id occurs in a prompt: a marked padding would not show in the scores"
    emb = torch.randn(4, 256, device="cuda", generator=_gen(11)).bfloat16()      # the image embeddings of row 0
    batch = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), image_grid_thw=grids.cuda(), mm_token_type_ids=(ids == HQ.IMAGE).int().cuda(),
                 image_embeds=emb)
    alone_kw = [dict(_cuda(s), **({"image_embeds": emb} if b == 0 else {})) for b, s in enumerate(singles)]
    uni = torch.rand(NEW, 3, generator=torch.Generator().manual_seed(11)).cuda()
    s = dict(hip=hip, one=one, greedy_enc=greedy, default=default, batch=batch, alone_kw=alone_kw, lens=lens, L=ids.shape[1], uni=uni)
    s["default0"] = default.generate(**alone_kw[1], **FULL)
    s["sampled"] = hip.generate(**batch, **FULL, **SAMPLED, uniforms=uni, output_scores=True)
    s["sampled2"] = hip.generate(**batch, **FULL, **SAMPLED, uniforms=uni, output_scores=True)
    s["penalised"] = hip.generate(**batch, **FULL, **PENALISED, output_scores=True)
    s["unpenalised"] = hip.generate(**batch, **FULL, do_sample=False)
    s["greedy"] = greedy.generate(**batch, **FULL)
    s["alone_sampled"] = [one.generate(**kw, **FULL, **SAMPLED, uniforms=uni[:, b].contiguous(), output_scores=True) for b, kw in enumerate(alone_kw)]
    s["alone_penalised"] = [one.generate(**kw, **FULL, **PENALISED, output_scores=True) for kw in alone_kw]
    s["default1"] = default.generate(**alone_kw[1], **FULL)
    return s


def _rows_equal_their_own_generate(s, out, alone):
    seq, L = out.sequences, s["L"]
    assert seq.dtype == torch.int64 and tuple(seq.shape) == (3, L + NEW) and torch.equal(seq[:, :L], s["batch"]["input_ids"])
    for name in ("logits", "scores"):
        t = getattr(out, name)
        assert len(t) == NEW and all(tuple(x.shape) == (3, HQ.VOCAB) and x.dtype == torch.float32 for x in t), name
    z, sc = torch.stack(out.logits), torch.stack(out.scores)                     # [NEW, 3, V]
    for b, n in enumerate(s["lens"]):
        a = alone[b]
        assert torch.equal(seq[b, L:], a.sequences[0, n:]), (b, "tokens")
        assert torch.equal(z[:, b], torch.cat(a.logits)), (b, "logits")
        assert torch.equal(sc[:, b], torch.cat(a.scores)), (b, "scores: a marked pad id, or another row's seen bytes, would show here")


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_every_row_of_a_sampled_batch_equals_its_own_sampled_generate_bit_for_bit(weights):
    s = _run(weights)
    _rows_equal_their_own_generate(s, s["sampled"], s["alone_sampled"])
    assert not torch.equal(s["sampled"].sequences, s["greedy"].sequences)
    plain = s["hip"].generate(**s["batch"], max_new_tokens=NEW, **SAMPLED, uniforms=s["uni"])
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, s["sampled"].sequences)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_every_row_of_a_penalised_greedy_batch_equals_its_own_generate_and_differs_from_the_unpenalised_batch(weights):
    s = _run(weights)
    _rows_equal_their_own_generate(s, s["penalised"], s["alone_penalised"])
    assert not torch.equal(s["penalised"].sequences, s["unpenalised"].sequences), "the penalty changed no token"
    # the scores are the whole penalised rows (nothing is filtered), the pad id's entry included
    assert all(bool(torch.isfinite(x).all()) for x in s["penalised"].scores)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_a_sampled_batch_is_reproducible(weights):
    s = _run(weights)
    a, b = s["sampled"], s["sampled2"]
    assert torch.equal(a.sequences, b.sequences)
    assert all(torch.equal(x, y) for x, y in zip(a.logits, b.logits)) and all(torch.equal(x, y) for x, y in zip(a.scores, b.scores))
    g = [s["hip"].generate(**s["batch"], max_new_tokens=NEW, **SAMPLED, generator=_gen(5)) for _ in range(2)]
    assert torch.equal(g[0], g[1])
    cpu = [s["hip"].generate(**s["batch"], max_new_tokens=NEW, **SAMPLED, generator=torch.Generator().manual_seed(5)) for _ in range(2)]
    assert torch.equal(cpu[0], cpu[1])
    want = torch.rand(NEW, 3, generator=torch.Generator().manual_seed(5)).cuda()  # the generator fills [T, B] once, before the loop
    assert torch.equal(cpu[0], s["hip"].generate(**s["batch"], max_new_tokens=NEW, **SAMPLED, uniforms=want))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_eos_cut_pad_fill_and_n_new_of_a_sampled_batch_do_not_depend_on_sync_every(weights):
    s = _run(weights)
    L, seq = s["L"], s["sampled"].sequences
    new = seq[:, L:].cpu()
    pad = next(t for t in range(HQ.VOCAB) if t not in new)
    # an EOS id from the run's own tokens that not every row meets at step 0; then one per row, so that every row finishes
    eos = [int(new[0, 3])]
    eos_all = [int(new[0, 1]), int(new[1, 4]), int(new[2, 2])]
    for ids, fill in ((eos, pad), (eos_all, None)):
        want = QB.greedy_search_rule(s["batch"]["input_ids"].cpu(), new.t(), ids, ids[0] if fill is None else fill)
        for every in (1, 3, 64):
            res = s["hip"].generate(**s["batch"], max_new_tokens=NEW, **SAMPLED, uniforms=s["uni"], eos_token_id=ids, sync_every=every,
                                    return_dict_in_generate=True, output_scores=True, **({} if fill is None else {"pad_token_id": fill}))
            assert torch.equal(res.sequences.cpu(), want), (weights, ids, every)
            assert len(res.scores) == want.shape[1] - L and res.logits is None
            assert all(torch.equal(a, b) for a, b in zip(res.scores, s["sampled"].scores))
    assert want.shape[1] < L + NEW, "every row met an EOS: the search stops at the largest cut"


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_the_greedy_batch_and_the_default_adoption_keep_their_bits(weights):
    s = _run(weights)
    a, b = s["unpenalised"], s["greedy"]                                         # greedy as before on the batch_sampling adoption
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.logits, b.logits)) and a.scores is None
    a, b = s["default0"], s["default1"]
    assert torch.equal(a.sequences, b.sequences) and all(torch.equal(x, y) for x, y in zip(a.logits, b.logits))
    # B = 1 under the opt-in: rgn_lm_pick_rows at B = 1 is rgn_lm_pick
    got = s["hip"].generate(**s["alone_kw"][1], **FULL, **SAMPLED, uniforms=s["uni"][:, 1].contiguous(), output_scores=True)
    want = s["alone_sampled"][1]
    assert torch.equal(got.sequences, want.sequences) and all(torch.equal(x, y) for x, y in zip(got.scores, want.scores))


def test_a_warm_sampled_batch_dispatches_only_library_kernels_one_rows_pick_per_step_and_a_greedy_batch_none():
    s = _run("bf16")
    hip, batch, T = s["hip"], s["batch"], 4
    uni = s["uni"][:T].contiguous()
    seq, names = _kernels(lambda: hip.generate(**batch, max_new_tokens=T, **SAMPLED, uniforms=uni))
    ok = lambda n: ("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset"))
    foreign = sorted({n[:120] for n in names if not ok(n)})
    assert foreign == [], foreign
    assert sum("lm_pick_rows_kernel" in n for n in names) == T and sum("lm_seen_mark_kernel" in n for n in names) == 3
    assert not any("lm_pick_kernel" in n for n in names) and sum("lm_head_finalize_rows_kernel" in n for n in names) == T
    assert torch.equal(seq, s["sampled"].sequences[:, :s["L"] + T])
    _, base = _kernels(lambda: s["greedy_enc"].generate(**batch, max_new_tokens=T))
    _, same = _kernels(lambda: hip.generate(**batch, max_new_tokens=T, do_sample=False))
    rgn = lambda ns: sorted(n for n in ns if "rgn::" in n)
    assert not any("lm_pick" in n or "lm_seen_mark" in n for n in base + same)
    assert rgn(base) == rgn(same)
    assert len(rgn(names)) == len(rgn(base)) + T + 3                             # one pick per step and one mark per row, nothing else


def test_the_hosted_switch_answers_a_sampled_batched_generate_on_the_hip_path_and_its_absence_refuses_as_before():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    ids, mask, _, _ = QB.left_padded(QB.rows(QB.PROMPTS[1:]))
    kw = dict(input_ids=ids.cuda(), attention_mask=mask.cuda())
    L = ids.shape[1]
    uni = torch.rand(4, 2, generator=torch.Generator().manual_seed(2)).cuda()
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_sampling, pipe._regione_hip_text_batch, pipe._regione_hip_text_batch_sampling = True, 3, True
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        enc = pipe.text_encoder
        assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.batch_sampling is True and enc.sampling is True and enc.max_batch == 3
        got = enc.generate(**kw, max_new_tokens=4, do_sample=True, top_k=5, repetition_penalty=1.1, uniforms=uni)
    assert pipe.text_encoder is m and fired == []
    assert tuple(got.shape) == (2, L + 4) and torch.equal(got[:, :L].cpu(), ids) and int(got.max()) < HQ.VOCAB
    assert torch.equal(pipe._regione_hip_qwen_text.generate(**kw, max_new_tokens=4, do_sample=True, top_k=5, repetition_penalty=1.1, uniforms=uni), got)
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_sampling, pipe._regione_hip_text_batch = True, 3
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        assert pipe.text_encoder.batch_sampling is False
        with pytest.raises(_lib.RegionEHipError, match="rgn_lm_pick is one sequence"):
            pipe.text_encoder.generate(**kw, max_new_tokens=4, do_sample=True, top_k=5, uniforms=uni)
    assert fired == []
