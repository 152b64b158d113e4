"""`HipQwen25VLTextEncoder(batch_kernels="mfma")` on the GPU: generate over up to 32 left-padded rows on the MFMA row GEMM of
csrc/decode.hip.  The oracle of every row is the B = 1 generate of the SAME adoption on that row's unpadded prompt, and every such
comparison is torch.equal (tokens, fp32 logits, scores, n_new).  Against the default ("fma") adoption the sums differ in their last bits,
so that comparison is a bound on the step-0 logits and token agreement wherever the top-2 gap is well above the bound.  The tiny seeded
module and the left-padding helpers are those of the batched tests (host_qwen_text_pipeline, qwen_batch_model)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_qwen_text_pipeline as HQ  # noqa: E402
import qwen_batch_model as QB  # noqa: E402
from regione_amd import _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu

NEW = 8
WORDS = QB.ONE.split()
# 32 prompts of 32 different shapes: row 0 carries an image, lengths run from 1 to 62 words (the longest cache crosses 64 rows)
PROMPTS = ("<image> make the square red and keep the rest",) + tuple(
    " ".join(WORDS[(i * 5 + j * (i % 3 + 1)) % len(WORDS)] for j in range(1 + (i * 7) % 31 + (31 if i % 5 == 0 else 0))) for i in range(1, 32))
FULL = dict(max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.1)


_gen, _cuda, _module, _kernel_names = QB.gen, QB.cuda, QB.module, QB.kernel_names


@functools.lru_cache(maxsize=None)
def _singles():
    return QB.rows(PROMPTS)


def _emb():
    return torch.randn(4, 256, device="cuda", generator=_gen(11)).bfloat16()     # the image embeddings of prompt 0


def _batch(order):
    """The left-padded batch of the prompts `order` (indices into PROMPTS); the image row's embeddings travel with it."""
    singles = [_singles()[i] for i in order]
    ids, mask, grids, _ = QB.left_padded(singles)
    kw = dict(input_ids=ids.cuda(), attention_mask=mask.cuda())
    if 0 in order:
        kw.update(image_grid_thw=grids.cuda(), mm_token_type_ids=(ids == HQ.IMAGE).int().cuda(), image_embeds=_emb())
    return kw, ids.shape[1]


def _alone_kw(i):
    return dict(_cuda(_singles()[i]), **({"image_embeds": _emb()} if i == 0 else {}))


@functools.lru_cache(maxsize=None)
def _run(weights):
    """Per weight format, once: the "mfma" adoption, the B = 1 generate of each of the 32 prompts under it, and the batches of 12 and 32."""
    hip = QT.HipQwen25VLTextEncoder(_module(), weights=weights, max_batch=32, batch_kernels="mfma")
    alone = [hip.generate(**_alone_kw(i), **FULL) for i in range(32)]
    out = {}
    for B in (12, 32):
        kw, L = _batch(tuple(range(B)))
        out[B] = (hip.generate(**kw, **FULL), kw, L)
    lens = [s.input_ids.shape[1] for s in _singles()]
    assert len(set(lens)) >= 20 and max(lens) + NEW > 64 > min(lens)
    return dict(hip=hip, alone=alone, out=out, lens=lens)


def _rows_equal(res, L, order, alone, lens, what):
    seq = res.sequences
    z = torch.stack(res.logits)                                                  # [n_new, B, V]
    assert seq.dtype == torch.int64 and tuple(seq.shape) == (len(order), L + NEW) and len(res.logits) == NEW
    for b, i in enumerate(order):
        a = alone[i]
        assert a.sequences.shape[1] == lens[i] + NEW                             # n_new
        assert torch.equal(seq[b, L:], a.sequences[0, lens[i]:]), (what, b, i, "tokens")
        assert torch.equal(z[:, b], torch.cat(a.logits)), (what, b, i, "logits")


# ---- validation -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_the_default_adoption_keeps_its_text():
    m = _module()
    with pytest.raises(_lib.RegionEHipError, match=r"batch_kernels='mma' \(one of \('fma', 'mfma'\)"):
        QT.HipQwen25VLTextEncoder(m, batch_kernels="mma")
    with pytest.raises(_lib.RegionEHipError, match=r"max_batch=33 under batch_kernels=\"mfma\" \(an int in \[1, 32\]"):
        QT.HipQwen25VLTextEncoder(m, max_batch=33, batch_kernels="mfma")
    with pytest.raises(_lib.RegionEHipError, match=r"max_batch=0 under batch_kernels=\"mfma\" \(an int in \[1, 32\]"):
        QT.HipQwen25VLTextEncoder(m, max_batch=0, batch_kernels="mfma")
    with pytest.raises(_lib.RegionEHipError, match=r"max_batch=9 \(an int in \[1, 8\]: the rows one generate decodes from one weight stream\)"):
        QT.HipQwen25VLTextEncoder(m, max_batch=9)
    with pytest.raises(_lib.RegionEHipError, match=r"max_batch=9 \(an int in \[1, 8\]"):
        QT.HipQwen25VLTextEncoder(m, max_batch=9, batch_kernels="fma")
    hip = _run("bf16")["hip"]
    wide13 = QT.HipQwen25VLTextEncoder(m, max_batch=12, batch_kernels="mfma")
    kw13, _ = _batch(tuple(range(13)))
    with pytest.raises(_lib.RegionEHipError, match="B = 13: this adoption takes 1 <= B <= max_batch = 12"):
        wide13.generate(**kw13, max_new_tokens=2)
    assert hip.batch_kernels == "mfma" and hip.max_batch == 32


# ---- the batch is invariant ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
@pytest.mark.parametrize("B", [12, 32])
def test_every_row_of_a_wide_batch_equals_its_own_generate_bit_for_bit(B, weights):
    s = _run(weights)
    res, kw, L = s["out"][B]
    assert torch.equal(res.sequences[:, :L], kw["input_ids"])
    _rows_equal(res, L, tuple(range(B)), s["alone"], s["lens"], (weights, B))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_the_same_12_prompts_inside_a_shuffled_batch_of_32_give_the_same_rows(weights):
    s = _run(weights)
    order = tuple(torch.randperm(32, generator=torch.Generator().manual_seed(5)).tolist())
    assert order[:12] != tuple(range(12))
    kw, L = _batch(order)
    res = s["hip"].generate(**kw, **FULL)
    _rows_equal(res, L, order, s["alone"], s["lens"], (weights, "shuffled"))
    twelve, _, L12 = s["out"][12]
    for i in range(12):                                                          # and row i of the batch of 12 is that row of the batch of 32
        b = order.index(i)
        assert torch.equal(res.sequences[b, L:], twelve.sequences[i, L12:])
        assert all(torch.equal(x[b], y[i]) for x, y in zip(res.logits, twelve.logits))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_every_row_of_a_sampled_batch_of_20_equals_its_own_sampled_generate(weights):
    m = _module()
    hip = QT.HipQwen25VLTextEncoder(m, weights=weights, sampling=True, max_batch=32, batch_sampling=True, batch_kernels="mfma")
    order = tuple(range(20))
    kw, L = _batch(order)
    uni = torch.rand(NEW, 20, generator=torch.Generator().manual_seed(11)).cuda()
    res = hip.generate(**kw, **FULL, **SAMPLED, uniforms=uni, output_scores=True)
    z, sc = torch.stack(res.logits), torch.stack(res.scores)
    lens = [s.input_ids.shape[1] for s in _singles()]
    greedy = _run(weights)["out"][32][0].sequences[:20]
    assert not torch.equal(res.sequences[:, L:], greedy[:, -NEW:])
    for b in order:
        a = hip.generate(**_alone_kw(b), **FULL, **SAMPLED, uniforms=uni[:, b].contiguous(), output_scores=True)
        assert torch.equal(res.sequences[b, L:], a.sequences[0, lens[b]:]), (weights, b, "tokens")
        assert torch.equal(z[:, b], torch.cat(a.logits)), (weights, b, "logits")
        assert torch.equal(sc[:, b], torch.cat(a.scores)), (weights, b, "scores")


def test_eos_cut_pad_fill_and_n_new_do_not_depend_on_sync_every_at_20_rows():
    s = _run("bf16")
    kw, L = _batch(tuple(range(20)))
    new = s["out"][32][0].sequences[:20, -NEW:].cpu()
    counts = torch.bincount(new[:, 1:].flatten(), minlength=HQ.VOCAB)
    eos = [int(counts.argmax())]                                                 # the most frequent token after step 0: rows meet it at different steps
    pad = next(t for t in range(HQ.VOCAB) if t not in new)
    want = QB.greedy_search_rule(kw["input_ids"].cpu(), new.t(), eos, pad)
    cuts = QT.eos_cuts(new.t().contiguous(), eos)
    assert len({c for c in cuts}) >= 2
    for every in (1, 3, 64):
        got = s["hip"].generate(**kw, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad, sync_every=every)
        assert torch.equal(got.cpu(), want), every
    eos_all = sorted({int(new[b, 1 + b % 3]) for b in range(20)})                # every row finishes
    want = QB.greedy_search_rule(kw["input_ids"].cpu(), new.t(), eos_all, pad)
    assert want.shape[1] < L + NEW
    for every in (1, 3, 64):
        res = s["hip"].generate(**kw, max_new_tokens=NEW, eos_token_id=eos_all, pad_token_id=pad, sync_every=every, return_dict_in_generate=True,
                                output_logits=True)
        assert torch.equal(res.sequences.cpu(), want) and len(res.logits) == want.shape[1] - L, every


def test_one_pick_launch_over_32_rows_gives_every_row_the_bits_of_the_grouped_launches():
    """rgn_lm_pick_wide is the kernel of rgn_lm_pick_rows with up to 32 blocks: tokens, scores and seen bytes equal those of four
    rgn_lm_pick_rows calls over 8 rows each (which the batched-sampling tests pin to rgn_lm_pick row by row)."""
    from regione_amd import ops
    lib, V, B = _lib.lib(), 4097, 32
    z = torch.randn(B, V, device="cuda", generator=_gen(3)) * 3
    uni = torch.rand(B, device="cuda", generator=_gen(4))
    seen0 = (torch.rand(B, V, device="cuda", generator=_gen(5)) < 0.05).to(torch.uint8)
    ws1 = lib.rgn_lm_pick_workspace_bytes(V)

    def run(entry, groups):
        seen, tok = seen0.clone(), torch.full((B,), -1, dtype=torch.int64, device="cuda")
        sc = torch.full((B, V), -7.0, device="cuda")
        ws = torch.empty(B * ws1 // 4, dtype=torch.float32, device="cuda")
        for g0, Bg in groups:
            rc = entry(z[g0].data_ptr(), V, Bg, V, seen[g0].data_ptr(), V, 1.1, 1, 0.7, 20, 0.8, uni[g0:].data_ptr(), tok[g0:].data_ptr(), 1,
                       sc[g0].data_ptr(), V, ws.data_ptr() + ws1 * g0, Bg * ws1, ops._stream())
            _lib.check(rc, "pick")
        torch.cuda.synchronize()
        return tok, sc, seen
    a = run(lib.rgn_lm_pick_wide, [(0, 32)])
    b = run(lib.rgn_lm_pick_rows, [(g0, 8) for g0 in range(0, 32, 8)])
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[0].min()) >= 0 and len(set(a[0].tolist())) > 8
    tok = torch.zeros(40, dtype=torch.int64, device="cuda")
    ws = torch.empty(33 * ws1 // 4, dtype=torch.float32, device="cuda")
    for bad in (0, 33):
        assert lib.rgn_lm_pick_wide(z.data_ptr(), V, bad, V, seen0.data_ptr(), V, 1.1, 1, 0.7, 20, 0.8, uni.data_ptr(), tok.data_ptr(), 1, None, 0,
                                    ws.data_ptr(), 33 * ws1, ops._stream()) != 0 and b"B outside [1, 32]" in lib.rgn_last_error()
    assert lib.rgn_lm_pick_rows(z.data_ptr(), V, 9, V, seen0.data_ptr(), V, 1.1, 1, 0.7, 20, 0.8, uni.data_ptr(), tok.data_ptr(), 1, None, 0,
                                ws.data_ptr(), 33 * ws1, ops._stream()) != 0 and b"B outside [1, 8]" in lib.rgn_last_error()


# ---- against the "fma" adoption ---------------------------------------------------------------------------------------------------------------
def _head_bound(one, seqs, lens, head):
    """G [12, NEW]: max over the vocabulary of K 2^-23 sum |w x| + 2^-24 |ref64| for the lm_head product of each step, on the "fma" path's
    operands: x = the final-norm hidden state at the position that predicts token k, from one forward over the row's prompt + new tokens."""
    G = torch.zeros(12, NEW, dtype=torch.float64)
    W = head.double()
    for i in range(12):
        hs = one(input_ids=seqs[i][None, :-1].cuda()).last_hidden_state[0, lens[i] - 1:].double()     # [NEW, d]
        ref, S = hs @ W.t(), hs.abs() @ W.abs().t()
        G[i] = (W.shape[1] * 2.0 ** -23 * S + 2.0 ** -24 * ref.abs()).amax(dim=1).cpu()
    return G


def test_against_the_fma_adoption_step_0_logits_are_within_twice_the_bound_and_clear_rows_keep_their_tokens():
    s = _run("bf16")
    one = QT.HipQwen25VLTextEncoder(_module(), max_batch=8)                      # "fma": the default kernels
    fma = []
    for g0 in (0, 8):                                                            # the same 12 prompts, 8 + 4 rows
        order = tuple(range(g0, min(g0 + 8, 12)))
        kw, L = _batch(order)
        r = one.generate(**kw, **FULL)
        fma += [(r.sequences[b, L - s["lens"][i]:], torch.stack(r.logits)[:, b]) for b, i in enumerate(order)]
    G = _head_bound(one, [t for t, _ in fma], s["lens"], one.lm_head)
    excused = []
    for i in range(12):
        seq_f, z_f = fma[i]
        a = s["alone"][i]
        z_m = torch.cat(a.logits)
        d0 = float((z_m[0].double() - z_f[0].double()).abs().max())
        top = torch.topk(z_f, 2, dim=1).values.double().cpu()
        gap = (top[:, 0] - top[:, 1])
        clear = bool((gap > 4 * G[i]).all())
        print(f"row {i}: step-0 |dz| {d0:.3e} (2 G = {2 * float(G[i, 0]):.3e}); smallest gap / G = {float((gap / G[i]).min()):.1f}; "
              f"same tokens: {torch.equal(seq_f, a.sequences[0])}")
        assert d0 <= 2 * float(G[i, 0]), (i, d0, float(G[i, 0]))
        if clear:
            assert torch.equal(seq_f, a.sequences[0]), (i, "a row with every top-2 gap above 4 G changed a token")
        else:
            excused.append(i)
    assert len(excused) <= 1, excused


# ---- what runs ----------------------------------------------------------------------------------------------------------------------------
def test_a_sampled_wide_step_is_one_pick_launch():
    hip = QT.HipQwen25VLTextEncoder(_module(), sampling=True, max_batch=32, batch_sampling=True, batch_kernels="mfma")
    kw, _ = _batch(tuple(range(20)))
    uni = torch.rand(3, 20, generator=torch.Generator().manual_seed(2)).cuda()
    names = _kernel_names(lambda: hip.generate(**kw, max_new_tokens=3, eos_token_id=[], uniforms=uni, **SAMPLED))
    assert sum("lm_pick_rows_kernel" in n for n in names) == 3 and not any("lm_pick_kernel" in n for n in names)


def test_a_warm_wide_generate_dispatches_only_libregione_hip_kernels_and_one_row_runs_the_new_kernels():
    s = _run("bf16")
    _, kw, L = s["out"][32]
    names = _kernel_names(lambda: s["hip"].generate(**kw, max_new_tokens=3))
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    for k in ("lm_gemm_rows_kernel", "lm_kv_append_rows_kernel", "lm_decode_attention_rows_kernel", "lm_decode_merge_rows_kernel",
              "lm_head_finalize_rows_kernel"):
        assert any(k in n for n in names), k
    assert not any("lm_gemv" in n for n in names)
    names = _kernel_names(lambda: s["hip"].generate(**_alone_kw(3), max_new_tokens=3))
    assert sum("lm_gemm_rows_kernel" in n for n in names) == 2 * (4 * 2) + 3 and not any("lm_gemv" in n for n in names)
    fp8 = _run("fp8")["hip"]
    names = _kernel_names(lambda: fp8.generate(**_alone_kw(3), max_new_tokens=3))
    assert sum("lm_gemm_rows_kernel" in n for n in names) == 2 * (4 * 2) + 3 and not any("lm_gemv" in n for n in names)


def test_the_hosted_switch_binds_batch_kernels():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_batch_kernels = "mma"
    with pytest.raises(ValueError, match='"fma" and "mfma" are accepted'):
        with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
            pass
    assert "_regione_hip_qwen_text" not in pipe.__dict__
    pipe._regione_hip_text_batch_kernels = "mfma"
    pipe._regione_hip_text_batch = 33
    with pytest.raises(ValueError, match="1..32"):
        with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
            pass
    del pipe._regione_hip_text_batch_kernels
    pipe._regione_hip_text_batch = 12
    with pytest.raises(ValueError, match="1..8"):
        with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
            pass
    pipe._regione_hip_text_batch_kernels = "mfma"
    ids, mask, _, _ = QB.left_padded(QB.rows(PROMPTS[1:13]))
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        enc = pipe.text_encoder
        assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.max_batch == 12 and enc.batch_kernels == "mfma"
        got = enc.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), max_new_tokens=4, do_sample=False)
    assert pipe.text_encoder is m
    assert tuple(got.shape) == (12, ids.shape[1] + 4) and torch.equal(got[:, :ids.shape[1]].cpu(), ids) and int(got.max()) < HQ.VOCAB
