"""-m gpu: generate() of the Qwen2.5-VL prompt encoder over a batch (`max_batch=`; regione_amd/qwen_text_encoder.py, the `_rows` entries of
csrc/decode.hip).  The batch is invariant, so nothing here has a tolerance: the oracle is always the unchanged one-sequence entry, or the
B = 1 `generate`, and every comparison is torch.equal.  (The one-sequence entries are pinned to fp64 bounds and to the transformers module
by test_gpu_qwen_generate.py and test_gpu_qwen_fp8.py.)

Kernel level: rgn_lm_gemv_bf16_rows / rgn_lm_gemv_w8_rows (B in {1, 2, 3, 5, 8}, K past one 4096-wide round, strides wider than the rows,
plain / bias / resid / bias + resid / Y aliasing resid, sentinels, repeat), rgn_lm_head_argmax_rows (tokens and logits per row, a planted
tie while another row's maximum sits in the last block), rgn_lm_kv_append_bf16_rows, rgn_lm_decode_attention_bf16_rows (n = [1, 64, 65, 257]
in one launch, NaN past n[b], the exact probe in a different slice per row).
Model level, tiny genuine module, bf16 and fp8 weights: a left-padded batch of three prompts (one with image placeholders) against the
B = 1 generate of each unpadded prompt; EOS cut, pad fill and n_new whatever sync_every; determinism; B = 1 under max_batch = 8 against
the default adoption; kernel-only dispatch; the hosted opt-in."""
import ctypes
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
BATCHES = (1, 2, 3, 5, 8)
SENTINEL = -7.0
_gen, _cuda, _kernel_names = QB.gen, QB.cuda, QB.kernel_names


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


# ---- rgn_lm_gemv_bf16_rows / rgn_lm_gemv_w8_rows ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemv_case(N, K, w8):
    """Weights, 8 rows of x / resid with strides wider than the rows, and the one-row entry's answer for every row and variant."""
    g = _gen(N * 7 + K + int(w8))
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    if w8:
        W = ops.quantize_w8(W)
    ldx, ldn = K + 8, (N + 7) // 8 * 8 + 8
    X = torch.randn(8, ldx, device="cuda", generator=g).bfloat16()
    R = torch.randn(8, ldn + 8, device="cuda", generator=g).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g).bfloat16()
    lib = _lib.lib()
    want = {}
    for name, b, r in (("plain", None, False), ("bias", bias, False), ("resid", None, True), ("bias+resid", bias, True)):
        rows = []
        for i in range(8):
            y = torch.empty(ldn, dtype=torch.bfloat16, device="cuda")             # 16-byte aligned, as the fp8 entry wants
            res = R[i] if r else None
            if w8:
                rc = lib.rgn_lm_gemv_w8(_p(W), _p(W._rgn_scale), _p(X[i]), _p(b), _p(res), _p(y), N, K, _stream())
            else:
                rc = lib.rgn_lm_gemv_bf16(_p(W), _p(X[i]), _p(b), _p(res), _p(y), N, K, _stream())
            _lib.check(rc, "the one-row entry")
            rows.append(y[:N].clone())
        want[name] = torch.stack(rows)
    return W, X, R, bias, want


def _gemv_rows(W, X, bias, resid, Y, B, N, K, w8):
    lib = _lib.lib()
    ldr = 0 if resid is None else resid.stride(0)
    if w8:
        rc = lib.rgn_lm_gemv_w8_rows(_p(W), _p(W._rgn_scale), _p(X), X.stride(0), _p(bias), _p(resid), ldr, _p(Y), Y.stride(0), B, N, K, _stream())
    else:
        rc = lib.rgn_lm_gemv_bf16_rows(_p(W), _p(X), X.stride(0), _p(bias), _p(resid), ldr, _p(Y), Y.stride(0), B, N, K, _stream())
    _lib.check(rc, "rgn_lm_gemv_*_rows")
    return Y


def _check_gemv_rows(N, K, w8, batches):
    W, X, R, bias, want = _gemv_case(N, K, w8)
    ldn = (N + 7) // 8 * 8 + 8
    for B in batches:
        for name, b, r in (("plain", None, False), ("bias", bias, False), ("resid", None, True), ("bias+resid", bias, True)):
            Y = torch.full((8, ldn), SENTINEL, dtype=torch.bfloat16, device="cuda")
            got = _gemv_rows(W, X, b, R if r else None, Y, B, N, K, w8)
            for i in range(B):
                assert torch.equal(got[i, :N], want[name][i]), (N, K, w8, B, name, i)
            assert bool((got[B:] == SENTINEL).all()) and bool((got[:, N:] == SENTINEL).all()), "rows >= B and columns >= N are never written"
            Y2 = torch.full_like(Y, SENTINEL)
            assert torch.equal(_gemv_rows(W, X, b, R if r else None, Y2, B, N, K, w8), got), "a repeated call must be bit-identical"
        Ra = R.clone()                                                           # Y is resid: the same stride for both
        got = _gemv_rows(W, X, bias, Ra, Ra, B, N, K, w8)
        for i in range(B):
            assert torch.equal(got[i, :N], want["bias+resid"][i]), (N, K, w8, B, "alias", i)
        assert torch.equal(got[B:], R[B:]) and torch.equal(got[:, N:], R[:, N:])


@pytest.mark.parametrize("N,K", [(1, 64), (5, 64), (257, 192), (9, 4160)])
def test_gemv_rows_bf16_equals_the_one_row_entry_per_row(N, K):
    _check_gemv_rows(N, K, False, BATCHES)


@pytest.mark.parametrize("N,K", [(1, 64), (5, 64), (257, 192), (9, 4112)])
def test_gemv_rows_w8_equals_the_one_row_entry_per_row(N, K):
    _check_gemv_rows(N, K, True, BATCHES)


@pytest.mark.parametrize("w8", [False, True])
def test_gemv_rows_at_the_ff_down_shape(w8):
    _check_gemv_rows(3584, 18944, w8, (8,))


# ---- rgn_lm_head_argmax_rows --------------------------------------------------------------------------------------------------------
HK = 256


def _head_one(W, x):
    lib = _lib.lib()
    V, K = W.shape
    nb = lib.rgn_lm_head_workspace_bytes(V)
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    tok = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    z = torch.full((V,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.rgn_lm_head_argmax(_p(W), _p(x), V, K, _p(tok), _p(z), _p(ws), nb, _stream()), "rgn_lm_head_argmax")
    return int(tok), z


def _head_rows(W, X, B, with_logits=True, stride=1):
    lib = _lib.lib()
    V, K = W.shape
    nb = B * lib.rgn_lm_head_workspace_bytes(V)
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    tok = torch.full((8 * stride,), -1, dtype=torch.int64, device="cuda")
    z = torch.full((8, V + 3), float("nan"), dtype=torch.float32, device="cuda") if with_logits else None
    rc = lib.rgn_lm_head_argmax_rows(_p(W), _p(X), X.stride(0), B, V, K, _p(tok), stride, _p(z), V + 3, _p(ws), nb, _stream())
    _lib.check(rc, "rgn_lm_head_argmax_rows")
    return tok, z


@pytest.mark.parametrize("V", [5, 1030, 4096, 152064])                           # 4096: whole 8-row blocks; 152064: the real vocabulary
def test_head_rows_equal_the_one_row_entry_per_row(V):
    g = _gen(V)
    W = (torch.randn(V, HK, device="cuda", generator=g) * HK ** -0.5).bfloat16()
    X = torch.randn(8, HK + 8, device="cuda", generator=g).bfloat16()
    ones = [_head_one(W, X[i, :HK]) for i in range(8)]
    for B in (BATCHES if V < 100000 else (3, 8)):
        for stride in (1, 3):
            tok, z = _head_rows(W, X, B, stride=stride)
            for i in range(B):
                assert int(tok[i * stride]) == ones[i][0], (V, B, i)
                assert torch.equal(z[i, :V], ones[i][1]), (V, B, i)
            assert bool(z[B:].isnan().all()) and bool(z[:, V:].isnan().all())
            assert bool((tok.view(8, stride)[B:] == -1).all()) and bool((tok.view(8, stride)[:, 1:] == -1).all())
        tok2, _ = _head_rows(W, X, B, with_logits=False)
        assert tok2[:B].tolist() == [ones[i][0] for i in range(B)]               # logits_out = NULL picks the same tokens


@pytest.mark.parametrize("V", [1030, 4096])
def test_head_rows_give_a_tie_to_the_lower_index_while_another_rows_maximum_is_in_the_last_block(V):
    g = _gen(V + 1)
    W = (torch.randn(V, HK, device="cuda", generator=g) * HK ** -0.5).bfloat16()
    u = torch.randn(HK, device="cuda", generator=g).bfloat16()
    v = torch.randn(HK, device="cuda", generator=g).bfloat16()
    a, b = 17, V // 2 + 300
    W[a] = u
    W[b] = u                                                                     # two equal rows: equal fp32 logits for every x
    W[V - 1] = v                                                                 # |v|^2 ~ 256 against N(0, 1): row 1's maximum, in the last block
    X = torch.zeros(8, HK, dtype=torch.bfloat16, device="cuda")
    X[0], X[1], X[2] = u, v, u
    tok, z = _head_rows(W, X, 3)
    assert float(z[0, a]) == float(z[0, b]) == float(z[0, :V].max()) and float(z[1, V - 1]) == float(z[1, :V].max())
    assert tok[:3].tolist() == [a, V - 1, a]
    for i in range(3):
        one = _head_one(W, X[i])
        assert int(tok[i]) == one[0] and torch.equal(z[i, :V], one[1])


# ---- rgn_lm_kv_append_bf16_rows -----------------------------------------------------------------------------------------------------
def test_kv_append_rows_copies_each_row_into_its_own_cache_at_its_own_row():
    Hq, Hkv, cap, B = 4, 2, 96, 5
    ld, width = (Hq + 2 * Hkv) * 128 + 8, 2 * Hkv * 128
    stride = cap * width + 16                                                     # caches further apart than their rows
    qkv = torch.randn(8, ld, device="cuda", generator=_gen(5)).bfloat16()
    flat = torch.full((8 * stride,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    row0 = [0, 37, 95, 64, 1]
    rc = _lib.lib().rgn_lm_kv_append_bf16_rows(_p(qkv), ld, _p(flat), stride, cap, _ints(row0), B, Hq, Hkv, _stream())
    _lib.check(rc, "rgn_lm_kv_append_bf16_rows")
    want = torch.full_like(flat, SENTINEL)
    for b in range(B):
        at = b * stride + row0[b] * width
        want[at:at + width] = qkv[b, Hq * 128:(Hq + 2 * Hkv) * 128]
    assert torch.equal(flat, want)                                               # the copies bit for bit, sentinels everywhere else


# ---- rgn_lm_decode_attention_bf16_rows ----------------------------------------------------------------------------------------------
NS = [1, 64, 65, 257]


def _attention_one(q, cache, n, Hq, Hkv, scale):
    lib = _lib.lib()
    nb = lib.rgn_lm_decode_attention_workspace_bytes(Hq, n)
    ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda")
    o = torch.empty(Hq * 128, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.rgn_lm_decode_attention_bf16(_p(q), _p(cache), _p(o), n, Hq, Hkv, scale, _p(ws), nb, _stream()), "rgn_lm_decode_attention_bf16")
    return o


def _attention_rows(Q, caches, ns, Hq, Hkv, scale):
    lib = _lib.lib()
    B = len(ns)
    nb = B * lib.rgn_lm_decode_attention_workspace_bytes(Hq, max(ns))
    ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda")
    O = torch.full((B + 1, Hq * 128 + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    rc = lib.rgn_lm_decode_attention_bf16_rows(_p(Q), Q.stride(0), _p(caches), caches.stride(0), _p(O), O.stride(0), _ints(ns), B, Hq, Hkv, scale,
                                               _p(ws), nb, _stream())
    _lib.check(rc, "rgn_lm_decode_attention_bf16_rows")
    return O


@pytest.mark.parametrize("heads", [(2, 1), (28, 4)])
def test_attention_rows_equal_the_one_query_entry_per_row_and_never_read_past_n(heads):
    Hq, Hkv = heads
    g = _gen(Hq)
    B, cap, scale = len(NS), max(NS) + 3, 128 ** -0.5
    Q = torch.randn(B, (Hq + 2 * Hkv) * 128, device="cuda", generator=g).bfloat16()      # the q columns of packed QKV rows
    caches = torch.randn(B, cap, 2 * Hkv * 128, device="cuda", generator=g).bfloat16()
    for b, n in enumerate(NS):
        caches[b, n:] = 0
    want = [_attention_one(Q[b], caches[b], n, Hq, Hkv, scale) for b, n in enumerate(NS)]
    got = _attention_rows(Q, caches, NS, Hq, Hkv, scale)
    for b in range(B):
        assert torch.equal(got[b, :Hq * 128], want[b]), (heads, b)
    assert bool((got[B:] == SENTINEL).all()) and bool((got[:, Hq * 128:] == SENTINEL).all())
    assert torch.equal(_attention_rows(Q, caches, NS, Hq, Hkv, scale), got), "a repeated call must be bit-identical"
    for b, n in enumerate(NS):
        caches[b, n:] = float("nan")                                             # rows >= n[b] of every cache are never read
    assert torch.equal(_attention_rows(Q, caches, NS, Hq, Hkv, scale), got)
    order = [3, 0, 2, 1]                                                         # the longest cache first: the grid is sized for the longest
    got2 = _attention_rows(Q[order].contiguous(), caches[order].contiguous(), [NS[i] for i in order], Hq, Hkv, scale)
    for i, b in enumerate(order):
        assert torch.equal(got2[i, :Hq * 128], want[b])


@pytest.mark.parametrize("heads", [(2, 1), (28, 4)])
def test_a_key_60_above_the_rest_returns_its_value_row_bit_for_bit_in_a_different_slice_per_row(heads):
    Hq, Hkv = heads
    G = Hq // Hkv
    ns, js = [1, 65, 257, 257], [0, 64, 130, 200]                                # slices 0, 1, 2 and 3
    B, cap, scale = len(ns), 257, 128 ** -0.5
    g = _gen(Hq + 60)
    gain = 1.0 + 0.5 * (torch.arange(Hq, device="cuda") % 3).float()             # the heads of a group differ, every one still points at u
    Q = torch.zeros(B, Hq * 128, dtype=torch.bfloat16, device="cuda")
    caches = torch.randn(B, cap, 2 * Hkv * 128, device="cuda", generator=g)
    caches[:, :, :Hkv * 128] *= 0.01
    for b in range(B):
        u = torch.randn(Hkv, 128, device="cuda", generator=g)
        Q[b] = (u.repeat_interleave(G, dim=0) * gain[:, None]).bfloat16().reshape(Hq * 128)
        caches[b, js[b], :Hkv * 128] = (8.0 * u).reshape(-1)
    caches = caches.bfloat16()
    for b in range(1, B):                                                        # the probe is what it says
        n = ns[b]
        k = caches[b, :n, :Hkv * 128].double().view(n, Hkv, 128).transpose(0, 1).repeat_interleave(G, dim=0)
        s = scale * torch.einsum("hd,hnd->hn", Q[b].double().view(Hq, 128), k)
        rest = s.clone()
        rest[:, js[b]] = float("-inf")
        assert float((s[:, js[b]] - rest.max(dim=1).values).min()) >= 60.0
    got = _attention_rows(Q, caches, ns, Hq, Hkv, scale)
    for b in range(B):
        want = caches[b, js[b], Hkv * 128:].view(Hkv, 128).repeat_interleave(G, dim=0).reshape(Hq * 128)
        assert torch.equal(got[b, :Hq * 128], want), (heads, b)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
NEW = 12


@functools.lru_cache(maxsize=None)
def _run(weights):
    """One batched generate (twice) and the B = 1 generate of every unpadded row, shared by the tests below."""
    torch.manual_seed(0)
    m = HQ.tiny_qwen25vl(layers=2).cuda()
    hip = QT.HipQwen25VLTextEncoder(m, weights=weights, max_batch=8)
    one = QT.HipQwen25VLTextEncoder(m, weights=weights)                          # the default adoption: the oracle
    singles = QB.rows()
    ids, mask, grids, _ = QB.left_padded(singles)
    lens = [s.input_ids.shape[1] for s in singles]
    assert len(set(lens)) == 3 and int((ids[0] == HQ.IMAGE).sum()) == 4
    emb = torch.randn(4, 256, device="cuda", generator=_gen(11)).bfloat16()      # the image embeddings of row 0
    batch = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), image_grid_thw=grids.cuda(), mm_token_type_ids=(ids == HQ.IMAGE).int().cuda(),
                 image_embeds=emb)
    out = hip.generate(**batch, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    out2 = hip.generate(**batch, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    alone = []
    for b, s in enumerate(singles):
        kw = _cuda(s)
        if b == 0:
            kw["image_embeds"] = emb
        alone.append(one.generate(**kw, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True))
    return dict(hip=hip, one=one, batch=batch, singles=singles, lens=lens, out=out, out2=out2, alone=alone, L=ids.shape[1])


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_every_row_of_a_left_padded_batch_equals_its_own_generate_bit_for_bit(weights):
    s = _run(weights)
    seq, L = s["out"].sequences, s["L"]
    assert seq.dtype == torch.int64 and tuple(seq.shape) == (3, L + NEW) and torch.equal(seq[:, :L], s["batch"]["input_ids"])
    assert len(s["out"].logits) == NEW and all(tuple(z.shape) == (3, HQ.VOCAB) and z.dtype == torch.float32 for z in s["out"].logits)
    z = torch.stack(s["out"].logits)                                             # [NEW, 3, V]
    for b, n in enumerate(s["lens"]):
        a = s["alone"][b]
        assert torch.equal(seq[b, L:], a.sequences[0, n:]), (weights, b)
        assert torch.equal(z[:, b], torch.cat(a.logits)), (weights, b)
    plain = s["hip"].generate(**s["batch"], max_new_tokens=NEW)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, seq)


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_two_identical_batched_calls_are_equal(weights):
    s = _run(weights)
    assert torch.equal(s["out"].sequences, s["out2"].sequences)
    assert all(torch.equal(a, b) for a, b in zip(s["out"].logits, s["out2"].logits))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_eos_cut_pad_fill_and_n_new_do_not_depend_on_sync_every(weights):
    s = _run(weights)
    L, seq = s["L"], s["out"].sequences
    new = seq[:, L:].cpu()
    # an EOS id that two rows meet at different steps and one row never does, if the tokens offer one; else one only row 0 meets
    pick = None
    for t in new.flatten().tolist():
        hit = [(new[b] == t).nonzero().flatten().tolist() for b in range(3)]
        firsts = [h[0] for h in hit if h]
        if len(firsts) == 2 and firsts[0] != firsts[1]:
            pick = t
            break
    eos = [pick if pick is not None else int(new[0, 3])]
    pad = next(t for t in range(HQ.VOCAB) if t not in new)
    want = QB.greedy_search_rule(s["batch"]["input_ids"].cpu(), new.t(), eos, pad)
    for every in (1, 3, 64):
        got = s["hip"].generate(**s["batch"], max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad, sync_every=every)
        assert torch.equal(got.cpu(), want), (weights, every)
    for b, n in enumerate(s["lens"]):                                            # up to its EOS every row is still its own generate
        a = s["one"].generate(**dict(_cuda(s["singles"][b]), **({"image_embeds": s["batch"]["image_embeds"]} if b == 0 else {})),
                              max_new_tokens=NEW, eos_token_id=eos)
        k = a.shape[1] - n
        assert torch.equal(want[b, L:L + k], a[0, n:].cpu()) and bool((want[b, L + k:] == pad).all())
    # every row finishes: n_new is the largest cut, and the logits stop there
    eos_all = [int(new[0, 1]), int(new[1, 4]), int(new[2, 2])]
    want = QB.greedy_search_rule(s["batch"]["input_ids"].cpu(), new.t(), eos_all, eos_all[0])
    assert want.shape[1] < L + NEW
    for every in (1, 3, 64):
        res = s["hip"].generate(**s["batch"], max_new_tokens=NEW, eos_token_id=eos_all, sync_every=every, return_dict_in_generate=True,
                                output_logits=True)                              # no pad id anywhere: the first EOS id fills
        assert torch.equal(res.sequences.cpu(), want), (weights, every)
        assert len(res.logits) == want.shape[1] - L
        assert all(torch.equal(a, b) for a, b in zip(res.logits, s["out"].logits))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_one_row_under_max_batch_is_the_default_adoption(weights):
    s = _run(weights)
    kw = _cuda(s["singles"][1])
    got = s["hip"].generate(**kw, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    assert torch.equal(got.sequences, s["alone"][1].sequences)
    assert all(torch.equal(a, b) for a, b in zip(got.logits, s["alone"][1].logits))


def test_one_row_under_max_batch_launches_the_one_row_kernels():
    """B = 1 of a `_rows` entry is the one-row entry: a max_batch=8 adoption decodes one unpadded row on the one-row kernels, greedy and
    sampled, and launches no `_rows` kernel of csrc/decode.hip at all (they are all named lm_*_rows_kernel; rms_norm_rows_kernel is the
    row norm of csrc/norm.hip, which every decode step runs at M = B)."""
    s = _run("bf16")
    kw, T = _cuda(s["singles"][1]), 4

    def batched(names):
        return [n for n in names if "_rows_kernel" in n and "rms_norm_rows_kernel" not in n]
    names = _kernel_names(lambda: s["hip"].generate(**kw, max_new_tokens=T, eos_token_id=[]))
    for k in ("lm_gemv_kernel", "lm_decode_attention_kernel", "lm_decode_merge_kernel", "lm_head_finalize_kernel"):
        assert any(k in n for n in names), k
    assert batched(names) == []
    sampled = QT.HipQwen25VLTextEncoder(s["hip"].module, sampling=True, max_batch=8, batch_sampling=True)
    uni = torch.rand(T, device="cuda", generator=_gen(5))
    names = _kernel_names(lambda: sampled.generate(**kw, max_new_tokens=T, eos_token_id=[], do_sample=True, temperature=0.7, top_k=20,
                                                   top_p=0.8, repetition_penalty=1.05, uniforms=uni))
    assert sum("lm_pick_kernel" in n for n in names) == T
    assert batched(names) == []


def test_a_warm_batched_generate_dispatches_only_libregione_hip_kernels():
    from torch.profiler import ProfilerActivity, profile
    s = _run("bf16")
    hip, batch = s["hip"], s["batch"]
    hip.generate(**batch, max_new_tokens=4)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        seq = hip.generate(**batch, max_new_tokens=4)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    for k in ("lm_gemv_rows_kernel", "lm_kv_append_rows_kernel", "lm_decode_attention_rows_kernel", "lm_decode_merge_rows_kernel",
              "lm_head_finalize_rows_kernel"):
        assert any(k in n for n in names), k
    assert torch.equal(seq, s["out"].sequences[:, :s["L"] + 4])


def test_the_hosted_opt_in_binds_max_batch():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_batch = 9
    with pytest.raises(ValueError, match="1..8"):
        with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
            pass
    pipe._regione_hip_text_batch = 3
    ids, mask, _, _ = QB.left_padded(QB.rows(QB.PROMPTS[1:]))
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        enc = pipe.text_encoder
        assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.max_batch == 3
        got = enc.generate(input_ids=ids.cuda(), attention_mask=mask.cuda(), max_new_tokens=4, do_sample=False)
    assert pipe.text_encoder is m
    assert tuple(got.shape) == (2, ids.shape[1] + 4) and torch.equal(got[:, :ids.shape[1]].cpu(), ids) and int(got.max()) < HQ.VOCAB
