"""-m gpu: greedy generate() of the Qwen2.5-VL prompt encoder on the HIP kernels (regione_amd/qwen_text_encoder.py, csrc/decode.hip).

Kernel level, against fp64 with derived bounds:
  * rgn_lm_gemv_bf16: |got - ref| <= r 2^-8 |ref| + K 2^-24 sum_k |W x| (+ 2^-8 |resid|), r = 1 roundings without resid, 2 with; the real
    extremes (3584, 18944) and (152064, 3584) included; y aliasing resid; a repeated call is bit-identical;
  * rgn_lm_kv_append_bf16: torch.equal against the slice, rows outside [row0, row0 + L) keep a sentinel;
  * rgn_lm_decode_attention_bf16: n across every slice boundary, three head layouts, the inputs and the 2e-2 bound of
    test_lm_attention_matches_fp32_softmax; exact probes (a key 60 above the rest returns its V row bit for bit; NaN in rows >= n changes
    nothing);
  * rgn_lm_head_argmax: planted maxima, exact ties (the lower index wins, in one block or across blocks), all-negative logits.
Model level, the genuine tiny module in fp32 as reference and its eager bf16 copy as yardstick, teacher-forced over HIP's own sequence:
tokens are the argmax of HIP's own logits; PSNR and max error against fp32 within the standing margins of eager bf16; a control with
text-only decode positions that the parity assertion must see; EOS cut independent of sync_every; determinism; kernel-only dispatch; the
hosted binding.  Token equality with eager `generate` is deliberately NOT asserted: on the tiny model the fp32 top-2 gap (0.0007 - 0.008)
is below the eager bf16 logit error (0.009 - 0.012)."""
import copy
import functools
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
from regione_amd import _lib, ops  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- rgn_lm_gemv_bf16 ---------------------------------------------------------------------------------------------------------------
def _gemv(W, x, bias, resid, y):
    N, K = W.shape
    _lib.check(_lib.lib().rgn_lm_gemv_bf16(_p(W), _p(x), _p(bias), _p(resid), _p(y), N, K, _stream()), "rgn_lm_gemv_bf16")
    return y


@pytest.mark.parametrize("N,K", [(1, 64), (5, 64), (257, 192), (4608, 3584), (3584, 18944), (152064, 3584)])
def test_lm_gemv_matches_fp64_within_the_derived_bound(N, K):
    g = _gen(N * 7 + K)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    x = torch.randn(K, device="cuda", generator=g).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g).bfloat16()
    resid = torch.randn(N, device="cuda", generator=g).bfloat16()
    if N > 4608:                                                                 # the vocabulary: 512 seeded rows, the first and the last
        rows = torch.cat([torch.tensor([0, N - 1]), torch.randint(0, N, (512,), generator=torch.Generator().manual_seed(N))]).cuda()
    else:
        rows = torch.arange(N, device="cuda")
    Wd, xd = W[rows].double(), x.double()
    dot = Wd @ xd
    slack = K * 2.0 ** -24 * (Wd.abs() @ xd.abs())
    bd, rd = bias[rows].double(), resid[rows].double()
    for name, b, r in (("plain", None, None), ("bias", bias, None), ("resid", None, resid), ("bias+resid", bias, resid),
                       ("bias+resid, y is resid", bias, "alias")):
        y = resid.clone() if isinstance(r, str) else torch.full((N,), float("nan"), dtype=torch.bfloat16, device="cuda")
        got = _gemv(W, x, b, y if isinstance(r, str) else r, y)
        ref = dot + (bd if b is not None else 0)
        bound = slack.clone()
        if r is not None:
            ref = ref + rd
            bound = bound + 2.0 ** -8 * rd.abs()
        bound = bound + (2 if r is not None else 1) * 2.0 ** -8 * ref.abs()
        err = (got[rows].double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"lm_gemv N={N} K={K} {name}: max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (N, K, name, worst)
        y2 = resid.clone() if isinstance(r, str) else torch.empty_like(y)
        assert torch.equal(_gemv(W, x, b, y2 if isinstance(r, str) else r, y2), got), "a repeated call must be bit-identical"


# ---- rgn_lm_kv_append_bf16 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row0", [0, 37])
@pytest.mark.parametrize("L", [1, 64, 65])
def test_kv_append_copies_the_kv_columns_bit_for_bit_and_touches_nothing_else(row0, L):
    Hq, Hkv, cap = 4, 2, 128
    ld = (Hq + 2 * Hkv) * 128 + 8                                                # a row stride wider than the columns
    g = _gen(row0 + L)
    qkv = torch.randn(L, ld, device="cuda", generator=g).bfloat16()
    cache = torch.full((cap, 2 * Hkv * 128), -7.0, dtype=torch.bfloat16, device="cuda")
    rc = _lib.lib().rgn_lm_kv_append_bf16(_p(qkv), ld, _p(cache), cap, row0, L, Hq, Hkv, _stream())
    _lib.check(rc, "rgn_lm_kv_append_bf16")
    assert torch.equal(cache[row0:row0 + L], qkv[:, Hq * 128:(Hq + 2 * Hkv) * 128])
    assert bool((cache[:row0] == -7.0).all()) and bool((cache[row0 + L:] == -7.0).all())


# ---- rgn_lm_decode_attention_bf16 ---------------------------------------------------------------------------------------------------
def _decode_attention(q, cache, n, Hq, Hkv, scale):
    lib = _lib.lib()
    nb = lib.rgn_lm_decode_attention_workspace_bytes(Hq, n)
    ws = torch.empty(nb // 4, dtype=torch.float32, device="cuda")
    o = torch.empty(Hq * 128, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.rgn_lm_decode_attention_bf16(_p(q), _p(cache), _p(o), n, Hq, Hkv, scale, _p(ws), nb, _stream()), "rgn_lm_decode_attention_bf16")
    return o


def _decode_attention_ref(q, cache, n, Hq, Hkv, scale):
    G = Hq // Hkv
    k = cache[:n, :Hkv * 128].float().view(n, Hkv, 128).transpose(0, 1).repeat_interleave(G, dim=0)      # [Hq, n, 128]
    v = cache[:n, Hkv * 128:].float().view(n, Hkv, 128).transpose(0, 1).repeat_interleave(G, dim=0)
    s = scale * torch.einsum("hd,hnd->hn", q.float().view(Hq, 128), k)
    return torch.einsum("hn,hnd->hd", torch.softmax(s, -1), v).reshape(Hq * 128)


@pytest.mark.parametrize("heads", [(2, 1), (4, 4), (28, 4)])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 257, 1500, 4096])
def test_decode_attention_matches_fp32_softmax(n, heads):
    Hq, Hkv = heads
    g = _gen(n * 131 + Hq)
    q = torch.randn(Hq * 128, device="cuda", generator=g).bfloat16()
    cap = min(n + 3, 4096)
    cache = torch.randn(cap, 2 * Hkv * 128, device="cuda", generator=g).bfloat16()
    scale = 128 ** -0.5
    cache[n:] = 0
    got = _decode_attention(q, cache, n, Hq, Hkv, scale)
    err = float((got.float() - _decode_attention_ref(q, cache, n, Hq, Hkv, scale)).abs().max())
    print(f"lm_decode_attention n={n} Hq={Hq} Hkv={Hkv}: max abs err {err:.3e}")
    assert err <= 2e-2, (n, heads, err)
    assert torch.equal(got, _decode_attention(q, cache, n, Hq, Hkv, scale)), "a repeated call must be bit-identical"
    cache[n:] = float("nan")                                                     # rows >= n are never read
    assert torch.equal(got, _decode_attention(q, cache, n, Hq, Hkv, scale))


@pytest.mark.parametrize("heads", [(2, 1), (4, 4), (28, 4)])
@pytest.mark.parametrize("n,j", [(1, 0), (65, 64), (257, 100), (4096, 4095)])
def test_a_key_60_above_the_rest_returns_its_value_row_bit_for_bit(n, j, heads):
    Hq, Hkv = heads
    G = Hq // Hkv
    g = _gen(n + j + Hq)
    u = torch.randn(Hkv, 128, device="cuda", generator=g)
    gain = 1.0 + 0.5 * (torch.arange(Hq, device="cuda") % 3).float()             # the heads of a group differ, every one still points at u
    q = (u.repeat_interleave(G, dim=0) * gain[:, None]).bfloat16().reshape(Hq * 128)
    cache = torch.randn(n, 2 * Hkv * 128, device="cuda", generator=g)
    cache[:, :Hkv * 128] *= 0.01
    cache[j, :Hkv * 128] = (8.0 * u).reshape(-1)
    cache = cache.bfloat16()
    scale = 128 ** -0.5
    k = cache[:, :Hkv * 128].double().view(n, Hkv, 128).transpose(0, 1).repeat_interleave(G, dim=0)
    s = scale * torch.einsum("hd,hnd->hn", q.double().view(Hq, 128), k)
    if n > 1:
        rest = s.clone()
        rest[:, j] = float("-inf")
        assert float((s[:, j] - rest.max(dim=1).values).min()) >= 60.0           # the probe is what it says
    got = _decode_attention(q, cache, n, Hq, Hkv, scale)
    want = cache[j, Hkv * 128:].view(Hkv, 128).repeat_interleave(G, dim=0).reshape(Hq * 128)
    assert torch.equal(got, want)


# ---- rgn_lm_head_argmax -------------------------------------------------------------------------------------------------------------
HK = 256


def _head(W, x, with_logits=True):
    lib = _lib.lib()
    V, K = W.shape
    nb = lib.rgn_lm_head_workspace_bytes(V)
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    tok = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    z = torch.full((V,), float("nan"), dtype=torch.float32, device="cuda") if with_logits else None
    _lib.check(lib.rgn_lm_head_argmax(_p(W), _p(x), V, K, _p(tok), _p(z), _p(ws), nb, _stream()), "rgn_lm_head_argmax")
    return int(tok), z


def _first_argmax(z):
    return int(torch.nonzero(z == z.max())[0])


def _check_logits(W, x, z):
    Wd, xd = W.double(), x.double()
    err, bound = (z.double() - Wd @ xd).abs(), W.shape[1] * 2.0 ** -24 * (Wd.abs() @ xd.abs())
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


@functools.lru_cache(maxsize=None)
def _head_inputs(V):
    g = _gen(V)
    W = (torch.randn(V, HK, device="cuda", generator=g) * HK ** -0.5).bfloat16()
    x = torch.randn(HK, device="cuda", generator=g).bfloat16()
    return W, x


@pytest.mark.parametrize("V", [1, 1000, 1024, 152064])
def test_head_argmax_finds_a_planted_maximum_and_its_logits_match_fp64(V):
    W0, x = _head_inputs(V)
    for at in sorted({0, V // 2, V - 1}):
        W = W0.clone()
        W[at] = x                                                                # z[at] = |x|^2 ~ 256 against N(0, 1) elsewhere
        tok, z = _head(W, x)
        assert tok == at == _first_argmax(z), (V, at, tok)
        _check_logits(W, x, z)
        assert _head(W, x, with_logits=False)[0] == at                           # logits_out = NULL picks the same token
        assert _head(W, x)[0] == at and torch.equal(_head(W, x)[1], z)           # a repeated call is bit-identical


@pytest.mark.parametrize("V", [1000, 1024, 152064])
def test_head_argmax_gives_an_exact_tie_to_the_lower_index(V):
    W0, x = _head_inputs(V)
    pairs = [(0, 1), (2, 9), (15, 16), (5, V - 3), (V - 2, V - 1), (V // 2 - 7, V // 2 + 300), (17, 16 * 256 + 17 if V > 5000 else 16 * 40 + 1)]
    for a, b in pairs:                                                           # same block, neighbouring blocks, far apart
        assert 0 <= a < b < V
        W = W0.clone()
        W[a] = x
        W[b] = x                                                                 # two equal rows: equal fp32 logits
        tok, z = _head(W, x)
        assert float(z[a]) == float(z[b]) == float(z.max())
        assert tok == a, (V, a, b, tok)


@pytest.mark.parametrize("V", [1, 1000, 152064])
def test_head_argmax_over_all_negative_logits(V):
    _, x = _head_inputs(V)
    a = 0.5 + 1.5 * torch.rand(V, device="cuda", generator=_gen(V + 1))
    W = (-a[:, None] * x.float()[None, :]).bfloat16()                            # z[v] ~ -a_v |x|^2 < 0
    tok, z = _head(W, x)
    assert float(z.max()) < 0
    assert tok == _first_argmax(z)
    _check_logits(W, x, z)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
ONE = "make the square red and keep the rest of the picture as it is"
LONG = " ".join([ONE] * 3)                                                       # text-only: L = 53, the cache crosses 64 while decoding
GQA = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=1024)
CASES = {"one_image": (1, ONE, None, 31), "two_images": (2, ONE + " with three birds", None, 46), "text": (0, LONG, None, 53),
         "text_gqa": (0, LONG, GQA, 53)}
NEW = 16


def _inputs(n_images, prompt):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    base = "".join(f"Picture {i + 1}: <image> " if n_images > 1 else "<image> " for i in range(n_images))
    mi = HQ.ToyProcessor()(text=[base + prompt], images=images or None).to("cuda")
    kw = dict(input_ids=mi.input_ids, attention_mask=mi.attention_mask)
    if n_images:
        kw.update(pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw, mm_token_type_ids=(mi.input_ids == HQ.IMAGE).int())
    return kw


@functools.lru_cache(maxsize=None)
def _run(case):
    """One teacher-forced comparison per case, shared by the tests below: HIP's generate (twice, a __call__ before and between), then the
    fp32 module and its eager bf16 copy once over HIP's own full sequence."""
    n_images, prompt, text_kw, L = CASES[case]
    torch.manual_seed(0)
    ref = HQ.tiny_qwen25vl(text_kw=text_kw, dtype=torch.float32, layers=2).cuda()
    bf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = QT.HipQwen25VLTextEncoder(bf)
    kw = _inputs(n_images, prompt)
    assert kw["input_ids"].shape == (1, L)
    call0 = hip(**kw).last_hidden_state
    out = hip.generate(**kw, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    call1 = hip(**kw).last_hidden_state
    out2 = hip.generate(**kw, max_new_tokens=NEW, return_dict_in_generate=True, output_logits=True)
    seq = out.sequences
    full = dict(input_ids=seq, attention_mask=torch.ones_like(seq))
    if n_images:
        full.update(pixel_values=kw["pixel_values"], image_grid_thw=kw["image_grid_thw"], mm_token_type_ids=(seq == HQ.IMAGE).int())
    with torch.no_grad():
        r = ref(**full).logits[0, L - 1:L + NEW - 1].float()
        e = bf(**full).logits[0, L - 1:L + NEW - 1].float()
        c = None
        if n_images:                                                             # the control: text-only positions for the new tokens
            pos = hip.position_ids_for(kw["input_ids"], kw["attention_mask"], kw["image_grid_thw"], None, kw["mm_token_type_ids"])
            tail = torch.arange(L, L + NEW, device=pos.device).view(1, 1, -1).expand(3, 1, -1)
            wrong = dict(full, position_ids=torch.cat([pos, tail], dim=2))
            c = ref(**wrong).logits[0, L - 1:L + NEW - 1].float()
    h = torch.cat(out.logits, dim=0)
    return dict(hip=hip, kw=kw, L=L, out=out, out2=out2, call0=call0, call1=call1, r=r, e=e, h=h, c=c)


@pytest.mark.parametrize("case", list(CASES))
def test_generate_returns_the_prompt_and_the_argmax_of_its_own_logits(case):
    s = _run(case)
    seq, L = s["out"].sequences, s["L"]
    assert seq.dtype == torch.int64 and seq.shape == (1, L + NEW) and seq.device == s["kw"]["input_ids"].device
    assert torch.equal(seq[:, :L], s["kw"]["input_ids"])
    assert len(s["out"].logits) == NEW and all(z.shape == (1, HQ.VOCAB) and z.dtype == torch.float32 for z in s["out"].logits)
    for k in range(NEW):
        assert int(seq[0, L + k]) == _first_argmax(s["h"][k]), k
    plain = s["hip"].generate(**s["kw"], max_new_tokens=NEW)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, seq)


@pytest.mark.parametrize("case", list(CASES))
def test_generate_logits_are_as_close_to_fp32_as_eager_bf16(case):
    s = _run(case)
    r, e, h = s["r"], s["e"], s["h"]
    ph, pe = psnr(h, r), psnr(e, r)
    eh, ee = float((h - r).abs().max()), float((e - r).abs().max())
    toks = s["out"].sequences[0, s["L"]:]
    regret = float((r.max(dim=1).values - r.gather(1, toks[:, None])[:, 0]).max())
    print(f"generate {case}: HIP {ph:.2f} dB / max err {eh:.4f}, eager bf16 {pe:.2f} dB / max err {ee:.4f} against fp32; "
          f"largest fp32 regret of a HIP token {regret:.4f}")
    assert ph >= pe - 1.0, (ph, pe)
    assert eh <= 2 * ee, (eh, ee)
    assert regret <= 4 * ee, (regret, ee)


@pytest.mark.parametrize("case", ["one_image", "two_images"])
def test_the_parity_assertion_would_see_text_only_decode_positions(case):
    s = _run(case)
    pc, pe = psnr(s["c"], s["r"]), psnr(s["e"], s["r"])
    print(f"generate {case}: fp32 with text-only decode positions {pc:.2f} dB, eager bf16 {pe:.2f} dB against fp32")
    assert pc <= pe - 3.0, (pc, pe)


def test_eos_cuts_after_its_first_occurrence_whatever_sync_every():
    tried = 0
    for case in CASES:
        s = _run(case)
        L, seq = s["L"], s["out"].sequences
        new = seq[0, L:].tolist()
        js = [j for j in range(2, NEW) if new[j] not in new[:j]]
        if not js:
            continue
        j = js[len(js) // 2]
        tried += 1
        other = next(t for t in range(HQ.VOCAB) if t not in new)
        for eos in (new[j], [other, new[j]]):
            for every in (1, 4, 8):
                got = s["hip"].generate(**s["kw"], max_new_tokens=NEW, eos_token_id=eos, sync_every=every)
                assert torch.equal(got, seq[:, :L + j + 1]), (case, j, every)
        res = s["hip"].generate(**s["kw"], max_new_tokens=NEW, eos_token_id=new[j], return_dict_in_generate=True, output_logits=True)
        assert len(res.logits) == j + 1 and torch.equal(torch.cat(res.logits), s["h"][:j + 1])
    assert tried >= 1, "no case produced a token that first occurs at a new index >= 2"


@pytest.mark.parametrize("case", list(CASES))
def test_generate_is_deterministic_and_leaves_the_encoder_call_alone(case):
    s = _run(case)
    assert torch.equal(s["out"].sequences, s["out2"].sequences)
    assert all(torch.equal(a, b) for a, b in zip(s["out"].logits, s["out2"].logits))
    assert torch.equal(s["call0"], s["call1"])


def test_a_warm_generate_dispatches_only_libregione_hip_kernels():
    from torch.profiler import ProfilerActivity, profile
    s = _run("text")
    hip, kw = s["hip"], s["kw"]
    hip.generate(**kw, max_new_tokens=4)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        seq = hip.generate(**kw, max_new_tokens=4)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    foreign = sorted({n[:120] for n in names if not (("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset")))})
    assert foreign == [], foreign
    for k in ("lm_gemv_kernel", "lm_kv_append_kernel", "lm_decode_attention_kernel", "lm_decode_merge_kernel", "lm_head_finalize_kernel"):
        assert any(k in n for n in names), k
    assert torch.equal(seq, s["out"].sequences[:, :s["L"] + 4])


def test_the_hosted_binding_answers_generate_on_the_hip_path():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    kw = _inputs(1, ONE)
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        assert isinstance(pipe.text_encoder, QT.HipQwen25VLTextEncoder)
        got = pipe.text_encoder.generate(**kw, max_new_tokens=4, do_sample=False)
    assert pipe.text_encoder is m and fired == []
    assert got.shape == (1, 31 + 4) and torch.equal(got[:, :31], kw["input_ids"]) and int(got.max()) < HQ.VOCAB
    assert torch.equal(pipe._regione_hip_qwen_text.generate(**kw, max_new_tokens=4), got)
