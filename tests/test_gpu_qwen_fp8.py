"""-m gpu: the Qwen2.5-VL language model on fp8 weights (HipQwen25VLTextEncoder(weights="fp8"), rgn_lm_gemv_w8 of csrc/decode.hip).

Kernel level:
  * an exact probe of the decode and the scale: column k of every row holds byte code k, x = e_k; y[n] must be bf16(fp32(s[n]) value(k))
    bit for bit, the value taken from torch.float8_e4m3fn on the CPU (sees a fnuz decode, a swapped byte or word, a dropped scale, a scale
    per element).  Two details of the probe: the columns of the two NaN codes (0x7f, 0xff, which quantize_w8 cannot produce) hold code 0,
    since NaN * 0 would poison every sum; and for code 0x80 the reference product is -0 while a sum that also holds +0 terms (the other
    columns times the zeros of x, and the +0 the accumulator starts from) is +0 in IEEE arithmetic, so both zero codes must give +0;
  * |got - ref| <= r 2^-8 |ref| + (K + 1) 2^-24 s[n] sum_k |q x| (+ 2^-8 |resid|) against fp64, r = 1 without resid and 2 with: the bound
    of test_lm_gemv_matches_fp64_within_the_derived_bound plus one fp32 rounding for the scale multiply; the five variants of that test;
    K one 16-byte vector below, at and above each period of the kernel's loop; the four layer shapes; a repeated call is bit-identical;
  * rows >= N are not written.
Model level, on the tiny genuine module (layers = 2): the reference is the fp32 module whose projection matrices hold the dequantised
values q * scale of their own quantize_w8, the yardstick its eager bf16 copy, teacher-forced over HIP's own sequence; the standing margins
of the bf16 tests; a control against the fp32 module with the ORIGINAL weights that bf16 weights used by mistake could not pass."""
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
FP8 = torch.float8_e4m3fn

# csrc/decode.hip, lm_gemv_w8_kernel: a lane takes 16 weights per 16-byte load, a step of the wave is 64 lanes x 16, a round is W8_U steps;
# a wave takes W8_ROWS rows and a block 4 waves (N = 5 and 257 leave a wave with one row, N = 1 a block with one wave)
W8_VEC, W8_STEP, W8_U, W8_ROWS = 16, 64 * 16, 4, 2
W8_ROUND = W8_STEP * W8_U
PERIOD_KS = [W8_STEP - W8_VEC, W8_STEP, W8_STEP + W8_VEC, W8_ROUND - W8_VEC, W8_ROUND, W8_ROUND + W8_VEC]
LAYER_SHAPES = [(4608, 3584), (3584, 3584), (37888, 3584), (3584, 18944)]


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _gemv8(q, scale, x, bias, resid, y, N=None):
    n, K = q.shape
    rc = _lib.lib().rgn_lm_gemv_w8(_p(q), _p(scale), _p(x), _p(bias), _p(resid), _p(y), n if N is None else N, K, _stream())
    _lib.check(rc, "rgn_lm_gemv_w8")
    return y


# ---- 1. the exact probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", ["ones", "seeded"])
def test_every_finite_code_times_the_scale_comes_back_bit_for_bit(scales):
    N, K = 5, 256
    codes = torch.arange(256, dtype=torch.uint8)
    value = codes.view(FP8).float()                                              # the CPU's OCP e4m3fn decode
    finite = [k for k in range(256) if k not in (0x7f, 0xff)]
    assert bool(torch.isfinite(value[finite]).all()) and float(value[0x7e]) == 448.0 and float(value[0x01]) == 2.0 ** -9
    held = codes.clone()
    held[0x7f] = held[0xff] = 0                                                  # NaN * 0 would poison every sum
    q = held.view(FP8)[None, :].repeat(N, 1).contiguous().cuda()
    s = torch.ones(N) if scales == "ones" else 0.5 + torch.rand(N, generator=torch.Generator().manual_seed(11))
    assert s.dtype == torch.float32
    want = (s[:, None] * value[None, :]).bfloat16()                              # bf16(fp32(s[n]) value(code)), [N, 256]
    sd = s.cuda()
    got = torch.empty(N, 256, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(N, dtype=torch.bfloat16, device="cuda")
    x = torch.zeros(K, dtype=torch.bfloat16, device="cuda")
    for k in finite:
        x.zero_()
        x[k] = 1.0
        got[:, k] = _gemv8(q, sd, x, None, None, y)
    gb, wb = got.cpu().view(torch.int16), want.view(torch.int16)
    zero = [0x00, 0x80]
    rest = [k for k in finite if k not in zero]
    bad = [(k, n) for k in rest for n in range(N) if int(gb[n, k]) != int(wb[n, k])]
    assert bad == [], bad[:8]
    assert bool((gb[:, zero] == 0).all())                                        # +0: see the module docstring


# ---- 2. the fp64 bound ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemv_inputs(N, K):
    g = _gen(N * 7 + K)
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    q = ops.quantize_w8(W)
    x = torch.randn(K, device="cuda", generator=g).bfloat16()
    bias = torch.randn(N, device="cuda", generator=g).bfloat16()
    resid = torch.randn(N, device="cuda", generator=g).bfloat16()
    return q, q._rgn_scale, x, bias, resid


@pytest.mark.parametrize("N,K", [(N, K) for N in (1, 5, 257) for K in PERIOD_KS] + LAYER_SHAPES)
def test_lm_gemv_w8_matches_fp64_within_the_derived_bound(N, K):
    q, s, x, bias, resid = _gemv_inputs(N, K)
    assert q.dtype == FP8 and s.dtype == torch.float32 and s.shape == (N,)
    if N > 4608:                                                                 # 512 seeded rows, the first and the last
        rows = torch.cat([torch.tensor([0, N - 1]), torch.randint(0, N, (512,), generator=torch.Generator().manual_seed(N))]).cuda()
    else:
        rows = torch.arange(N, device="cuda")
    qd, xd, sd = q[rows].float().double(), x.double(), s[rows].double()
    dot = sd * (qd @ xd)
    slack = (K + 1) * 2.0 ** -24 * sd * (qd.abs() @ xd.abs())
    bd, rd = bias[rows].double(), resid[rows].double()
    for name, b, r in (("plain", None, None), ("bias", bias, None), ("resid", None, resid), ("bias+resid", bias, resid),
                       ("bias+resid, y is resid", bias, "alias")):
        y = resid.clone() if isinstance(r, str) else torch.full((N,), float("nan"), dtype=torch.bfloat16, device="cuda")
        got = _gemv8(q, s, x, b, y if isinstance(r, str) else r, y)
        ref = dot + (bd if b is not None else 0)
        bound = slack.clone()
        if r is not None:
            ref = ref + rd
            bound = bound + 2.0 ** -8 * rd.abs()
        bound = bound + (2 if r is not None else 1) * 2.0 ** -8 * ref.abs()
        err = (got[rows].double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"lm_gemv_w8 N={N} K={K} {name}: max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
        assert bool((err <= bound).all()), (N, K, name, worst)
        y2 = resid.clone() if isinstance(r, str) else torch.empty_like(y)
        assert torch.equal(_gemv8(q, s, x, b, y2 if isinstance(r, str) else r, y2), got), "a repeated call must be bit-identical"


# ---- 3. rows >= N --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 4 * W8_ROWS, 4 * W8_ROWS + 1, 257])
def test_rows_past_n_are_not_written(N):
    K = W8_STEP + W8_VEC
    q, s, x, bias, _ = _gemv_inputs(N + 3, K)
    y = torch.full((N + 3,), -7.0, dtype=torch.bfloat16, device="cuda")
    _gemv8(q, s, x, bias, None, y, N=N)
    full = _gemv8(q, s, x, bias, None, torch.empty(N + 3, dtype=torch.bfloat16, device="cuda"))
    assert torch.equal(y[:N], full[:N]) and bool((y[N:] == -7.0).all())


# ---- the model ----------------------------------------------------------------------------------------------------------------------
ONE = "make the square red and keep the rest of the picture as it is"
LONG = " ".join([ONE] * 3)                                                       # text-only: L = 53, the cache crosses 64 while decoding
GQA = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=1024)
CASES = {"text": (0, LONG, None, 53), "text_gqa": (0, LONG, GQA, 53), "one_image": (1, ONE, None, 31)}
NEW = 16
MATRICES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _inputs(n_images, prompt):
    g = torch.Generator().manual_seed(3)
    images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(n_images)]
    base = "".join(f"Picture {i + 1}: <image> " if n_images > 1 else "<image> " for i in range(n_images))
    mi = HQ.ToyProcessor()(text=[base + prompt], images=images or None).to("cuda")
    kw = dict(input_ids=mi.input_ids, attention_mask=mi.attention_mask)
    if n_images:
        kw.update(pixel_values=mi.pixel_values, image_grid_thw=mi.image_grid_thw, mm_token_type_ids=(mi.input_ids == HQ.IMAGE).int())
    return kw


def _dequantised(orig, bf):
    """The fp32 module `orig` with its 7 projection matrices per layer replaced by q * scale of quantize_w8 of the bf16 module's (what
    the fp8 adoption of `bf` computes on); the scale is per row, so q, k and v alone quantise as their concatenation does."""
    deq = copy.deepcopy(orig)
    n = 0
    for lb, ld in zip(bf.model.language_model.layers, deq.model.language_model.layers):
        for name in MATRICES:
            q = ops.quantize_w8(lb.get_submodule(name).weight.data)
            ld.get_submodule(name).weight.data.copy_(q.float() * q._rgn_scale[:, None])
            n += 1
    assert n == 7 * len(bf.model.language_model.layers)
    return deq


@functools.lru_cache(maxsize=None)
def _run(case):
    """One teacher-forced comparison per case, shared by the tests below: HIP's fp8 generate (twice, a __call__ before and between), then
    the dequantised fp32 module, its eager bf16 copy and the fp32 module with the original weights once over HIP's own full sequence."""
    n_images, prompt, text_kw, L = CASES[case]
    torch.manual_seed(0)
    orig = HQ.tiny_qwen25vl(text_kw=text_kw, dtype=torch.float32, layers=2).cuda()
    bf = copy.deepcopy(orig).to(torch.bfloat16)
    ref = _dequantised(orig, bf)
    ebf = copy.deepcopy(ref).to(torch.bfloat16)
    hip = QT.HipQwen25VLTextEncoder(bf, weights="fp8")
    assert hip.weights == "fp8" and all(p[k].dtype == FP8 for p in hip.layers for k in ("wqkv", "wo", "wgu", "wdown"))
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
        r, e, o = (m(**full).logits[0, L - 1:L + NEW - 1].float() for m in (ref, ebf, orig))
        hr, he, ho = (m(**kw, output_hidden_states=True).hidden_states[-1].float() for m in (ref, ebf, orig))
    h = torch.cat(out.logits, dim=0)
    return dict(hip=hip, kw=kw, L=L, out=out, out2=out2, call0=call0, call1=call1, r=r, e=e, o=o, h=h, hr=hr, he=he, ho=ho)


def _first_argmax(z):
    return int(torch.nonzero(z == z.max())[0])


@pytest.mark.parametrize("case", list(CASES))
def test_fp8_call_is_as_close_to_the_dequantised_fp32_module_as_eager_bf16(case):
    s = _run(case)
    h, r, e = s["call0"].float(), s["hr"], s["he"]
    assert s["call0"].dtype == torch.bfloat16 and h.shape == r.shape
    ph, pe = psnr(h, r), psnr(e, r)
    print(f"fp8 __call__ {case}: HIP {ph:.2f} dB, eager bf16 {pe:.2f} dB against the dequantised fp32 module; "
          f"HIP against the ORIGINAL fp32 module {psnr(h, s['ho']):.2f} dB")
    assert ph >= pe - 1.0, (ph, pe)                                              # the margins of test_gpu_qwen_text_encoder._parity
    assert ph >= 35.0, ph


@pytest.mark.parametrize("case", list(CASES))
def test_fp8_generate_logits_are_as_close_to_the_dequantised_fp32_module_as_eager_bf16(case):
    s = _run(case)
    r, e, h = s["r"], s["e"], s["h"]
    ph, pe = psnr(h, r), psnr(e, r)
    eh, ee = float((h - r).abs().max()), float((e - r).abs().max())
    toks = s["out"].sequences[0, s["L"]:]
    regret = float((r.max(dim=1).values - r.gather(1, toks[:, None])[:, 0]).max())
    print(f"fp8 generate {case}: HIP {ph:.2f} dB / max err {eh:.4f}, eager bf16 {pe:.2f} dB / max err {ee:.4f} against the dequantised fp32 "
          f"module; largest fp32 regret of a HIP token {regret:.4f}")
    assert ph >= pe - 1.0, (ph, pe)
    assert eh <= 2 * ee, (eh, ee)
    assert regret <= 4 * ee, (regret, ee)


@pytest.mark.parametrize("case", list(CASES))
def test_the_original_weights_are_at_least_10_db_further_away(case):
    """The control: had the kernels read bf16 weights by mistake, HIP would be as close to the ORIGINAL fp32 module as eager bf16 is to
    its reference.  On the references alone the quantisation sits 18 dB below that (38.1 against 56.6 dB for `text`, 34.6 against 53.4 dB
    for `text_gqa`)."""
    s = _run(case)
    po, pe = psnr(s["h"], s["o"]), psnr(s["e"], s["r"])
    print(f"fp8 generate {case}: HIP against the ORIGINAL fp32 module {po:.2f} dB, eager bf16 against its own reference {pe:.2f} dB")
    assert po <= pe - 10.0, (po, pe)


@pytest.mark.parametrize("case", list(CASES))
def test_fp8_generate_returns_the_prompt_and_the_argmax_of_its_own_logits(case):
    s = _run(case)
    seq, L = s["out"].sequences, s["L"]
    assert seq.dtype == torch.int64 and seq.shape == (1, L + NEW) and torch.equal(seq[:, :L], s["kw"]["input_ids"])
    assert len(s["out"].logits) == NEW and all(z.shape == (1, HQ.VOCAB) and z.dtype == torch.float32 for z in s["out"].logits)
    for k in range(NEW):
        assert int(seq[0, L + k]) == _first_argmax(s["h"][k]), k


@pytest.mark.parametrize("case", list(CASES))
def test_fp8_generate_is_deterministic_and_leaves_the_encoder_call_alone(case):
    s = _run(case)
    assert torch.equal(s["out"].sequences, s["out2"].sequences)
    assert all(torch.equal(a, b) for a, b in zip(s["out"].logits, s["out2"].logits))
    assert torch.equal(s["call0"], s["call1"])


def test_fp8_eos_cuts_after_its_first_occurrence_whatever_sync_every():
    s = _run("text")
    L, seq = s["L"], s["out"].sequences
    new = seq[0, L:].tolist()
    js = [j for j in range(2, NEW) if new[j] not in new[:j]]
    assert js, "no token that first occurs at a new index >= 2"
    j = js[len(js) // 2]
    for every in (1, 8):
        got = s["hip"].generate(**s["kw"], max_new_tokens=NEW, eos_token_id=new[j], sync_every=every)
        assert torch.equal(got, seq[:, :L + j + 1]), (j, every)


def test_a_warm_fp8_generate_dispatches_only_libregione_hip_kernels_and_the_fp8_gemv():
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
    n_w8, n_bf16 = sum("lm_gemv_w8_kernel" in n for n in names), sum("lm_gemv_kernel" in n for n in names)
    # 3 one-row steps x 2 layers x 4 projections on the fp8 kernel; lm_gemv_kernel appears as the 4 vocabulary picks only
    assert n_w8 == 3 * 2 * 4 and n_bf16 == 4, (n_w8, n_bf16)
    assert torch.equal(seq, s["out"].sequences[:, :s["L"] + 4])


def test_the_hosted_binding_adopts_in_fp8_when_the_pipeline_asks_for_it():
    import host_standins as HS
    from regione_amd import adapters
    m = HQ.tiny_qwen25vl().cuda()
    fired = []
    for layer in m.model.language_model.layers:
        layer.register_forward_hook(lambda mod, i, o: fired.append(type(mod).__name__))
    pipe = HQ.QwenImageEditPipeline(HS.stub_trunk("qwen"), m)
    pipe._regione_hip_text_weights = "fp8"
    kw = _inputs(1, ONE)
    image = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(5))
    with adapters._hip_qwen_text_encoder(pipe, torch.device("cuda")):
        enc = pipe.text_encoder
        assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.weights == "fp8" and enc.layers[0]["wqkv"].dtype == FP8
        pe, pm = pipe.encode_prompt(image=image, prompt="add a red hat", device=torch.device("cuda"))
        got = enc.generate(**kw, max_new_tokens=4, do_sample=False)
    assert pipe.text_encoder is m and fired == []
    assert pe.dtype == torch.bfloat16 and pe.shape[2] == 256 and bool(torch.isfinite(pe.float()).all()) and bool(pm.bool().all())
    assert got.shape == (1, 31 + 4) and torch.equal(got[:, :31], kw["input_ids"]) and int(got.max()) < HQ.VOCAB
    ref = QT.HipQwen25VLTextEncoder(m, weights="fp8")                            # the same adoption by hand: the same tokens
    assert torch.equal(ref.generate(**kw, max_new_tokens=4), got)
