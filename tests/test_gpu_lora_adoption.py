"""A host transformer with LoRA adapters loaded (PEFT layout, tests/host_lora.py on the tiny trunks of tests/host_trunks.py) goes on the
HIP engine: merged on the device at adoption (rgn_lora_merge_bf16 into the packed layouts), re-merged when the adapter state changes.

The numerical reference is the stand-in's OWN fp32 forward with the side path unmerged (base(x) + sum scaling * B(A(x))); the weight
checks go slot by slot through FluxTransformer2DModel.weight_slots against the fp64 merge of tests/lora_merge_model.py, so a wrong row
offset in w_kvq / w_kvqm / mod_w is caught; hot-swaps are compared bit for bit with a fresh adoption of a host in that state.  The by-name
refusals need no GPU: they happen before anything is allocated."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_lora as HL  # noqa: E402
import host_standins as HS  # noqa: E402
import lora_merge_model as M  # noqa: E402
from oracle import regione_oracle as O  # noqa: E402  (PSNR helper only)
from regione_amd import adapters as A, ops, synth  # noqa: E402

gpu = pytest.mark.gpu

# attention, feed-forward, proj_mlp, the AdaLN linears, the embedders (host names of the three families)
TARGETS = ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out", "net.0.proj", "net.2", "proj_mlp",
           "proj_out", "norm1.linear", "norm1_context.linear", "norm.linear", "img_mod.1", "txt_mod.1", "x_embedder", "img_in", "linear_1")
ADAPTERS = (("style", 4, 16.0, 1), ("steps", 12, 24.0, 2))          # name, rank, alpha, seed: scalings 4 and 2
CASES = [("flux", "FluxKontextPipeline"), ("step1x", "Step1XEditPipelineV1P2"), ("qwen", "QwenImageEditPipeline")]


def _lora_host(family, adapters=ADAPTERS):
    mod = HS.stub_trunk(family)
    for name, r, alpha, seed in adapters:
        hit = HL.inject(mod, TARGETS, r, alpha, name, seed=seed)
        assert any(h.endswith("to_q") for h in hit) and any(h.endswith(("x_embedder", "img_in")) for h in hit)
    return mod


def _pipe(cls, mod):
    pipe = type(cls, (), {"vae_scale_factor": 8})()
    pipe.transformer, pipe.scheduler = mod, None
    return pipe


def _tensors(eng):
    """{(slot owner index, attribute): tensor} of every engine weight tensor the slot table names."""
    out, owners = {}, {}
    for name, (obj, attr, lo, hi) in eng.transformer.weight_slots().items():
        if hasattr(obj, attr):
            out[(owners.setdefault(id(obj), len(owners)), attr)] = getattr(obj, attr)
    return out


def _assert_same_weights(a, b):
    ta, tb = _tensors(a), _tensors(b)
    assert ta.keys() == tb.keys()
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and torch.equal(ta[k].view(torch.uint8) if ta[k].dtype == ops.FP8 else ta[k],
                                                          tb[k].view(torch.uint8) if tb[k].dtype == ops.FP8 else tb[k]), k
        sa, sb = getattr(ta[k], "_rgn_scale", None), getattr(tb[k], "_rgn_scale", None)
        assert (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb)), k
    assert torch.equal(a.transformer.mod_b, b.transformer.mod_b)


GUIDANCE = 2.0
TIMESTEPS = (1000.0, 500.0, 125.0)
# The stock pipelines hand the trunk `timestep / 1000` in bf16 and the trunk multiplies by 1000 again before the sinusoids: in bf16 that
# product is rounded, in an fp32 forward it is not, and at arguments of hundreds of radians the two embeddings are unrelated.  The fp32
# reference is therefore taken at timesteps (and a guidance) for which t / 1000 and t are both exact in bf16, so that both precisions feed the
# same angles and what is compared is the trunk.


def _engine_forward(family, eng, lat, img, prompt, y, h, w, t):
    tr = eng.transformer
    x = torch.cat([lat, img], dim=1).cuda()
    T = prompt.shape[1]
    ts = t.expand(1).to(torch.bfloat16) / 1000
    if family == "flux":
        return tr(hidden_states=x, encoder_hidden_states=prompt.cuda(), pooled_projections=y.cuda(), timestep=ts,
                  img_ids=synth.flux_latent_ids(h, w), txt_ids=torch.zeros(T, 3), guidance=torch.full([1], GUIDANCE), return_dict=False)[0]
    if family == "step1x":
        tr.set_vec((y.cuda(),))
        return tr(hidden_states=x, encoder_hidden_states=prompt.cuda(), prompt_embeds_mask=None, timestep=ts, guidance=None,
                  img_ids=synth.flux_latent_ids(h, w), txt_ids=torch.zeros(T, 3), return_dict=False)[0]
    return tr(hidden_states=x, encoder_hidden_states=prompt.cuda(), timestep=ts, img_shapes=[[(1, h, w), (1, h, w)]],
              latent_ids=torch.arange(2 * h * w), return_dict=False)[0]


def _host_forward_fp32(family, mod, lat, img, prompt, y, h, w, t):
    """The host trunk's own forward in fp32 (the module's bf16 weights and the bf16 inputs, converted exactly)."""
    x = torch.cat([lat, img], dim=1).float()
    T = prompt.shape[1]
    ts = (t.expand(1).to(torch.bfloat16) / 1000).float()
    prompt, y = prompt.float(), y.float()
    with torch.no_grad():
        if family == "flux":
            return mod(hidden_states=x, encoder_hidden_states=prompt, pooled_projections=y, timestep=ts,
                       img_ids=synth.flux_latent_ids(h, w), txt_ids=torch.zeros(T, 3), guidance=torch.full([1], GUIDANCE), return_dict=False)[0]
        if family == "step1x":
            mod.set_vec(prompt, y)
            return mod(hidden_states=x, encoder_hidden_states=prompt, prompt_embeds_mask=None, timestep=ts,
                       img_ids=synth.flux_latent_ids(h, w), txt_ids=torch.zeros(T, 3), return_dict=False)[0]
        return mod(hidden_states=x, encoder_hidden_states=prompt, timestep=ts, img_shapes=[[(1, h, w), (1, h, w)]],
                   txt_seq_lens=[T], return_dict=False)[0]


@gpu
@pytest.mark.parametrize("family,cls", CASES)
def test_adopted_engine_with_lora_matches_the_hosts_unmerged_fp32_forward(family, cls):
    """adopt_engine succeeds on a host with two adapters (ranks 4 and 12) on attention, feed-forward, proj_mlp, the AdaLN linears and the
    embedders, and the engine's forward meets the 40 dB bar of tests/test_adapters.py against the host's own side-path forward - while
    the same host WITHOUT the adapters is below 30 dB from it, so an engine that ignored them could not pass."""
    mod = _lora_host(family)
    eng = A.adopt_engine(_pipe(cls, mod))
    cfg = eng.transformer.cfg_model
    h = w = 16
    lat, img, prompt, y = synth.make_edit_inputs(h, w, 32, cfg, seed=9, dtype=torch.bfloat16)
    ref_mod = _lora_host(family).float()                    # the same module tree again (seeded), weights converted exactly
    for t in map(torch.tensor, TIMESTEPS):
        HL.disable(ref_mod, False)
        ref = _host_forward_fp32(family, ref_mod, lat, img, prompt, y, h, w, t)
        HL.disable(ref_mod, True)
        plain = _host_forward_fp32(family, ref_mod, lat, img, prompt, y, h, w, t)
        apart = O.psnr(plain, ref)
        assert apart < 30.0, (cls, float(t), apart)                                  # CPU side: the pair discriminates
        got = _engine_forward(family, eng, lat, img, prompt, y, h, w, t).cpu()
        p = O.psnr(got.float(), ref)
        print(f"[lora adoption] {cls} t={float(t):.0f}: {p:.1f} dB vs the host's unmerged fp32 forward ({apart:.1f} dB without the adapters)")
        assert torch.isfinite(got.float()).all() and p >= 40.0, (cls, float(t), p)


def _check_slots(eng, pipe, family, scale=1.0):
    sd, names, lora = A._lora_plan(pipe, family, ("connector.",))
    host_key = {A.map_key(s, family): k for k, s in names.items()}
    n_lora = 0
    for name, (obj, attr, lo, hi) in eng.transformer.weight_slots().items():
        if name not in host_key:
            continue
        t = getattr(obj, attr)
        rows = (t[lo:hi] if hi is not None else t).float().cpu().double().numpy()
        W = sd[host_key[name]].detach().float().double().numpy()
        m = lora.get(name)
        terms = [] if m is None else [(m.lora_A[a].weight.detach().float().numpy(), m.lora_B[a].weight.detach().float().numpy(),
                                       float(m.scaling[a]) * scale) for a in A._lora_active(m)]
        assert rows.shape == W.shape, name
        if not terms:
            assert np.array_equal(rows, W), name
            continue
        n_lora += 1
        ok = M.accepted(rows, W, terms)
        assert ok.all(), (name, attr, lo, int((~ok).sum()))
        assert not np.array_equal(rows, W), name
    return n_lora


@gpu
@pytest.mark.parametrize("family,cls", CASES)
def test_every_engine_weight_lies_within_the_kernel_bound_of_the_fp64_merge_slot_by_slot(family, cls):
    mod = _lora_host(family)
    pipe = _pipe(cls, mod)
    eng = A.adopt_engine(pipe)
    assert _check_slots(eng, pipe, family) >= 20


@gpu
def test_hot_swap_equals_a_fresh_adoption_and_an_unchanged_fingerprint_launches_nothing():
    family, cls = "flux", "FluxKontextPipeline"
    mod = _lora_host(family)
    pipe = _pipe(cls, mod)
    eng = A.adopt_engine(pipe)
    # unchanged: nothing happens - same tensors, same versions
    before = {k: (t.data_ptr(), t._version) for k, t in _tensors(eng).items()}
    assert A.lora_sync(pipe, eng) is False
    assert {k: (t.data_ptr(), t._version) for k, t in _tensors(eng).items()} == before
    # set_adapters weight
    HL.set_scale(mod, "style", 0.5)
    assert A.lora_sync(pipe, eng) is True and A.lora_sync(pipe, eng) is False
    _assert_same_weights(eng, A.adopt_engine(pipe))
    assert _check_slots(eng, pipe, family) >= 20
    # one adapter deleted
    HL.delete(mod, "style")
    assert A.lora_sync(pipe, eng) is True
    _assert_same_weights(eng, A.adopt_engine(pipe))
    # disable_lora: the adoption of the same host without any adapter
    HL.disable(mod, True)
    assert A.lora_sync(pipe, eng) is True
    _assert_same_weights(eng, A.adopt_engine(_pipe(cls, HS.stub_trunk(family))))
    # and back on; then unloaded altogether (the wrappers are gone)
    HL.disable(mod, False)
    assert A.lora_sync(pipe, eng) is True
    _assert_same_weights(eng, A.adopt_engine(pipe))
    HL.unload(mod)
    assert A.lora_sync(pipe, eng) is True and A.lora_sync(pipe, eng) is False
    _assert_same_weights(eng, A.adopt_engine(_pipe(cls, HS.stub_trunk(family))))
    # the host's tensors were never written
    ref = HS.stub_trunk(family).state_dict()
    assert all(torch.equal(v, ref[k]) for k, v in mod.state_dict().items())


@gpu
def test_adapters_loaded_after_the_adoption_are_merged_at_the_next_attach():
    family, cls = "qwen", "QwenImageEditPipeline"
    mod = HS.stub_trunk(family)
    pipe = _pipe(cls, mod)
    eng = A.attach(pipe)
    for name, r, alpha, seed in ADAPTERS:
        HL.inject(mod, TARGETS, r, alpha, name, seed=seed)
    assert A.attach(pipe) is eng
    _assert_same_weights(eng, A.adopt_engine(pipe))
    assert _check_slots(eng, pipe, family) >= 20


@gpu
@pytest.mark.parametrize("family,cls", [("flux", "FluxKontextPipeline")])
def test_already_merged_host_is_adopted_as_is(family, cls):
    mod = _lora_host(family)
    HL.merge(mod)                                               # merged_adapters set, base weights pre-merged on the CPU
    plain = _lora_host(family)
    HL.merge(plain)
    HL.unload(plain)                                            # a plain host with those weights
    assert not HL.layers(plain) and HL.layers(mod)
    _assert_same_weights(A.adopt_engine(_pipe(cls, mod)), A.adopt_engine(_pipe(cls, plain)))


@gpu
def test_fp8_trunk_quantises_the_merged_weights_and_hot_swaps_like_a_fresh_adoption():
    family, cls = "flux", "FluxKontextPipeline"
    mod = _lora_host(family)
    pipe = _pipe(cls, mod)
    eng = A.adopt_engine(pipe)
    merged = {k: t.clone() for k, t in _tensors(eng).items()}                        # the kernel-merged bf16 weights
    eng.transformer.quantize_fp8_()
    n8 = 0
    for k, t in _tensors(eng).items():
        if t.dtype == ops.FP8:
            q = ops.quantize_w8(merged[k])
            assert torch.equal(t.view(torch.uint8), q.view(torch.uint8)) and torch.equal(t._rgn_scale, q._rgn_scale), k
            n8 += 1
        else:
            assert torch.equal(t, merged[k]), k
    assert n8 >= 10
    HL.set_scale(mod, "steps", -0.75)
    assert A.lora_sync(pipe, eng) is True
    fresh = A.adopt_engine(pipe)
    fresh.transformer.quantize_fp8_()
    _assert_same_weights(eng, fresh)


# ---- hosted calls -------------------------------------------------------------------------------------------------------------------------
def _picture(h=256, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(1, 3, h, w, generator=g)
    p[:, :, h // 4: h // 4 + h // 3, w // 3: w // 3 + w // 3] = 0.0
    return p


def _call(pipe, **kw):
    return pipe(image=_picture(), prompt="make the square red", generator=torch.Generator().manual_seed(1), output_type="latent",
                guidance_scale=2.5, preferred_resolutions=[(256, 256)], **kw).images


@gpu
def test_hosted_pipe_call_with_a_lora_loaded_through_the_helper_and_the_call_time_scale():
    """The user's path: load a LoRA, RegionEHelper(pipe).enable(), pipe(image=, prompt=).  `joint_attention_kwargs={"scale": s}` equals an
    adoption with every scaling multiplied by s, for that call only; any other key stays refused."""
    from regione_amd import RegionEHelper
    pipe = HS.FluxKontextPipeline(_lora_host("flux"))
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()                                              # KeyError on a tree that does not know the PEFT layout
    eng = pipe._regione_engine
    first = _call(pipe)
    assert torch.isfinite(first.float()).all()
    plain = HS.FluxKontextPipeline(HS.stub_trunk("flux"))
    h2 = RegionEHelper(plain)
    h2.set_params(threshold=0.5)
    h2.enable()
    assert not torch.equal(_call(plain), first)                 # the adapters change the edit
    w1 = {k: t.clone() for k, t in _tensors(eng).items()}
    scaled = _call(pipe, joint_attention_kwargs={"scale": 0.5})
    half = _lora_host("flux")
    for name, *_ in ADAPTERS:
        HL.set_scale(half, name, 0.5)
    _assert_same_weights(eng, A.adopt_engine(_pipe("FluxKontextPipeline", half)))
    assert not torch.equal(scaled, first)
    again = _call(pipe, joint_attention_kwargs=None)
    assert torch.equal(again, first)
    assert all(torch.equal(t, w1[k]) for k, t in _tensors(eng).items())
    with pytest.raises(NotImplementedError, match="joint_attention_kwargs"):
        _call(pipe, joint_attention_kwargs={"scale": 0.5, "ip_adapter_masks": 1})
    helper.disable()
    ref = _lora_host("flux").state_dict()
    assert all(torch.equal(v, ref[k]) for k, v in pipe.transformer.state_dict().items())          # the engine never writes to host tensors


# ---- declined by name, before anything is allocated or launched (no GPU needed) -------------------------------------------------------------
def _declined(mod, match, cls="FluxKontextPipeline"):
    with pytest.raises(NotImplementedError, match=match):
        A.adopt_engine(_pipe(cls, mod))


def _one_layer(targets=("to_q",), rank=4):
    mod = HS.stub_trunk("flux")
    hit = HL.inject(mod, targets, rank, 8.0, "a", seed=1)
    return mod, HL.layers(mod)[hit[0]]


def test_dora_is_declined():
    mod, layer = _one_layer()
    layer.use_dora["a"] = True
    _declined(mod, "DoRA")
    mod, layer = _one_layer()
    layer.lora_magnitude_vector["a"] = torch.nn.Linear(4, 4, bias=False)
    _declined(mod, "DoRA")


def test_lora_bias_is_declined():
    mod, layer = _one_layer()
    layer.lora_B["a"] = torch.nn.Linear(4, layer.base_layer.weight.shape[0], bias=True).to(torch.bfloat16)
    _declined(mod, "lora_bias")


def test_lora_embedding_is_declined():
    mod, layer = _one_layer()
    layer.lora_embedding_A["a"] = torch.nn.Parameter(torch.zeros(4, 8))
    _declined(mod, "lora_embedding_")


def test_lora_on_a_module_that_is_not_a_linear_of_the_layout_is_declined():
    mod = HS.stub_trunk("flux")
    hit = HL.inject(mod, ("norm_q",), 4, 8.0, "a")              # an RMSNorm weight
    assert hit
    _declined(mod, "not a Linear the trunk layout knows")
    mod = HS.stub_trunk("flux")
    mod.extra_conv = torch.nn.Conv2d(4, 4, 1)
    HL.inject(mod, ("extra_conv",), 4, 8.0, "a")
    _declined(mod, "Conv2d, not a Linear the trunk layout knows")
    mod = HS.stub_trunk("flux")
    mod.extra_linear = torch.nn.Linear(8, 8)                    # a Linear, but not one of the trunk layout
    HL.inject(mod, ("extra_linear",), 4, 8.0, "a")
    _declined(mod, "extra_linear, not a Linear the trunk layout knows")


@pytest.mark.parametrize("prefix", ["lokr_w1", "hada_w1_a", "ia3_l"])
def test_other_peft_tuners_are_declined(prefix):
    mod = HS.stub_trunk("flux")
    mod.transformer_blocks[0].attn.to_q.register_parameter(prefix, torch.nn.Parameter(torch.zeros(2, 2)))
    _declined(mod, "non-LoRA PEFT tuner")


def test_rank_above_1024_and_more_than_8_active_adapters_are_declined():
    mod, _ = _one_layer(("x_embedder",), rank=1025)
    _declined(mod, "rank 1025 > 1024")
    mod = HS.stub_trunk("flux")
    for i in range(9):
        HL.inject(mod, ("x_embedder",), 2, 2.0, f"a{i}", seed=i)
    _declined(mod, "9 active adapters")
    HL.delete(mod, "a8")                                        # eight are fine as far as the checks go: the next refusal is not about LoRA
    A._lora_checked(mod, mod.state_dict(), ("connector.",))


def test_adapter_shapes_that_do_not_fit_the_base_weight_are_declined():
    mod, layer = _one_layer()
    layer.lora_A["a"] = torch.nn.Linear(layer.base_layer.weight.shape[1] + 8, 4, bias=False)
    _declined(mod, "do not fit the base weight")


def test_a_non_peft_unknown_name_still_raises_the_layout_keyerror():
    mod, _ = _one_layer()
    mod.controlnet_x_embedder = torch.nn.Linear(4, 4)
    with pytest.raises(KeyError, match="unexpected"):
        A.adopt_engine(_pipe("FluxKontextPipeline", mod))


def test_fingerprint_uses_host_side_state_only_and_sees_every_change():
    mod = _lora_host("flux")
    fp = lambda s=1.0: A._lora_fingerprint(A.lora_layers(mod), s)
    base = fp()
    assert fp() == base and len(base) >= 20 and fp(0.5) != base
    HL.set_scale(mod, "style", 0.25)
    a = fp()
    assert a != base
    HL.disable(mod, True)
    b = fp()
    assert b != a
    HL.disable(mod, False)
    assert fp() == a
    layer = next(iter(HL.layers(mod).values()))
    with torch.no_grad():
        layer.lora_A["style"].weight.mul_(2.0)                  # an in-place edit: the version counter moves
    assert fp() != a
    HL.delete(mod, "steps")
    assert fp() != a


@pytest.mark.parametrize("key", ["joint_attention_kwargs", "attention_kwargs"])
def test_call_time_scale_is_taken_out_of_the_refused_arguments_and_nothing_else_is(key):
    """`{key: {"scale": s}}` is consumed (FLUX / Step1X: joint_attention_kwargs, Qwen: attention_kwargs); any other content stays in the
    dict that `_refuse_unused` then refuses, None stays ignorable."""
    eng = type("E", (), {"transformer": type("T", (), {})()})()          # an engine that was not adopted from a host: lora_sync returns at once
    host = type("H", (), {"transformer": HS.stub_trunk("flux")})()
    assert A._lora_call(host, eng, {key: {"scale": 0.5}, "other": 1}, key) == {"other": 1}
    for kept in ({key: {"scale": 0.5, "tag": "cond"}}, {key: {"scale": "0.5"}}, {key: {"scale": True}}, {key: None}, {key: {}}):
        assert A._lora_call(host, eng, dict(kept), key) == kept
    with pytest.raises(NotImplementedError, match=key):
        A._refuse_unused("call", A._lora_call(host, eng, {key: {"scale": 0.5, "tag": "cond"}}, key))
    A._refuse_unused("call", A._lora_call(host, eng, {key: {"scale": 0.5}}, key))
    A._refuse_unused("call", A._lora_call(host, eng, {key: None}, key))


def test_stand_in_names_match_a_real_peft_injection():
    peft = pytest.importorskip("peft")
    net = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))
    real = peft.inject_adapter_in_model(peft.LoraConfig(r=2, lora_alpha=4, target_modules=["0", "1"]), copy.deepcopy(net), adapter_name="a")
    HL.inject(net, ("0", "1"), 2, 4.0, "a")
    assert set(real.state_dict()) == set(net.state_dict())
    rl, sl = real[0], net[0]
    for attr in ("base_layer", "lora_A", "lora_B", "scaling", "active_adapters", "disable_adapters", "merged_adapters", "use_dora",
                 "lora_embedding_A", "lora_magnitude_vector"):
        assert hasattr(rl, attr) and hasattr(sl, attr), attr
    assert rl.scaling["a"] == sl.scaling["a"] and list(rl.active_adapters) == list(sl.active_adapters)
