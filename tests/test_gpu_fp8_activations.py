"""-m gpu: the trunk with fp8 activations, `FluxTransformer2DModel.quantize_fp8_(activations=True)` (tiny FLUX, Step1X-v1p2, Qwen trunks).

  a. activations=False is the method as it was: a 28-step RegionE edit (full steps, the partition step, region steps) on a trunk
     quantised with `quantize_fp8_(activations=False)` gives bit for bit the latents of the same edit on `quantize_fp8_()`, in one
     process, and allocates no fp8 activation buffer;
  b. activations=True: under torch.profiler (the mechanism of tests/test_gpu_no_eager_kernels.py) every GEMM with the fused Q/K/V or the
     GELU epilogue - the launches that read the LN-modulate output - ran the fp8 x fp8 kernel variant (last template argument 10), no
     fp8-weight kernel of the widening variants (8 / 9) ran any epilogue but the gated residual (w_out, ff_w2, w_po), the LN-modulate
     launches of the block bodies are the `_a8` kernels, and no eager kernel ran;
  c. one double + one single block: PSNR of the A8 engine against the oracle's fp32 block functions with `_lin` patched HERE (dequantised
     weights; for the five projections fed by the normed rows also the input fake-quantised per row by the CPU quantiser model; the
     Linears outside the blocks - embedders, AdaLN tables, proj_out - in bf16 as the engine runs them) stays
     within 3 dB of the yardstick - the fp8-weight engine (activations=False, the code as it was) against the same oracle with
     dequantised weights only.  The only new error mechanism is a code flip where the device's bf16 row differs from the oracle's by a
     rounding; if that more than doubled the error power, flips would not be rare and the quantiser would disagree with its model.
     Measured on an MI355X: 27.55 dB yardstick, 27.52 dB with fp8 activations - both set by the oracle's fp32 embedders, not by the
     blocks.  The test also PRINTS the pair with the conditioning path matched to the engine's bf16: 57.25 dB against 53.67 dB, i.e.
     3.6 dB apart (52.23 dB against a model without the activation quantiser).  There the flips show: the engine's bf16 row follows the
     eager rounding sequence of four bf16 roundings, the fp32 oracle rounds once, so rows differ by a bf16 ulp in many elements and one
     in ~30 of those lands on the other side of an e4m3fn boundary (a full 2^-3 step).  The quantiser itself is bit-exact on equal bf16
     rows (tests/test_gpu_quantize_rows.py); the figures are in profiles/r23_fp8_activations_notes.md;
  d. the 28-step edit runs, a repeated run is bit-identical, `helper.disable()` restores the pipeline (the full-token loop runs, again
     without eager kernels)."""
import re

import pytest
import torch
import torch.nn.functional as F

import gemm_a8_model as A
import gemm_model as G
from oracle import regione_oracle as O
from regione_amd import RegionEHelper, ops, synth
from regione_amd.harness import flux as H
from test_gpu_no_eager_kernels import _build, _foreign, _gpu_activity_names

pytestmark = pytest.mark.gpu
FAMILIES = ["flux", "step1x_v1p2", "qwen"]
KERNEL = re.compile(r"gemm_bf16_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>")


def _edit(pipe, kw, **more):
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    out = pipe(**kw, **more)[0]
    torch.cuda.synchronize()
    return helper, out


@pytest.mark.parametrize("family", FAMILIES)
def test_activations_false_is_the_fp8_weight_path_bit_for_bit(family, golden):
    outs = []
    for kwargs in ({}, dict(activations=False)):
        pipe, kw = _build(family, golden)
        pipe.transformer.quantize_fp8_(**kwargs)
        _, out = _edit(pipe, kw)
        M = pipe._regione_manager
        assert 0 < int(M.edited_ids.shape[1]) < 256, "the edit must contain region steps"
        assert not pipe.transformer.ws.a8 and not hasattr(pipe.transformer.ws, "nrm8")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("family", FAMILIES)
def test_every_gemm_fed_by_the_normed_rows_runs_fp8_x_fp8_and_the_edit_repeats(family, golden):
    pipe, kw = _build(family, golden)
    pipe.transformer.quantize_fp8_(activations=True)
    assert pipe.transformer.ws.a8
    helper, warm = _edit(pipe, kw)                                       # warm: workspaces, rotary tables, cache slabs
    M = pipe._regione_manager
    assert 0 < int(M.edited_ids.shape[1]) < 256, "the edit must contain region steps"
    out, names = _gpu_activity_names(lambda: pipe(trace=None, **kw)[0])
    assert torch.isfinite(out.float()).all() and torch.equal(out, warm), "a repeated run must be bit-identical"
    assert _foreign(names) == [], _foreign(names)
    gemms = [tuple(int(x) for x in m.groups()) for m in map(KERNEL.search, names) if m]
    fed = [g for g in gemms if g[0] in (1, 3)]                          # RGN_EPI_GELU / RGN_EPI_QKV: Q/K/V(+MLP) and first feed-forward GEMMs
    assert len(fed) > 20 and all(g[6] == 10 for g in fed), sorted({g for g in fed if g[6] != 10})
    # (g[5] == 1: the K pieces of a split launch carry no epilogue - theirs is the reduce pass's; fp8-activation launches are never split)
    assert all(g[0] == 2 for g in gemms if g[6] in (8, 9) and g[5] != 1), sorted({g for g in gemms if g[6] in (8, 9) and g[0] != 2})
    assert not any(g[5] != 0 for g in gemms if g[6] == 10)
    assert any(g[6] in (8, 9) for g in gemms) and any(g[6] == 10 and g[0] == 3 for g in gemms)
    ln8 = sum(1 for n in names if "ln_modulate" in n and "a8" in n)
    ln16 = sum(1 for n in names if "ln_modulate" in n and "a8" not in n)
    assert ln8 > ln16 > 0, (ln8, ln16)                                    # bf16 rows only for norm_out: one launch per forward and branch
    # the full-token loop on the same engine
    helper.disable()
    pipe(**kw)
    out2, names = _gpu_activity_names(lambda: pipe(**kw)[0])
    assert _foreign(names) == [] and torch.isfinite(out2.float()).all()
    gemms = [tuple(int(x) for x in m.groups()) for m in map(KERNEL.search, names) if m]
    assert all(g[6] == 10 for g in gemms if g[0] in (1, 3)) and all(g[0] == 2 for g in gemms if g[6] in (8, 9) and g[5] != 1)


def _is_block_weight(name):
    return name.startswith(("transformer_blocks.", "single_transformer_blocks.")) and not synth.is_modulation(name + ".weight")


def _reads_normed_rows(name):
    return name.rsplit(".attn.", 1)[-1] in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj") or name.endswith((".net.0.proj", ".proj_mlp"))


def _patched_lin(fake_quantise_inputs, outside_in_bf16=False):
    tab = G.e4m3fn_table().float()
    cache = {}

    def lin(w, name, x):
        W = w[name + ".weight"]
        if outside_in_bf16 and not _is_block_weight(name):
            # embedders, AdaLN tables, norm_out / proj_out: bf16 Linears as the engine runs them, so that the comparison is about the blocks
            b = w.get(name + ".bias")
            y = F.linear(x.to(torch.bfloat16), W.to(torch.bfloat16), b.to(torch.bfloat16) if b is not None else None)
            return y if x.dtype == torch.bfloat16 else y.float()
        if _is_block_weight(name):
            if name not in cache:
                q = ops.quantize_w8(W.to(torch.bfloat16))                # per output channel, as quantize_fp8_ stores it
                cache[name] = tab[q.view(torch.uint8).long()] * q._rgn_scale[:, None]
            W = cache[name]
            if fake_quantise_inputs and _reads_normed_rows(name):
                codes, s = A.quantize_rows(x.reshape(-1, x.shape[-1]).to(torch.bfloat16))
                x = (tab[codes.long()] * s[:, None]).reshape(x.shape)
        return F.linear(x, W, w.get(name + ".bias"))
    return lin


def test_one_double_and_one_single_block_stay_within_3_db_of_the_fp8_weight_path(golden, monkeypatch):
    g = golden("toy_bf16")
    h, w, T = g["h"], g["w"], g["T"]
    toy = dict(synth.TOY, n_double=1, n_single=1)
    cfg = synth.FluxConfig(**toy)
    wts = synth.make_flux_weights(cfg, seed=42, dtype=torch.bfloat16, w_std=g["w_std"])
    lat, _, prompt, pooled = synth.make_edit_inputs(h, w, T, cfg, seed=g["seed"], dtype=torch.bfloat16)
    img, ids = g["image_latents"], synth.flux_latent_ids(h, w)
    st = O.RegionState()
    st.set_parameters(28, 6, 2, "16", 0.5, 0.04, True)
    st.refresh(img, ids, T, h, w)
    _, ts = O.flow_match_schedule(28, h * w)
    x = torch.cat([lat, img], 1)
    tstep = ts[0].expand(1).to(torch.bfloat16) / 1000
    guidance = torch.full([1], 2.5)
    w32 = {k: v.float() for k, v in wts.items()}

    embed = O.time_text_embed

    def oracle(fake_quantise_inputs, matched=False):
        """matched: the Linears OUTSIDE the blocks and the conditioning vector in bf16, as the engine forms them - a measurement beside
        the check, which uses the oracle in fp32 throughout with `_lin` patched for the quantised formats only."""
        monkeypatch.setattr(O, "_lin", _patched_lin(fake_quantise_inputs, matched))
        monkeypatch.setattr(O, "time_text_embed", embed if not matched else
                            lambda w_, t_, g_, p_, scale=1.0: embed(w_, t_.to(torch.bfloat16), g_.to(torch.bfloat16), p_.to(torch.bfloat16), scale).float())
        with torch.no_grad():
            return O.transformer_forward(w32, O.FluxCfg(**toy), st, [O.KVCache() for _ in range(cfg.n_layers)], x.float(), prompt.float(),
                                         pooled.float(), tstep.float(), ids, torch.zeros(T, 3), guidance)

    def engine(activations):
        tr = H.FluxTransformer2DModel(cfg, "cuda").load_state_dict(wts).quantize_fp8_(activations=activations)
        return tr(hidden_states=x.cuda(), timestep=tstep, guidance=guidance, pooled_projections=pooled.cuda(), encoder_hidden_states=prompt.cuda(),
                  txt_ids=torch.zeros(T, 3), img_ids=ids, return_dict=False)[0].cpu()
    e_w8, e_a8 = engine(False), engine(True)
    yard = O.psnr(e_w8, oracle(False))
    a8 = O.psnr(e_a8, oracle(True))
    print(f"PSNR fp8-weight engine vs oracle(dequantised weights) {yard:.2f} dB; A8 engine vs oracle(+ fake-quantised inputs) {a8:.2f} dB")
    # beside the check: the same two figures with everything outside the blocks matched to the engine's bf16 (the fp32 embedders alone
    # cost ~30 dB and hide the blocks), and the A8 engine against the oracle that does not model the activation quantiser at all
    m_yard, m_a8, m_cross = O.psnr(e_w8, oracle(False, True)), O.psnr(e_a8, oracle(True, True)), O.psnr(e_a8, oracle(False, True))
    print(f"matched conditioning path: fp8-weight engine {m_yard:.2f} dB; A8 engine vs its model {m_a8:.2f} dB; A8 engine vs the model "
          f"without the activation quantiser {m_cross:.2f} dB")
    assert a8 >= yard - 3.0, (a8, yard)
