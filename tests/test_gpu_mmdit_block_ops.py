"""`regione_mi.mmdit_double_block_` / `mmdit_single_block_` (rgn_mmdit_*_block, csrc/block.hip) on the GPU.

The measure is the Python block sequence of the same commit on the same inputs (`harness.flux.BLOCK_OPS = False`), which the existing
suite pins to the reference fixtures.  The op makes the same launches with the same arguments, so the bar is `torch.equal` on the
residual stream `x`, the K slab and the V^T slab - no tolerance anywhere in this file."""
import functools

import pytest
import torch

from regione_amd import RegionEHelper, _lib, ops, synth
from regione_amd import torch_ops as TO
from regione_amd.harness import flux as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0.4375             # exact in bf16; what cache rows a step must not touch hold


class _Proc(H.FluxAttnProcessor):
    """A processor whose K / V destination the test chooses; it keeps FluxAttnProcessor.__call__, like the RegionE processors."""

    def __init__(self, single, target):
        super().__init__(single)
        self.target = target

    def kv_target(self, attn, ctx):
        return self.target


@functools.lru_cache(maxsize=None)
def _model(heads, fp8):
    cfg = synth.FluxConfig(n_double=1, n_single=2, heads=heads, head_dim=128, joint_dim=256, pooled_dim=64)   # d = 128 heads, d_ff = 4 d
    wts = synth.make_flux_weights(cfg, seed=11, dtype=torch.bfloat16, w_std=0.05)
    m = H.FluxTransformer2DModel(cfg, DEV).load_state_dict(wts)
    if fp8:
        m.quantize_fp8_()
    return m


def _block(m, single):
    b = m.single_transformer_blocks[0] if single else m.transformer_blocks[0]       # neither is the trunk's last block
    assert not getattr(b, "is_last", False)
    return b


@functools.lru_cache(maxsize=None)
def _inputs(heads, T, M, skv):
    """Seeded x rows, AdaLN table, rotary tables of `skv` joint rows - computed once, shared, never written."""
    m = _model(heads, False)
    d = m.cfg_model.d
    g = torch.Generator(device=DEV).manual_seed(1000 * heads + T + M)
    x0 = torch.randn(T + M, d, generator=g, device=DEV).bfloat16()
    vec = (0.1 * torch.randn(1, m.mod_total, generator=g, device=DEV)).bfloat16()
    assert skv - T == 512                                              # [text ; 256 noise tokens ; 256 condition tokens] of a 16 x 16 grid
    ids = torch.cat((torch.zeros(T, 3), synth.flux_latent_ids(16, 16)))
    cos, sin = m.pos_embed(ids, DEV)
    return x0, vec, (cos.contiguous(), sin.contiguous())


def _slabs(d, skv, fill):
    pad = ops.padded(skv)
    return (torch.full((pad, d), fill, dtype=torch.bfloat16, device=DEV), torch.full((d, pad), fill, dtype=torch.bfloat16, device=DEV))


def _ctx(m, T, M, vec, skv):
    m.ws.ensure(T + M, skv)
    ctx = H.FwdCtx(m.ws, T, M, H.Modulation(vec, m.cfg_model.d))
    ctx.rowbands = False
    return ctx


def _python_block(m, single, ctx, x0, target, rope_q):
    """The launch-by-launch sequence of the harness with the K / V destination `target`; returns x."""
    assert H.BLOCK_OPS is False
    blk = _block(m, single)
    R = ctx.T + ctx.M
    m.ws.x[:R].copy_(x0)
    old = blk.attn.processor
    blk.attn.set_processor(_Proc(single, target))
    try:
        blk(hidden_states=m.ws.x[ctx.T:R], encoder_hidden_states=m.ws.x[:ctx.T], temb=ctx, image_rotary_emb=rope_q)
    finally:
        blk.attn.set_processor(old)
    torch.cuda.synchronize()
    return m.ws.x[:R].clone()


def _op_args(m, single, ctx, target, rope_q):
    blk = _block(m, single)
    a, d, vec = blk.attn, m.cfg_model.d, ctx.mods.vec[0]
    k_slab, vt_slab, kv_rows, skv, rope_k = target
    rope_k = rope_k if rope_k is not None else rope_q
    if single:
        ada = dict(adaln=vec[blk.mo:blk.mo + 3 * d])
        w, b, n = [a.w_kvqm, blk.w_po], [a.b_kvqm, blk.b_po], [a.norm_q, a.norm_k]
    else:
        ada = dict(adaln_img=vec[blk.mo_img:blk.mo_img + 6 * d], adaln_txt=vec[blk.mo_ctx:blk.mo_ctx + 6 * d])
        w = [a.w_kvq, a.w_add_kvq, a.w_out, a.w_add_out, blk.ff_w1, blk.ffc_w1, blk.ff_w2, blk.ffc_w2]
        b = [a.b_kvq, a.b_add_kvq, a.b_out, a.b_add_out, blk.ff_b1, blk.ffc_b1, blk.ff_b2, blk.ffc_b2]
        n = [a.norm_q, a.norm_k, a.norm_added_q, a.norm_added_k]
    return dict(x=m.ws.x, nrm=m.ws.nrm, wide=m.ws.wide, **ada, weights=w, biases=b, norms=n, cos_q=rope_q[0], sin_q=rope_q[1], cos_k=rope_k[0],
                sin_k=rope_k[1], kv_rows=kv_rows, k_cache=k_slab, vt_cache=vt_slab, T=ctx.T, M=ctx.M, heads=a.heads, skv=skv,
                score_bound=a.score_bound(), rowbands=False)


def _call(single, args):
    fn = TO.R.mmdit_single_block_ if single else TO.R.mmdit_double_block_
    fn(*args.values())                                 # the dict is in schema order (minus `scales`, which TO.R fills in)


def _op_block(m, single, ctx, x0, target, rope_q, **change):
    R = ctx.T + ctx.M
    m.ws.x[:R].copy_(x0)
    args = _op_args(m, single, ctx, target, rope_q)
    args.update(change)
    _call(single, args)
    if args["rowbands"]:
        ops.rowband_join()                             # the caller joins at the end of the chain
    torch.cuda.synchronize()
    return m.ws.x[:R].clone()


def _region_rows(T):
    ids = torch.randperm(256, generator=torch.Generator().manual_seed(5))[:100].sort().values          # K_e = 100 of a 16 x 16 grid
    return torch.cat((torch.arange(T), T + ids)).to(DEV)


def _compare(m, single, T, case):
    d = m.cfg_model.d
    heads = m.cfg_model.heads
    if case == "region":
        M, skv = 100, T + 512
        x0, vec, full = _inputs(heads, T, M, skv)
        rows = _region_rows(T)
        rope_q = (full[0][rows].contiguous(), full[1][rows].contiguous())
        ctx = _ctx(m, T, M, vec, skv)
        mk = lambda: _slabs(d, skv, SENTINEL) + (rows, skv, full)
    else:
        M, skv = 512, T + 512
        x0, vec, rope_q = _inputs(heads, T, M, skv)
        ctx = _ctx(m, T, M, vec, skv)
        if case == "plain":
            mk = lambda: (m.ws.k_scratch.zero_(), m.ws.vt_scratch.zero_(), None, skv, None)
        else:
            mk = lambda: _slabs(d, skv, 0.0) + (None, skv, None)
    t_py, t_op = mk(), mk()
    x_py = _python_block(m, single, ctx, x0, t_py, rope_q)
    k_py, v_py = t_py[0].clone(), t_py[1].clone()
    if case == "plain":                 # both runs share the trunk's scratch slabs: the op has to fill them again
        t_op[0].zero_(), t_op[1].zero_()
    x_op = _op_block(m, single, ctx, x0, t_op, rope_q)
    assert torch.isfinite(x_py.float()).all() and not torch.equal(x_py, x0)
    assert torch.equal(x_op, x_py), "x differs from the Python block sequence"
    assert torch.equal(t_op[0], k_py) and torch.equal(t_op[1], v_py), "K / V^T slab differs from the Python block sequence"
    return ctx, x0, rope_q, t_op, x_op


@pytest.mark.parametrize("case", ["plain", "store", "region"])
@pytest.mark.parametrize("T", [40, 72])
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
def test_block_op_equals_the_python_block_sequence(single, heads, T, case):
    m = _model(heads, False)
    ctx, x0, rope_q, tgt, x_op = _compare(m, single, T, case)
    if case != "region":
        return
    # cache rows outside kv_rows still hold the sentinel, bit for bit; every V^T column written belongs to one of the T + M rows
    k, vt, rows, skv, full = tgt
    keep = torch.ones(k.shape[0], dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert (k[keep] == SENTINEL).all() and not (k[rows] == SENTINEL).all(dim=1).any()
    touched = (vt != SENTINEL).any(dim=0)
    assert 0 < int(touched.sum()) <= rows.numel() and not touched[ops.padded(skv, 16):].any()     # V^T positions permute inside 16-groups
    # the rewritten rows carry the fp16 round trip: a store-style (identity rows) call on the same inputs rounds K once and differs
    ident = _slabs(m.cfg_model.d, skv, SENTINEL) + (None, ctx.T + ctx.M, None)
    x_id = _op_block(m, single, ctx, x0, ident, rope_q)
    R = ctx.T + ctx.M
    assert not torch.equal(ident[0][:R], k[rows]), "partial update without the fp16 round trip"
    if not single:          # only the image rows of a double block are partial: its text rows round once in both
        assert torch.equal(ident[0][:ctx.T], k[rows[:ctx.T]])


@pytest.mark.parametrize("case", ["plain", "store", "region"])
@pytest.mark.parametrize("T", [40, 72])
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
def test_block_op_on_fp8_weights_equals_the_python_block_sequence(single, heads, T, case):
    """The cases of the bf16 test with `ops.quantize_w8` weights, against the Python sequence on the same quantised weights."""
    m = _model(heads, True)
    assert _block(m, single).attn.norm_q.dtype == torch.bfloat16 and (m.single_transformer_blocks[0].w_po.dtype == ops.FP8)
    assert m.transformer_blocks[0].attn.w_kvq.dtype == ops.FP8 and m.transformer_blocks[0].ff_w2.dtype == ops.FP8
    _compare(m, single, T, case)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
def test_rowbands_true_forks_behind_the_attention_and_changes_no_bit(single, fp8):
    """M = 512 under gemm_pieces = 1: the 256-row cut exists, the stages behind the attention run as two bands (band-1 launches are
    counted by the library) and the result is the unbanded call's - with bf16 weights and with fp8 weights (the banded GEMM launches
    then take the fp8 weight path)."""
    m = _model(2, fp8)
    T, M, skv = 40, 512, 40 + 512
    x0, vec, rope_q = _inputs(2, T, M, skv)
    ctx = _ctx(m, T, M, vec, skv)
    d = m.cfg_model.d
    with _lib.plan_override(gemm_pieces=1):
        t0, t1 = _slabs(d, skv, 0.0) + (None, skv, None), _slabs(d, skv, 0.0) + (None, skv, None)
        whole = _op_block(m, single, ctx, x0, t0, rope_q)
        before = ops.rowband_side_launches()
        banded = _op_block(m, single, ctx, x0, t1, rope_q, rowbands=True)
        assert ops.rowband_side_launches() > before, "rowbands=True sent nothing to the side stream"
    assert torch.equal(banded, whole) and torch.equal(t0[0], t1[0]) and torch.equal(t0[1], t1[1])


def test_control_swapped_adaln_vectors_do_not_pass():
    """The comparison can fail: against the Python block sequence, the same double-block op call with the text and image AdaLN vectors
    swapped is not `torch.equal` (and the unswapped call is)."""
    m = _model(2, False)
    T, M, skv = 40, 512, 40 + 512
    x0, vec, rope_q = _inputs(2, T, M, skv)
    ctx = _ctx(m, T, M, vec, skv)
    d = m.cfg_model.d
    want = _python_block(m, False, ctx, x0, _slabs(d, skv, 0.0) + (None, skv, None), rope_q)
    good = _op_block(m, False, ctx, x0, _slabs(d, skv, 0.0) + (None, skv, None), rope_q)
    a = _op_args(m, False, ctx, _slabs(d, skv, 0.0) + (None, skv, None), rope_q)
    bad = _op_block(m, False, ctx, x0, _slabs(d, skv, 0.0) + (None, skv, None), rope_q, adaln_img=a["adaln_txt"], adaln_txt=a["adaln_img"])
    assert torch.equal(good, want) and not torch.equal(bad, want)


@pytest.mark.parametrize("single", [False, True], ids=["double", "single"])
def test_extent_checks_fire_before_anything_is_written(single):
    """Every tensor one row, one column or one element too small is an error (TORCH_CHECK on the C++ registration, RegionEHipError on the
    Python one), and nothing is launched: x, nrm, wide and both slabs, filled with a sentinel, come back untouched."""
    m = _model(2, False)
    T, M = 40, 100
    skv = T + 512
    R = T + M
    d, ff = m.cfg_model.d, 4 * m.cfg_model.d
    x0, vec, full = _inputs(2, T, M, skv)
    rows = _region_rows(T)
    rope_q = (full[0][rows].contiguous(), full[1][rows].contiguous())
    ctx = _ctx(m, T, M, vec, skv)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    outs = dict(x=torch.full((R + 8, d), SENTINEL, **bf), nrm=torch.full((R + 8, d), SENTINEL, **bf), wide=torch.full((R + 8, 3 * d + ff), SENTINEL, **bf))
    k, vt = _slabs(d, skv, SENTINEL)
    base = _op_args(m, single, ctx, (k, vt, rows, skv, full), rope_q)
    base.update(outs)

    def refused(**change):
        args = dict(base)
        args.update(change)
        with pytest.raises(RuntimeError):
            _call(single, args)
    for name in ("x", "nrm", "wide"):
        refused(**{name: outs[name][:R - 1]})                                           # one row short
        refused(**{name: outs[name][:, :-8]})                                           # columns
    refused(wide=torch.full((R, 3 * d + ff + 8), SENTINEL, **bf))
    refused(kv_rows=rows[:-1].contiguous())
    refused(kv_rows=torch.cat((rows, rows[-1:])))
    refused(kv_rows=rows.int())
    refused(cos_q=rope_q[0][:-1].contiguous(), sin_q=rope_q[1][:-1].contiguous())       # query rotary rows
    refused(cos_k=full[0][:-1].contiguous(), sin_k=full[1][:-1].contiguous())           # key rotary rows by cache row
    refused(sin_q=rope_q[1][:-1].contiguous())
    refused(skv=k.shape[0] + 1)
    refused(skv=0)
    refused(vt_cache=vt[:, :-64].contiguous())
    refused(k_cache=k[:-64], vt_cache=vt)
    refused(k_cache=k[:, :-128].contiguous())
    refused(kv_rows=None, skv=R - 1)                                                    # identity rows past skv
    for key in ("adaln",) if single else ("adaln_img", "adaln_txt"):
        refused(**{key: base[key][:-1]})
    for i in range(len(base["weights"])):
        w, b = list(base["weights"]), list(base["biases"])
        w[i] = w[i][:-1]
        refused(weights=w)
        w = list(base["weights"])
        w[i] = w[i][:, :-64].contiguous()
        refused(weights=w)
        b[i] = b[i][:-1]
        refused(biases=b)
    refused(weights=base["weights"][:-1])
    refused(biases=base["biases"][:-1])
    n = list(base["norms"])
    n[-1] = n[-1][:-1]
    refused(norms=n)
    refused(norms=base["norms"][:-1])
    refused(heads=3)
    refused(M=0)
    refused(T=-1)
    torch.cuda.synchronize()
    for t in list(outs.values()) + [k, vt]:
        assert (t == SENTINEL).all(), "a refused call wrote to an output"
    _call(single, base)                                                                 # and the valid call runs
    torch.cuda.synchronize()
    assert not (outs["x"][:R] == SENTINEL).all() and (outs["x"][R:] == SENTINEL).all() and (outs["nrm"][R:] == SENTINEL).all()
    assert (outs["wide"][R:] == SENTINEL).all()


# ---- engine level: harness.flux.BLOCK_OPS ---------------------------------------------------------------------------------------------
def _edit(pipe, kw, monkeypatch, flag):
    from collections import Counter
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        """Op names per denoising step: a step ends with its split_euler_step."""

        def __init__(self):
            super().__init__()
            self.steps, self.cur = [], Counter()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if name.startswith("regione_mi."):
                op = name.split(".")[1]
                self.cur[op] += 1
                if op == "split_euler_step":
                    self.steps.append(self.cur)
                    self.cur = Counter()
            return func(*args, **(kwargs or {}))

    monkeypatch.setattr(H, "BLOCK_OPS", flag)
    trace = {}
    with Recorder() as rec:
        out = pipe(trace=trace, **kw)[0].clone()
    torch.cuda.synchronize()
    return out, [x.clone() for x in trace["latents"]], pipe._regione_manager.edited_ids.clone(), trace["kind"], rec.steps


@pytest.mark.parametrize("family", ["flux", "step1x"])
def test_engine_with_block_ops_runs_the_same_28_step_edit(family, golden, monkeypatch):
    """The toy 28-step RegionE edit with BLOCK_OPS on and off: all 28 latents, the ids and the result are `torch.equal`; the op ran in
    full (F) and in region (R) steps, and the trunk's last block - the row-skipping one - kept the Python sequence.  (`multi` is not
    covered by BLOCK_OPS, so the Step1X case runs its two CFG branches as two forwards.)"""
    from regione_amd.harness import step1x as HS
    h = w = 16
    if family == "flux":
        cfg = synth.FluxConfig(**synth.TOY)
        wts = synth.make_flux_weights(cfg, seed=42, dtype=torch.bfloat16, w_std=0.05)
        lat, _, prompt, pooled = synth.make_edit_inputs(h, w, 32, cfg, seed=42, dtype=torch.bfloat16)
        img = golden("toy_bf16")["image_latents"]          # a condition image whose partition is a compact region: F and R steps both occur
        pipe = H.FluxKontextPipeline(H.FluxTransformer2DModel(cfg, "cuda:0").load_state_dict(wts))
        kw = dict(image=img.cuda(), prompt_embeds=prompt.cuda(), pooled_prompt_embeds=pooled.cuda(), height=h * 16, width=w * 16,
                  latents=lat.cuda(), guidance_scale=2.5, return_dict=False)
        forwards = 1
    else:
        monkeypatch.setenv("RGN_BATCH_BRANCHES", "0")
        monkeypatch.setenv("RGN_BRANCH_STREAMS", "0")
        cfg = synth.FluxConfig(guidance_embeds=False, **synth.TOY)
        wts = synth.make_flux_weights(cfg, seed=5, dtype=torch.bfloat16, w_std=0.05)
        lat, _, prompt, y = synth.make_edit_inputs(h, w, 32, cfg, seed=9, dtype=torch.bfloat16)
        img = golden("s1x_toy_bf16")["image_latents"]
        _, _, nprompt, ny = synth.make_edit_inputs(h, w, 32, cfg, seed=10, dtype=torch.bfloat16)
        pipe = HS.Step1XEditPipeline(HS.Step1XEditTransformer2DModel(cfg, "cuda").load_state_dict(wts))
        kw = dict(image=img.cuda(), prompt_embeds=prompt.cuda(), pooled_prompt_embeds=y.cuda(), negative_prompt_embeds=nprompt.cuda(),
                  negative_pooled_prompt_embeds=ny.cuda(), height=h * 16, width=w * 16, latents=lat.cuda(), true_cfg_scale=4.0, return_dict=False)
        forwards = 2
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    off = _edit(pipe, kw, monkeypatch, False)
    on = _edit(pipe, kw, monkeypatch, True)
    assert len(on[1]) == 28 and len(off[1]) == 28 and on[3] == off[3] and "F" in on[3] and "R" in on[3]
    assert torch.equal(on[2], off[2]) and on[2].numel() > 0
    assert all(torch.equal(a, b) for a, b in zip(on[1], off[1])), "a step's latents differ with BLOCK_OPS on"
    assert torch.equal(on[0], off[0])
    nb = cfg.n_double + cfg.n_single
    for kind, c_on, c_off in zip(on[3], on[4], off[4]):
        assert c_off["mmdit_double_block_"] == 0 and c_off["mmdit_single_block_"] == 0
        if kind == "C":
            assert c_on["mmdit_double_block_"] == 0 and c_on["mmdit_single_block_"] == 0
            continue
        assert c_on["mmdit_double_block_"] == forwards * cfg.n_double, (kind, c_on)
        assert c_on["mmdit_single_block_"] == forwards * (cfg.n_single - 1), (kind, c_on)
        # the last block took the Python path: its attention is the only one dispatched as an op of its own
        assert c_on["region_attention"] == forwards and c_off["region_attention"] == forwards * nb, (kind, c_on, c_off)
