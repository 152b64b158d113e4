"""-m gpu: row bands (rgn_rowband_fork / rgn_rowband_join) - a banded launch is BIT-IDENTICAL to the unbanded, unsplit one.

The band boundary is a multiple of 256 rows from the cut problem's first row, so every tile of a band is a tile of the unbanded launch
with the same arithmetic; a band launch runs whole tiles only, which is the accumulation order of `gemm_pieces=1`.  Every comparison
here is torch.equal against the same call under gemm_pieces=1 without a fork.  Nothing is timed."""
import pytest
import torch

from regione_amd import RegionEHelper, _lib, ops, synth
from regione_amd.harness import flux as H

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _rand(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _both(make, launch):
    """launch(make()) unbanded and banded, both unsplit; returns the two results and the number of band-1 launches of the banded run.
    make() builds the operands and outputs BEFORE the fork - the side stream waits for what is enqueued at the fork, not for a fill or a
    copy the caller's stream gets later - and launch() only enqueues: band 1's rows may be read after the join."""
    with _lib.plan_override(gemm_pieces=1):
        n0 = ops.rowband_side_launches()
        ref = launch(make())
        torch.cuda.synchronize()
        assert ops.rowband_side_launches() == n0, "no fork: nothing may reach the side stream"
        state = make()
        ops.rowband_fork()
        try:
            got = launch(state)
        finally:
            ops.rowband_join()
        torch.cuda.synchronize()
        return ref, got, ops.rowband_side_launches() - n0


EPILOGUES = [("bias", ops.EPI_BIAS, 0), ("gelu", ops.EPI_GELU, 256), ("gate_resid", ops.EPI_GATE_RESID, 0)]


def _problem(A, W, b, epi, seed):
    M, N = A.shape[0], W.shape[0]
    out = torch.full((M, N), 7.0, dtype=BF, device="cuda")
    if epi == ops.EPI_GATE_RESID:
        return ops.Problem(A, W, b, out, gate=_rand(N, seed=seed + 1), resid=_rand(M, N, seed=seed + 2))
    return ops.Problem(A, W, b, out)


@pytest.mark.parametrize("name,epi,gelu_from", EPILOGUES)
def test_gemm_group_one_problem_ragged_last_tile_in_band_1(name, epi, gelu_from):
    M, N, K = 3 * 256 + 40, 512, 512
    A, W, b = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=0.05), _rand(N, seed=3)
    assert ops.rowband_query([M]) == (0, 512)

    def run(p):
        ops.gemm_group([p], epilogue=epi, gelu_from_col=gelu_from)
        return p.out, _lib.lib().rgn_gemm_last_plan()
    (ref, plan0), (got, plan1), side = _both(lambda: _problem(A, W, b, epi, 10), run)
    assert side == 1 and plan1 == plan0 | 0x800 and not plan0 & 0x800
    assert torch.isfinite(ref.float()).all() and torch.equal(got, ref)


@pytest.mark.parametrize("name,epi,gelu_from", EPILOGUES)
def test_gemm_group_text_image_pair_boundary_inside_the_image_problem(name, epi, gelu_from):
    T, M, N, K = 300, 600, 512, 512
    x = _rand(T + M, K, seed=4)                          # [text ; image] rows of one buffer, as the engine lays them out
    Wi, Wt, bi, bt = _rand(N, K, seed=5, scale=0.05), _rand(N, K, seed=6, scale=0.05), _rand(N, seed=7), _rand(N, seed=8)
    assert ops.rowband_query([T, M]) == (1, 256)

    def run(ps):
        ops.gemm_group(ps, epilogue=epi, gelu_from_col=gelu_from)              # image first, like the engine's pair launches
        return ps[1].out, ps[0].out                                           # read only after the join
    ref, got, side = _both(lambda: [_problem(x[T:], Wi, bi, epi, 20), _problem(x[:T], Wt, bt, epi, 30)], run)
    assert side == 1
    for r, g in zip(ref, got):
        assert torch.isfinite(r.float()).all() and torch.equal(g, r)


@pytest.mark.parametrize("gathered", [False, True])
def test_fused_qkv_epilogue_keeps_rotary_rows_cache_rows_and_slab_positions(gathered):
    H_, d, K, M, pad = 2, 256, 256, 520, 640
    N = 3 * d + 256                                       # [k | v | q | mlp]
    A, W, b = _rand(M, K, seed=40), _rand(N, K, seed=41, scale=0.06), _rand(N, seed=42)
    wq, wk = _rand(128, seed=43).abs() + 0.5, _rand(128, seed=44).abs() + 0.5
    ang = torch.rand(pad, 128, generator=torch.Generator().manual_seed(45)) * 6.28
    rope = (ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda())
    kv_rows = torch.randperm(pad, generator=torch.Generator().manual_seed(46))[:M].contiguous().cuda() if gathered else None
    k0, v0, o0 = _rand(pad, d, seed=47), _rand(d, pad, seed=48), _rand(M, N, seed=49)      # what no band owns must stay as it is
    assert ops.rowband_query([M]) == (0, 512)

    def run(state):
        k_slab, vt_slab, out = state
        epi = ops.qkv_epilogue(wq=wq, wk=wk, rope_q=rope, rope_k=rope, k_slab=k_slab, vt_slab=vt_slab, H=H_, k_col=0, v_col=d,
                               q_col=2 * d, kv_rows=kv_rows, rows=M)
        ops.gemm_qkv(A, W, b, out, epi, gelu_from_col=3 * d)
        return out, k_slab, vt_slab
    (o_ref, k_ref, v_ref), (o, k, v), side = _both(lambda: (k0.clone(), v0.clone(), o0.clone()), run)
    assert side == 1
    assert torch.equal(o[:, 2 * d:3 * d], o_ref[:, 2 * d:3 * d]) and torch.equal(o[:, 3 * d:], o_ref[:, 3 * d:])     # Q in place, MLP
    assert torch.equal(o, o_ref) and torch.equal(o[:, :2 * d], o0[:, :2 * d])           # K / V columns of C are never written
    assert torch.equal(k, k_ref) and torch.equal(v, v_ref)
    rows = kv_rows.cpu() if gathered else torch.arange(M)
    free = torch.ones(pad, dtype=torch.bool)
    free[rows] = False
    assert torch.equal(k[free.cuda()], k0[free.cuda()]), "K slab rows no band owns are untouched"
    assert not torch.equal(k[(~free).cuda()], k0[(~free).cuda()])


@pytest.mark.parametrize("d", [512, 384])                 # wave-per-row kernel / block-per-row kernel
def test_ln_modulate_text_image_segments(d):
    T, M = 300, 600
    x = _rand(T + M, d, seed=50)
    sh0, sc0, sh1, sc1 = (_rand(d, seed=51 + i, scale=0.3) for i in range(4))

    def out():
        return torch.full_like(x, 7.0)
    ref, got, side = _both(out, lambda o: ops.ln_modulate(x, o, sh1, sc1, split_row=T, shift0=sh0, scale0=sc0))
    assert side == 1 and torch.equal(got, ref)
    ref2, got2, side = _both(out, lambda o: ops.ln_modulate_segs(x, o, [(T, sh0, sc0), (T + M, sh1, sc1)]))
    assert side == 1 and torch.equal(got2, ref2) and torch.equal(ref2, ref)
    # the text segment larger than the image one: the cut segment is not the last, band 0 also owns the rows behind it
    ref3, got3, side = _both(out, lambda o: ops.ln_modulate(x, o, sh1, sc1, split_row=M, shift0=sh0, scale0=sc0))
    assert side == 1 and torch.equal(got3, ref3)


# ---- the toy trunk: fork / join around every attention, the chain across block boundaries and the double -> single transition --------------
@pytest.fixture(scope="module")
def toy(golden):
    g = golden("toy_bf16")
    h, w, T = g["h"], g["w"], g["T"]
    cfg = synth.FluxConfig(**synth.TOY)
    wts = synth.make_flux_weights(cfg, seed=42, dtype=BF, w_std=g["w_std"])
    lat, _, prompt, pooled = synth.make_edit_inputs(h, w, T, cfg, seed=g["seed"], dtype=BF)
    tr = H.FluxTransformer2DModel(cfg, "cuda").load_state_dict(wts)
    return dict(g=g, h=h, w=w, T=T, tr=tr, lat=lat.cuda(), img=g["image_latents"].cuda(), prompt=prompt.cuda(), pooled=pooled.cuda())


def _forward(t):
    x = torch.cat([t["lat"], t["img"]], 1)
    ts = torch.full([1], 0.7, dtype=BF)
    return t["tr"](hidden_states=x, timestep=ts, guidance=torch.full([1], 2.5), pooled_projections=t["pooled"],
                   encoder_hidden_states=t["prompt"], txt_ids=torch.zeros(t["T"], 3), img_ids=synth.flux_latent_ids(t["h"], t["w"]),
                   return_dict=False)[0]


def _unbanded_and_banded(fn):
    with _lib.plan_override(gemm_pieces=1, rowbands=0):
        n0 = ops.rowband_side_launches()
        ref = fn()
        torch.cuda.synchronize()
        assert ops.rowband_side_launches() == n0
    with _lib.plan_override(gemm_pieces=1):
        got = fn()
        torch.cuda.synchronize()
    return ref, got, ops.rowband_side_launches() - n0


def test_toy_full_step_banded_equals_unbanded(toy):
    # [text 32 | image 512] cuts the image rows at 256, the joint 544 rows of a single block at 512: the bands meet at the transition
    assert H._band_row((toy["T"], 512)) != H._band_row((toy["T"] + 512,))
    ref, got, side = _unbanded_and_banded(lambda: _forward(toy))
    assert side > 0, "the full step must run banded"
    assert torch.isfinite(ref.float()).all() and torch.equal(got, ref)


def test_toy_28_step_edit_banded_equals_unbanded(toy):
    g = toy["g"]
    pipe = H.FluxKontextPipeline(toy["tr"])
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=g["threshold"])
    helper.enable()

    def edit():
        trace = {}
        out = pipe(image=toy["img"], prompt_embeds=toy["prompt"], pooled_prompt_embeds=toy["pooled"], height=toy["h"] * 16,
                   width=toy["w"] * 16, latents=toy["lat"], guidance_scale=2.5, return_dict=False, trace=trace)[0]
        return out, trace
    try:
        (ref, tr0), (got, tr1), side = _unbanded_and_banded(edit)
    finally:
        helper.disable()
    assert "".join(tr1["kind"]) == "".join(tr0["kind"]) == "".join(g["kinds"].tolist())
    assert side > 0 and torch.equal(got, ref)
    for a, b in zip(tr0["latents"], tr1["latents"]):
        assert torch.equal(a, b)


def test_no_launch_reaches_the_side_stream_while_launches_are_timed_one_by_one(toy, monkeypatch):
    """bench.py's per-launch timer sets ATTN_BRANCH_STREAMS = False: a launch must then have the chip to itself."""
    monkeypatch.setattr(H, "ATTN_BRANCH_STREAMS", False)
    n0 = ops.rowband_side_launches()
    out = _forward(toy)
    torch.cuda.synchronize()
    assert ops.rowband_side_launches() == n0 and torch.isfinite(out.float()).all()
    monkeypatch.undo()
    _forward(toy)
    torch.cuda.synchronize()
    assert ops.rowband_side_launches() > n0
