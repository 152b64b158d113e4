"""-m gpu: Step1X-Edit's per-step connector on the HIP kernels (regione_amd/step1x_connector.py, csrc/connector.hip; SURVEY.md section 8
row f4) against the stand-in of the public layout (tests/host_step1x_connector.py).

  kernels  * rgn_masked_mean_rows against fp64: |err| <= 2^-7 |ref| + 1e-6 (two bf16 roundings of <= 2^-9 relative each; the fp32 sum over
             <= 130 terms is far below that); rows past n_valid are never read (they hold inf);
           * rgn_head_rms_norm_bf16 bit-equal to rgn_rms_norm_rows on a contiguous [L H, 128] copy of the q and the k heads, dense and
             padded row stride; v columns and pad columns bit-unchanged;
           * rgn_gate_resid_rows bit-equal to torch's bf16 `resid + gate * p`, also in place on resid;
           * rgn_vision_attention_bf16 driven by `connector_items`: padded rows bit-equal v[0] of their head, valid rows against an fp64
             softmax within the head-128 kernel's bounds (tests/test_gpu_qwen_text_encoder.py: max abs 2e-2, >= 40 dB on N(0, 1));
  module   * enc and y against the stand-in in fp32 on the bf16 weights: HIP at most 1 dB below the eager bf16 stand-in on each output (the
             rule of the encoder stacks; both values printed); hoist=True bit-equal to hoist=False; a repeated step bit-equal; another t
             differs; after a new prepare nothing of the old embeddings survives; only rgn:: kernels and runtime copies / fills;
  hosted   * Step1X and Step1X-v1p2 stand-in pipelines with this connector: the module's forward is never called, the trace has F, R and C
             steps, two runs are bit-equal, against the host-module run the kinds are equal and the latents >= 40 dB (the loop bar);
             `_regione_hip_connector = False` and a ToyConnector host give today's call counts.
"""
import copy
import math

import pytest
import torch

import regione_amd.torch_ops  # noqa: F401  (registers torch.ops.regione_mi.*)
from regione_amd import RegionEHelper, _lib, ops, step1x_connector as SC

import host_standins as HS
import host_step1x_connector as HC

pytestmark = pytest.mark.gpu
_p, _stream = ops._p, ops._stream
DEV = "cuda"


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def _randn(*shape, seed=0, std=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std).to(torch.bfloat16).to(DEV)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.0898])
@pytest.mark.parametrize("L,n,d", [(1, 1, 64), (65, 65, 192), (130, 65, 256), (80, 1, 256)])
def test_masked_mean_rows_against_fp64(L, n, d, scale):
    x = _randn(L, d, seed=L + d)
    x[n:] = float("inf")                                          # a row past n_valid that is read shows up as inf / nan
    got = ops.masked_mean_rows(x, n, scale)
    ref = x[:n].double().mean(0) * scale
    err = (got.double() - ref).abs()
    print(f"masked_mean_rows L={L} n={n} d={d} scale={scale}: max |err| {float(err.max()):.3e}, max |err| / bound "
          f"{float((err / (2.0 ** -7 * ref.abs() + 1e-6)).max()):.3f}")
    assert got.shape == (d,) and got.dtype == torch.bfloat16
    assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-6).all())
    assert torch.equal(got, ops.masked_mean_rows(x, n, scale)), "a repeated call must be bit-identical"
    # a padded row stride (a column slice of a wider buffer) gives the same bits
    wide = torch.full((L, d + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, :d] = x
    assert torch.equal(ops.masked_mean_rows(wide[:, :d], n, scale), got)
    assert torch.equal(torch.ops.regione_mi.masked_mean_rows(x, n, scale), got)


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("L,H", [(1, 1), (67, 3)])
def test_head_rms_norm_is_rms_norm_rows_on_the_heads(L, H, pad):
    d = H * 128
    buf = _randn(L, 3 * d + pad, seed=L + H + pad, std=2.0)
    qkv = buf[:, :3 * d] if pad else buf
    wq, wk = _randn(128, seed=1) * 0.1 + 1, _randn(128, seed=2) * 0.1 + 1
    before = buf.clone()
    want_q = ops.rms_norm_rows(before[:, :d].reshape(L * H, 128).contiguous(), wq, 1e-6).view(L, d)
    want_k = ops.rms_norm_rows(before[:, d:2 * d].reshape(L * H, 128).contiguous(), wk, 1e-6).view(L, d)
    ops.head_rms_norm_(qkv, wq, wk, H, 1e-6)
    assert torch.equal(buf[:, :d], want_q) and torch.equal(buf[:, d:2 * d], want_k)
    assert torch.equal(buf[:, 2 * d:], before[:, 2 * d:]), "v columns and pad columns are not written"
    again = before.clone()
    torch.ops.regione_mi.head_rms_norm_(again[:, :3 * d] if pad else again, wq, wk, H, 1e-6)
    assert torch.equal(again, buf)


@pytest.mark.parametrize("M,N", [(1, 64), (67, 384)])
def test_gate_resid_rows_is_torchs_bf16_gated_residual(M, N):
    p, resid, gate = _randn(M, N, seed=M), _randn(M, N, seed=N), _randn(N, seed=M + N)
    want = resid + gate * p                                       # torch's bf16 ops on the device: bf16(gate * p), then bf16(resid + .)
    got = ops.gate_resid_rows(p, gate, resid)
    assert torch.equal(got, want)
    r2 = resid.clone()
    assert ops.gate_resid_rows(p, gate, r2, out=r2) is r2 and torch.equal(r2, want)          # y may be resid
    r3 = resid.clone()
    torch.ops.regione_mi.gate_resid_rows_(p, gate, r3, r3)
    assert torch.equal(r3, want)
    # and the fused epilogue it is the elementwise half of: RGN_EPI_GATE_RESID on a projection equals the bare projection + this kernel
    if N % 64 == 0:
        A, W, b = _randn(M, 128, seed=5), _randn(N, 128, seed=6, std=0.1), _randn(N, seed=7, std=0.1)
        bare, fused = torch.empty(M, N, dtype=torch.bfloat16, device=DEV), torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        ops.gemm(A, W, b, bare)
        ops.gemm(A, W, b, fused, epilogue=ops.EPI_GATE_RESID, gate=gate, resid=resid)
        assert torch.equal(ops.gate_resid_rows(bare, gate, resid), fused)


@pytest.mark.parametrize("L,n,H", [(130, 65, 2), (80, 1, 2), (64, 64, 3)])
def test_attention_with_connector_items(L, n, H):
    D = 128
    qkv = _randn(L, 3 * H * D, seed=L + n)
    items = SC.connector_items(L, n).to(DEV)
    o = torch.full((L, H * D), 9.0, dtype=torch.bfloat16, device=DEV)
    scale = D ** -0.5
    rc = _lib.lib().rgn_vision_attention_bf16(_p(qkv), _p(o), L, H, D, scale, _p(items), items.shape[0], _stream())
    _lib.check(rc, "rgn_vision_attention_bf16")
    v = qkv[:, 2 * H * D:]
    if n < L:
        assert torch.equal(o[n:], v[0:1].expand(L - n, H * D)), "a padded row sees key 0 alone: its output is v[0] of the head, bit for bit"
    q, k, vv = (qkv[:, i * H * D:(i + 1) * H * D].double().view(L, H, D).transpose(0, 1) for i in range(3))
    s = (q[:, :n] @ k[:, :n].transpose(1, 2)) * scale
    ref = (torch.softmax(s, -1) @ vv[:, :n]).transpose(0, 1).reshape(n, H * D)
    err, p = float((o[:n].double() - ref).abs().max()), psnr(o[:n], ref)
    print(f"connector attention L={L} n={n} H={H}: max abs err {err:.3e}, PSNR {p:.2f} dB")
    assert err <= 2e-2 and p >= 40.0, (err, p)


# ---- module ---------------------------------------------------------------------------------------------------------------------------------
TS = (0.02, 0.5, 1.0)
POOLED = 256
_cache = {}


def _case(i_, h, heads, L, n, depth):
    """One module case, built once and shared: the bf16 stand-in on the device, inputs, masks, and the fp32 / eager bf16 references at TS."""
    key = (i_, h, heads, L, n, depth)
    if key in _cache:
        return _cache[key]
    mod = HC.make_connector(i_, h, heads, depth, POOLED, seed=h + L).to(DEV)
    n2 = L if n < L // 2 else max(1, n // 2)                     # the two branches have different valid lengths
    x = _randn(2, L, i_, seed=L + n)
    mask = torch.zeros(2, L, device=DEV)
    mask[0, :n], mask[1, :n2] = 1, 1
    f32 = copy.deepcopy(mod).float()
    ref, eager = {}, {}
    with torch.no_grad():
        for t in TS:
            tt = torch.full((2,), t, device=DEV)
            ref[t] = f32(x.float(), tt, mask)
            eager[t] = mod(x, tt, mask)
    _cache[key] = dict(mod=mod, x=x, mask=mask, ref=ref, eager=eager, ns=(n, n2))
    return _cache[key]


def _outs(res):
    return torch.cat([e for e, _ in res], 0), torch.cat([y for _, y in res], 0)


CASES = [(256, 256, 2, 96, 70, 2), (192, 384, 3, 130, 65, 2), (256, 256, 2, 64, 64, 2), (256, 256, 2, 80, 1, 2), (256, 256, 2, 96, 70, 1)]


@pytest.mark.parametrize("i_,h,heads,L,n,depth", CASES)
def test_connector_matches_the_stand_in(i_, h, heads, L, n, depth):
    c = _case(i_, h, heads, L, n, depth)
    hip = SC.HipStep1XConnector(c["mod"], DEV)
    hip.prepare([c["x"][0], c["x"][1]], [c["mask"][0:1], c["mask"][1:2]])
    for t in TS:
        enc, y = _outs(hip.step(t))
        assert enc.shape == (2, L, h) and y.shape == (2, POOLED) and enc.dtype == y.dtype == torch.bfloat16
        assert torch.isfinite(enc.float()).all() and torch.isfinite(y.float()).all()
        (re, ry), (ee, ey) = c["ref"][t], c["eager"][t]
        he, be, hy, by = psnr(enc, re), psnr(ee, re), psnr(y, ry), psnr(ey, ry)
        print(f"connector {(i_, h, heads, L, c['ns'], depth)} t={t}: enc HIP {he:.2f} dB, eager bf16 {be:.2f} dB; y HIP {hy:.2f} dB, eager bf16 {by:.2f} dB")
        assert he >= be - 1.0, (t, he, be)
        assert hy >= by - 1.0, (t, hy, by)


@pytest.mark.parametrize("i_,h,heads,L,n,depth", CASES)
def test_hoisting_repetition_and_rebinding_keep_the_bits(i_, h, heads, L, n, depth):
    c = _case(i_, h, heads, L, n, depth)
    rows, masks = [c["x"][0], c["x"][1]], [c["mask"][0:1], c["mask"][1:2]]
    hip, plain = SC.HipStep1XConnector(c["mod"], DEV), SC.HipStep1XConnector(c["mod"], DEV, hoist=False)
    assert hip.embed[0].data_ptr() == c["mod"].S.input_embedder.weight.data_ptr(), "bf16 device weights are adopted without a copy"
    hip.prepare(rows, masks)
    plain.prepare(rows, masks)
    a = _outs(hip.step(0.5))
    b = _outs(plain.step(0.5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "hoist=True must equal hoist=False bit for bit"
    a2 = _outs(hip.step(0.5))
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1]), "a second step at the same t is bit-equal"
    d = _outs(hip.step(0.02))
    assert not torch.equal(d[0], a[0]) and torch.equal(d[1], a[1]), "enc depends on t, y does not"
    assert torch.equal(_outs(hip.step(torch.tensor([0.5, 0.5])))[0], a[0])
    # new embeddings (other values, other lengths, no mask) on the same object == a fresh object's
    x2 = [_randn(L - 7, i_, seed=77), _randn(L, i_, seed=78)]
    m2 = [None, masks[0]]
    hip.prepare(x2, m2)
    fresh = SC.HipStep1XConnector(c["mod"], DEV)
    fresh.prepare(x2, m2)
    for got, want in zip(hip.step(1.0), fresh.step(1.0)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    hip.prepare(rows, masks)                                      # and back: the first result again
    back = _outs(hip.step(0.5))
    assert torch.equal(back[0], a[0]) and torch.equal(back[1], a[1])


def _gpu_activity_names(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]


def _foreign(names):
    ok = lambda n: ("rgn::" in n) or n.startswith("__amd_rocclr_") or n.lower().startswith(("memcpy", "memset"))
    return sorted({n[:120] for n in names if not ok(n)})


def test_prepare_and_step_dispatch_only_rgn_kernels():
    c = _case(*CASES[0])
    rows, masks = [c["x"][0], c["x"][1]], [c["mask"][0:1], c["mask"][1:2]]
    hip = SC.HipStep1XConnector(c["mod"], DEV)
    hip.prepare(rows, masks)
    hip.step(0.5)                                                 # warm: buffers, workspaces
    torch.cuda.synchronize()

    def run():
        hip.prepare(rows, masks)
        return hip.step(0.5)
    _, names = _gpu_activity_names(run)
    assert _foreign(names) == [], _foreign(names)
    for k in ("masked_mean_rows_kernel", "head_rms_norm_kernel", "gate_resid_rows_kernel", "vision_attention_kernel", "gemm_bf16_kernel",
              "gemv_bf16_kernel", "layer_norm_rows_kernel"):
        assert any(k in n for n in names), (k, sorted(set(names)))


# ---- hosted -----------------------------------------------------------------------------------------------------------------------------------
class CountingConnector(HC.Qwen2Connector):
    calls = 0

    def forward(self, x, t, mask):
        self.calls += 1
        return super().forward(x, t, mask)


def _picture(h=256, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(1, 3, h, w, generator=g)
    p[:, :, h // 4: h // 4 + h // 3, w // 3: w // 3 + w // 3] = 0.0
    return p


def _hosted(v1p2, connector=None, hip=True):
    cls = HS.Step1XEditPipelineV1P2 if v1p2 else HS.Step1XEditPipeline
    trunk = HS.stub_trunk("step1x")
    pipe = cls(trunk)
    if connector is None:
        connector = HC.make_connector(256, 256, 2, 2, 64, seed=4)
        connector.__class__ = CountingConnector
    object.__setattr__(trunk, "connector", connector)
    if not hip:
        pipe._regione_hip_connector = False
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    helper.enable()
    return pipe, connector, helper


def _edit(pipe, v1p2):
    trace = {}
    kw = dict(image=_picture(), prompt="turn the sky green", generator=torch.Generator().manual_seed(1), output_type="latent", trace=trace)
    if v1p2:
        kw.update(enable_thinking_mode=False, enable_reflection_mode=False)
    else:
        kw["latents"] = None
    out = pipe(**kw).images
    return out, "".join(trace["kind"])


@pytest.mark.parametrize("v1p2", [False, True])
def test_hosted_edit_never_calls_the_connector_module(v1p2):
    from oracle import regione_oracle as O
    pipe, conn, helper = _hosted(v1p2)
    a, kinds = _edit(pipe, v1p2)
    assert conn.calls == 0, "the connector runs on the HIP kernels: the module's forward is never called"
    assert isinstance(pipe._regione_hip_connector, SC.HipStep1XConnector)
    assert len(kinds) == 28 and all(k in kinds for k in "FRC"), kinds
    assert a.shape == (1, 256, 64) and torch.isfinite(a.float()).all()
    assert "connector" not in helper._engine().transformer.__dict__          # hook removed after the call
    # the second run under the profiler: the whole hosted call - encode stage (bind_text), loop (prepare, step, the ttm add, the adapter's
    # copies), the trunk around them - records only rgn:: kernels and runtime copies / fills
    (b, kinds_b), names = _gpu_activity_names(lambda: _edit(pipe, v1p2))
    assert torch.equal(a, b) and kinds_b == kinds and conn.calls == 0
    assert _foreign(names) == [], _foreign(names)
    assert any("gate_resid_rows_kernel" in n for n in names) and any("head_rms_norm_kernel" in n for n in names)
    # the same pipeline with the host module driving the connector, per branch per computed step as before
    host, hconn, hhelper = _hosted(v1p2, hip=False)
    r, kinds_r = _edit(host, v1p2)
    computed = kinds_r.count("F") + kinds_r.count("R")
    assert hconn.calls == 2 * computed and host._regione_hip_connector is False
    p = O.psnr(a.float().cpu(), r.float().cpu())
    print(f"hosted Step1X{'-v1p2' if v1p2 else ''} {kinds}: HIP connector against the host module {p:.2f} dB")
    assert kinds == kinds_r
    assert p >= 40.0, p
    helper.disable()
    hhelper.disable()


@pytest.mark.parametrize("v1p2", [False, True])
def test_a_toy_connector_host_behaves_as_before(v1p2):
    toy = HS.ToyConnector().to(torch.bfloat16)
    pipe, conn, helper = _hosted(v1p2, connector=toy)
    _, kinds = _edit(pipe, v1p2)
    assert conn.calls == 2 * (kinds.count("F") + kinds.count("R")) and kinds.count("C") > 0
    assert pipe._regione_hip_connector is None
    helper.disable()
