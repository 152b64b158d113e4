"""-m gpu: the two invariants regione_amd/vae.py keeps through `_wrote`, checked where they are made.
  * `PaddedImage.border_zero` tells the truth about every image that enters a pool, and the only images that enter with it false are the
    materialised mid-block attention's outputs (the P V GEMM writes the border rows; rgn_vae_attention_bf16 does not write them, so its
    output keeps the zero border of the Q image it overwrites);
  * a write to the image whose GroupNorm statistics the stream's workspace holds drops the hand-off: the next groupnorm_silu runs its own
    statistics pass (precomputed_blocks = 0 in the launch record) and gives the standalone pass's bits."""
import os
import sys

import pytest
import torch

from regione_amd import _lib, vae as V
from tests.test_gpu_vae import _border_is_zero
from tests.test_gpu_vae_reuse import _SIZES, _family, _inputs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import vae_bits as B  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("attention", ["materialized", "fused"])
@pytest.mark.parametrize("kind", ["kl_fused", "kl_unfused", "qwen"])
def test_border_flag_of_every_image_entering_a_pool(kind, attention, monkeypatch):
    make_dec, make_enc, decode, encode = _family(kind)
    state = {"in_attention": False, "dirty": 0, "puts": 0, "attentions": 0}
    put, run_attention = V._Pool.put, V._KLBase._run_attention
    dirty_per_call = 1 if attention == "materialized" else 0

    def checked_put(pool, img):
        state["puts"] += 1
        if img.border_zero:
            torch.cuda.synchronize()
            assert _border_is_zero(img), f"a {img.H} x {img.W} x {img.C} image enters the pool with border_zero set and a non-zero border"
        else:
            assert state["in_attention"], "an image that is not an attention output enters the pool with border_zero false"
            state["dirty"] += 1
        put(pool, img)

    def watched_attention(obj, x):
        state["in_attention"], before = True, state["dirty"]
        try:
            out = run_attention(obj, x)
        finally:
            state["in_attention"] = False
        assert state["dirty"] == before + dirty_per_call          # exactly the one output image of the P V GEMM
        state["attentions"] += 1
        return out

    monkeypatch.setattr(V._Pool, "put", checked_put)
    monkeypatch.setattr(V._KLBase, "_run_attention", watched_attention)
    dec, enc = make_dec(), make_enc()
    dec.attention = enc.attention = attention
    for hw in _SIZES:
        z, x = _inputs(*hw)
        decode(dec, z)
        encode(enc, x)
    assert state["attentions"] == 2 * len(_SIZES) and state["dirty"] == dirty_per_call * state["attentions"] and state["puts"] > 100
    for obj in (dec, enc):                                        # at rest every pooled image has been rewritten by a border-zeroing kernel
        assert all(img.border_zero for lst in obj.pool.free.values() for img in lst)


def _image(H, W, C, seed):
    img = V.PaddedImage(H, W, C, "cuda")
    x = torch.randn(H, W, C, generator=torch.Generator().manual_seed(seed)).to("cuda", torch.bfloat16)
    img.t.view(img.Hp, img.Wp, C)[1:-1, 1:-1] = x                 # the border stays zero
    return img


@pytest.mark.parametrize("writer", ["conv_s2", "upsample2x", "gemm_into"])
def test_a_write_to_the_owner_drops_the_groupnorm_handoff(writer):
    H, W, C = 16, 16, 128
    g = torch.Generator().manual_seed(11)
    w3 = (torch.randn(C, 3, 3, C, generator=g) / (3 * C ** 0.5)).cuda()
    bias = (0.1 * torch.randn(C, generator=g)).cuda()
    gamma, beta = (1.0 + 0.2 * torch.randn(C, generator=g)).to("cuda", torch.bfloat16), (0.1 * torch.randn(C, generator=g)).to("cuda", torch.bfloat16)
    cw = V.ConvWeights(w3, bias)
    x, y = _image(H, W, C, 1), V.PaddedImage(H, W, C, "cuda")
    V.conv(x, cw, y, gn=True)
    owner, nblk = V.gn_handoff(y.t.device)
    assert owner is y and nblk > 0
    if writer == "conv_s2":
        V.conv_s2(_image(2 * H, 2 * W, C, 2), cw, y, V.downsample_rows(2 * H, 2 * W, "cuda"))
    elif writer == "upsample2x":
        V.upsample2x(_image(H // 2, W // 2, C, 3), y)
    else:
        V.gemm_into(x.t, w3[:, 1, 1].to(torch.bfloat16).contiguous(), None, y)
        assert V.gn_handoff(y.t.device)[0] is None and not y.border_zero
        with pytest.raises(_lib.RegionEHipError, match="not known to be zero"):
            V.groupnorm_silu(y, gamma, beta, V.PaddedImage(H, W, C, "cuda"))
        torch.cuda.synchronize()
        assert _border_is_zero(y)              # no bias, and the border rows of A = x are zero: this product's border rows are zero,
        y.border_zero = True                   # which the helper cannot know
    assert V.gn_handoff(y.t.device)[0] is None and y.border_zero
    y2, n, n2 = V.PaddedImage(H, W, C, "cuda"), V.PaddedImage(H, W, C, "cuda"), V.PaddedImage(H, W, C, "cuda")
    y2.t.copy_(y.t)
    with B.recording() as rec:
        V.groupnorm_silu(y, gamma, beta, n)
        V.groupnorm_silu(y2, gamma, beta, n2)                     # the standalone pass: nothing was ever handed off for y2
    launches = rec.named("rgn_groupnorm_silu")
    assert len(launches) == 2 and launches[0][1:] == launches[1][1:] and "10=0" in launches[0]     # argument 10: precomputed_blocks
    torch.cuda.synchronize()
    assert torch.equal(n.t, n2.t) and bool((n.t != 0).any())
