"""-m gpu: one VAE object called again and again at changing sizes, as the hosted pipelines call theirs (one decoder and one encoder per pipe
for the life of the pipe, at whatever resolution each edit resizes to).  Two invariants of regione_amd/vae.py, kept by `_wrote`:
  * every buffer in a `_Pool` has an all-zero border once a call is over (rgn_conv_s2_bf16 and rgn_conv_up2_bf16 do not write their
    outputs' borders, and the standalone GroupNorm statistics pass sums the border rows too); `PaddedImage.border_zero` says so;
  * the GroupNorm hand-off - whose partial sums the stream's shared workspace holds - is shared by every VAE object on the stream.
Latents h x w, 2h x 2w, h x w, h x 2w with h = 8: at 2h the mid-block attention runs at the size a later h x w call's first upsampling
convolution writes (and the encoder's last stride-2 convolution always writes the mid-block size); the same family's decoder and encoder
interleaved on one stream.  Each output must equal, bit for bit, the first call of a freshly built object at that size; after every call,
every pooled buffer has a zero border and the attention's V^T padding columns are still zero."""
import pytest
import torch

from regione_amd import qwen_vae as Q, vae as V
from tests import host_qwen_vae as HQ
from tests import host_vae
from tests.test_gpu_vae import _border_is_zero

pytestmark = pytest.mark.gpu

_SIZES = [(8, 8), (16, 16), (8, 8), (8, 16)]


def _family(kind):
    """(make_decoder, make_encoder, decode, encode) of one VAE family with seeded weights."""
    if kind == "qwen":
        sd = HQ.seeded(4).state_dict()
        return (lambda: Q.HipQwenVaeDecoder(sd, "cuda"), lambda: Q.HipQwenVaeEncoder(sd, "cuda"),
                lambda d, z: d.decode(z[:, :, None]), lambda e, x: e.encode(x[:, :, None]))
    fuse = kind == "kl_fused"
    sd = host_vae.seeded(3).state_dict()

    def dec():
        d = V.HipVaeDecoder(sd, "cuda")
        d.fuse_gn = d.fuse_upsample = fuse
        return d

    def enc():
        e = V.HipVaeEncoder(sd, "cuda")
        e.fuse_gn = fuse
        return e
    return dec, enc, lambda d, z: d.decode(z), lambda e, x: e.encode(x)


def _inputs(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    z = torch.randn(1, 16, h, w, generator=g).to("cuda", torch.bfloat16)
    x = (torch.rand(1, 3, 8 * h, 8 * w, generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    return z, x


def _check_buffers(obj, what):
    torch.cuda.synchronize()
    for key, lst in obj.pool.free.items():
        for img in lst:
            assert _border_is_zero(img), f"{what}: a pooled {key} buffer has a non-zero border"
    for key, bufs in obj._attn_buf.items():
        S, vt = bufs[0], bufs[1]
        assert bool((vt[:, S.shape[0]:] == 0).all()), f"{what}: V^T padding columns of the {key} attention buffers are not zero"


@pytest.mark.parametrize("kind", ["kl_fused", "kl_unfused", "qwen"])
def test_decoder_and_encoder_reused_across_sizes(kind):
    make_dec, make_enc, decode, encode = _family(kind)
    ref = {}
    for hw in dict.fromkeys(_SIZES):                              # first call of fresh objects at each size
        z, x = _inputs(*hw)
        ref[hw] = (decode(make_dec(), z), encode(make_enc(), x))
    torch.cuda.synchronize()
    dec, enc = make_dec(), make_enc()
    for i, hw in enumerate(_SIZES):
        z, x = _inputs(*hw)
        img = decode(dec, z)
        _check_buffers(dec, f"{kind} decode #{i} {hw}")
        mom = encode(enc, x)
        _check_buffers(enc, f"{kind} encode #{i} {hw}")
        _check_buffers(dec, f"{kind} decoder after encode #{i} {hw}")
        assert torch.equal(img, ref[hw][0]), f"{kind} decode #{i} at {hw} differs from a fresh decoder's first call"
        assert torch.equal(mom, ref[hw][1]), f"{kind} encode #{i} at {hw} differs from a fresh encoder's first call"
