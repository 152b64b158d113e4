"""CPU: the mid-block attention's dispatch rule (regione_amd/vae.py attention_path), the documented maximum image size of both VAE families
(checked before anything is allocated), and the argument checks of rgn_vae_attention_bf16 through ctypes - no device needed."""
import pytest
import torch

from regione_amd import _lib, qwen_vae as Q, vae as V
from tests import host_qwen_vae as HQ
from tests import host_vae


def test_auto_keeps_the_materialized_path_exactly_where_the_softmax_pass_runs():
    assert V.SOFTMAX_MAX_ROWS == Q.SOFTMAX_MAX_ROWS == 24576
    assert V.attention_path("auto", 130 * 130) == "materialized"
    assert V.attention_path("auto", 24576) == "materialized"
    assert V.attention_path("auto", 24577) == "fused"
    assert V.attention_path("auto", 162 * 162) == "fused"
    assert V.attention_path("fused", 3 * 3) == "fused"
    assert V.attention_path("materialized", 24576) == "materialized"
    with pytest.raises(_lib.RegionEHipError, match="24576"):
        V.attention_path("materialized", 24577)
    with pytest.raises(_lib.RegionEHipError):
        V.attention_path("flash", 100)


def test_the_documented_maximum_admits_2048_squared_and_4096_sides():
    for H, W in ((2048, 2048), (4096, 1024), (1024, 4096), (1280, 1280), (8, 8)):
        V.check_image_size(H, W, "x")
    for H, W in ((2056, 2048), (4104, 8), (8, 4104), (4096, 2048)):
        with pytest.raises(_lib.RegionEHipError, match="2048"):
            V.check_image_size(H, W, "x")


@pytest.fixture(scope="module")
def kl():
    return host_vae.seeded(1).state_dict()


def test_the_vaes_refuse_past_the_maximum_before_allocating(kl, monkeypatch):
    dec, enc = V.HipVaeDecoder(kl, "cpu"), V.HipVaeEncoder(kl, "cpu")
    qsd = HQ.seeded(2).state_dict()
    qdec, qenc = Q.HipQwenVaeDecoder(qsd, "cpu"), Q.HipQwenVaeEncoder(qsd, "cpu")
    for o in (dec, enc, qdec, qenc):
        monkeypatch.setattr(o.pool, "get", lambda *a: pytest.fail("allocated before the size check"))

    class FakeCuda(torch.Tensor):                   # passes the `is_cuda` check without a device; its data never gets read
        @property
        def is_cuda(self):
            return True

    def fake(*shape):
        return torch.zeros(*shape).as_subclass(FakeCuda)
    with pytest.raises(_lib.RegionEHipError, match="maximum"):
        dec.decode(fake(1, 16, 264, 256))
    with pytest.raises(_lib.RegionEHipError, match="maximum"):
        enc.encode(fake(1, 3, 2048, 2056))
    with pytest.raises(_lib.RegionEHipError, match="maximum"):
        qdec.decode(fake(1, 16, 1, 513, 8))
    with pytest.raises(_lib.RegionEHipError, match="maximum"):
        qenc.encode(fake(1, 3, 1, 4104, 8))
    assert dec.attention == enc.attention == qdec.attention == qenc.attention == "auto"


def test_vae_attention_argument_checks_without_a_device():
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()
    assert h.rgn_vae_attention_bf16(None, P, P, None, P, 10, 10, 512, 0.05, None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, None, 10, 10, 512, 0.05, None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 2, 10, 512, 0.05, None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 10, 2, 512, 0.05, None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 10, 10, 512, 0.0, None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 10, 10, 512, float("nan"), None) == -1
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 10, 10, 256, 0.05, None) == -2 and "384 or 512" in msg()
    assert h.rgn_vae_attention_bf16(P + 2, P, P, None, P, 10, 10, 512, 0.05, None) == -2 and "aligned" in msg()
    assert h.rgn_vae_attention_bf16(P, P, P, P + 2, P, 10, 10, 384, 0.05, None) == -2 and "aligned" in msg()
    assert h.rgn_vae_attention_bf16(P, P, P, None, P, 50000, 50000, 512, 0.05, None) == -2 and "too large" in msg()
