"""The rgn_image_* kernels (csrc/image.hip) through regione_amd.image_ops.HipImageOps against the numpy model of tests/image_model.py, which
tests/test_image_model.py pins to Pillow, the Qwen2-VL processor and torch bit for bit.  Every comparison is equality of bits.  Shapes: the
resize list of the model test (down, up, an unchanged dimension, a 49-tap row, one output pixel; row lengths that are and are not a
multiple of 4 bytes: the y pass's dword and byte paths); H * W a multiple of 8 / of 4 and not (the vector and the scalar forms of the two
layout kernels); every image larger than one 256-thread block's share."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import image_model as M  # noqa: E402
from test_image_model import FILTERS, RESIZE_SHAPES, edges, image  # noqa: E402
from regione_amd import _lib, image_ops, ops  # noqa: E402
from regione_amd._lib import RegionEHipError  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def io():
    return image_ops.HipImageOps("cuda")


def _bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _bf16_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16).cuda()


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_equals_the_model_byte_for_byte(io, shape, filt):
    (ih, iw), (oh, ow) = shape
    for src in (image(ih, iw), edges(ih, iw)):
        dev = io.upload(src)
        got = io.resize(dev, oh, ow, filt)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, 3) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), M.resize(src, oh, ow, filt))
        assert torch.equal(io.resize(dev, oh, ow, filt), got)                         # a repeated call is bit-identical
        assert np.array_equal(dev.cpu().numpy(), src)                                 # the source is read only


def test_resize_equals_pillow_on_a_pil_image(io):
    Image = pytest.importorskip("PIL.Image")
    pil = Image.fromarray(image(72, 96, seed=5))
    for filt in FILTERS:
        want = np.asarray(pil.resize((40, 56), getattr(Image.Resampling, filt.upper())))
        got = io.to_pil(io.resize(io.upload(pil), 56, 40, filt))
        assert got.mode == "RGB" and got.size == (40, 56) and np.array_equal(np.asarray(got), want)
    same = io.resize(io.upload(pil), 72, 96, "lanczos")                                # both passes skipped: a copy, as Image.resize
    assert np.array_equal(same.cpu().numpy(), np.asarray(pil))


def test_vae_input_is_exact_for_every_code_and_channel(io):
    rng = np.random.default_rng(0)
    src = np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(3)], axis=-1)      # every code in every channel
    got = io.to_vae_input(io.upload(src))
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, 3, 16, 16)
    assert np.array_equal(_bits(got), M.to_vae_input(src))
    host = (2.0 * torch.from_numpy(src.astype(np.float32) / 255.0).permute(2, 0, 1)[None] - 1.0).to(torch.bfloat16)
    assert torch.equal(got.cpu(), host)


@pytest.mark.parametrize("hw", [(24, 40), (37, 53), (72, 96), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_vae_input_equals_the_model(io, hw):
    src = image(*hw, seed=2)
    dev = io.upload(src)
    got = io.to_vae_input(dev)
    assert np.array_equal(_bits(got), M.to_vae_input(src))
    assert torch.equal(io.to_vae_input(dev), got)


@pytest.mark.parametrize("hw", [(56, 84), (84, 56), (28, 28)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_patch_rows_equal_the_model_in_both_modes(io, hw):
    src = image(*hw, seed=7)
    dev = io.upload(src)
    want = M.patch_rows(src)
    rows = io.to_patch_rows(dev)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == want.shape
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), want.view(np.uint32))
    Kp = ops.padded(1176, 64)
    pad = io.to_patch_rows(dev, out="padded_bf16", Kp=Kp)
    assert pad.dtype == torch.bfloat16 and tuple(pad.shape) == (want.shape[0], Kp)
    assert np.array_equal(_bits(pad), M.pad_rows_bf16(want, Kp))
    # the padded mode IS rgn_cast_pad_rows of the fp32 mode
    ref = torch.full((want.shape[0], Kp), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(_lib.lib().rgn_cast_pad_rows(rows.data_ptr(), ops.F32, rows.stride(0), ref.data_ptr(), rows.shape[0], 1176, Kp,
                                            torch.cuda.current_stream().cuda_stream), "rgn_cast_pad_rows")
    assert torch.equal(pad, ref)
    assert torch.equal(io.to_patch_rows(dev), rows) and torch.equal(io.to_patch_rows(dev, out="padded_bf16", Kp=Kp), pad)


def test_patch_rows_equal_the_processor(io):
    Image = pytest.importorskip("PIL.Image")
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    src = image(72, 96, seed=3)                                                        # resized by the processor: bicubic to smart_resize
    out = mod.Qwen2VLImageProcessorPil()(images=[Image.fromarray(src)], return_tensors="np")
    h, w = io.smart_resize(72, 96)
    rows = io.to_patch_rows(io.resize(io.upload(src), h, w, "bicubic"))
    assert out["image_grid_thw"].tolist() == [[1, h // 14, w // 14]]
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), np.asarray(out["pixel_values"]).view(np.uint32))


def _padded_image(bits_chw, C=8):
    """The decoder's padded pixel-major image holding bits_chw [3, H, W] in channels 0..2; border rows and the other channels carry a
    value that would be visible (0x4000 = 2.0 -> 255) if the kernel read them."""
    from regione_amd.vae import PaddedImage
    _, H, W = bits_chw.shape
    img = PaddedImage(H, W, C, "cuda")
    full = np.full((H + 2, W + 2, C), 0x4000, np.uint16)
    full[1:-1, 1:-1, :3] = bits_chw.transpose(1, 2, 0)
    img.t.copy_(_bf16_dev(full.reshape(-1, C)))
    return img


def test_bf16_to_u8_is_exact_over_every_finite_pattern_in_both_layouts(io):
    bits = M.all_bf16_image()                                                          # [3, 160, 136]
    want = M.unit_u8(bits).transpose(1, 2, 0)
    x = _bf16_dev(bits)[None]
    host = (x.cpu() * 0.5 + 0.5).clamp(0, 1)
    host = (host.permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8")[0]
    assert np.array_equal(want, host)
    got = io.to_uint8(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (160, 136, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    pad = _padded_image(bits)
    got_p = io.to_uint8(pad)
    assert np.array_equal(got_p.cpu().numpy(), want)
    assert torch.equal(io.to_uint8(x), got) and torch.equal(io.to_uint8(pad), got_p)


@pytest.mark.parametrize("hw", [(5, 7), (3, 3), (1, 1), (6, 10)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bf16_to_u8_tails_and_infinities(io, hw):
    """H * W not a multiple of 4 (the scalar NCHW form, the tail pixels of both layouts); the infinities clamp to 0 and 255."""
    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    bits = rng.choice(M.all_bf16_image().reshape(-1), size=(3, h, w)).astype(np.uint16)
    bits[0, 0, 0], bits[2, -1, -1] = 0x7F80, 0xFF80
    want = M.unit_u8(bits).transpose(1, 2, 0)
    assert want[0, 0, 0] == 255 and want[-1, -1, 2] == 0
    assert np.array_equal(io.to_uint8(_bf16_dev(bits)[None]).cpu().numpy(), want)
    assert np.array_equal(io.to_uint8(_padded_image(bits)).cpu().numpy(), want)


def test_uncovered_inputs_are_refused_by_name(io):
    Image = pytest.importorskip("PIL.Image")
    src = image(28, 28)
    dev = io.upload(src)
    for bad, why in ((Image.fromarray(src).convert("RGBA"), "RGBA"), (Image.fromarray(src).convert("L"), "'L'"),
                     (src.astype(np.float32), "float32"), (np.stack([src, src]), "no batches"), (src[:, :, :1], "no batches"),
                     ("a path", "str")):
        with pytest.raises(RegionEHipError, match=why):
            io.upload(bad)
    with pytest.raises(RegionEHipError, match="box"):
        io.resize(dev, 14, 14, "lanczos", box=(0, 0, 10, 10))
    with pytest.raises(RegionEHipError, match="reducing_gap"):
        io.resize(dev, 14, 14, "lanczos", reducing_gap=2.0)
    with pytest.raises(RegionEHipError, match="bilinear"):
        io.resize(dev, 14, 14, "bilinear")
    with pytest.raises(RegionEHipError, match="CPU tensor"):
        io.resize(torch.from_numpy(src), 14, 14)
    with pytest.raises(RegionEHipError, match="float32"):
        io.to_vae_input(dev.float())
    with pytest.raises(RegionEHipError, match="multiples of 28"):
        io.to_patch_rows(io.upload(image(30, 28)))
    with pytest.raises(RegionEHipError, match="out = 'fp16'"):
        io.to_patch_rows(dev, out="fp16")
    with pytest.raises(RegionEHipError, match="Kp = 1180"):
        io.to_patch_rows(dev, out="padded_bf16", Kp=1180)
    with pytest.raises(RegionEHipError, match="float32"):
        io.to_uint8(torch.zeros(1, 3, 8, 8, device="cuda"))
    with pytest.raises(RegionEHipError, match="no batches"):
        io.to_uint8(torch.zeros(2, 3, 8, 8, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(RegionEHipError, match="no CPU fallback"):
        image_ops.HipImageOps("cpu")
