"""The numpy model of the image kernels (tests/image_model.py) against the host code it restates - Pillow's resize, the Qwen2-VL image
processor, torch's bf16 arithmetic - bit for bit, and every named defect shown to change the output on a listed input.  No GPU."""
import numpy as np
import pytest
import torch

import image_model as M
from regione_amd import image_ops

# (in_h, in_w) -> (out_h, out_w): down, up, one unchanged dimension, a 49-tap row, mixed up / down, down to one pixel
RESIZE_SHAPES = [((37, 53), (16, 24)), ((48, 40), (112, 84)), ((61, 47), (61, 32)), ((200, 300), (64, 96)), ((33, 33), (96, 17)),
                 ((200, 8), (25, 8)), ((9, 9), (1, 1))]
FILTERS = ("lanczos", "bicubic")


def image(h, w, seed=0):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def edges(h, w):
    """Flat 0 / 255 regions with sharp edges: overshoot clips, exact ties at .5 and borders all occur."""
    a = np.zeros((h, w, 3), np.uint8)
    a[h // 3:, w // 4:] = 255
    a[:, ::5, 1] = 255
    a[::3, :, 2] = 128
    return a


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_model_resize_equals_pillow_byte_for_byte(shape, filt):
    Image = pytest.importorskip("PIL.Image")
    (ih, iw), (oh, ow) = shape
    for src in (image(ih, iw), edges(ih, iw)):
        want = np.asarray(Image.fromarray(src).resize((ow, oh), getattr(Image.Resampling, filt.upper())))
        got = M.resize(src, oh, ow, filt)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert int((got != want).sum()) == 0


@pytest.mark.parametrize("filt", FILTERS)
def test_product_table_equals_the_model_table(filt):
    """regione_amd.image_ops.resample_table (what the kernel is driven by) against the model's coefficients, every size pair of the shapes."""
    for (ih, iw), (oh, ow) in RESIZE_SHAPES + [((1365, 2048), (832, 1248))]:
        for n_in, n_out in ((iw, ow), (ih, oh)):
            b, w, k = image_ops.resample_table(n_in, n_out, filt)
            mb, mw, mk = M.coeffs(n_in, n_out, filt)
            assert k == mk and b.dtype == np.int32 and w.dtype == np.int32
            assert np.array_equal(b, mb) and np.array_equal(w, mw)
            assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k).all()
    rng = np.random.default_rng(5)                                                                    # and seeded size pairs, both directions
    for n_in, n_out in [tuple(int(v) for v in rng.integers(1, 500, 2)) for _ in range(40)] + [(1, 1), (1, 50), (50, 1), (999, 1000)]:
        b, w, k = image_ops.resample_table(n_in, n_out, filt)
        mb, mw, mk = M.coeffs(n_in, n_out, filt)
        assert k == mk and np.array_equal(b, mb) and np.array_equal(w, mw), (n_in, n_out)
    assert image_ops.resample_table(53, 24, filt) is image_ops.resample_table(53, 24, filt)          # cached
    assert image_ops.resample_table(200, 25, "lanczos")[2] == 49


def test_table_refuses_unknown_filters():
    from regione_amd._lib import RegionEHipError
    with pytest.raises(RegionEHipError, match="bilinear"):
        image_ops.resample_table(10, 5, "bilinear")


def test_vae_table_is_the_host_expression():
    want = (2.0 * (torch.arange(256, dtype=torch.float32) / 255.0) - 1.0).to(torch.bfloat16)
    assert np.array_equal(M.vae_table(), want.view(torch.int16).numpy().view(np.uint16))
    assert torch.equal(image_ops.vae_table(), want)
    # and that expression is what the host computes from an image: numpy's fp32 division, torch's 2 x - 1, the cast to the VAE's dtype
    src = image(24, 40)
    host = (2.0 * torch.from_numpy(src.astype(np.float32) / 255.0).permute(2, 0, 1)[None] - 1.0).to(torch.bfloat16)
    assert np.array_equal(M.to_vae_input(src), host.view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize("hw", [(56, 84), (84, 56)])
def test_model_patch_rows_equal_the_processor_bit_for_bit(hw):
    Image = pytest.importorskip("PIL.Image")
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    proc = mod.Qwen2VLImageProcessorPil()
    src = image(*hw, seed=7)
    out = proc(images=[Image.fromarray(src)], return_tensors="np")
    want = np.asarray(out["pixel_values"])
    assert out["image_grid_thw"].tolist() == [[1, hw[0] // 14, hw[1] // 14]]
    got = M.patch_rows(src)
    assert got.dtype == np.float32 and got.shape == want.shape == ((hw[0] // 14) * (hw[1] // 14), 1176)
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.array_equal(image_ops.patch_table().numpy().view(np.uint32), M.patch_table().view(np.uint32))
    assert tuple(proc.image_mean) == image_ops.OPENAI_CLIP_MEAN and tuple(proc.image_std) == image_ops.OPENAI_CLIP_STD


def test_processor_resizes_with_the_modelled_bicubic():
    """A size that is no multiple of 28: the processor's own smart_resize + bicubic resize, then its rows, equal the model's."""
    Image = pytest.importorskip("PIL.Image")
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    src = image(72, 96, seed=3)
    want = np.asarray(mod.Qwen2VLImageProcessorPil()(images=[Image.fromarray(src)], return_tensors="np")["pixel_values"])
    h, w = M.smart_resize(72, 96)
    assert (h, w) != (72, 96)
    assert np.array_equal(M.patch_rows(M.resize(src, h, w, "bicubic")).view(np.uint32), want.view(np.uint32))


def test_smart_resize_equals_transformers_over_a_grid():
    mod = pytest.importorskip("transformers.models.qwen2_vl.image_processing_pil_qwen2_vl")
    sizes = [1, 2, 13, 14, 27, 28, 29, 41, 42, 43, 55, 56, 57, 96, 100, 384, 1000, 1024, 1365, 2048, 4000]
    n = 0
    for h in sizes:
        for w in sizes:
            if max(h, w) / min(h, w) > 200:
                with pytest.raises(ValueError):
                    image_ops.smart_resize(h, w)
                continue
            for kw in ({}, {"min_pixels": 4 * 28 * 28, "max_pixels": 384 * 384}):
                want = mod.smart_resize(h, w, **kw)
                assert image_ops.smart_resize(h, w, **kw) == want == M.smart_resize(h, w, **kw)
                n += 1
    assert n > 500
    assert image_ops.HipImageOps.smart_resize(100, 100) == mod.smart_resize(100, 100)


def test_unit_u8_equals_torch_and_numpy_over_every_bf16_pattern():
    bits = M.all_bf16_image()
    x = torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)[None]                          # [1, 3, 160, 136]
    host = (x * 0.5 + 0.5).clamp(0, 1)
    host = (host.permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8")[0]
    assert np.array_equal(M.unit_u8(bits).transpose(1, 2, 0), host)
    assert M.unit_u8(np.array([0x7F80, 0xFF80], np.uint16)).tolist() == [255, 0]                          # +inf, -inf: what clamp makes of them


# ---- every named defect is visible on a listed input ------------------------------------------------------------------------------------
def _resize_outputs(defect):
    for (ih, iw), (oh, ow) in RESIZE_SHAPES:
        for filt in FILTERS:
            for src in (image(ih, iw), edges(ih, iw)):
                yield M.resize(src, oh, ow, filt), M.resize(src, oh, ow, filt, defect)


@pytest.mark.parametrize("defect", M.RESAMPLE_DEFECTS)
def test_every_resampler_defect_changes_a_listed_output(defect):
    assert any(not np.array_equal(good, bad) for good, bad in _resize_outputs(defect)), defect


def test_reciprocal_multiply_changes_the_vae_table():
    assert int((M.vae_table() != M.vae_table("reciprocal_multiply")).sum()) > 0


def test_swapped_temporal_and_channel_order_changes_the_patch_rows():
    for hw in ((56, 84), (84, 56)):
        src = image(*hw, seed=7)
        assert not np.array_equal(M.patch_rows(src), M.patch_rows(src, "temporal_channel_swapped"))


def test_round_half_up_changes_the_u8_map():
    bits = M.all_bf16_image()
    assert int((M.unit_u8(bits) != M.unit_u8(bits, "round_half_up")).sum()) > 0


def test_the_defect_list_is_covered():
    assert set(M.DEFECTS) == set(M.RESAMPLE_DEFECTS) | {"reciprocal_multiply", "temporal_channel_swapped", "round_half_up"}
