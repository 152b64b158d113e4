"""Host stand-ins for the image work around a hosted edit, with call counters.  Test infrastructure only.

  VaeImageProcessor   [EXT] diffusers' `VaeImageProcessor`, the PIL path restated (diffusers is not installable in this image):
                      resize = `PIL.Image.resize((w, h), LANCZOS)`; preprocess = resize, `np.array(im).astype(float32) / 255.0`, stack,
                      NHWC -> NCHW, `2.0 * x - 1.0`; postprocess = `(x * 0.5 + 0.5).clamp(0, 1)`, `.cpu().permute(0, 2, 3, 1).float().numpy()`,
                      `(a * 255).round().astype("uint8")`, `Image.fromarray`.  Tensor images take the toy path of tests/host_standins.py.
  QwenProcessor       the toy processor of tests/host_qwen_text_pipeline.py around a GENUINE `Qwen2VLImageProcessorPil`, called the way
                      transformers' ProcessorMixin calls it: `self.image_processor(images=images, return_tensors="pt")`.
"""
import collections
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402


class _Config(dict):
    __getattr__ = dict.__getitem__


def _is_pil(x):
    import PIL.Image
    return isinstance(x, PIL.Image.Image)


class VaeImageProcessor(HS.ImageProcessor):
    def __init__(self, vae_scale_factor=8, **overrides):
        self.config = _Config(do_resize=True, vae_scale_factor=vae_scale_factor, vae_latent_channels=16, resample="lanczos",
                              reducing_gap=None, do_normalize=True, do_binarize=False, do_convert_rgb=False, do_convert_grayscale=False)
        self.config.update(overrides)
        self.calls = collections.Counter()

    def get_default_height_width(self, image, height=None, width=None):
        if height is None:
            height = image.height if _is_pil(image) else image.shape[-2]
        if width is None:
            width = image.width if _is_pil(image) else image.shape[-1]
        f = self.config.vae_scale_factor
        return height - height % f, width - width % f

    def resize(self, image, height, width):
        self.calls["resize"] += 1
        if _is_pil(image):
            import PIL.Image
            return image.resize((width, height), resample=getattr(PIL.Image.Resampling, self.config.resample.upper()))
        return super().resize(image, height, width)

    def preprocess(self, image, height=None, width=None):
        self.calls["preprocess"] += 1
        images = image if isinstance(image, list) else [image]
        if not all(_is_pil(i) for i in images):
            return super().preprocess(image, height, width)
        height, width = self.get_default_height_width(images[0], height, width)
        import PIL.Image
        images = [i.resize((width, height), resample=getattr(PIL.Image.Resampling, self.config.resample.upper())) for i in images]
        arr = np.stack([np.array(i).astype(np.float32) / 255.0 for i in images], axis=0)
        x = torch.from_numpy(arr.transpose(0, 3, 1, 2))
        return 2.0 * x - 1.0

    def postprocess(self, image, output_type="pil"):
        self.calls["postprocess"] += 1
        x = (image * 0.5 + 0.5).clamp(0, 1)
        if output_type == "pt":
            return x
        a = x.cpu().permute(0, 2, 3, 1).float().numpy()
        if output_type == "np":
            return a
        import PIL.Image
        return [PIL.Image.fromarray(i) for i in (a * 255).round().astype("uint8")]


def counting_qwen2vl_image_processor(**kw):
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil

    class Counting(Qwen2VLImageProcessorPil):
        def preprocess(self, images, **kwargs):
            self.calls["preprocess"] += 1
            return super().preprocess(images, **kwargs)
    p = Counting(**kw)
    p.calls = collections.Counter()
    return p


class QwenProcessor(HQ.ToyProcessor):
    def __init__(self, **kw):
        self.image_processor = counting_qwen2vl_image_processor(**kw)
        self.seen = []                                      # (pixel_values, image_grid_thw) of every call with images

    def __call__(self, text, images=None, padding=True, return_tensors="pt"):
        images = [] if images is None else (list(images) if isinstance(images, (list, tuple)) else [images])
        pv, grids = None, []
        if images:
            feats = self.image_processor(images=images, return_tensors=return_tensors)
            pv, grids = feats["pixel_values"], [tuple(int(v) for v in g) for g in feats["image_grid_thw"].tolist()]
            self.seen.append((pv, feats["image_grid_thw"]))
        rows = []
        for t in text:
            ids, k = list(HQ.PREFIX), 0
            for w in t.split():
                if w == "<image>":
                    _, h, wd = grids[k]
                    ids += [HQ.VISION_START] + [HQ.IMAGE] * (h * wd // HQ.MERGE ** 2) + [HQ.VISION_END]
                    k += 1
                else:
                    ids += HQ.words_to_ids(w)
            assert k == len(images), "one <image> mark per image"
            rows.append(ids + HQ.SUFFIX)
        L = max(map(len, rows))
        out = HQ.ModelInputs(input_ids=torch.tensor([r + [HQ.PAD] * (L - len(r)) for r in rows], dtype=torch.int64),
                             attention_mask=torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows], dtype=torch.int64))
        assert len(rows) == 1 or pv is None, "one prompt per call with images"
        out["pixel_values"] = pv
        out["image_grid_thw"] = torch.as_tensor(feats["image_grid_thw"], dtype=torch.int64) if images else None
        return out
