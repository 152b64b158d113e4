"""Qwen-Image-Edit host stand-ins with a GENUINE transformers prompt encoder (a tiny Qwen2_5_VLForConditionalGeneration) and a toy
processor: `encode_prompt` / `_get_qwen_prompt_embeds` / `_extract_masked_hidden` restate diffusers' QwenImageEditPipeline (and ...Plus:
one `Picture k:` block per condition image), everything else is the stand-in of tests/host_standins.py.  diffusers is not installable in
this image, so the restatement is what the adapter's binding is tested against.  Test infrastructure only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_standins as HS  # noqa: E402

VOCAB = 1024
IMAGE, VIDEO, VISION_START, VISION_END, PAD = 1001, 1002, 1003, 1004, 1000
PREFIX = [1010, 1011, 1012, 1013, 1014, 1015, 1016, 1017]          # the chat template's system part: dropped from the embeddings
SUFFIX = [1018, 1019, 1020]                                         # <|im_end|> <|im_start|> assistant
PATCH, MERGE = 14, 2


def tiny_qwen25vl(text_kw=None, dtype=torch.bfloat16, layers=2, seed=31):
    """A genuine Qwen2_5_VLForConditionalGeneration: text model hidden 256 = 2 heads x 128, 1 KV head, `mrope_section` [16, 24, 24];
    a tiny vision tower with out_hidden_size 256 (patch 14, merge 2, window attention in block 0, full attention in block 1)."""
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    t = dict(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=layers, num_attention_heads=2, num_key_value_heads=1,
             rms_norm_eps=1e-6, max_position_embeddings=4096, rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[16, 24, 24]),
             tie_word_embeddings=False, bos_token_id=None, eos_token_id=None, pad_token_id=None)
    t.update(text_kw or {})
    v = dict(depth=2, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=256, patch_size=PATCH, spatial_merge_size=MERGE,
             temporal_patch_size=2, window_size=56, fullatt_block_indexes=[1], in_channels=3)
    cfg = Qwen2_5_VLConfig(text_config=t, vision_config=v, image_token_id=IMAGE, video_token_id=VIDEO, vision_start_token_id=VISION_START,
                           vision_end_token_id=VISION_END, bos_token_id=None, eos_token_id=None, pad_token_id=None)
    torch.manual_seed(seed)
    return Qwen2_5_VLForConditionalGeneration(cfg).eval().to(dtype)


def words_to_ids(text):
    return [3 + sum(ord(c) * (i + 1) for i, c in enumerate(w)) % 990 for w in text.split()]


class ModelInputs(dict):
    __getattr__ = dict.__getitem__

    def to(self, device):
        return ModelInputs({k: None if v is None else v.to(device) for k, v in self.items()})


class ToyProcessor:
    """`processor(text=[...], images=[...], padding=True, return_tensors="pt")`: per row the template prefix, one
    vision_start / image-token run / vision_end per `<image>` mark, the instruction ids and the template suffix; right padding;
    `pixel_values` [n_patches, 1176] and `image_grid_thw` [n_images, 3] (image k is resized to 56 x 56 or 56 x 84 pixels: 4 or 6 tokens).
    The same images go to every row (their patches and grids are repeated per row, so placeholders and features match)."""

    GRIDS = ((4, 4), (4, 6))

    def pixels(self, img, k):
        h, w = self.GRIDS[k % 2]
        x = torch.nn.functional.interpolate(img.reshape(1, 3, *img.shape[-2:]).float(), size=(h * PATCH, w * PATCH), mode="bilinear")[0]
        p = x.unfold(1, PATCH, PATCH).unfold(2, PATCH, PATCH).permute(1, 2, 0, 3, 4).reshape(h * w, 3, 1, PATCH, PATCH)
        return p.expand(-1, -1, 2, -1, -1).reshape(h * w, 3 * 2 * PATCH * PATCH), (1, h, w)

    def __call__(self, text, images=None, padding=True, return_tensors="pt"):
        images = [] if images is None else (list(images) if isinstance(images, (list, tuple)) else [images])
        pv, grids = [], []
        for k, img in enumerate(images):
            p, g = self.pixels(img, k)
            pv.append(p)
            grids.append(g)
        rows = []
        for t in text:
            ids, k = list(PREFIX), 0
            for w in t.split():
                if w == "<image>":
                    _, h, wd = grids[k]
                    ids += [VISION_START] + [IMAGE] * (h * wd // MERGE ** 2) + [VISION_END]
                    k += 1
                else:
                    ids += words_to_ids(w)
            assert k == len(images), "one <image> mark per image"
            rows.append(ids + SUFFIX)
        L = max(map(len, rows))
        out = ModelInputs(input_ids=torch.tensor([r + [PAD] * (L - len(r)) for r in rows], dtype=torch.int64),
                          attention_mask=torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows], dtype=torch.int64))
        out["pixel_values"] = torch.cat(pv * len(rows)) if pv else None           # one copy of the images per row
        out["image_grid_thw"] = torch.tensor(grids * len(rows), dtype=torch.int64) if grids else None
        return out


class QwenImageEditPipeline(HS.QwenImageEditPipeline):     # the adapter dispatches on the class NAME, like the reference
    prompt_template_encode = "{}"
    prompt_template_encode_start_idx = len(PREFIX)
    PLUS = False

    def __init__(self, trunk, text_encoder):
        super().__init__(trunk)
        self.text_encoder, self.processor = text_encoder, ToyProcessor()
        self.encoded, self.last_image = [], None

    def _extract_masked_hidden(self, hidden_states, mask):
        bool_mask = mask.bool()
        valid_lengths = bool_mask.sum(dim=1)
        selected = hidden_states[bool_mask]
        return torch.split(selected, valid_lengths.tolist(), dim=0)

    def _get_qwen_prompt_embeds(self, prompt=None, image=None, device=None, dtype=None):
        device = device or self._execution_device
        dtype = dtype or self.text_encoder.dtype
        prompt = [prompt] if isinstance(prompt, str) else prompt
        if self.PLUS:                                       # "Picture k: <|vision_start|><|image_pad|><|vision_end|>" per image
            images = image if isinstance(image, list) else ([] if image is None else [image])
            base = "".join(f"Picture {i + 1}: <image> " for i in range(len(images)))
        else:
            images = None if image is None else [image]
            base = "" if image is None else "<image> "
        txt = [self.prompt_template_encode.format(base + e) for e in prompt]
        drop_idx = self.prompt_template_encode_start_idx
        model_inputs = self.processor(text=txt, images=images, padding=True, return_tensors="pt").to(device)
        outputs = self.text_encoder(input_ids=model_inputs.input_ids, attention_mask=model_inputs.attention_mask,
                                    pixel_values=model_inputs.pixel_values, image_grid_thw=model_inputs.image_grid_thw,
                                    output_hidden_states=True)
        hidden_states = outputs.hidden_states[-1]
        split_hidden_states = self._extract_masked_hidden(hidden_states, model_inputs.attention_mask)
        split_hidden_states = [e[drop_idx:] for e in split_hidden_states]
        attn_mask_list = [torch.ones(e.size(0), dtype=torch.long, device=e.device) for e in split_hidden_states]
        max_seq_len = max([e.size(0) for e in split_hidden_states])
        prompt_embeds = torch.stack([torch.cat([u, u.new_zeros(max_seq_len - u.size(0), u.size(1))]) for u in split_hidden_states])
        encoder_attention_mask = torch.stack([torch.cat([u, u.new_zeros(max_seq_len - u.size(0))]) for u in attn_mask_list])
        return prompt_embeds.to(dtype=dtype, device=device), encoder_attention_mask.to(device)

    def encode_prompt(self, prompt=None, image=None, device=None, num_images_per_prompt=1, prompt_embeds=None, prompt_embeds_mask=None,
                      max_sequence_length=1024):
        self.calls.append(("encode_prompt", prompt, len(image) if isinstance(image, list) else 1))
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt) if prompt_embeds is None else prompt_embeds.shape[0]
        if prompt_embeds is None:
            self.last_image = image
            prompt_embeds, prompt_embeds_mask = self._get_qwen_prompt_embeds(prompt, image, device)
            self.encoded.append((prompt_embeds, prompt_embeds_mask))
        _, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len, -1)
        prompt_embeds_mask = prompt_embeds_mask.repeat(1, num_images_per_prompt, 1).view(batch_size * num_images_per_prompt, seq_len)
        return prompt_embeds, prompt_embeds_mask


class QwenImageEditPlusPipeline(QwenImageEditPipeline):
    PLUS = True
