"""A FLUX.1-Kontext host stand-in with GENUINE transformers text encoders (tiny CLIPTextModel / T5EncoderModel) and a toy tokenizer:
its `encode_prompt` restates diffusers' FluxKontextPipeline.encode_prompt / `_get_clip_prompt_embeds` / `_get_t5_prompt_embeds` (the calls
the reference makes at FluxKontext/inplace.py:185-211), everything else is the stand-in of tests/host_standins.py.  Test infrastructure only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_standins as HS  # noqa: E402

VOCAB, BOS, EOS = 1000, 998, 999             # EOS is the largest id, as in CLIP's vocabulary (eos_token_id == 2: argmax picks it)


class ToyTokenizer:
    """Words -> ids by a fixed hash; `padding="max_length"` pads (and truncates) like the HF tokenizers' `input_ids`."""

    def __init__(self, clip: bool, model_max_length: int):
        self.clip, self.model_max_length = clip, model_max_length

    def _ids(self, text):
        ids = [3 + sum(ord(c) * (i + 1) for i, c in enumerate(w)) % (VOCAB - 10) for w in text.split()]
        return [BOS] + ids + [EOS] if self.clip else ids + [1]

    def __call__(self, prompt, padding="max_length", max_length=None, truncation=True, return_tensors="pt", **kw):
        n = max_length or self.model_max_length
        rows = []
        for p in prompt:
            ids = self._ids(p)
            if truncation and len(ids) > n:
                ids = ids[: n - 1] + ids[-1:]
            if padding == "max_length":
                ids = ids + [EOS if self.clip else 0] * (n - len(ids))
            rows.append(ids)

        class Out:
            input_ids = torch.tensor(rows, dtype=torch.int64)
        return Out


def tiny_text_encoders(clip_kw=None, t5_kw=None, dtype=torch.bfloat16):
    """(CLIPTextModel, T5EncoderModel) of the widths the flux stub trunk takes: pooled 64, context 256."""
    from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    c = dict(vocab_size=VOCAB, hidden_size=64, intermediate_size=256, num_hidden_layers=2, num_attention_heads=1, max_position_embeddings=77,
             bos_token_id=BOS, eos_token_id=2, pad_token_id=EOS)
    c.update(clip_kw or {})
    t = dict(vocab_size=VOCAB, d_model=256, d_kv=64, d_ff=512, num_layers=2, num_heads=4, feed_forward_proj="gated-gelu", is_encoder_decoder=False)
    t.update(t5_kw or {})
    torch.manual_seed(21)
    clip = CLIPTextModel(CLIPTextConfig(**c)).eval().to(dtype)
    t5 = T5EncoderModel(T5Config(**t)).eval().to(dtype)
    return clip, t5


class FluxKontextPipeline(HS.FluxKontextPipeline):          # the adapter dispatches on the class NAME, like the reference
    tokenizer_max_length = 77

    def __init__(self, trunk, text_encoder, text_encoder_2):
        super().__init__(trunk)
        self.text_encoder, self.text_encoder_2 = text_encoder, text_encoder_2
        self.tokenizer, self.tokenizer_2 = ToyTokenizer(True, 77), ToyTokenizer(False, 512)
        self.encoded = []

    def _get_t5_prompt_embeds(self, prompt=None, num_images_per_prompt=1, max_sequence_length=512, device=None, dtype=None):
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        text_input_ids = self.tokenizer_2(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                                          return_length=False, return_overflowing_tokens=False, return_tensors="pt").input_ids
        prompt_embeds = self.text_encoder_2(text_input_ids.to(device), output_hidden_states=False)[0]
        dtype = self.text_encoder_2.dtype
        prompt_embeds = prompt_embeds.to(dtype=dtype, device=device)
        _, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
        return prompt_embeds.view(batch_size * num_images_per_prompt, seq_len, -1)

    def _get_clip_prompt_embeds(self, prompt, num_images_per_prompt=1, device=None):
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        text_input_ids = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer_max_length, truncation=True,
                                        return_overflowing_tokens=False, return_length=False, return_tensors="pt").input_ids
        prompt_embeds = self.text_encoder(text_input_ids.to(device), output_hidden_states=False)
        prompt_embeds = prompt_embeds.pooler_output
        prompt_embeds = prompt_embeds.to(dtype=self.text_encoder.dtype, device=device)
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt)
        return prompt_embeds.view(batch_size * num_images_per_prompt, -1)

    def encode_prompt(self, prompt=None, prompt_2=None, prompt_embeds=None, pooled_prompt_embeds=None, device=None,
                      num_images_per_prompt=1, max_sequence_length=512, lora_scale=None):
        self.calls.append(("encode_prompt", prompt))
        prompt = [prompt] if isinstance(prompt, str) else prompt
        if prompt_embeds is None:
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            pooled_prompt_embeds = self._get_clip_prompt_embeds(prompt=prompt, device=device, num_images_per_prompt=num_images_per_prompt)
            prompt_embeds = self._get_t5_prompt_embeds(prompt=prompt_2, num_images_per_prompt=num_images_per_prompt,
                                                       max_sequence_length=max_sequence_length, device=device)
        dtype = self.text_encoder.dtype if self.text_encoder is not None else self.transformer.dtype
        text_ids = torch.zeros(prompt_embeds.shape[1], 3).to(device=device, dtype=dtype)
        self.encoded.append((prompt_embeds, pooled_prompt_embeds))
        return prompt_embeds, pooled_prompt_embeds, text_ids
