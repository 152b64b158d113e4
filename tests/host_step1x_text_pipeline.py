"""Step1X-Edit host stand-ins with a GENUINE transformers prompt encoder (the tiny Qwen2_5_VLForConditionalGeneration of
tests/host_qwen_text_pipeline.py) and its toy processor: `encode_prompt` restates the public Step1X-Edit embedder (template prefix, the
reference image, the caption; `hidden_states[-1]`; the prefix rows dropped; zero padding to a fixed length with a mask), for v1p2 as the
record its `__call__` reads; a `ToyThinker` with the three calls of the fork's Step1XEditThinker whose text comes from
`model.generate(**inputs, max_new_tokens=8)`.  Everything else is the stand-in of tests/host_standins.py.  Test infrastructure only."""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402

DROP = len(HQ.PREFIX)            # the template's system part (217 tokens in the real embedder)
MAX_LENGTH = 40                  # the fixed length the embeddings are padded to (640 in the real embedder)
THINK_TOKENS = 8


class _QwenPrompt:
    """What both stand-ins add to the ones of tests/host_standins.py: the prompt encoder, the processor, and what they were handed."""

    DROP, MAX_LENGTH = DROP, MAX_LENGTH                # a subclass at another scale (tools/step1x_vlm_bench.py) sets its own

    def __init__(self, trunk, text_encoder):
        super().__init__(trunk)
        object.__setattr__(trunk, "connector", HS.ToyConnector().to(torch.bfloat16))     # the trunk class's own `connector` is a method
        self.text_encoder, self.processor = text_encoder, HQ.ToyProcessor()
        self.encoded, self.images_in = [], []              # (model inputs, embeddings, mask) per encode_prompt; encode_image's images

    def encode_image(self, image, width, height, *rest):
        self.images_in.append(image)
        if image.dim() == 3:                               # an edited image going round again (the real pipelines take PIL images)
            image = image.unsqueeze(0)
        return super().encode_image(image, width, height, *rest)

    def _qwen_embeds(self, ref_image, prompt, device):
        enc = self.text_encoder
        mi = self.processor(text=["<image> " + (prompt or "")], images=[ref_image], padding=True, return_tensors="pt").to(device)
        out = enc(input_ids=mi.input_ids, attention_mask=mi.attention_mask, pixel_values=mi.pixel_values,
                  image_grid_thw=mi.image_grid_thw, output_hidden_states=True)
        emb = out.hidden_states[-1]
        n = min(self.MAX_LENGTH, emb.shape[1] - self.DROP)
        embs = torch.zeros(1, self.MAX_LENGTH, emb.shape[2], dtype=torch.bfloat16, device=emb.device)
        masks = torch.zeros(1, self.MAX_LENGTH, dtype=torch.long, device=emb.device)
        embs[0, :n] = emb[0, self.DROP:][:self.MAX_LENGTH]
        masks[0, :n] = 1
        embs, masks = embs.to(device), masks.to(device)
        self.encoded.append((mi, embs, masks))
        return embs, masks


class Step1XEditPipeline(_QwenPrompt, HS.Step1XEditPipeline):           # the adapter dispatches on the class NAME, like the reference
    def encode_prompt(self, ref_image=None, prompt=None, prompt_embeds=None, prompt_embeds_mask=None, device=None,
                      num_images_per_prompt=1):
        self.calls.append(("encode_prompt", prompt))
        if prompt_embeds is None:
            prompt_embeds, prompt_embeds_mask = self._qwen_embeds(ref_image, prompt, device or self._execution_device)
        return prompt_embeds, prompt_embeds_mask, torch.zeros(prompt_embeds.shape[1], 3)


class Step1XEditPipelineV1P2(_QwenPrompt, HS.Step1XEditPipelineV1P2):
    def encode_prompt(self, ref_image=None, prompt=None, device=None, num_images_per_prompt=1):
        self.calls.append(("encode_prompt", prompt))
        r = self.Record()
        r.embedding, r.mask = self._qwen_embeds(ref_image, prompt, device or self._execution_device)
        r.txt_ids = torch.zeros(r.embedding.shape[1], 3)
        r.text_embeds, r.text_masks = HS._pseudo((prompt or "") + "t", 1, self.MAX_LENGTH, 32), r.mask.to(torch.bfloat16)
        return r


class ToyThinker:
    """`Step1XEditThinker(model, processor)`: `think` shows the image and the prompt to `model.generate`, `reflect` both images; the new
    ids, spelled out, are the text.  `verdicts` scripts `format_text` ((success, refine_prompt) per call; (True, None) once it runs
    out), `scores` the best_info of `reflect` ((score1 list, score2 list) per call; ([1], [1]) once it runs out).  `said` keeps every
    (model inputs, generated ids, text)."""

    new_tokens = THINK_TOKENS

    def __init__(self, model, processor, verdicts=(), scores=()):
        self.model, self.processor, self.verdicts, self.scores, self.said = model, processor, list(verdicts), list(scores), []

    def _say(self, images, text):
        images = [i.detach().float().cpu() for i in images]       # an edited image comes back on the device (the real thinker takes PIL)
        mi = self.processor(text=[text], images=images, padding=True, return_tensors="pt").to(self.model.device)
        ids = self.model.generate(**mi, max_new_tokens=self.new_tokens)
        words = " ".join(f"w{int(i)}" for i in ids[0, mi.input_ids.shape[1]:])
        self.said.append((mi, ids, words))
        return words

    def think(self, image, prompt):
        return self._say([image], "<image> " + prompt)

    def reflect(self, ref_image, image, prompt):
        text = self._say([ref_image, image], "<image> <image> " + prompt)
        s1, s2 = self.scores.pop(0) if self.scores else ([1], [1])
        return text, {"score1": {"score": list(s1)}, "score2": {"score": list(s2)}}

    def format_text(self, text):
        return self.verdicts.pop(0) if self.verdicts else (True, None)


def install_thinker_class(monkeypatch, cls):
    """`diffusers.pipelines.step1x_edit.pipeline_step1x_edit_thinker.Step1XEditThinker` is `cls` for the length of a test (the fork of
    diffusers that has it is not installed): the module path `thinker_for` imports, every level of it, put into sys.modules."""
    path = "diffusers.pipelines.step1x_edit.pipeline_step1x_edit_thinker".split(".")
    for i in range(1, len(path) + 1):
        name = ".".join(path[:i])
        mod = types.ModuleType(name)
        mod.__path__ = []
        monkeypatch.setitem(sys.modules, name, mod)
    sys.modules[".".join(path)].Step1XEditThinker = cls
