"""Step1X-Edit v1p2's thinking / reflection retry loop around the hosted edit (Step1XEditV1P2/inplace.py:192-212, :470-543): the thinker
a host pipeline brings (`thinker_for`), and the loop itself in plain Python (`reflection_loop`: no tensor in it, the CPU suite drives it
with a scripted thinker).  The last module of the package: `Retry` below is what hosted.py's `_hosted_step1x` runs, through the slot
hosted.py keeps for it (hosted.py imports nothing from here).  The text a thinker produces comes from `generate` of the object it was built on - the adopted
HIP prompt encoder when there is one."""
from __future__ import annotations

import contextlib
import time
import warnings

from .components import _hip_qwen_image_processor, _host_name, _step1x_text_sampling_default, hip_qwen_text_encoder_for
from .hosted import _STEP1X_RETRY

THINKER_MODULE = "diffusers.pipelines.step1x_edit.pipeline_step1x_edit_thinker"
SUCCESS_MARK = "<#Success>"                                                        # Step1XEditV1P2/inplace.py:506


def _thinker_class():
    """`Step1XEditThinker` of the Step1X-Edit fork of diffusers (what Step1XEditV1P2/inplace.py:196 constructs), or None without it."""
    import importlib
    try:
        return getattr(importlib.import_module(THINKER_MODULE), "Step1XEditThinker", None)
    except ImportError:
        return None


def thinker_for(host, dev, switch: str = "enable_thinking_mode"):
    """The object whose `think(image, prompt) -> str`, `reflect(ref_image, image, prompt) -> (str, dict)` and
    `format_text(str) -> (bool, str | None)` the retry loop calls (Step1XEditV1P2/inplace.py:198, :471, :472):
    `host._regione_thinker` when the caller set one; else the fork's `Step1XEditThinker(model, host.processor)` when that class imports
    and the host has a Qwen2.5-VL `text_encoder` and a `processor` - `model` is the adopted HIP encoder, or, where its adoption was
    refused or opted out of, the host module with one warning that generation runs there.  A host with neither cannot think: the
    NotImplementedError names `switch`, the argument that asked."""
    own = getattr(host, "_regione_thinker", None)
    if own is not None:
        return own
    cls = _thinker_class()
    mod, proc = getattr(host, "text_encoder", None), getattr(host, "processor", None)
    if cls is None or proc is None or type(mod).__name__ != "Qwen2_5_VLForConditionalGeneration":
        raise NotImplementedError(f"{_host_name(host)}.__call__: {switch}=True (the VLM thinking / reflection retry loop, "
                                  "Step1XEditV1P2/inplace.py:192-212) is not hosted by the HIP loop; pass False")
    model = hip_qwen_text_encoder_for(host, dev, sampling_default=_step1x_text_sampling_default(host))
    if model is None:
        warnings.warn(f"{_host_name(host)}.__call__: the prompt encoder is not adopted - the thinker's generate runs on the host module",
                      RuntimeWarning, stacklevel=4)
        model = mod
    return cls(model, proc)


class TimedThinker:
    """A thinker whose `think` / `reflect` run inside `bind()` (a context manager per call) and add their wall-clock seconds to
    `seconds["think_s"]` / `seconds["reflect_s"]`; `sync()` runs before each reading of the clock."""

    def __init__(self, thinker, bind=contextlib.nullcontext, sync=lambda: None):
        self.thinker, self.bind, self.sync, self.seconds = thinker, bind, sync, {"think_s": 0.0, "reflect_s": 0.0}

    def _timed(self, key, fn, *args):
        self.sync()
        t = time.perf_counter()
        with self.bind():
            out = fn(*args)
        self.sync()
        self.seconds[key] += time.perf_counter() - t
        return out

    def think(self, image, prompt):
        return self._timed("think_s", self.thinker.think, image, prompt)

    def reflect(self, ref_image, image, prompt):
        return self._timed("reflect_s", self.thinker.reflect, ref_image, image, prompt)

    def format_text(self, text):
        return self.thinker.format_text(text)


class LoopResult:
    """What `reflection_loop` hands back: `images` (one per try under reflection, else the one attempt's image list), `final_images`,
    `think_info` / `best_info` (one entry per try under reflection), `reformat_prompt` (None unless thinking was on), `tries`."""

    def __init__(self, images, final_images, think_info, best_info, reformat_prompt, tries):
        self.images, self.final_images, self.think_info, self.best_info = images, final_images, think_info, best_info
        self.reformat_prompt, self.tries = reformat_prompt, tries


def best_index(think_info, best_info) -> int:
    """The try whose image is `final_images[0]` (Step1XEditV1P2/inplace.py:496-519): score = min(score1.score) * min(score2.score); a
    strictly larger score wins; on a tie an entry whose thinking text holds "<#Success>" beats one without, and with equal success
    status the later entry wins."""
    best, top, best_ok = 0, -1, False
    for i, info in enumerate(best_info):
        score = min(info["score1"]["score"]) * min(info["score2"]["score"])
        ok = SUCCESS_MARK in (think_info[i] if i < len(think_info) else "")
        if score > top:
            best, top, best_ok = i, score, ok
        elif score == top:
            if ok and not best_ok:
                best, best_ok = i, True
            elif ok == best_ok:
                best = i
    return best


def reflection_loop(edit_once, thinker, image, prompt, enable_thinking_mode, enable_reflection_mode, max_try_cnt=3) -> LoopResult:
    """Step1XEditV1P2/inplace.py:192-212 and :470-543 around `edit_once(image, prompt) -> images` (one hosted edit: what the reference
    runs from `encode_image` to `_output_process_image`; whatever else carries over between tries - width and height, the generator -
    is `edit_once`'s own state).  `thinker` is only touched when a switch is on."""
    try_cnt, success, reformat_prompt = 0, False, None
    thinking = bool(enable_reflection_mode or enable_thinking_mode)
    if thinking:                                                                   # :195-204
        reformat_prompt = thinker.think(image, prompt) if enable_thinking_mode else prompt
        prompt = reformat_prompt
        out_images, out_think_info, best_think_info = [], [], []
    else:                                                                          # :205-207
        max_try_cnt, out_images, out_think_info, best_think_info = 1, None, None, None
    original_image, original_prompt = image, prompt                               # :209-210
    tries = 0
    while not success and try_cnt < max_try_cnt:                                   # :212
        images = edit_once(image, prompt)
        tries += 1
        if not enable_reflection_mode:                                             # :484-486
            out_images = images
            break
        thinking_info, best_info = thinker.reflect(original_image, images[0], original_prompt)       # :471
        success, refine_prompt = thinker.format_text(thinking_info)
        out_images.append(images[0])
        out_think_info.append(thinking_info)
        best_think_info.append(best_info)
        if not success:                                                            # :476-483
            if refine_prompt is not None:
                prompt, image = refine_prompt, images[0]
            else:
                image, prompt = original_image, reformat_prompt
            try_cnt += 1
    final_images = [out_images[0]] if out_images is not None and len(out_images) > 0 else []             # :491
    if thinking and best_think_info and len(out_images) > 0:                       # :493-521
        final_images = [out_images[best_index(out_think_info, best_think_info)]]
    return LoopResult(out_images, final_images, out_think_info, best_think_info, reformat_prompt if enable_thinking_mode else None, tries)


class Retry:
    """What `_hosted_step1x` runs when a v1p2 switch is on: the host's thinker (`thinker_for`: may raise), its calls timed and run with
    the VLM image processor on the device, and `reflection_loop` around the call's `edit_once`."""

    def __init__(self, host, dev, switch):
        def sync():
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize(dev)
        self.thinker = TimedThinker(thinker_for(host, dev, switch), lambda: _hip_qwen_image_processor(host, dev), sync)

    def __call__(self, edit_once, image, prompt, enable_thinking_mode, enable_reflection_mode, max_try_cnt) -> LoopResult:
        return reflection_loop(edit_once, self.thinker, image, prompt, bool(enable_thinking_mode), bool(enable_reflection_mode), max_try_cnt)


_STEP1X_RETRY[:] = [Retry]                                                         # hosted.py's slot for the module after it
