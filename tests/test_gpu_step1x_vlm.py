"""GPU: the hosted Step1X-Edit call with its VLM on the HIP kernels (regione_amd/adapters/hosted.py `_hosted_step1x`, adapters/thinking.py):
both `encode_prompt` calls on the adopted Qwen2.5-VL encoder, v1p2's thinking / reflection loop on its `generate`.  The tiny trunk of
tests/host_standins.py, a 256 x 256 picture, five-word prompts, the 2-layer VLM of tests/host_qwen_text_pipeline.py."""
import math
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402
import host_step1x_text_pipeline as H1  # noqa: E402
from regione_amd import RegionEHelper, _lib  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")
PROMPT, NEGATIVE = "turn the sky deep green", "blurry dull and washed out"


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def _picture(seed=5):
    return torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(seed))


def _gen():
    return torch.Generator().manual_seed(1)


def _counted(m):
    """[forwards, generates] of the host module, counted from here on."""
    n = [0, 0]
    m.register_forward_hook(lambda mod, i, o: n.__setitem__(0, n[0] + 1))
    own = m.generate

    def generate(*a, **kw):
        n[1] += 1
        return own(*a, **kw)
    m.generate = generate
    return n


def _enabled(cls, text_encoder, **attrs):
    pipe = cls(HS.stub_trunk("step1x"), text_encoder)
    for k, v in attrs.items():
        setattr(pipe, k, v)
    helper = RegionEHelper(pipe)
    helper.set_params(threshold=0.5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        helper.enable()
    assert [str(r.message) for r in rec if "kept on the host module" in str(r.message)] == []
    return pipe, helper


def _off(cls):
    return dict(enable_thinking_mode=False, enable_reflection_mode=False) if cls.V1P2 else {}


def _thinkers(monkeypatch, verdicts=(), scores=()):
    """The fork's thinker class is a ToyThinker with this script; the list of the instances the hosted call builds."""
    made = []

    class Step1XEditThinker(H1.ToyThinker):
        def __init__(self, model, processor):
            super().__init__(model, processor, verdicts, scores)
            made.append(self)
    H1.install_thinker_class(monkeypatch, Step1XEditThinker)
    return made


@pytest.mark.parametrize("cls", [H1.Step1XEditPipeline, H1.Step1XEditPipelineV1P2])
def test_hosted_step1x_encodes_both_prompts_on_the_adopted_encoder(cls):
    m = HQ.tiny_qwen25vl()
    n = _counted(m)
    pipe, helper = _enabled(cls, m)
    enc = pipe._regione_hip_qwen_text
    assert isinstance(enc, QT.HipQwen25VLTextEncoder) and enc.sampling is cls.V1P2 and enc.vision is not None
    trace, image = {}, _picture()
    lat = pipe(image=image, prompt=PROMPT, negative_prompt=NEGATIVE, generator=_gen(), output_type="latent", trace=trace, **_off(cls)).images
    assert n == [0, 0]                                                             # 2 forwards of the host module before this feature
    assert len(trace["kind"]) == 28 and torch.isfinite(lat.float()).all()
    assert pipe.text_encoder is m and "text_encoder" in pipe.__dict__              # the binding is undone
    assert [c[1] for c in pipe.calls if c[0] == "encode_prompt"] == [PROMPT, NEGATIVE] and len(pipe.encoded) == 2
    for (mi, pe, pm), prompt in zip(list(pipe.encoded), (PROMPT, NEGATIVE)):
        k = int(pm.sum())
        direct = enc(input_ids=mi.input_ids, attention_mask=mi.attention_mask, pixel_values=mi.pixel_values,
                     image_grid_thw=mi.image_grid_thw, output_hidden_states=True).hidden_states[-1]
        assert pe.shape == (1, H1.MAX_LENGTH, 256) and pe.dtype == torch.bfloat16 and k == direct.shape[1] - H1.DROP
        assert torch.equal(pe[0, :k].cpu(), direct[0, H1.DROP:].cpu()) and not bool(pe[0, k:].any())
        he, hm = pipe._qwen_embeds(image, prompt, CPU)                             # the host module, on the CPU
        print(f"hosted {cls.__name__} encode_prompt {prompt!r}: {psnr(pe.cpu(), he):.1f} dB against the host module")
        assert torch.equal(pm.cpu(), hm) and psnr(pe.cpu(), he) >= 40.0
    assert n == [2, 0]                                                             # the two references above
    helper.disable()


class _PassThrough:
    """The host module behind an object of another class: nothing adopts it."""

    def __init__(self, m):
        self.m, self.device, self.dtype, self.calls = m, m.device, m.dtype, 0

    def __call__(self, **kw):
        self.calls += 1
        return self.m(**kw)


@pytest.mark.parametrize("cls", [H1.Step1XEditPipeline, H1.Step1XEditPipelineV1P2])
def test_hip_text_false_keeps_the_host_module_and_its_bits(cls):
    m = HQ.tiny_qwen25vl()
    n = _counted(m)
    pipe, helper = _enabled(cls, m, _regione_hip_text=False)
    assert pipe._regione_engine is not None and "_regione_hip_qwen_text" not in pipe.__dict__
    kw = dict(image=_picture(), prompt=PROMPT, negative_prompt=NEGATIVE, output_type="latent", **_off(cls))
    a = pipe(generator=_gen(), **kw).images
    assert n == [2, 0]
    helper.disable()
    wrapped = _PassThrough(m)
    pipe, helper = _enabled(cls, wrapped)
    assert pipe._regione_hip_qwen_text is None
    b = pipe(generator=_gen(), **kw).images
    assert wrapped.calls == 2 and n == [4, 0] and torch.equal(a, b) and torch.isfinite(a.float()).all()
    helper.disable()


def test_thinking_rewrites_the_prompt_with_the_adopted_encoders_generate(monkeypatch):
    made = _thinkers(monkeypatch)
    m = HQ.tiny_qwen25vl()
    n = _counted(m)
    pipe, helper = _enabled(H1.Step1XEditPipelineV1P2, m)
    enc = pipe._regione_hip_qwen_text
    out = pipe(image=_picture(), prompt=PROMPT, generator=_gen(), output_type="latent", enable_thinking_mode=True, enable_reflection_mode=False,
               return_dict=False)                                                  # a HostedOutput whatever return_dict says (:523-530)
    assert len(made) == 1 and made[0].model is enc and made[0].processor is pipe.processor and n == [0, 0]
    (mi, ids, words), = made[0].said
    direct = enc.generate(**mi, max_new_tokens=H1.THINK_TOKENS)
    assert ids.shape == (1, mi.input_ids.shape[1] + H1.THINK_TOKENS) and torch.equal(ids.cpu(), direct.cpu())
    assert out.reformat_prompt == out["reformat_prompt"] == words and len(words.split()) == H1.THINK_TOKENS
    assert [c[1] for c in pipe.calls if c[0] == "encode_prompt"] == [words, ""]   # the edit runs on the rewritten prompt
    assert out.think_info == [] and out.best_info == [] and torch.isfinite(out.images.float()).all()
    assert out.timing["think_s"] > 0 and out.timing["reflect_s"] == 0 and len(out.timing["tries"]) == 1
    helper.disable()


def test_reflection_retries_on_the_edited_image_with_the_refined_prompt(monkeypatch):
    refined = "make the sky much greener"
    # try 1 fails with a refine prompt and scores 3 * 3, try 2 succeeds and scores min(2, 9) * 3: neither text carries "<#Success>", the
    # strictly larger score wins (Step1XEditV1P2/inplace.py:508) - final_images is the FIRST try's image
    made = _thinkers(monkeypatch, verdicts=[(False, refined), (True, None)], scores=[([3], [3]), ([2, 9], [3])])
    m = HQ.tiny_qwen25vl()
    n = _counted(m)
    pipe, helper = _enabled(H1.Step1XEditPipelineV1P2, m)
    enc = pipe._regione_hip_qwen_text
    image, g = _picture(), _gen()
    out = pipe(image=image, prompt=PROMPT, generator=g, output_type="pt", enable_thinking_mode=False, enable_reflection_mode=True, max_try_cnt=3)
    assert n == [0, 0] and len(made) == 1
    assert [c[0] for c in pipe.calls].count("prepare_latents") == 2 and len(out.timing["tries"]) == 2       # two engine loops
    assert all(set(t) == {"encode_s", "loop_s", "decode_s"} for t in out.timing["tries"])
    assert out.timing["loop_s"] == sum(t["loop_s"] for t in out.timing["tries"]) and out.timing["reflect_s"] > 0 and out.timing["think_s"] == 0
    assert len(out.images) == 2 and all(tuple(i.shape) == (3, 256, 256) and torch.isfinite(i.float()).all() for i in out.images)
    assert len(out.final_images) == 1 and out.final_images[0] is out.images[0]
    assert not hasattr(out, "reformat_prompt") and len(out.think_info) == 2
    assert out.best_info == [{"score1": {"score": [3]}, "score2": {"score": [3]}}, {"score1": {"score": [2, 9]}, "score2": {"score": [3]}}]
    # the second try edited the first try's output with the refined prompt; reflect saw the original picture and prompt both times
    assert len(pipe.images_in) == 2 and pipe.images_in[0] is image and torch.equal(pipe.images_in[1], out.images[0])
    assert pipe.images_in[1].data_ptr() == out.images[0].data_ptr()
    assert [c[1] for c in pipe.calls if c[0] == "encode_prompt"] == [PROMPT, "", refined, ""]
    said = made[0].said
    assert len(said) == 2 and [w for _, _, w in said] == out.think_info
    for (mi, ids, _), edited in zip(said, out.images):
        assert mi.image_grid_thw.shape[0] == 2 and mi.input_ids[0].tolist()[-len(HQ.SUFFIX) - 5:-len(HQ.SUFFIX)] == HQ.words_to_ids(PROMPT)
        both = HQ.ToyProcessor()(text=["<image> <image> " + PROMPT], images=[image, edited.float().cpu()])
        assert torch.equal(mi.pixel_values.cpu(), both.pixel_values)
        assert torch.equal(ids.cpu(), enc.generate(**mi, max_new_tokens=H1.THINK_TOKENS).cpu())
    assert not torch.equal(out.images[0], out.images[1])
    helper.disable()


def test_a_sampling_generation_config_thinks_on_the_v1p2_default_and_is_refused_without_it(monkeypatch):
    made = _thinkers(monkeypatch)
    m = HQ.tiny_qwen25vl()
    m.generation_config.do_sample, m.generation_config.top_k, m.generation_config.repetition_penalty = True, 1, 1.05
    n = _counted(m)
    pipe, helper = _enabled(H1.Step1XEditPipelineV1P2, m)
    enc = pipe._regione_hip_qwen_text
    assert enc.sampling is True and enc.generation_config is m.generation_config
    out = pipe(image=_picture(), prompt=PROMPT, generator=_gen(), output_type="latent", enable_thinking_mode=True, enable_reflection_mode=False)
    (mi, ids, words), = made[0].said
    direct = QT.HipQwen25VLTextEncoder(m, torch.device("cuda"), sampling=True, vision=enc.vision)
    assert torch.equal(ids.cpu(), direct.generate(**mi, max_new_tokens=H1.THINK_TOKENS).cpu()) and out.reformat_prompt == words
    assert n == [0, 0] and torch.isfinite(out.images.float()).all()
    helper.disable()
    pipe, helper = _enabled(H1.Step1XEditPipelineV1P2, m, _regione_hip_text_sampling=False)
    assert pipe._regione_hip_qwen_text.sampling is False
    with pytest.raises(_lib.RegionEHipError, match="do_sample: sampling is not implemented"):
        pipe(image=_picture(), prompt=PROMPT, generator=_gen(), output_type="latent", enable_thinking_mode=True, enable_reflection_mode=False)
    assert n == [0, 0] and not any(c[0] == "encode_image" for c in pipe.calls)     # raised by name, never emulated on the host
    helper.disable()
