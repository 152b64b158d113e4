"""CPU: the host side of the hosted Step1X-Edit prompt encoder and thinker (regione_amd/adapters) with a recorder in place of
HipQwen25VLTextEncoder: `attach()` adopts for both Step1X pipeline names, an absent `_regione_hip_text_sampling` means True for
Step1XEditPipelineV1P2 only, every switch message of `hip_qwen_text_encoder_for` is what it was, `thinker_for` finds the thinker or
raises the refusal the hosted call always raised.  No GPU is touched."""
import warnings

import pytest
import torch

transformers = pytest.importorskip("transformers")

import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402
import host_step1x_text_pipeline as H1  # noqa: E402
from regione_amd import adapters  # noqa: E402
from regione_amd import qwen_text_encoder as QT  # noqa: E402
from regione_amd.adapters import hosted, thinking  # noqa: E402

CPU = torch.device("cpu")
STEP1X = (H1.Step1XEditPipeline, H1.Step1XEditPipelineV1P2)


@pytest.fixture(scope="module")
def module():
    return HQ.tiny_qwen25vl()


@pytest.fixture
def recorder(monkeypatch):
    seen = []

    class Recorder:
        device, dtype = CPU, torch.bfloat16

        def __init__(self, module, device=None, weights="bf16", **kw):
            self.module, self.kw = module, dict(kw, weights=weights)
            seen.append(self)
    monkeypatch.setattr(QT, "HipQwen25VLTextEncoder", Recorder)
    Recorder.seen = seen
    return Recorder


class _Engine:
    class transformer:
        device = CPU


def _attach(monkeypatch, pipe):
    monkeypatch.setattr(hosted, "adopt_engine", lambda p, device: _Engine())
    monkeypatch.setattr(hosted, "hip_vae_for", lambda p, dev: None)
    monkeypatch.setattr(hosted, "hip_vae_encoder_for", lambda p, dev: None)
    return adapters.attach(pipe, "cpu")


def _pipe(cls, module, trunk="step1x", **attrs):
    p = cls(HS.stub_trunk(trunk), module)
    p._regione_hip_vision = False                                                # the language model alone
    for k, v in attrs.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("cls", STEP1X)
def test_attach_adopts_the_prompt_encoder_of_both_step1x_pipelines(monkeypatch, recorder, module, cls):
    p = _pipe(cls, module)
    _attach(monkeypatch, p)
    assert len(recorder.seen) == 1 and p._regione_hip_qwen_text is recorder.seen[0] and recorder.seen[0].module is module
    v1p2 = cls is H1.Step1XEditPipelineV1P2
    assert recorder.seen[0].kw == ({"weights": "bf16", "sampling": True} if v1p2 else {"weights": "bf16"})
    assert adapters.hip_qwen_text_encoder_for(p, CPU) is recorder.seen[0] and len(recorder.seen) == 1       # kept: one adoption per host
    with adapters._hip_qwen_text_encoder(p, CPU):
        assert p.text_encoder is recorder.seen[0]
    assert p.text_encoder is module


def test_the_sampling_default_is_true_for_v1p2_only_and_an_explicit_false_is_honoured(monkeypatch, recorder, module):
    for cls, attrs, want in ((H1.Step1XEditPipelineV1P2, {}, True), (H1.Step1XEditPipelineV1P2, {"_regione_hip_text_sampling": False}, False),
                             (H1.Step1XEditPipelineV1P2, {"_regione_hip_text_sampling": True}, True), (H1.Step1XEditPipeline, {}, False),
                             (H1.Step1XEditPipeline, {"_regione_hip_text_sampling": True}, True)):
        _attach(monkeypatch, _pipe(cls, module, **attrs))
        assert recorder.seen[-1].kw.get("sampling", False) is want, (cls.__name__, attrs)
    for cls in (HQ.QwenImageEditPipeline, HQ.QwenImageEditPlusPipeline):        # the Qwen hosts: as before
        _attach(monkeypatch, _pipe(cls, module, trunk="qwen"))
        assert "sampling" not in recorder.seen[-1].kw
    # called as always, the function behaves as always for every host: the default is the caller's keyword
    for cls in STEP1X:
        adapters.hip_qwen_text_encoder_for(_pipe(cls, module), CPU)
        assert "sampling" not in recorder.seen[-1].kw
    adapters.hip_qwen_text_encoder_for(_pipe(HQ.QwenImageEditPipeline, module, trunk="qwen"), CPU, sampling_default=True)
    assert recorder.seen[-1].kw["sampling"] is True


def test_a_step1x_stand_in_without_a_qwen_module_is_left_alone(monkeypatch, recorder):
    for make in (HS.make_step1x, HS.make_step1x_v1p2):
        p = make()
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _attach(monkeypatch, p)
        assert recorder.seen == [] and p._regione_hip_qwen_text is None


MESSAGES = (
    ({"_regione_hip_text_weights": "int4"}, "pipe._regione_hip_text_weights = 'int4': \"bf16\" and \"fp8\" are accepted"),
    ({"_regione_hip_text_sampling": 1}, "pipe._regione_hip_text_sampling = 1: True and False are accepted"),
    ({"_regione_hip_text_batch_kernels": "wmma"}, "pipe._regione_hip_text_batch_kernels = 'wmma': \"fma\" and \"mfma\" are accepted"),
    ({"_regione_hip_text_batch": 9}, "pipe._regione_hip_text_batch = 9: an int in 1..8 is accepted"),
    ({"_regione_hip_text_batch": 33, "_regione_hip_text_batch_kernels": "mfma"}, "pipe._regione_hip_text_batch = 33: an int in 1..32 is accepted"),
    ({"_regione_hip_text_batch_sampling": "yes"}, "pipe._regione_hip_text_batch_sampling = 'yes': True and False are accepted"),
    ({"_regione_hip_text_batch_sampling": True, "_regione_hip_text_sampling": False, "_regione_hip_text_batch": 2},
     "pipe._regione_hip_text_batch_sampling = True needs pipe._regione_hip_text_sampling = True"),
    ({"_regione_hip_text_batch_sampling": True, "_regione_hip_text_sampling": True},
     "pipe._regione_hip_text_batch_sampling = True needs pipe._regione_hip_text_batch = N with N in 2..8"),
    ({"_regione_hip_text_lookup": "on"}, "pipe._regione_hip_text_lookup = 'on': True and False are accepted"),
)


@pytest.mark.parametrize("cls", STEP1X + (HQ.QwenImageEditPipeline,))
def test_every_switch_message_is_what_it_was(monkeypatch, recorder, module, cls):
    """The messages are written out here as they stand in the parent commit's `hip_qwen_text_encoder_for`."""
    trunk = "qwen" if cls is HQ.QwenImageEditPipeline else "step1x"
    for attrs, message in MESSAGES:
        p = _pipe(cls, module, trunk=trunk, **attrs)
        with pytest.raises(ValueError) as e:
            _attach(monkeypatch, p)
        assert str(e.value) == message
        assert "_regione_hip_qwen_text" not in p.__dict__ and recorder.seen == []              # nothing adopted, nothing cached
    p = _pipe(cls, module, trunk=trunk, _regione_hip_text=False)
    _attach(monkeypatch, p)
    assert recorder.seen == [] and adapters.hip_qwen_text_encoder_for(p, CPU) is None
    # the switches reach the constructor as they did
    p = _pipe(cls, module, trunk=trunk, _regione_hip_text_weights="fp8", _regione_hip_text_batch=4, _regione_hip_text_lookup=True,
              _regione_hip_text_sampling=False)
    _attach(monkeypatch, p)
    assert recorder.seen[-1].kw == {"weights": "fp8", "max_batch": 4, "lookup": True}


def test_a_refused_module_keeps_the_host_with_the_same_warning(monkeypatch, recorder):
    m = HQ.tiny_qwen25vl(text_kw=dict(use_sliding_window=True, sliding_window=4096, max_window_layers=1))
    with pytest.warns(RuntimeWarning, match="text_encoder kept on the host module: sliding-window"):
        _attach(monkeypatch, _pipe(H1.Step1XEditPipelineV1P2, m))
    assert recorder.seen == []


# ---- thinker_for --------------------------------------------------------------------------------------------------------------------
OLD_REFUSAL = ("Step1XEditPipelineV1P2.__call__: {k}=True (the VLM thinking / reflection retry loop, "
               "Step1XEditV1P2/inplace.py:192-212) is not hosted by the HIP loop; pass False")


@pytest.mark.parametrize("k", ["enable_thinking_mode", "enable_reflection_mode"])
def test_a_host_without_a_thinker_raises_the_refusal_it_always_raised(monkeypatch, recorder, module, k):
    for p in (HS.make_step1x_v1p2(), _pipe(H1.Step1XEditPipelineV1P2, module)):        # no Qwen module; one, but no thinker class
        with pytest.raises(NotImplementedError) as e:
            thinking.thinker_for(p, CPU, k)
        assert str(e.value) == OLD_REFUSAL.format(k=k)
        monkeypatch.setattr(hosted, "lora_sync", lambda *a, **k: None)
        with pytest.raises(NotImplementedError) as e:                                 # and through the hosted call, before anything runs
            hosted._hosted_step1x(p, _Engine(), image=torch.zeros(1, 3, 32, 32), prompt="x", **{k: True})
        assert str(e.value) == OLD_REFUSAL.format(k=k) and p.calls == []


def test_the_callers_own_thinker_is_used_as_it_is(module):
    p = HS.make_step1x_v1p2()
    p._regione_thinker = own = object()
    assert thinking.thinker_for(p, CPU) is own


def test_the_forks_thinker_is_built_on_the_adopted_encoder(monkeypatch, recorder, module):
    H1.install_thinker_class(monkeypatch, H1.ToyThinker)
    p = _pipe(H1.Step1XEditPipelineV1P2, module)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        t = thinking.thinker_for(p, CPU)
    assert isinstance(t, H1.ToyThinker) and t.model is recorder.seen[0] and t.processor is p.processor
    assert recorder.seen[0].kw.get("sampling") is True and p._regione_hip_qwen_text is t.model     # v1p2's default, also when it adopts here


def test_without_an_adoption_the_thinker_runs_on_the_host_module_with_one_warning(monkeypatch, recorder, module):
    H1.install_thinker_class(monkeypatch, H1.ToyThinker)
    p = _pipe(H1.Step1XEditPipelineV1P2, module, _regione_hip_text=False)
    with pytest.warns(RuntimeWarning, match="the thinker's generate runs on the host module") as rec:
        t = thinking.thinker_for(p, CPU)
    assert len(rec) == 1 and t.model is module and recorder.seen == []


def test_reflection_on_latents_is_refused_by_name(monkeypatch, recorder, module):
    p = _pipe(H1.Step1XEditPipelineV1P2, module)
    p._regione_thinker = H1.ToyThinker(None, None)
    monkeypatch.setattr(hosted, "lora_sync", lambda *a, **k: None)
    with pytest.raises(ValueError, match=r"enable_reflection_mode=True.*output_type=\"latent\""):
        hosted._hosted_step1x(p, _Engine(), image=torch.zeros(1, 3, 32, 32), prompt="x", enable_reflection_mode=True, output_type="latent")
    assert p.calls == []


def test_hosted_output_carries_the_v1p2_fields():
    o = adapters.HostedOutput(["a", "b"], {"loop_s": 1.0}, final_images=["b"], think_info=["t"], best_info=[{}], reformat_prompt="r")
    assert o.images == o["images"] == ["a", "b"] and o.final_images == o["final_images"] == ["b"] and o.reformat_prompt == "r"
    assert o.think_info == ["t"] and o.best_info == [{}] and o.timing == {"loop_s": 1.0}
    plain = adapters.HostedOutput("x")
    assert dict(plain) == {"images": "x"} and not hasattr(plain, "final_images")                   # the other families: as before


def test_the_retry_of_the_hosted_call_is_the_one_of_thinking_py():
    assert hosted._STEP1X_RETRY == [thinking.Retry]                                # put there when the package is imported
