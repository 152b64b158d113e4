"""Host-pipeline adapter: a STOCK diffusers editing pipeline on the HIP engine, with the
reference's call shape (RegionE/README.md:85-113):

    helper = RegionEHelper(pipe)                # FluxKontext / Step1XEdit(V1P2) / QwenImageEdit(Plus)Pipeline object
    helper.set_params(...); helper.enable()     # adopts the transformer weights once, patches the engine, swaps pipe.__class__
    image = pipe(image=pil_image, prompt="...").images[0]        # the user keeps calling the pipeline itself
    helper.disable()                            # pipe is the stock pipeline again

Lower levels, for callers that want them:
    engine = adopt_engine(pipe)                 # latent-level HIP pipeline of the host's family (weights adopted)
    hosted = adopt(pipe)                        # wrapper object: hosted(image=..., prompt=...) without touching pipe.__class__

`adopt_engine` reads the host transformer's `state_dict()` (tensor by tensor, straight to the GPU in bf16), infers the
trunk dimensions from the tensor shapes, maps the family's parameter names onto the engine's FLUX-layout names and
returns the matching `regione_amd.harness` pipeline (latent-level API).  `adopt` additionally keeps the host pipeline for
everything OUTSIDE the denoise loop - image preprocessing, prompt encoders, VAE encode / decode, post-processing - calling
the host's own methods in the order the reference's patched `__call__` does (RegionE/FluxKontext/inplace.py:112-240 and
:396-410), and runs the loop itself (:240-394) on the engine.

diffusers is not installed in the build image: the call sequence follows the reference's copy of the diffusers
`__call__`, and is exercised in tests/test_adapters.py against host-pipeline stand-ins with the same method surface
(tests/host_trunks.py module trees, whose own vanilla forward the adopted engine is compared with).  Treat the first run against a real checkpoint as the remaining validation step.

LoRA adapters loaded into the host transformer (PEFT layers: `load_lora_weights` without `fuse_lora`) are merged into the engine's weights
on the device at adoption and re-merged when the adapter state changes (`lora_sync`, the LoRA section of trunk.py): no per-step side path.

Five modules, each importing only from the ones before it; this file re-exports their names and holds no logic:
    trunk.py        the transformer's weights onto the engine: name maps, layout check, LoRA merge and `lora_sync`, `adopt_engine`
    components.py   VAE, text encoders, Qwen2.5-VL language model / vision tower, image ops: adoption (`hip_*_for`), binders, refusals
    connector.py    Step1X-Edit's per-step connector: the host-module and the HIP object behind the engine's `connector` hook
    hosted.py       the three hosted `__call__`s, `HostedPipeline`, `adopt`, `attach`, `swap_host_class`
    thinking.py     Step1X-Edit v1p2's thinking / reflection retry loop in plain Python, the thinker a host brings (`thinker_for`), and the
                    `Retry` that hosted.py's Step1X call runs through the slot it keeps for it
"""
from .trunk import (_FAMILY_OF, _KEYMAPS, _lora_active, _lora_checked, _lora_fingerprint, _lora_plan,  # noqa: F401
                    adopt_engine, infer_config, lora_layers, lora_sync, map_key)
from .components import (IMAGE_STAGES, IMAGE_STAGES_DEFAULT, _HipQwen2VLImageProcessor, _adopt_or_keep, _bound,  # noqa: F401
                         _decode_image, _decode_qwen_image, _hip_qwen_image_processor, _hip_qwen_text_encoder, _hip_text_encoders,
                         _hip_vae_encode, _image_inputs_on_device, _postprocess_image, _postprocess_qwen_image,
                         _qwen2vl_processor_refusal, _qwen_vae_refusal, hip_image_ops_for, hip_qwen_text_encoder_for,
                         hip_text_encoders_for, hip_vae_encoder_for, hip_vae_for)
from .connector import _HipConnector, _HostConnector, hip_step1x_connector_for  # noqa: F401
from .hosted import (PREFERRED_KONTEXT_RESOLUTIONS, QWEN_CONDITION_IMAGE_SIZE, QWEN_VAE_IMAGE_SIZE, STEP1X_DEFAULT_NEGATIVE,  # noqa: F401
                     HostedFluxKontextPipeline, HostedOutput, HostedPipeline, _host_name, _hosted_flux, _hosted_qwen, _hosted_step1x,
                     _lora_call, _refuse_unused, adopt, attach, is_engine_pipeline, restore_host_class, swap_host_class)
from .thinking import LoopResult, Retry, TimedThinker, best_index, reflection_loop, thinker_for  # noqa: F401
