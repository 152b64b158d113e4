"""CPU: the shared helpers of the host-pipeline adapter package (regione_amd/adapters/components.py: `_bound`, `_adopt_or_keep`), the
names the package re-exports, and the one-way dependency of its modules.  Neither a GPU nor the library is touched."""
import ast
import os
import warnings

import pytest

from regione_amd import _lib, adapters as A

PKG = os.path.dirname(A.__file__)
MODULES = ("trunk", "components", "connector", "hosted")            # each imports only from the ones before it

# what regione_amd/, tools/ and tests/ reach through `regione_amd.adapters`
REEXPORTED = (
    "HostedPipeline", "HostedFluxKontextPipeline", "IMAGE_STAGES", "IMAGE_STAGES_DEFAULT", "PREFERRED_KONTEXT_RESOLUTIONS", "_HipConnector",
    "_KEYMAPS", "_decode_qwen_image", "_hip_qwen_image_processor", "_hip_qwen_text_encoder", "_hip_text_encoders", "_hip_vae_encode",
    "_host_name", "_hosted_qwen", "_image_inputs_on_device", "_lora_active", "_lora_call", "_lora_checked", "_lora_fingerprint", "_lora_plan",
    "_qwen2vl_processor_refusal", "_qwen_vae_refusal", "_refuse_unused", "adopt", "adopt_engine", "attach", "hip_image_ops_for",
    "hip_qwen_text_encoder_for", "hip_step1x_connector_for", "hip_text_encoders_for", "hip_vae_encoder_for", "hip_vae_for", "infer_config",
    "is_engine_pipeline", "lora_layers", "lora_sync", "map_key", "restore_host_class", "swap_host_class")


class _Obj:
    x = "class"


def test_bound_restores_a_previous_instance_value():
    o = _Obj()
    o.x = "mine"
    with A._bound(o, "x", "bound") as v:
        assert v == "bound" and o.x == "bound"
    assert o.__dict__["x"] == "mine"


def test_bound_deletes_an_absent_key_so_the_class_attribute_shows_again():
    o = _Obj()
    with A._bound(o, "x", "bound"):
        assert o.x == "bound"
    assert "x" not in o.__dict__ and o.x == "class"


def test_bound_undoes_both_when_the_body_raises():
    had, none = _Obj(), _Obj()
    had.x = "mine"
    for o in (had, none):
        with pytest.raises(KeyError):
            with A._bound(o, "x", "bound"):
                raise KeyError("body")
    assert had.__dict__ == {"x": "mine"} and none.__dict__ == {}


def test_bound_nests_and_unwinds_in_order():
    o = _Obj()
    with A._bound(o, "x", 1):
        with A._bound(o, "x", 2):
            assert o.x == 2
        assert o.x == 1
    assert o.__dict__ == {} and o.x == "class"


def test_adopt_or_keep_returns_the_object_without_a_warning():
    made = object()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert A._adopt_or_keep("thing", None, lambda: made, stacklevel=1) is made


def _one_warning(why, make):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert A._adopt_or_keep("thing", why, make, stacklevel=1) is None
    assert len(w) == 1 and w[0].category is RuntimeWarning
    assert w[0].filename == __file__                                # stacklevel counts from the caller, not from the helper
    return str(w[0].message)


def test_adopt_or_keep_turns_a_refusal_into_one_runtime_warning():
    def make():
        raise AssertionError("a refused module is not constructed")
    assert _one_warning("head dim 96", make) == "thing kept on the host module: head dim 96"


def test_adopt_or_keep_turns_a_library_error_of_make_into_the_same_warning():
    def make():
        raise _lib.RegionEHipError("no bf16 weights")
    assert _one_warning(None, make) == "thing kept on the host module: no bf16 weights"


def test_every_name_callers_use_is_reexported():
    missing = [n for n in REEXPORTED if not hasattr(A, n)]
    assert not missing, missing
    assert A.HostedFluxKontextPipeline is A.HostedPipeline


def test_no_module_of_the_package_imports_a_later_one():
    for i, name in enumerate(MODULES):
        with open(os.path.join(PKG, name + ".py")) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):                                  # function-level imports included
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                siblings = [node.module] if node.module else [a.name for a in node.names]
                for s in siblings:
                    assert s.split(".")[0] in MODULES[:i], f"{name}.py imports .{s}"
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                names = [node.module or ""] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
                assert not any(n.startswith(("regione_amd.adapters", "adapters")) for n in names), f"{name}.py imports {names}"   # no way round
    with open(os.path.join(PKG, "__init__.py")) as f:
        body = ast.parse(f.read()).body
    assert all(isinstance(n, ast.ImportFrom) or (isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant)) for n in body)   # no logic
