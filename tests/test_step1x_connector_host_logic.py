"""CPU: the host side of the Step1X-Edit connector on the HIP kernels (regione_amd/step1x_connector.py, the adapter's
`hip_step1x_connector_for`) - no kernel runs here.

  * `connector_items(L, n)` expanded to a boolean [L, L] equals the stand-in's attention mask formula (`A[i, j] = mask[i] & mask[j]`,
    then `A[:, 0] = True`); every row lies in exactly one item, every item has at most 64 queries;
  * `connector_refusal` names each refused case; a `ToyConnector` host is "not this layout" and gets no warning;
  * `mask_prefix` refuses holes, left padding, empty masks and other values;
  * the parameter table equals the stand-in's state_dict keys (and shapes);
  * the three new entry points validate their arguments before any launch.
"""
import warnings

import pytest
import torch
import torch.nn as nn

from regione_amd import adapters as A, step1x_connector as SC

import host_standins as HS
import host_step1x_connector as HC


@pytest.mark.parametrize("L,n", [(1, 1), (64, 64), (65, 64), (130, 65), (80, 1), (200, 129)])
def test_connector_items_are_the_modules_attention_mask(L, n):
    items = SC.connector_items(L, n)
    assert items.dtype == torch.int32 and items.shape[1] == 4
    got = torch.zeros(L, L, dtype=torch.bool)
    cover = torch.zeros(L, dtype=torch.int64)
    for q0, nq, klo, khi in items.tolist():
        assert 1 <= nq <= 64 and 0 <= q0 and q0 + nq <= L and 0 <= klo < khi <= L
        got[q0:q0 + nq, klo:khi] = True
        cover[q0:q0 + nq] += 1
    assert bool((cover == 1).all()), "every row in exactly one item"
    mask = torch.zeros(L, dtype=torch.bool)
    mask[:n] = True
    want = (mask[:, None] & mask[None, :]).clone()                   # the stand-in's formula (IndividualTokenRefiner.forward)
    want[:, 0] = True
    assert torch.equal(got, want)
    # with a base row the same table, shifted: two branches share one buffer
    assert torch.equal(SC.connector_items(L, n, 300), items + torch.tensor([300, 0, 300, 300], dtype=torch.int32))


def test_connector_items_refuse_an_empty_or_overlong_valid_run():
    for L, n in ((8, 0), (8, 9)):
        with pytest.raises(ValueError):
            SC.connector_items(L, n)


def test_parameter_table_equals_the_stand_ins_state_dict():
    for args in ((256, 256, 2, 2, 64), (192, 384, 3, 1, 128)):
        mod = HC.Qwen2Connector(*args)
        cfg = SC.connector_config(mod)
        assert (cfg.in_channels, cfg.hidden_size, cfg.heads_num, cfg.depth, cfg.pooled_dim) == args
        want = SC.connector_param_shapes(cfg)
        sd = mod.state_dict()
        assert set(want) == set(sd)
        assert all(tuple(sd[k].shape) == v for k, v in want.items())
        assert SC.connector_refusal(mod.to(torch.bfloat16)) is None
    assert abs(float(HC.Qwen2Connector(64, 128, 1, 1, 64).scale_factor.detach()) + 0.91) < 1e-6


def _sd(**edit):
    sd = dict(HC.make_connector(256, 256, 2).state_dict())
    for k, v in edit.items():
        if v is None:
            sd.pop(k.replace("__", "."))
        else:
            sd[k.replace("__", ".")] = v
    return sd


def test_connector_refusal_names_each_case():
    assert SC.connector_refusal(HC.make_connector(256, 256, 2)) is None
    assert "head dim 64" in SC.connector_refusal(HC.make_connector(256, 256, 4))
    assert "not multiples of 64" in SC.connector_refusal(HC.make_connector(160, 256, 2)) and "in_channels" in SC.connector_refusal(HC.make_connector(160, 256, 2))
    assert "pooled_dim" in SC.connector_refusal(HC.make_connector(256, 256, 2, pooled_dim=40))
    assert "non-bf16" in SC.connector_refusal(HC.make_connector(256, 256, 2, dtype=torch.float32))
    assert "missing" in SC.connector_refusal(_sd(**{"S__c_embedder__linear_2__bias": None}))
    assert "extra" in SC.connector_refusal(_sd(**{"S__extra__weight": torch.zeros(4, dtype=torch.bfloat16)}))
    why = SC.connector_refusal(_sd(**{"S__t_embedder__mlp__0__weight": torch.zeros(256, 128, dtype=torch.bfloat16)}))
    assert "shape" in why and "S.t_embedder.mlp.0.weight" in why
    # PEFT / LoRA: wrapped layers rename `x.weight` to `x.base_layer.weight` and add lora_A / lora_B
    sd = _sd()
    w = sd.pop("S.input_embedder.weight")
    sd.update({"S.input_embedder.base_layer.weight": w, "S.input_embedder.lora_A.default.weight": torch.zeros(4, 256, dtype=torch.bfloat16),
               "S.input_embedder.lora_B.default.weight": torch.zeros(256, 4, dtype=torch.bfloat16)})
    assert SC.is_connector_layout(sd) and "LoRA" in SC.connector_refusal(sd)
    assert "not the Qwen2Connector layout" in SC.connector_refusal(HS.ToyConnector())
    assert not SC.is_connector_layout(HS.ToyConnector()) and not SC.is_connector_layout(None) and not SC.is_connector_layout(lambda *a: a)


class _Host:
    def __init__(self, connector):
        self.transformer = nn.Module()
        object.__setattr__(self.transformer, "connector", connector)


def test_a_toy_connector_host_is_left_alone_without_a_warning():
    host = _Host(HS.ToyConnector())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert A.hip_step1x_connector_for(host, "cuda") is None
        assert host._regione_hip_connector is None
        assert A.hip_step1x_connector_for(host, "cuda") is None            # cached
        off = _Host(HC.make_connector(256, 256, 2))
        off._regione_hip_connector = False                                  # the opt-out: silent, and the module is not even looked at
        assert A.hip_step1x_connector_for(off, "cuda") is None and off._regione_hip_connector is False
        assert A.hip_step1x_connector_for(_Host(None), "cuda") is None


class _Adopted:
    """What `hip_step1x_connector_for` needs of an adopted connector, without a device."""

    def __init__(self, module):
        self._src = {k: (v, v._version) for k, v in module.state_dict().items()}
    stale = SC.HipStep1XConnector.stale


def test_an_adopted_connector_is_checked_against_the_module_at_every_call():
    mod = HC.make_connector(256, 256, 2)
    host = _Host(mod)
    host._regione_hip_connector = hip = _Adopted(mod)
    assert not hip.stale(mod) and A.hip_step1x_connector_for(host, "cuda") is hip
    with torch.no_grad():
        mod.S.input_embedder.bias.add_(1.0)                                 # an in-place update: the version counter moves
    assert hip.stale(mod)
    host._regione_hip_connector = hip = _Adopted(mod)
    mod.S.input_embedder.weight = nn.Parameter(mod.S.input_embedder.weight.detach().clone())          # a weight swap
    assert hip.stale(mod)
    host._regione_hip_connector = hip = _Adopted(mod)
    mod.S.input_embedder.lora_A = nn.Linear(256, 4, bias=False).to(torch.bfloat16)                     # a LoRA loaded after adoption
    assert hip.stale(mod)
    with pytest.warns(RuntimeWarning, match="connector kept on the host module: PEFT / LoRA"):
        assert A.hip_step1x_connector_for(host, "cuda") is None
    assert host._regione_hip_connector is None


def test_the_layout_with_an_unsupported_config_warns_once_and_keeps_the_host_module():
    host = _Host(HC.make_connector(256, 256, 4))                            # heads of 64
    with pytest.warns(RuntimeWarning, match="connector kept on the host module: head dim 64"):
        assert A.hip_step1x_connector_for(host, "cuda") is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert A.hip_step1x_connector_for(host, "cuda") is None            # once per pipeline


def test_mask_prefix_refuses_holes_and_left_padding():
    t = lambda *v: torch.tensor([v], dtype=torch.float32)
    assert SC.mask_prefix(None, 7) == 7
    assert SC.mask_prefix(t(1, 1, 1, 0, 0), 5) == 3 and SC.mask_prefix(t(1, 1, 1), 3) == 3 and SC.mask_prefix(t(1, 0, 0), 3) == 1
    assert SC.mask_prefix(torch.tensor([[True, True, False]]), 3) == 2 and SC.mask_prefix(t(1, 1, 0).to(torch.bfloat16), 3) == 2
    assert SC.mask_prefix(t(1, 0, 1, 0), 4) is None                         # a hole
    assert SC.mask_prefix(t(0, 1, 1, 1), 4) is None                         # left padding
    assert SC.mask_prefix(t(0, 0, 0), 3) is None                            # no valid row
    assert SC.mask_prefix(t(1, 0.5, 0), 3) is None                          # weights, not a mask
    assert SC.mask_prefix(t(1, 1, 0), 4) is None                            # another length
    masks, embeds = [t(1, 1, 0), t(1, 0, 1)], [torch.zeros(1, 3, 8), torch.zeros(1, 3, 8)]
    why, ns = A._HipConnector.parse(masks, embeds)
    assert ns is None and "negative prompt mask" in why
    assert A._HipConnector.parse([masks[0], None], embeds) == (None, [2, 3])
    why, ns = A._HipConnector.parse([None, None], [embeds[0], torch.zeros(2, 3, 8)])          # the reason names what it is, not a mask
    assert ns is None and "embeddings of shape (2, 3, 8)" in why
    assert SC.mask_prefix(2, 3) == 2 and SC.mask_prefix(0, 3) is None and SC.mask_prefix(4, 3) is None       # a parsed length


def test_new_entry_points_validate_before_any_launch():
    from regione_amd import _lib
    h = _lib.lib()
    P = 0x10000

    def msg():
        return h.rgn_last_error().decode()
    # rgn_masked_mean_rows(x, ldx, L, d, n_valid, scale, out, stream)
    assert h.rgn_masked_mean_rows(None, 64, 4, 64, 4, 1.0, P, None) < 0 and "masked_mean_rows" in msg()
    assert h.rgn_masked_mean_rows(P, 64, 4, 60, 4, 1.0, P, None) < 0                     # d % 8
    assert h.rgn_masked_mean_rows(P, 32, 4, 64, 4, 1.0, P, None) < 0                     # ldx < d
    assert h.rgn_masked_mean_rows(P, 64, 4, 64, 0, 1.0, P, None) < 0                     # n_valid < 1
    assert h.rgn_masked_mean_rows(P, 64, 4, 64, 5, 1.0, P, None) < 0                     # n_valid > L
    assert h.rgn_masked_mean_rows(P, 64, 4, 64, 4, float("nan"), P, None) < 0
    assert h.rgn_masked_mean_rows(P + 2, 64, 4, 64, 4, 1.0, P, None) < 0 and "aligned" in msg()
    # rgn_head_rms_norm_bf16(QKV, ld, wq, wk, L, H, eps, stream)
    assert h.rgn_head_rms_norm_bf16(P, 768, P, P, 0, 2, 1e-6, None) == 0                 # nothing to do
    assert h.rgn_head_rms_norm_bf16(None, 768, P, P, 4, 2, 1e-6, None) < 0 and "head_rms_norm" in msg()
    assert h.rgn_head_rms_norm_bf16(P, 760, P, P, 4, 2, 1e-6, None) < 0                  # ld < 3 H 128
    assert h.rgn_head_rms_norm_bf16(P, 768, P, P, 4, 0, 1e-6, None) < 0
    assert h.rgn_head_rms_norm_bf16(P, 768, P, P, 4, 2, -1.0, None) < 0
    assert h.rgn_head_rms_norm_bf16(P, 768, P + 8, P, 4, 2, 1e-6, None) < 0 and "aligned" in msg()
    # rgn_gate_resid_rows(p, ldp, gate, resid, ldr, y, ldy, M, N, stream)
    assert h.rgn_gate_resid_rows(P, 64, P, P, 64, P, 64, 0, 64, None) == 0
    assert h.rgn_gate_resid_rows(P, 64, None, P, 64, P, 64, 4, 64, None) < 0 and "gate_resid_rows" in msg()
    assert h.rgn_gate_resid_rows(P, 64, P, P, 64, P, 64, 4, 60, None) < 0                # N % 8
    assert h.rgn_gate_resid_rows(P, 64, P, P, 32, P, 64, 4, 64, None) < 0                # ldr < N
    assert h.rgn_gate_resid_rows(P, 64, P, P, 64, P + 4, 64, 4, 64, None) < 0 and "aligned" in msg()
    # the wrappers refuse what the C ABI cannot see
    from regione_amd import ops
    with pytest.raises(_lib.RegionEHipError):
        ops.masked_mean_rows(torch.zeros(4, 64), 4)                                     # fp32 rows
    with pytest.raises(_lib.RegionEHipError):
        SC.HipStep1XConnector(HC.make_connector(256, 256, 2), "cpu")


def test_the_row_ops_are_registered_beside_the_region_ops():
    import regione_amd.torch_ops as T
    assert set(T.registered_row_ops()) == {"masked_mean_rows", "head_rms_norm_", "gate_resid_rows_"} and not set(T.registered_row_ops()) & set(T.registered())
    assert "Tensor(a!) qkv" in str(torch.ops.regione_mi.head_rms_norm_.default._schema)
    assert "Tensor(a!) out" in str(torch.ops.regione_mi.gate_resid_rows_.default._schema)
    for n, s in T.ROW_SCHEMAS.items():
        got = str(getattr(torch.ops.regione_mi, n).default._schema)
        assert got == str(torch._C.parse_schema(f"regione_mi::{n}{s}")), (got, s)
