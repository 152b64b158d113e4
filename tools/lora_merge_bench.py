"""LoRA adoption and hot-swap at FLUX.1 dimensions (regione_amd.adapters `adopt_engine` / `lora_sync`, rgn_lora_merge_bf16): what `enable()` and a later
`set_adapters` / call-time scale cost.

A FLUX-size host transformer (the module tree of tests/host_trunks.py at the public dimensions: 19 double + 38 single blocks, d = 3072,
synthetic bf16 weights on the device) gets LoRA adapters on ALL its Linear layers through the PEFT-layout stand-in of tests/host_lora.py:
ranks 16 and 128, one and two adapters.  Timed (wall clock around a device synchronisation):
  * `adopt_engine` without adapters and with them (the merge runs inside the weight stream);
  * a scale-only hot-swap (`set_scale` on every layer, then `lora_sync`): every LoRA-carrying weight is re-staged and re-merged.
Reported, not asserted: the streaming floor of a hot-swap - read + write of the touched weights at 6.3 TB/s - and the fp32 FMA count.

    python tools/lora_merge_bench.py [--out profiles/r22_lora_merge_bench.json] [--toy]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

HBM_TBS = 6.3
FLUX = dict(in_channels=64, n_double=19, n_single=38, heads=24, head_dim=128, joint_dim=4096, pooled_dim=768)
TOY = dict(in_channels=64, n_double=2, n_single=2, heads=2, head_dim=128, joint_dim=256, pooled_dim=64)


def _s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _host(dims, dev):
    import host_trunks as HT
    torch.manual_seed(0)
    with torch.device(dev):
        mod = HT.FluxTransformer2DModel(**dims).to(torch.bfloat16)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if p.dim() == 2:
                p.normal_(0.0, 0.02)
    return HT.install_vanilla_processors(mod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_lora_merge_bench.json"))
    ap.add_argument("--toy", action="store_true", help="toy dimensions (debugging only: not a valid record)")
    a = ap.parse_args()
    import host_lora as HL
    from regione_amd import adapters as A
    dev = torch.device("cuda")
    dims = TOY if a.toy else FLUX
    pipe = type("FluxKontextPipeline", (), {"vae_scale_factor": 8})()
    pipe.scheduler = None
    linear = lambda mod: sorted(n for n, m in mod.named_modules() if isinstance(m, torch.nn.Linear))
    res = {"config": dict(dims, toy=a.toy), "device": torch.cuda.get_device_name(0), "hbm_tb_s_for_the_floor": HBM_TBS, "cases": []}
    pipe.transformer = _host(dims, dev)
    _s(lambda: A.adopt_engine(pipe))                                                     # warm: library load, allocator
    res["adopt_without_adapters_s"] = [_s(lambda: A.adopt_engine(pipe))[0] for _ in range(2)]
    for rank, n_adapters in ((16, 1), (16, 2), (128, 1), (128, 2)):
        mod = _host(dims, dev)
        targets = linear(mod)
        for i in range(n_adapters):
            HL.inject(mod, targets, rank, float(rank), f"a{i}", seed=i)
        mod.to(dev)                                                                      # the adapters' own tensors (created on the CPU)
        pipe.transformer = mod
        layers = HL.layers(mod)
        elems = sum(m.base_layer.weight.numel() for m in layers.values())
        fma = sum(m.base_layer.weight.numel() * rank * n_adapters for m in layers.values())
        t_adopt, eng = _s(lambda: A.adopt_engine(pipe))
        swaps = []
        for w in (0.5, 0.75, 1.0):
            for i in range(n_adapters):
                HL.set_scale(mod, f"a{i}", w)
            dt, did = _s(lambda: A.lora_sync(pipe, eng))
            assert did
            swaps.append(dt)
        t_same, did = _s(lambda: A.lora_sync(pipe, eng))
        assert not did
        floor = 2 * 2 * elems / (HBM_TBS * 1e12)                                          # bf16 read + write of the touched weights
        res["cases"].append({"rank": rank, "adapters": n_adapters, "lora_layers": len(layers), "merged_weight_elements": elems,
                             "fp32_fma": fma, "adopt_with_adapters_s": t_adopt, "scale_hot_swap_s": swaps,
                             "unchanged_fingerprint_s": t_same, "hot_swap_streaming_floor_s": floor,
                             "hot_swap_fma_tflops": 2 * fma / min(swaps) / 1e12})
        del eng, mod, layers
        pipe.transformer = None
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
