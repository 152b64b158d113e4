"""Qwen2.5-VL prompt encoder, vision tower: HIP (regione_amd/qwen_vision.py) against the eager bf16 transformers module, same process.

The tower at full size (depth 32, d 1280, 16 heads of 80, MLP 3420, out 3584, patch 14, merge 2, window 112, full attention in blocks
7 / 15 / 23 / 31; transformers' seeded init, built on the device).  Two grids: (1, 28, 28) = 784 patches, the condition image of an
Edit-Plus prompt (384^2 area), and (1, 74, 74) = 5476 patches, the one of an Edit prompt (1024^2 area).

Per grid: the two sides are called ALTERNATELY (HIP, eager, HIP, ...), every call synchronised; the median and min / max of `--iters`
warm calls per side, the algorithmic FLOP of one call (projections, MLP, merger, attention inside its segments, real widths) and the
achieved share of the bf16 dense peak.  The claim checked: HIP's median not above eager's (`hip_not_slower`).  `--parity` adds the fp32
module and records HIP's and eager bf16's PSNR against it on `pooler_output` at the 28 x 28 grid.

    python tools/qwen_vision_bench.py [--iters 10] [--parity] [--out profiles/r11_qwen_vision_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/qwen_vision_bench.py --hip-only --grid 74 --warmup 1 --iters 1   # the kernel listing
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16_FLOPS = 2.5e15          # MI355X dense bf16 MFMA peak
GRIDS = ((1, 28, 28), (1, 74, 74))


def full_size_config():
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLVisionConfig
    return Qwen2_5_VLVisionConfig(depth=32, hidden_size=1280, intermediate_size=3420, num_heads=16, out_hidden_size=3584, patch_size=14,
                                  spatial_merge_size=2, temporal_patch_size=2, window_size=112, fullatt_block_indexes=[7, 15, 23, 31],
                                  in_channels=3, hidden_act="silu")


def work(vc, tab, N):
    """(algorithmic FLOP, attention FLOP) of one call at the real widths; attention counts every (query, key) pair of a segment."""
    d, F, m = vc.hidden_size, vc.intermediate_size, vc.spatial_merge_size ** 2
    K = vc.in_channels * vc.temporal_patch_size * vc.patch_size ** 2
    per = 2 * N * d * 3 * d + 2 * N * d * d + 2 * N * d * 2 * F + 2 * N * F * d
    pairs = {k: sum(int(b - a) ** 2 for a, b in zip(tab[k].tolist()[:-1], tab[k].tolist()[1:])) for k in ("cu_seqlens", "cu_window_seqlens")}
    n_full = len(vc.fullatt_block_indexes)
    attn = 2 * 2 * d * (n_full * pairs["cu_seqlens"] + (vc.depth - n_full) * pairs["cu_window_seqlens"])
    merger = 2 * (N // m) * (m * d) * (m * d + vc.out_hidden_size)
    return 2 * N * K * d + vc.depth * per + attn + merger, attn


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def timed(fns, iters, warmup=2):
    """Alternating, synchronised calls of every fn: {name: stats}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ts.items()}


def psnr(a, ref):
    a, ref = a.double(), ref.double()
    return 10 * math.log10(float(ref.abs().max()) ** 2 / float(((a - ref) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grid", type=int, default=None, help="only the (1, G, G) grid")
    ap.add_argument("--hip-only", action="store_true", help="only the HIP calls (for a kernel-trace run)")
    ap.add_argument("--parity", action="store_true", help="also build the fp32 module and record both PSNRs against it at 28 x 28")
    a = ap.parse_args()
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VisionTransformerPretrainedModel
    from regione_amd import build
    from regione_amd import qwen_vision as QV
    vc = full_size_config()
    torch.manual_seed(0)
    with torch.device("cuda"):
        ref = Qwen2_5_VisionTransformerPretrainedModel(vc).eval()
    grids = [g for g in GRIDS if a.grid is None or g[1] == a.grid]
    gen = torch.Generator().manual_seed(1)
    px = {g: torch.randn(g[1] * g[2], 1176, generator=gen).cuda() for g in grids}
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": build.csrc_hash(), "iters": a.iters,
           "stat": "median and min / max of warm, synchronised calls, the two sides alternating",
           "model": "Qwen2.5-VL vision tower at full size, seeded init, N(0, 1) pixel_values"}
    want32 = None
    if a.parity and not a.hip_only and GRIDS[0] in grids:
        with torch.no_grad():
            want32 = ref(px[GRIDS[0]], torch.tensor([GRIDS[0]], device="cuda")).pooler_output
    mod = ref.to(torch.bfloat16)
    del ref
    torch.cuda.empty_cache()
    hip = QV.HipQwen25VLVisionTower(mod)
    for g in grids:
        N = g[1] * g[2]
        thw = torch.tensor([g], device="cuda")
        flop, attn_flop = work(vc, QV.vision_tables(vc, hip.inv_freq, torch.tensor([g])), N)
        r = {"grid_thw": list(g), "patches": N, "flop": flop, "attention_flop": attn_flop, "bound_compute_ms": flop / PEAK_BF16_FLOPS * 1e3}
        fns = {"hip": lambda: hip(px[g], thw)}
        if not a.hip_only:
            def eager():
                with torch.no_grad():
                    return mod(px[g], thw)
            fns["eager_bf16"] = eager
        r.update(timed(fns, a.iters, a.warmup))
        if not a.hip_only:
            e, h = eager().pooler_output, hip(px[g], thw).pooler_output
            r["speedup"] = r["eager_bf16"]["median_ms"] / r["hip"]["median_ms"]
            r["hip_not_slower"] = r["hip"]["median_ms"] <= r["eager_bf16"]["median_ms"]
            r["hip_vs_eager_psnr_db"] = psnr(h, e)
            if want32 is not None and g == GRIDS[0]:
                r["hip_psnr_db_vs_fp32"], r["eager_bf16_psnr_db_vs_fp32"] = psnr(h, want32), psnr(e, want32)
        for k in ("hip", "eager_bf16"):
            if k in r:
                s = r[k]["median_ms"] * 1e-3
                r[k].update(tflops=flop / s / 1e12, share_of_peak_flops=flop / s / PEAK_BF16_FLOPS)
        res[f"grid{g[1]}x{g[2]}"] = r
        print(f"grid {g}", json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
