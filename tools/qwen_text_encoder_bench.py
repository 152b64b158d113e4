"""Qwen2.5-VL prompt encoder, language model: HIP (regione_amd/qwen_text_encoder.py) against the eager bf16 transformers module, same process.

The language model at full size (hidden 3584, 28 layers, 28 query / 4 KV heads, intermediate 18944, vocab 152064, eps 1e-6, theta 1e6,
mrope sections 16/24/24; transformers' seeded init, built on the device; a tiny vision tower that no call here runs), text-only ids.
Two lengths: L = 1500 and L = 300.  These are ESTIMATES of a Qwen-Image-Edit prompt (64 template tokens + about 37 x 37 image tokens +
the instruction) and of an Edit-Plus prompt with one 384^2 condition image; neither was measured on a real pipeline.

Per length: the median and min / max of `--iters` warm, synchronised calls for both sides, the algorithmic FLOP and weight bytes of one
call, the achieved share of the bf16 dense peak and of the measured HBM bandwidth, and the two lower bounds they imply (computed, not
measured).  The claim checked: HIP's median below eager's by more than the larger of the two min-max spreads (`faster_beyond_spread`).
`--parity` adds the fp32 module (about 30 GB more) and records HIP's and eager bf16's PSNR against it at L = 1500.

    python tools/qwen_text_encoder_bench.py [--iters 10] [--parity] [--out profiles/r08_qwen_text_encoder_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/qwen_text_encoder_bench.py --hip-only --iters 3   # the kernel listing
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
HBM_BYTES_PER_S = 6.29e12         # measured stream bandwidth
LENGTHS = (1500, 300)             # estimates, see above


def full_size_config():
    from transformers import Qwen2_5_VLConfig
    t = dict(vocab_size=152064, hidden_size=3584, intermediate_size=18944, num_hidden_layers=28, num_attention_heads=28, num_key_value_heads=4,
             rms_norm_eps=1e-6, max_position_embeddings=128000, rope_parameters=dict(rope_type="default", rope_theta=1e6, mrope_section=[16, 24, 24]),
             tie_word_embeddings=False)
    v = dict(depth=2, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=3584, patch_size=14, spatial_merge_size=2,
             temporal_patch_size=2, window_size=56, fullatt_block_indexes=[1], in_channels=3)
    return Qwen2_5_VLConfig(text_config=t, vision_config=v)


def work(tc, L):
    """(algorithmic FLOP, weight bytes) of one call: the four projections and the MLP per layer, causal attention at half the L^2 work."""
    d, F, hq, hkv = tc.hidden_size, tc.intermediate_size, tc.num_attention_heads, tc.num_key_value_heads
    qkv = (hq + 2 * hkv) * 128
    per = 2 * L * d * qkv + 2 * L * hq * 128 * d + 2 * L * d * 2 * F + 2 * L * F * d
    attn = 2 * 2 * L * L * hq * 128 // 2
    wbytes = 2 * tc.num_hidden_layers * (d * qkv + hq * 128 * d + 3 * d * F)
    return tc.num_hidden_layers * (per + attn), tc.num_hidden_layers * attn, wbytes


def timed_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def psnr(a, ref):
    a, ref = a.double(), ref.double()
    return 10 * math.log10(float(ref.abs().max()) ** 2 / float(((a - ref) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="only the HIP calls (for a kernel-trace run)")
    ap.add_argument("--parity", action="store_true", help="also build the fp32 module and record both PSNRs against it at L = 1500")
    a = ap.parse_args()
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import qwen_text_encoder as QT
    cfg = full_size_config()
    tc = cfg.text_config
    torch.manual_seed(0)
    with torch.device("cuda"):
        ref = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    g = torch.Generator().manual_seed(1)
    ids = {L: torch.randint(0, 151000, (1, L), generator=g).cuda() for L in LENGTHS}
    masks = {L: torch.ones_like(ids[L]) for L in LENGTHS}
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "stat": "median and min / max of warm, synchronised calls",
           "lengths_are": "estimates of an Edit prompt (1500) and an Edit-Plus prompt with one 384^2 image (300), not measured on a pipeline",
           "model": "Qwen2.5-VL-7B language model, seeded init, text-only ids"}
    want32 = None
    if a.parity and not a.hip_only:
        with torch.no_grad():
            want32 = ref(input_ids=ids[1500], attention_mask=masks[1500], output_hidden_states=True).hidden_states[-1]
    mod = ref.to(torch.bfloat16)
    del ref
    torch.cuda.empty_cache()
    hip = QT.HipQwen25VLTextEncoder(mod)
    for L in LENGTHS:
        kw = dict(input_ids=ids[L], attention_mask=masks[L], output_hidden_states=True)
        flop, attn_flop, wbytes = work(tc, L)
        r = {"L": L, "flop": flop, "attention_flop": attn_flop, "weight_bytes": wbytes,
             "bound_compute_ms": flop / PEAK_BF16_FLOPS * 1e3, "bound_memory_ms": wbytes / HBM_BYTES_PER_S * 1e3}
        r["bound_that_applies"] = "compute" if r["bound_compute_ms"] >= r["bound_memory_ms"] else "memory"
        r["hip"] = timed_ms(lambda: hip(**kw), a.iters)
        if not a.hip_only:
            with torch.no_grad():
                r["eager_bf16"] = timed_ms(lambda: mod(**kw), a.iters)
                e = mod(**kw).hidden_states[-1]
            h = hip(**kw).hidden_states[-1]
            spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in ("hip", "eager_bf16"))
            r["larger_min_max_spread_ms"] = spread
            r["eager_minus_hip_median_ms"] = r["eager_bf16"]["median_ms"] - r["hip"]["median_ms"]
            r["faster_beyond_spread"] = r["eager_minus_hip_median_ms"] > spread
            r["speedup"] = r["eager_bf16"]["median_ms"] / r["hip"]["median_ms"]
            r["hip_vs_eager_psnr_db"] = psnr(h, e)
            if want32 is not None and L == 1500:
                r["hip_psnr_db_vs_fp32"], r["eager_bf16_psnr_db_vs_fp32"] = psnr(h, want32), psnr(e, want32)
        for k in ("hip", "eager_bf16"):
            if k in r:
                s = r[k]["median_ms"] * 1e-3
                r[k].update(tflops=flop / s / 1e12, share_of_peak_flops=flop / s / PEAK_BF16_FLOPS, share_of_hbm_bw=wbytes / s / HBM_BYTES_PER_S)
        res[f"L{L}"] = r
        print(f"L{L}", json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
