"""FLUX.1-Kontext text encoders: HIP (regione_amd/text_encoders.py) against the eager bf16 transformers modules, same process.

Full-size T5-XXL at 512 tokens and CLIP-L at 77 tokens (transformers' seeded init, built on the device); each figure is the median of
`--iters` warm, synchronised calls.  Also reported: the algorithmic FLOP and weight bytes of one call, the achieved share of the
bf16 dense peak and of the measured HBM bandwidth, and the two lower bounds they imply (computed, not measured).

    python tools/text_encoder_bench.py [--iters 20] [--out profiles/r07_text_encoder_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/text_encoder_bench.py --hip-only     # the kernel listing, a run of its own
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_BF16_FLOPS = 2.5e15          # MI355X dense bf16 MFMA peak
HBM_BYTES_PER_S = 6.29e12         # measured stream bandwidth


def t5_cfg():
    from transformers import T5Config
    return T5Config(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu",
                    relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6, is_encoder_decoder=False)


def clip_cfg():
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                          max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=49406, eos_token_id=2,
                          pad_token_id=1)


def t5_work(c, L):
    inner = c.num_heads * c.d_kv
    per = 2 * L * c.d_model * 3 * inner + 2 * L * inner * c.d_model + 2 * L * c.d_model * 2 * c.d_ff + 2 * L * c.d_ff * c.d_model
    per += 2 * 2 * L * L * inner
    wbytes = 2 * c.num_layers * (4 * c.d_model * inner + 3 * c.d_model * c.d_ff)
    return c.num_layers * per, wbytes


def clip_work(c, L):
    d, F = c.hidden_size, c.intermediate_size
    per = 2 * L * d * 4 * d + 2 * L * d * 2 * F + 2 * 2 * L * L * d // 2          # causal: half the score / PV work
    wbytes = 2 * c.num_hidden_layers * (4 * d * d + 2 * d * F)
    return c.num_hidden_layers * per, wbytes


def median_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="only the HIP calls (for a kernel-trace run)")
    a = ap.parse_args()
    from transformers import CLIPTextModel, T5EncoderModel
    from regione_amd import text_encoders as TE
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "stat": "median of warm, synchronised calls"}
    g = torch.Generator().manual_seed(1)
    for name, make, cfg, L, work in (("t5_xxl", T5EncoderModel, t5_cfg(), 512, t5_work), ("clip_l", CLIPTextModel, clip_cfg(), 77, clip_work)):
        with torch.device("cuda"):
            mod = make(cfg).eval()
        mod = mod.to(torch.bfloat16)
        hip = TE.HipT5EncoderModel(mod, max_length=L) if name == "t5_xxl" else TE.HipClipTextModel(mod)
        ids = torch.randint(3, cfg.vocab_size - 3, (1, L), generator=g).cuda()
        flop, wbytes = work(cfg, L)
        r = {"L": L, "flop": flop, "weight_bytes": wbytes,
             "bound_compute_ms": flop / PEAK_BF16_FLOPS * 1e3, "bound_memory_ms": wbytes / HBM_BYTES_PER_S * 1e3}
        r["bound_that_applies"] = "compute" if r["bound_compute_ms"] >= r["bound_memory_ms"] else "memory"
        r["hip_ms"] = median_ms(lambda: hip(ids), a.iters)
        if not a.hip_only:
            with torch.no_grad():
                r["eager_bf16_ms"] = median_ms(lambda: mod(ids), a.iters)
                ref = mod(ids)
            r["speedup"] = r["eager_bf16_ms"] / r["hip_ms"]
            out = hip(ids)
            d = (out.last_hidden_state.double() - ref.last_hidden_state.double())
            r["hip_vs_eager_psnr_db"] = 10 * torch.log10(ref.last_hidden_state.double().abs().max() ** 2 / (d * d).mean()).item()
        for k in ("hip", "eager_bf16"):
            if f"{k}_ms" in r:
                r[f"{k}_tflops"] = flop / (r[f"{k}_ms"] * 1e-3) / 1e12
                r[f"{k}_share_of_peak_flops"] = flop / (r[f"{k}_ms"] * 1e-3) / PEAK_BF16_FLOPS
                r[f"{k}_share_of_hbm_bw"] = wbytes / (r[f"{k}_ms"] * 1e-3) / HBM_BYTES_PER_S
        res[name] = r
        print(name, json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
        del mod, hip
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
