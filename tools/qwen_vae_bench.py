#!/usr/bin/env python3
"""f4, Qwen-Image VAE: time the HIP decode of a 128 x 128 x 16 latent frame (-> 1024 x 1024) and the HIP encode of a 1024 x 1024 image next
to the eager bf16 PyTorch stand-in of the same architecture (tests/host_qwen_vae.py: 3-D causal convolutions, as the host module runs them)
on the same GPU, and the RMS-norm pass's bandwidth (GPU box only).  Medians of --reps warm, device-synchronised calls; one JSON line
stamped with the kernel-source hash.  `rocprofv3 --kernel-trace --stats -- python tools/qwen_vae_bench.py --no-eager` gives the split.
    python tools/qwen_vae_bench.py [--reps 20] [--eager-reps 20] [--no-eager]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from regione_amd import qwen_vae as Q
from regione_amd.build import csrc_hash
from regione_amd.vae import PaddedImage
from tests import host_qwen_vae as HQ


def _median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return 1e3 * ts[len(ts) // 2], 1e3 * ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eager-reps", type=int, default=20)
    ap.add_argument("--no-eager", action="store_true")
    ns = ap.parse_args()
    m = HQ.seeded(4)
    sd = m.state_dict()
    dec, enc = Q.HipQwenVaeDecoder(sd, "cuda"), Q.HipQwenVaeEncoder(sd, "cuda")
    g = torch.Generator().manual_seed(1)
    z = torch.randn(1, 16, 1, 128, 128, generator=g).to("cuda", torch.bfloat16)
    x = (torch.rand(1, 3, 1, 1024, 1024, generator=g) * 2 - 1).to("cuda", torch.bfloat16)
    res = {"csrc_sha16": csrc_hash(), "device": torch.cuda.get_device_name(0), "reps": ns.reps, "latent": [128, 128], "image": [1024, 1024]}
    res["hip_decode_ms_median"], res["hip_decode_ms_min"] = _median_ms(lambda: dec.decode(z), ns.reps)
    res["hip_encode_ms_median"], res["hip_encode_ms_min"] = _median_ms(lambda: enc.encode(x), ns.reps)
    res["decode_algorithmic_tflop"], res["encode_algorithmic_tflop"] = dec.flops(128, 128) / 1e12, enc.flops(1024, 1024) / 1e12
    res["hip_decode_tflops"] = res["decode_algorithmic_tflop"] / (res["hip_decode_ms_median"] * 1e-3)
    res["hip_encode_tflops"] = res["encode_algorithmic_tflop"] / (res["hip_encode_ms_median"] * 1e-3)
    # the RMS-norm + SiLU pass of the 96-channel level (stored at 128) at 1024 x 1024: one read + one write of the padded image
    xi, xo = PaddedImage(1024, 1024, 128, "cuda"), PaddedImage(1024, 1024, 128, "cuda")
    xi.t.normal_()
    gb = torch.ones(128, device="cuda", dtype=torch.bfloat16)
    ms, _ = _median_ms(lambda: Q.rms_norm_silu(xi, gb, 96, xo), ns.reps)
    res["rms_norm_1024x1024x128_us_median"] = ms * 1e3
    res["rms_norm_bytes_per_s"] = 2 * xi.rows * 128 * 2 / (ms * 1e-3)
    del xi, xo
    if not ns.no_eager:
        mb = m.cuda().to(torch.bfloat16)
        with torch.no_grad():
            res["eager_bf16_decode_ms_median"], _ = _median_ms(lambda: mb.decode(z, return_dict=False), ns.eager_reps, warm=2)
            res["eager_bf16_encode_ms_median"], _ = _median_ms(lambda: mb.encode(x).latent_dist.mode(), ns.eager_reps, warm=2)
        res["eager_reps"] = ns.eager_reps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
