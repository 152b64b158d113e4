#!/usr/bin/env python3
"""The HIP VAEs at 2048 x 2048 and the fused mid-block attention (GPU box only): one JSON line.

  * AutoencoderKL decode (latent 256) and encode (2048^2 image): median wall time of warm, synchronised calls and the peak
    torch.cuda.max_memory_allocated of one call;
  * the mid-block attention at 1024^2 (130 x 130 x 512), attention = "fused" against "materialized", alternating in the same process;
  * rgn_vae_attention_bf16 alone on the 2048^2 mid block (258 x 258 x 512) with its algorithmic rate 4 (hw)^2 C / time.
`rocprofv3 --kernel-trace --stats -- python tools/vae_large_bench.py` gives the per-kernel split.
    python tools/vae_large_bench.py [--reps 10] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from regione_amd import _lib, ops, vae as V
from tests import host_vae


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * sorted(ts)[reps // 2]


def _peak_gib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 30, base / 2 ** 30


def _events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ns = ap.parse_args()
    m = host_vae.seeded(5)
    sd = m.state_dict()
    del m
    res = {}
    dec = V.HipVaeDecoder(sd, "cuda")
    z = torch.randn(1, 16, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
    peak, held = _peak_gib(lambda: dec.decode(z))
    res["decode_2048"] = {"ms_median": _median_ms(lambda: dec.decode(z), ns.reps), "peak_alloc_gib_first_call": peak,
                          "weights_gib": held, "score_buffers": len(dec._attn_buf)}
    del dec
    torch.cuda.empty_cache()
    enc = V.HipVaeEncoder(sd, "cuda")
    x = (torch.rand(1, 3, 2048, 2048, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    peak, held = _peak_gib(lambda: enc.encode(x))
    res["encode_2048"] = {"ms_median": _median_ms(lambda: enc.encode(x), ns.reps), "peak_alloc_gib_first_call": peak,
                          "weights_gib": held, "score_buffers": len(enc._attn_buf)}
    del enc
    torch.cuda.empty_cache()

    # 1024^2 mid-block attention, fused vs materialised, alternating (CUDA events around one _run_attention each)
    dec = V.HipVaeDecoder(sd, "cuda")
    xi = dec.pool.get(128, 128, 512)
    xi.t.normal_()
    xi.t.view(130, 130, 512)[[0, -1]] = 0
    xi.t.view(130, 130, 512)[:, [0, -1]] = 0
    t = {"fused": [], "materialized": []}
    cur = xi
    for i in range(2 * (ns.reps + 3)):
        mode = ("fused", "materialized")[i % 2]
        dec.attention = mode
        box = []
        ms = _events_ms(lambda: box.append(dec._run_attention(cur)))
        cur = box[0]
        if i >= 6:
            t[mode].append(ms)
    res["attention_1024"] = {k: {"ms_median": sorted(v)[len(v) // 2], "ms_min": min(v)} for k, v in t.items()}
    res["attention_1024"]["note"] = "whole block: GroupNorm, to_q/to_k/to_v, attention, to_out (events around one _run_attention call)"

    # the kernel alone on the 2048^2 mid block
    Hp = Wp = 258
    C = 512
    g = torch.Generator(device="cuda").manual_seed(3)
    q, k, v = (torch.randn(Hp * Wp, C, device="cuda", generator=g).mul_(0.3).bfloat16() for _ in range(3))
    o = torch.empty_like(q)
    h = _lib.lib()

    def run():
        _lib.check(h.rgn_vae_attention_bf16(ops._p(q), ops._p(k), ops._p(v), None, ops._p(o), Hp, Wp, C, 1.0 / math.sqrt(C),
                                            ops._stream()), "rgn_vae_attention_bf16")
    for _ in range(2):
        run()
    ks = sorted(_events_ms(run) for _ in range(ns.reps))
    flop = 4.0 * (256 * 256) ** 2 * C
    res["fused_kernel_2048"] = {"ms_median": ks[len(ks) // 2], "ms_min": ks[0], "algorithmic_tflop": flop / 1e12,
                                "pflops_median": flop / (ks[len(ks) // 2] * 1e-3) / 1e15}
    q2, k2, v2 = (t_[: 130 * 130].contiguous() for t_ in (q, k, v))
    o2 = torch.empty_like(q2)

    def run1024():
        _lib.check(h.rgn_vae_attention_bf16(ops._p(q2), ops._p(k2), ops._p(v2), None, ops._p(o2), 130, 130, C, 1.0 / math.sqrt(C),
                                            ops._stream()), "rgn_vae_attention_bf16")
    run1024()
    ks = sorted(_events_ms(run1024) for _ in range(ns.reps))
    res["fused_kernel_1024"] = {"ms_median": ks[len(ks) // 2], "pflops_median": 4.0 * (128 * 128) ** 2 * C / (ks[len(ks) // 2] * 1e-3) / 1e15}
    line = json.dumps(res)
    print(line)
    if ns.out:
        with open(ns.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
