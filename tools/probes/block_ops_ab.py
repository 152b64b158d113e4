#!/usr/bin/env python3
"""A/B of harness.flux.BLOCK_OPS (one op call per transformer block) at the headline shape: FLUX, 1024 x 1024, T = 512, K_e = 25 % - the
edit bench.py times (GPU box only; bench.py itself is not touched, its pipeline builder and region injection are imported).

    python tools/probes/block_ops_ab.py [--pairs 10] [--steps 20] [--warmup 5]

1. Host time to ENQUEUE one transformer forward of a full step and of a region step, Python sequence vs op, both in one process,
   alternating edit by edit.  The stream is drained before every forward, so the figure is enqueue time alone.  Per edit the median
   over its forwards of a kind; reported: the median over `--pairs` edits after one warm-up edit per mode.
2. Edit time under the `--steps 20 --warmup 5` protocol, off / on / off in one process: "on" is read against the spread between the two
   "off" runs."""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench as B  # noqa: E402
from regione_amd import RegionEHelper, synth  # noqa: E402
from regione_amd.harness import flux as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synth.FluxConfig()
    h = w = 64
    T = 512
    pipe = B.build_pipeline(cfg, dev, seed=42)
    lat, img, prompt, pooled = [t.to(dev) for t in synth.make_edit_inputs(h, w, T, cfg, seed=110, dtype=torch.bfloat16)]
    helper = RegionEHelper(pipe)
    with contextlib.redirect_stdout(sys.stderr):
        helper.set_params(threshold=0.88, cache_threshold=0.04, warmup_step=6, post_step=2, refresh_step="16")
    helper.enable()
    side = max(int(round((0.25 * h * w) ** 0.5)) - 2, 3)
    r0 = (h - side) // 2
    B.install_region_injection(pipe, h, w, (r0, r0 + side, r0, r0 + side), img[0:1], seed=7)

    def edit(trace=None):
        return pipe(image=img, prompt_embeds=prompt, pooled_prompt_embeds=pooled, height=1024, width=1024, latents=lat, guidance_scale=2.5,
                    return_dict=False, trace=trace)[0]

    tr = pipe.transformer
    orig = tr.forward
    rec = []

    def timed_forward(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = orig(*a, **k)
        rec.append((time.perf_counter() - t0, k.get("hidden_states", a[0] if a else None).shape[1]))
        return r

    def host_edit(flag):
        H.BLOCK_OPS = flag
        rec.clear()
        edit()
        torch.cuda.synchronize()
        full = max(n for _, n in rec)                               # a full step forwards every image row, a region step the edited ones
        return {"F": statistics.median(t for t, n in rec if n == full) * 1e3, "R": statistics.median(t for t, n in rec if n < full) * 1e3}

    print(f"# BLOCK_OPS A/B, FLUX 1024 x 1024, T = {T}, blocks {cfg.n_double} + {cfg.n_single}, device {torch.cuda.get_device_name(0)}")
    tr.forward = timed_forward
    for flag in (False, True):
        host_edit(flag)                                             # warm-up: tables, caches, workspaces of both paths
    host = {False: [], True: []}
    for _ in range(args.pairs):
        for flag in (False, True):
            host[flag].append(host_edit(flag))
    tr.forward = orig
    print(f"## host time to enqueue one forward (stream drained first), ms: median of {args.pairs} edits [min .. max], modes alternating")
    for kind, name in (("F", "full step  "), ("R", "region step")):
        for flag in (False, True):
            v = [e[kind] for e in host[flag]]
            print(f"{name}  BLOCK_OPS={'on ' if flag else 'off'}  {statistics.median(v):7.3f}  [{min(v):7.3f} .. {max(v):7.3f}]")

    def timed(flag):
        H.BLOCK_OPS = flag
        for _ in range(args.warmup):
            edit()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            edit()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    print(f"## edit time, ms per 28-step edit: {args.warmup} warm-up + {args.steps} timed edits per run, off / on / off in one process")
    a = timed(False)
    b = timed(True)
    c = timed(False)
    H.BLOCK_OPS = False
    lo, hi = min(a, c), max(a, c)
    print(f"off {a:9.2f}\non  {b:9.2f}\noff {c:9.2f}")
    print(f"spread between the two off runs: {hi - lo:.2f} ms ({(hi - lo) / lo * 100:.2f} %); on - mean(off) = {b - (a + c) / 2:+.2f} ms "
          f"({(b - (a + c) / 2) / ((a + c) / 2) * 100:+.2f} %); on is {'INSIDE' if lo <= b <= hi else 'OUTSIDE'} the off spread")


if __name__ == "__main__":
    main()
