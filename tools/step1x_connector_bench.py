"""Step1X-Edit's per-step connector: HIP (regione_amd/step1x_connector.py) against the eager bf16 stand-in of the public layout
(tests/host_step1x_connector.py), same process, alternating.

The public size: in 3584 -> hidden 4096, 32 heads of 128, depth 2, MLP 16384, pooled 768; L = 640 tokens per branch, both CFG branches
(valid lengths 640 and 500).  Timed: the median (and min / max) of `--iters` warm `step(t)` calls - both branches, what a computed step of a
hosted edit pays - alternating with the eager module called once per branch as `_HostConnector` does; `prepare` once (what an edit pays
once).  Also recorded: HIP with hoist=False (everything recomputed per step), and PSNR of both sides against the stand-in in fp32.

    python tools/step1x_connector_bench.py [--iters 10] [--out profiles/r15_step1x_connector_bench.json]
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

PUBLIC = dict(in_channels=3584, hidden_size=4096, heads_num=32, depth=2, pooled_dim=768)
L, VALID = 640, (640, 500)


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stat(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def psnr(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    mse = float(((a - ref) ** 2).mean())
    return float("inf") if mse == 0 else 10 * math.log10(float(ref.abs().max()) ** 2 / mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_step1x_connector_bench.json"))
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    import host_step1x_connector as HC
    from regione_amd import step1x_connector as SC
    dev = "cuda"
    with torch.device(dev):                       # seeded init on the device: 0.85 GB of weights
        torch.manual_seed(0)
        mod = HC.Qwen2Connector(PUBLIC["in_channels"], PUBLIC["hidden_size"], PUBLIC["heads_num"], PUBLIC["depth"], PUBLIC["pooled_dim"])
        with torch.no_grad():
            for n, p in mod.named_parameters():
                if n == "scale_factor":
                    continue
                if p.dim() == 2:
                    p.copy_(torch.randn_like(p) / math.sqrt(p.shape[1]))
                elif n.endswith("bias"):
                    p.copy_(0.02 * torch.randn_like(p))
                else:
                    p.copy_(1.0 + 0.1 * torch.randn_like(p))
        mod = mod.to(torch.bfloat16)
        x = torch.randn(2, L, PUBLIC["in_channels"]).to(torch.bfloat16)
        mask = torch.zeros(2, L)
        for b, n in enumerate(VALID):
            mask[b, :n] = 1
    rows, masks = [x[0], x[1]], [mask[0:1], mask[1:2]]
    t = torch.full((1,), 0.5, device=dev)

    @torch.no_grad()
    def eager():
        return [mod(x[b:b + 1], t, mask[b:b + 1]) for b in range(2)]
    hip, plain = SC.HipStep1XConnector(mod, dev), SC.HipStep1XConnector(mod, dev, hoist=False)
    prepare_ms = [_ms(lambda: hip.prepare(rows, masks)) for _ in range(3)]
    plain.prepare(rows, masks)
    for _ in range(2):                            # warm: buffers, workspaces, the eager side's kernels
        hip.step(0.5), plain.step(0.5), eager()
    th, tp, te = [], [], []
    for _ in range(a.iters):
        th.append(_ms(lambda: hip.step(0.5)))
        te.append(_ms(eager))
        tp.append(_ms(lambda: plain.step(0.5)))
    res = {"config": dict(PUBLIC, L=L, valid=list(VALID), branches=2, iters=a.iters), "device": torch.cuda.get_device_name(0),
           "hip_step": _stat(th), "hip_step_no_hoist": _stat(tp), "eager_bf16_step": _stat(te),
           "hip_prepare": {"first_ms": prepare_ms[0], "warm_median_ms": statistics.median(prepare_ms[1:])},
           "speedup_step": statistics.median(te) / statistics.median(th)}
    if not a.no_parity:
        f32 = copy.deepcopy(mod).float()
        with torch.no_grad():
            ref = [f32(x[b:b + 1].float(), t, mask[b:b + 1]) for b in range(2)]
        got, eg = hip.step(0.5), eager()
        cat = lambda rs, i: torch.cat([r[i].reshape(-1).float() for r in rs])
        res["psnr_db_vs_fp32"] = {"enc": {"hip": psnr(cat(got, 0), cat(ref, 0)), "eager_bf16": psnr(cat(eg, 0), cat(ref, 0))},
                                  "y": {"hip": psnr(cat(got, 1), cat(ref, 1)), "eager_bf16": psnr(cat(eg, 1), cat(ref, 1))}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
