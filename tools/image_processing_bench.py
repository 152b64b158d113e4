"""Image pre- and post-processing of a hosted edit: the host path against the device path (regione_amd/image_ops.py, rgn_image_*),
stage by stage, in ONE process on ONE machine - the legs alternate (host, device, host, device, ...), one untimed warm round first, the
median of 10 timed runs each.  Wall clock; a device leg ends in a device synchronisation and INCLUDES its upload and download.

  resize       PIL Lanczos on RGB uint8, 2048 x 1365 -> 1248 x 832 and -> 1024 x 1024   | device: upload, two passes, download
  preprocess   np.array(pil).astype(float32) / 255 -> NCHW -> 2 x - 1 at 1024 x 1024    | device: upload, table kernel (bf16 stays there)
  postprocess  bf16 (x * 0.5 + 0.5).clamp(0, 1) -> cpu -> float -> (a * 255).round().astype(uint8) -> PIL at 1024 x 1024, from a bf16
               image on the device                                                      | device: byte kernel, download, PIL
  vlm          Qwen2VLImageProcessorPil on one 1024 x 1024 image ([4900, 1176] fp32)    | device: upload, bicubic, patchify (rows stay there)

The resize stages carry a third, COLD figure: the device leg with the coefficient tables of its size pair built again (host float64
work, image_ops.resample_table) and uploaded again in every run - what the first call at a new image size pays.

Every device result is compared with the host leg's bits before it is timed.  The record carries the host's CPU model and thread count:
the comparison is this host against this device, nothing else.  No GPU: the tool fails (no fallback measurement).

    python tools/image_processing_bench.py [--out profiles/r24_image_processing_bench.json] [--runs 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _picture(h, w, seed):
    """A seeded picture with structure at every scale (smooth gradients + noise + hard edges): resampling has work to do."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 100 * np.sin(x / 37.0 + c) * np.cos(y / 53.0 - c) for c in range(3)], -1)
    a = np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    a[h // 3:h // 2, w // 4:w // 2] = (255, 255, 255)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_image_processing_bench.json"))
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_processing_bench: no GPU (the comparison is measured on the GPU host or not at all)")
    import PIL.Image
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    from regione_amd.image_ops import HipImageOps, resample_table
    io = HipImageOps("cuda")
    proc = Qwen2VLImageProcessorPil()
    big = PIL.Image.fromarray(_picture(1365, 2048, 0))
    sq = PIL.Image.fromarray(_picture(1024, 1024, 1))
    decoded = (torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(2)) * 0.6).to(torch.bfloat16).cuda()
    LANCZOS = PIL.Image.Resampling.LANCZOS

    def host_post():
        x = (decoded * 0.5 + 0.5).clamp(0, 1)
        arr = x.cpu().permute(0, 2, 3, 1).float().numpy()
        return PIL.Image.fromarray((arr * 255).round().astype("uint8")[0])

    def dev_vlm():
        u8 = io.upload(sq)
        h, w = io.smart_resize(u8.shape[0], u8.shape[1])
        return io.to_patch_rows(io.resize(u8, h, w, "bicubic"))
    same_img = lambda h, d: np.array_equal(np.asarray(h), np.asarray(d))
    stages = [
        ("resize 2048x1365 -> 1248x832", lambda: big.resize((1248, 832), LANCZOS), lambda: io.to_pil(io.resize(io.upload(big), 832, 1248, "lanczos")),
         same_img),
        ("resize 2048x1365 -> 1024x1024", lambda: big.resize((1024, 1024), LANCZOS), lambda: io.to_pil(io.resize(io.upload(big), 1024, 1024, "lanczos")),
         same_img),
        ("preprocess 1024x1024", lambda: 2.0 * torch.from_numpy((np.array(sq).astype(np.float32) / 255.0)[None].transpose(0, 3, 1, 2)) - 1.0,
         lambda: io.to_vae_input(io.upload(sq)), lambda h, d: torch.equal(h.to(torch.bfloat16), d.cpu())),
        ("postprocess 1024x1024", host_post, lambda: io.to_pil(io.to_uint8(decoded)), same_img),
        ("vlm processor 1024x1024", lambda: proc(images=[sq], return_tensors="pt")["pixel_values"], dev_vlm,
         lambda h, d: tuple(h.shape) == tuple(d.shape) and torch.equal(h, d.cpu())),
    ]
    res = {"device": torch.cuda.get_device_name(0), "host_cpu": _cpu_model(), "host_threads_torch": torch.get_num_threads(),
           "host_cpus_visible": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count(),
           "runs": a.runs, "method": "legs alternate in one process; one untimed warm round; median of the timed runs; wall clock around a "
                                     "device synchronisation; device legs include upload and download; cold = the resize tables rebuilt and uploaded in every run", "stages": []}
    for name, host, dev, same in stages:
        h0, d0 = host(), dev()                                                                        # warm + the bits
        torch.cuda.synchronize()
        if not same(h0, d0):
            raise SystemExit(f"image_processing_bench: {name}: the device result differs from the host's")
        th, td = [], []
        for _ in range(a.runs):
            th.append(_timed(host)[0])
            td.append(_timed(dev)[0])
        mh, md = statistics.median(th), statistics.median(td)
        row = {"stage": name, "bit_identical": True, "host_ms_median": mh * 1e3, "device_ms_median": md * 1e3,
               "host_ms_min_max": [min(th) * 1e3, max(th) * 1e3], "device_ms_min_max": [min(td) * 1e3, max(td) * 1e3],
               "device_beats_host": md < mh}
        cold = ""
        if name.startswith("resize"):
            tc = []
            for _ in range(a.runs):
                resample_table.cache_clear()
                io._tabs.clear()
                tc.append(_timed(dev)[0])
            mc = statistics.median(tc)
            row.update(device_cold_tables_ms_median=mc * 1e3, device_cold_tables_ms_min_max=[min(tc) * 1e3, max(tc) * 1e3],
                       device_cold_tables_beats_host=mc < mh)
            cold = f"   device, cold tables {mc * 1e3:8.2f} ms"
        res["stages"].append(row)
        print(f"{name:34s} host {mh * 1e3:8.2f} ms   device {md * 1e3:8.2f} ms{cold}", file=sys.stderr)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
