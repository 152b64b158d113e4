"""Qwen2.5-VL prompt encoder, greedy generate(): HIP (HipQwen25VLTextEncoder.generate, csrc/decode.hip) against the eager bf16 transformers
module's `generate(do_sample=False)`, same process, alternating.

The language model at full size (tools/qwen_text_encoder_bench.py: hidden 3584, 28 layers, 28 / 4 heads, intermediate 18944, vocab 152064;
seeded init on the device), text-only prompts of L = 300 and L = 1500, 64 new tokens, no EOS.  Per length and side: the median (and
min / max) of `--iters` warm runs of a 1-token call (prefill + the first pick) and of a 64-token call; ms per new token =
(t64 - t1) / 63 of the medians.  Batch-1 decode streams every weight once per token: the bytes of one step (decoder weights + lm_head +
the KV cache rows read at the middle of the run) over the measured time, against the 6.3 TB/s the HBM sustains, is the share reported.

The GEMV A/B: rgn_lm_gemv_bf16 against the AdaLN helper rgn_gemv_bf16 (B = 1) at the five (N, K) of a decode step, arms alternating
(new, parent, new again: the A/A arm gives the box's noise).  Each timed pass walks a ring of weight copies larger than the last-level
cache, as a decode step finds its weights in HBM.  `not_slower`: new's median minus parent's is at most the A/A spread.

`--weights fp8 | both` adopts the same module with the layers' projection matrices as fp8 e4m3fn (HipQwen25VLTextEncoder(weights="fp8"));
with `both` the bf16 and the fp8 encoder are built from the one synthetic state dict and alternate run by run (keys `hip_*` and `hip_fp8_*`),
the encoder call (`__call__`, the prefill alone) is timed for both, and every ratio is taken against the format's OWN streaming floor.  The
GEMV A/B leg is then rgn_lm_gemv_w8 against rgn_lm_gemv_bf16 on the four layer shapes, each format walking its own ring of weight copies.

`--sampling` adopts with `sampling=True` and adds two sampled legs per encoder, alternating with the greedy leg in the one process (a
sampling adoption asked for plain greedy search takes the default path, launch for launch): `*_s20` = (repetition_penalty 1.05, temperature
0.7, top_k 20, top_p 0.8) and `*_s0` = (1.1, 1.0, top_k off, 0.9), uniforms from a seeded generator filled before the loop; each step then
runs one rgn_lm_pick_rows (B = 1: the block of rgn_lm_pick) after lm_head.  `*_ms_per_new_token` of a sampled leg against the greedy
leg's is the cost of the pick.

    python tools/qwen_generate_bench.py [--iters 5] [--out profiles/r14_qwen_generate_bench.json] [--ab-out profiles/r14_lm_gemv_ab.txt]
    python tools/qwen_generate_bench.py --weights both --out profiles/r17_qwen_fp8_generate_bench.json --ab-out profiles/r17_lm_gemv_w8_ab.txt
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/qwen_generate_bench.py --hip-only --no-ab --iters 2    # the kernel listing
    python tools/qwen_generate_bench.py --weights both --sampling --hip-only --no-ab --out profiles/r19_qwen_sampling_bench.json

`--batch` times a `max_batch=8` adoption (bf16 and fp8 legs) at B = 1, 2, 4, 8 rows of the same length (no padding, no EOS), every leg
alternating in the one process, beside the B = 1 leg of a default (`max_batch=1`) adoption, which runs the same decode loop and issues
the same launches as B = 1 of the other (the one-row kernels: B = 1 of a `_rows` entry is the one-row entry).  Per leg: ms per step =
(t64 - t1) / 63 of the medians (the B prefills, which run row after row, cancel), tokens per second = B / that, the step against B times the B = 1 step, and against the streaming floor of ITS bytes (weights and lm_head once, B caches).

    python tools/qwen_generate_bench.py --batch --no-ab --out profiles/r26_qwen_batched_generate_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/qwen_generate_bench.py --batch --hip-only --no-ab --iters 1

`--batch --sampling` times a `max_batch=8, sampling=True, batch_sampling=True` adoption (bf16 and fp8) at B = 1, 2, 4, 8: a greedy leg and
the two sampled legs above per B, all alternating in the one process.  Per leg ms per step and tokens per second, and for a sampled leg
the time the pick adds per step = its step minus the greedy step at that B (every B runs one rgn_lm_pick_rows per step; at B = 1 that
entry launches the one block of rgn_lm_pick).  Before them `pick_rows_direct`: rgn_lm_pick_rows launched by itself at V = 152064 for
B = 1..8 beside rgn_lm_pick, whose launch B = 1 dispatches to (the two arms differ by the dispatch alone); `--pick-only` runs only that
(no model is built), which is what a kernel trace of the pick needs.

    python tools/qwen_generate_bench.py --batch --sampling --no-ab --out profiles/r27_qwen_batched_sampling_bench.json
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/qwen_generate_bench.py --batch --sampling --pick-only --no-ab

`--batch --wide` times the MFMA row GEMM path: per length and weight format a default-kernel adoption (`max_batch=8`) at B = 1 and 8 beside a
`batch_kernels="mfma", max_batch=32` adoption at B = 1, 8, 16 and 32, all alternating in the one process; with `--sampling` also the sampled
"mfma" legs at B = 16 and 32.  Per leg ms per step, tokens per second, the streaming floor (weights + B KV bytes at 6.3 TB/s) and the step in
units of the "fma" B = 8 step of the same run, which is what the wide path is judged against.  `--wide-kernels` (no model is built) writes
the kernel table: rgn_lm_gemm_rows_bf16 / _w8 at B = 1, 8, 16, 32 on the four layer shapes beside rgn_lm_gemv_bf16 / _w8 and the B = 8
`_rows` entries, in one process.

    python tools/qwen_generate_bench.py --batch --wide --sampling --no-ab --out profiles/r30_qwen_wide_batch_bench.json
    python tools/qwen_generate_bench.py --wide-kernels --no-ab --ab-out profiles/r30_qwen_wide_batch_kernel_stats.txt

`--lookup` times `lookup=True` adoptions ("fma" and "mfma", bf16 and fp8) whose steps carry drafted tokens, every leg alternating in the one
process with the SAME adoption's plain greedy generate.  The drafts are forced through `draft_tokens`, built from the greedy output: all
wrong (every step carries R = K + 1 rows and settles one token: ms per step at R = 2, 4, 8, and 16, 32 under "mfma"), half of each step's
drafts right, and all right (ms per new token at 0 %, 50 % and 100 % accepted, with the measured rate); a one-id guess gives R = 1 steps
through the speculative loop, whose distance from the plain step is the cost of the per-step host read.  ms per step = (t64 - t1) over the
steps `last_lookup_stats` counts.  The seeded model's own acceptance rate under prompt lookup means nothing and is not reported.

    python tools/qwen_generate_bench.py --lookup --no-ab --out profiles/r31_qwen_lookup_bench.json

`--lookup --sampling` times the same legs on `lookup=True, sampling=True, lookup_sampling=True` adoptions under the `s20` configuration
(penalty 1.05, T 0.7, top-k 20, top-p 0.8) with fixed `uniforms`: the plain leg is the same adoption's plain SAMPLED generate, the forced
drafts are built from its output, and every leg must reproduce its tokens.  It also times rgn_lm_pick_verify by itself at R = 1, 8, 32
beside rgn_lm_pick_wide (`--pick-only`: only those launches, for a kernel trace).

    python tools/qwen_generate_bench.py --lookup --sampling --no-ab --out profiles/r34_qwen_lookup_sampling_bench.json
    rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tools/qwen_generate_bench.py --lookup --sampling --no-ab --iters 1
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from qwen_text_encoder_bench import full_size_config  # noqa: E402

HBM_BYTES_PER_S = 6.3e12          # measured stream bandwidth (the microarchitecture guide's figure for HBM)
LENGTHS = (300, 1500)
NEW = 64
AB_SHAPES = ((4608, 3584), (3584, 3584), (37888, 3584), (3584, 18944), (152064, 3584))
LAYER_SHAPES = AB_SHAPES[:4]      # q|k|v, o, gate|up, down: the matrices `weights="fp8"` quantises (lm_head stays bf16)
RING_BYTES = 1 << 30              # weight copies walked per timed pass: four times the 256 MB last-level cache
SAMPLED = {"s20": dict(do_sample=True, repetition_penalty=1.05, temperature=0.7, top_k=20, top_p=0.8),
           "s0": dict(do_sample=True, repetition_penalty=1.1, temperature=1.0, top_p=0.9)}


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stat(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def step_bytes(tc, n, weights="bf16"):
    """Bytes one decode step reads: every decoder weight (fp8: one byte each plus one fp32 scale per output channel), lm_head (bf16 in
    both formats), and n cache rows per layer."""
    d, F, hq, hkv, nl = tc.hidden_size, tc.intermediate_size, tc.num_attention_heads, tc.num_key_value_heads, tc.num_hidden_layers
    w = 2 * nl * (d * (hq + 2 * hkv) * 128 + hq * 128 * d + 3 * d * F)
    if weights == "fp8":
        w = w // 2 + 4 * nl * ((hq + 2 * hkv) * 128 + d + 2 * F + d)
    return {"decoder_weights": w, "lm_head": 2 * tc.vocab_size * d, "kv_cache": 2 * nl * n * 2 * hkv * 128}


def gemv_ab(rounds=7):
    from regione_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for N, K in AB_SHAPES:
        copies = max(2, -(-RING_BYTES // (2 * N * K)))
        g = torch.Generator(device="cuda").manual_seed(N + K)
        W = torch.stack([(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16() for _ in range(copies)])
        x = torch.randn(K, device="cuda", generator=g).bfloat16()
        y = torch.empty(N, dtype=torch.bfloat16, device="cuda")
        ptrs, px, py = [W[c].data_ptr() for c in range(copies)], x.data_ptr(), y.data_ptr()

        def new():
            for p in ptrs:
                lib.rgn_lm_gemv_bf16(p, px, None, None, py, N, K, st)

        def parent():
            for p in ptrs:
                lib.rgn_gemv_bf16(px, K, p, None, py, N, 1, N, K, 0, st)
        new()
        a = y.clone()
        parent()
        max_diff = float((a.float() - y.float()).abs().max())

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / copies                            # us per GEMV
        for fn in (new, parent, new):
            timed(fn)
        t = {"new": [], "parent": [], "new_again": []}
        for _ in range(rounds):                                                  # the arms alternate
            t["new"].append(timed(new))
            t["parent"].append(timed(parent))
            t["new_again"].append(timed(new))
        med = {k: statistics.median(v) for k, v in t.items()}
        aa = abs(med["new"] - med["new_again"])
        rows.append(dict(N=N, K=K, copies=copies, new_us=med["new"], parent_us=med["parent"], new_again_us=med["new_again"], aa_spread_us=aa,
                         new_min_us=min(t["new"]), new_max_us=max(t["new"]), parent_min_us=min(t["parent"]), parent_max_us=max(t["parent"]),
                         new_tb_per_s=2 * N * K / med["new"] / 1e6, parent_tb_per_s=2 * N * K / med["parent"] / 1e6,
                         not_slower=bool(med["new"] - med["parent"] <= aa), max_abs_diff_of_outputs=max_diff))
        del W
        torch.cuda.empty_cache()
    return rows


def gemv_w8_ab(rounds=7):
    """rgn_lm_gemv_w8 against rgn_lm_gemv_bf16 on the layer shapes: arms alternating (fp8, bf16, fp8 again), each format over its own ring
    of weight copies >= RING_BYTES (twice as many copies for fp8).  `not_slower`: the fp8 median is at most the bf16 median."""
    from regione_amd import _lib, ops
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for N, K in LAYER_SHAPES:
        c16, c8 = max(2, -(-RING_BYTES // (2 * N * K))), max(2, -(-RING_BYTES // (N * K)))
        g = torch.Generator(device="cuda").manual_seed(N + K)
        W = torch.stack([(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16() for _ in range(c16)])
        W8 = torch.empty(c8, N, K, dtype=ops.FP8, device="cuda")
        scales = []
        for c in range(c8):
            q = ops.quantize_w8(W[c % c16])
            W8[c] = q
            scales.append(q._rgn_scale)
        x = torch.randn(K, device="cuda", generator=g).bfloat16()
        y = torch.empty(N, dtype=torch.bfloat16, device="cuda")
        p16, p8, px, py = [W[c].data_ptr() for c in range(c16)], [(W8[c].data_ptr(), scales[c].data_ptr()) for c in range(c8)], x.data_ptr(), y.data_ptr()

        def fp8():
            for p, s in p8:
                lib.rgn_lm_gemv_w8(p, s, px, None, None, py, N, K, st)

        def bf16():
            for p in p16:
                lib.rgn_lm_gemv_bf16(p, px, None, None, py, N, K, st)
        lib.rgn_lm_gemv_w8(p8[0][0], p8[0][1], px, None, None, py, N, K, st)
        a = y.clone()
        lib.rgn_lm_gemv_bf16(p16[0], px, None, None, py, N, K, st)
        max_diff = float((a.float() - y.float()).abs().max())                    # the quantisation of W, not a kernel error

        def timed(fn, copies):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / copies                            # us per GEMV
        for fn, c in ((fp8, c8), (bf16, c16), (fp8, c8)):
            timed(fn, c)
        t = {"fp8": [], "bf16": [], "fp8_again": []}
        for _ in range(rounds):                                                  # the arms alternate
            t["fp8"].append(timed(fp8, c8))
            t["bf16"].append(timed(bf16, c16))
            t["fp8_again"].append(timed(fp8, c8))
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append(dict(N=N, K=K, copies_fp8=c8, copies_bf16=c16, fp8_us=med["fp8"], bf16_us=med["bf16"], fp8_again_us=med["fp8_again"],
                         aa_spread_us=abs(med["fp8"] - med["fp8_again"]), fp8_min_us=min(t["fp8"]), fp8_max_us=max(t["fp8"]),
                         bf16_min_us=min(t["bf16"]), bf16_max_us=max(t["bf16"]), fp8_tb_per_s=N * K / med["fp8"] / 1e6,
                         bf16_tb_per_s=2 * N * K / med["bf16"] / 1e6, fp8_over_bf16=med["fp8"] / med["bf16"],
                         not_slower=bool(med["fp8"] <= med["bf16"]), max_abs_diff_of_outputs=max_diff))
        del W, W8
        torch.cuda.empty_cache()
    return rows


BATCHES = (1, 2, 4, 8)


def batched(a, res):
    """The `--batch` legs (module docstring): res["L300"], res["L1500"]."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import qwen_text_encoder as QT
    cfg = full_size_config()
    tc = cfg.text_config
    torch.manual_seed(0)
    with torch.device("cuda"):
        mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    mod = mod.to(torch.bfloat16)
    torch.cuda.empty_cache()
    encs = {}
    for fmt in ("bf16", "fp8"):
        encs[fmt] = QT.HipQwen25VLTextEncoder(mod, weights=fmt, max_batch=max(BATCHES))
        encs[f"{fmt}_default"] = QT.HipQwen25VLTextEncoder(mod, weights=fmt)
    res["batches"], res["weights"] = list(BATCHES), "both"
    g = torch.Generator().manual_seed(1)
    for L in LENGTHS:
        ids = torch.randint(0, 151000, (max(BATCHES), L), generator=g).cuda()
        arms = {}
        for fmt in ("bf16", "fp8"):
            for n in (1, NEW):
                arms[f"{fmt}_default_{n}"] = lambda fmt=fmt, n=n: encs[f"{fmt}_default"].generate(ids[:1], max_new_tokens=n, eos_token_id=[])
                for B in BATCHES:
                    arms[f"{fmt}_b{B}_{n}"] = lambda fmt=fmt, n=n, B=B: encs[fmt].generate(ids[:B], max_new_tokens=n, eos_token_id=[])
        ts = {k: [] for k in arms}
        with torch.no_grad():
            for fn in arms.values():
                fn()                                                             # warm
            for _ in range(a.iters):
                for k, fn in arms.items():                                       # the legs alternate
                    ts[k].append(_ms(fn))
            r = {"L": L, **{k: _stat(v) for k, v in ts.items()}}
            for fmt in ("bf16", "fp8"):                                          # the batch is invariant, here too
                full = encs[fmt].generate(ids, max_new_tokens=NEW, eos_token_id=[])
                assert tuple(full.shape) == (max(BATCHES), L + NEW)
                assert torch.equal(full[:1], encs[f"{fmt}_default"].generate(ids[:1], max_new_tokens=NEW, eos_token_id=[]))
        for fmt in ("bf16", "fp8"):
            per = {leg: (r[f"{fmt}_{leg}_{NEW}"]["median_ms"] - r[f"{fmt}_{leg}_1"]["median_ms"]) / (NEW - 1)
                   for leg in ("default", *(f"b{B}" for B in BATCHES))}
            sb = step_bytes(tc, L + NEW // 2, fmt)
            rows = [dict(leg="default adoption, B = 1", B=1, ms_per_step=per["default"], tokens_per_s=1e3 / per["default"])]
            for B in BATCHES:
                by = sb["decoder_weights"] + sb["lm_head"] + B * sb["kv_cache"]
                floor = by / HBM_BYTES_PER_S * 1e3
                rows.append(dict(leg=f"max_batch = 8, B = {B}", B=B, ms_per_step=per[f"b{B}"], tokens_per_s=B * 1e3 / per[f"b{B}"],
                                 over_B_times_the_b1_step=per[f"b{B}"] / (B * per["b1"]), step_bytes=by, streaming_floor_ms=floor,
                                 over_its_streaming_floor=per[f"b{B}"] / floor))
            r[f"{fmt}_table"] = rows
        res[f"L{L}"] = r
        print(f"L{L}", json.dumps({k: v for k, v in r.items() if k.endswith("_table")}), flush=True)


WIDE_LEGS = (("fma", 1), ("fma", 8), ("mfma", 1), ("mfma", 8), ("mfma", 16), ("mfma", 32))
WIDE_SAMPLED = (("mfma", 16), ("mfma", 32))


def wide(a, res):
    """The `--batch --wide` legs: per length and weight format, a default-kernel ("fma", max_batch = 8) adoption at B = 1 and 8 and a
    batch_kernels="mfma" adoption (max_batch = 32) at B = 1, 8, 16 and 32, alternating in one process; with --sampling also the sampled
    "mfma" legs at B = 16 and 32.  ms per step = (t64 - t1) / 63 of the medians; the streaming floor is weights + B KV bytes at 6.3 TB/s."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import qwen_text_encoder as QT
    cfg = full_size_config()
    tc = cfg.text_config
    torch.manual_seed(0)
    with torch.device("cuda"):
        mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    mod = mod.to(torch.bfloat16)
    torch.cuda.empty_cache()
    res["legs"], res["weights"] = [f"{k} B={B}" for k, B in WIDE_LEGS], "both"
    g = torch.Generator().manual_seed(1)
    for fmt in ("bf16", "fp8"):
        kw = dict(sampling=True, batch_sampling=True) if a.sampling else {}
        encs = {"fma": QT.HipQwen25VLTextEncoder(mod, weights=fmt, max_batch=8),
                "mfma": QT.HipQwen25VLTextEncoder(mod, weights=fmt, max_batch=32, batch_kernels="mfma", **kw)}
        for L in LENGTHS:
            ids = torch.randint(0, 151000, (32, L), generator=g).cuda()
            uni = torch.rand(NEW, 32, generator=g).cuda()
            arms = {}
            for n in (1, NEW):
                for k, B in WIDE_LEGS:
                    arms[f"{k}_b{B}_{n}"] = lambda k=k, n=n, B=B: encs[k].generate(ids[:B], max_new_tokens=n, eos_token_id=[])
                if a.sampling:
                    for k, B in WIDE_SAMPLED:
                        arms[f"{k}_s20_b{B}_{n}"] = lambda k=k, n=n, B=B: encs[k].generate(
                            ids[:B], max_new_tokens=n, eos_token_id=[], uniforms=uni[:n, :B].contiguous(), **SAMPLED["s20"])
            ts = {k: [] for k in arms}
            with torch.no_grad():
                for fn in arms.values():
                    fn()                                                         # warm
                for _ in range(a.iters):
                    for k, fn in arms.items():                                   # the legs alternate
                        ts[k].append(_ms(fn))
            r = {"L": L, "weights": fmt, **{k: _stat(v) for k, v in ts.items()}}
            legs = [f"{k}_b{B}" for k, B in WIDE_LEGS] + ([f"{k}_s20_b{B}" for k, B in WIDE_SAMPLED] if a.sampling else [])
            per = {leg: (r[f"{leg}_{NEW}"]["median_ms"] - r[f"{leg}_1"]["median_ms"]) / (NEW - 1) for leg in legs}
            sb = step_bytes(tc, L + NEW // 2, fmt)
            rows = []
            for leg in legs:
                B = int(leg.rsplit("_b", 1)[1])
                by = sb["decoder_weights"] + sb["lm_head"] + B * sb["kv_cache"]
                floor = by / HBM_BYTES_PER_S * 1e3
                rows.append(dict(leg=leg, B=B, ms_per_step=per[leg], tokens_per_s=B * 1e3 / per[leg], step_bytes=by, streaming_floor_ms=floor,
                                 over_its_streaming_floor=per[leg] / floor, fma_b8_steps=per[leg] / per["fma_b8"]))
            r["table"] = rows
            r["mfma_b16_under_two_fma_b8_steps"] = bool(per["mfma_b16"] < 2 * per["fma_b8"])
            r["mfma_b32_under_four_fma_b8_steps"] = bool(per["mfma_b32"] < 4 * per["fma_b8"])
            res[f"{fmt}_L{L}"] = r
            print(f"{fmt} L{L}", json.dumps(rows), flush=True)
        del encs
        torch.cuda.empty_cache()


def wide_kernels(a, res):
    """The `--wide-kernels` table: achieved TB/s of rgn_lm_gemm_rows_bf16 / _w8 at B = 1, 8, 16, 32 on the four layer shapes beside
    rgn_lm_gemv_bf16 / _w8 (one row) and the B = 8 `_rows` entries, in one process; every arm walks a ring of weight copies >= 1 GiB."""
    from regione_amd import _lib, ops
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for N, K in LAYER_SHAPES:
        c16, c8 = max(2, -(-RING_BYTES // (2 * N * K))), max(2, -(-RING_BYTES // (N * K)))
        g = torch.Generator(device="cuda").manual_seed(N + K)
        W = torch.stack([(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16() for _ in range(c16)])
        W8 = torch.empty(c8, N, K, dtype=ops.FP8, device="cuda")
        scales = []
        for c in range(c8):
            q = ops.quantize_w8(W[c % c16])
            W8[c] = q
            scales.append(q._rgn_scale)
        X = torch.randn(32, K, device="cuda", generator=g).bfloat16()
        Y = torch.empty(32, N, dtype=torch.bfloat16, device="cuda")
        p16, p8, px, py = [W[c].data_ptr() for c in range(c16)], [(W8[c].data_ptr(), scales[c].data_ptr()) for c in range(c8)], X.data_ptr(), Y.data_ptr()
        arms = {"gemv_bf16 B=1": (lambda: [lib.rgn_lm_gemv_bf16(p, px, None, None, py, N, K, st) for p in p16], c16, 2),
                "gemv_w8 B=1": (lambda: [lib.rgn_lm_gemv_w8(p, s, px, None, None, py, N, K, st) for p, s in p8], c8, 1),
                "gemv_bf16_rows B=8": (lambda: [lib.rgn_lm_gemv_bf16_rows(p, px, K, None, None, 0, py, N, 8, N, K, st) for p in p16], c16, 2),
                "gemv_w8_rows B=8": (lambda: [lib.rgn_lm_gemv_w8_rows(p, s, px, K, None, None, 0, py, N, 8, N, K, st) for p, s in p8], c8, 1)}
        for B in (1, 8, 16, 32):
            arms[f"gemm_rows_bf16 B={B}"] = (lambda B=B: [lib.rgn_lm_gemm_rows_bf16(p, px, K, None, None, 0, py, N, B, N, K, st) for p in p16], c16, 2)
            arms[f"gemm_rows_w8 B={B}"] = (lambda B=B: [lib.rgn_lm_gemm_rows_w8(p, s, px, K, None, None, 0, py, N, B, N, K, st) for p, s in p8], c8, 1)

        def timed(fn, copies):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / copies                            # us per call
        for fn, c, _ in arms.values():
            timed(fn, c)
        t = {k: [] for k in arms}
        for _ in range(7):                                                       # the arms alternate
            for k, (fn, c, _) in arms.items():
                t[k].append(timed(fn, c))
        for k, (_, _, es) in arms.items():
            med = statistics.median(t[k])
            rows.append(dict(N=N, K=K, arm=k, us=med, min_us=min(t[k]), max_us=max(t[k]), tb_per_s=es * N * K / med / 1e6))
        del W, W8
        torch.cuda.empty_cache()
    res["wide_kernels"] = rows
    lines = ["# the MFMA row GEMM (rgn_lm_gemm_rows_*) beside the one-row GEMV and the B = 8 `_rows` entries on the four layer shapes: median us per",
             f"# call of 7 alternating rounds, each arm over a ring of weight copies >= {RING_BYTES >> 20} MiB; TB/s = weight bytes / time.",
             f"# csrc_sha16 {res['csrc_sha16']}  {res['device']}", f"{'N':>7} {'K':>6}  {'arm':<22} {'us':>9} {'[min':>9} {'max]':>9} {'TB/s':>6}"]
    lines += [f"{r['N']:>7} {r['K']:>6}  {r['arm']:<22} {r['us']:>9.2f} {r['min_us']:>9.2f} {r['max_us']:>9.2f} {r['tb_per_s']:>6.2f}" for r in rows]
    print("\n".join(lines), flush=True)
    if a.ab_out:
        with open(a.ab_out, "w") as f:
            f.write("\n".join(lines) + "\n")


def pick_rows_direct(res, rounds=20):
    """rgn_lm_pick_rows by itself at the real vocabulary, B = 1..8 rows of z = 4 randn with 300 seen ids each, beside rgn_lm_pick on one
    row: median us per launch of `rounds` event-timed launches per arm, the arms alternating.  Under rocprofv3 --kernel-trace the grid
    size of a lm_pick_rows_kernel dispatch is B x 1024, which is how a trace tells the B of a launch."""
    from regione_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    V, R = 152064, 8
    g = torch.Generator(device="cuda").manual_seed(7)
    z = (4 * torch.randn(R, V, device="cuda", generator=g)).float()
    seen = torch.zeros(R, V, dtype=torch.uint8, device="cuda")
    ids = torch.randint(0, V, (R, 300), device="cuda", generator=g)
    for b in range(R):
        _lib.check(lib.rgn_lm_seen_mark(ids[b].data_ptr(), 300, seen[b].data_ptr(), V, st), "rgn_lm_seen_mark")
    seen0 = seen.clone()
    uni = torch.rand(R, device="cuda", generator=g)
    tok = torch.empty(R, dtype=torch.int64, device="cuda")
    ws = torch.empty(R, V, dtype=torch.float32, device="cuda")
    nb = lib.rgn_lm_pick_workspace_bytes(V)
    out = {}
    for leg, skw in SAMPLED.items():
        pen, T, k, p = skw["repetition_penalty"], skw["temperature"], skw.get("top_k", 0), skw["top_p"]
        arms = {"one_row": lambda: lib.rgn_lm_pick(z.data_ptr(), V, seen.data_ptr(), pen, 1, T, k, p, uni.data_ptr(), tok.data_ptr(), None,
                                                   ws.data_ptr(), nb, st)}
        for B in range(1, R + 1):
            arms[f"rows_b{B}"] = lambda B=B: lib.rgn_lm_pick_rows(z.data_ptr(), V, B, V, seen.data_ptr(), V, pen, 1, T, k, p, uni.data_ptr(),
                                                                  tok.data_ptr(), 1, None, V, ws.data_ptr(), B * nb, st)
        ts = {name: [] for name in arms}
        for r in range(rounds + 2):                                              # two warm rounds
            for name, fn in arms.items():
                seen.copy_(seen0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn()
                e1.record()
                e1.synchronize()
                _lib.check(rc, name)
                if r >= 2:
                    ts[name].append(e0.elapsed_time(e1) * 1e3)
        out[leg] = {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in ts.items()}
    res["pick_rows_direct"] = dict(V=V, rounds=rounds, stat="event-timed single launches (launch overhead included), arms alternating", **out)
    print("pick_rows_direct", json.dumps(out), flush=True)


def batched_sampling(a, res):
    """The `--batch --sampling` legs (module docstring): res["L300"], res["L1500"]."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import qwen_text_encoder as QT
    cfg = full_size_config()
    torch.manual_seed(0)
    with torch.device("cuda"):
        mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    mod = mod.to(torch.bfloat16)
    torch.cuda.empty_cache()
    encs = {fmt: QT.HipQwen25VLTextEncoder(mod, weights=fmt, sampling=True, max_batch=max(BATCHES), batch_sampling=True) for fmt in ("bf16", "fp8")}
    res["batches"], res["weights"], res["sampled_legs"] = list(BATCHES), "both", SAMPLED
    g = torch.Generator().manual_seed(1)
    gu = torch.Generator().manual_seed(2)
    # one row's uniforms are [n], a batch's [n, B]
    uni = {(n, B): (torch.rand(n, generator=gu) if B == 1 else torch.rand(n, B, generator=gu)).cuda() for n in (1, NEW) for B in BATCHES}
    legs = {"greedy": dict(do_sample=False), **SAMPLED}
    for L in LENGTHS:
        ids = torch.randint(0, 151000, (max(BATCHES), L), generator=g).cuda()
        arms = {}
        for fmt in ("bf16", "fp8"):
            for B in BATCHES:
                for leg, skw in legs.items():
                    for n in (1, NEW):
                        extra = {} if leg == "greedy" else {"uniforms": uni[(n, B)]}
                        arms[f"{fmt}_b{B}_{leg}_{n}"] = lambda fmt=fmt, B=B, skw=skw, n=n, extra=extra: encs[fmt].generate(
                            ids[:B], max_new_tokens=n, eos_token_id=[], **skw, **extra)
        ts = {k: [] for k in arms}
        with torch.no_grad():
            for fn in arms.values():
                fn()                                                             # warm
            for _ in range(a.iters):
                for k, fn in arms.items():                                       # the greedy and the sampled legs alternate
                    ts[k].append(_ms(fn))
        r = {"L": L, **{k: _stat(v) for k, v in ts.items()}}
        for fmt in ("bf16", "fp8"):
            rows = []
            for B in BATCHES:
                per = {leg: (r[f"{fmt}_b{B}_{leg}_{NEW}"]["median_ms"] - r[f"{fmt}_b{B}_{leg}_1"]["median_ms"]) / (NEW - 1) for leg in legs}
                for leg in legs:
                    row = dict(leg=leg, B=B, ms_per_step=per[leg], tokens_per_s=B * 1e3 / per[leg])
                    if leg != "greedy":
                        row["pick_adds_ms_per_step"] = per[leg] - per["greedy"]
                        row["over_the_greedy_step"] = per[leg] / per["greedy"]
                    rows.append(row)
            r[f"{fmt}_table"] = rows
        res[f"L{L}"] = r
        print(f"L{L}", json.dumps({k: v for k, v in r.items() if k.endswith("_table")}), flush=True)

LOOKUP_ROWS = {"fma": (2, 4, 8), "mfma": (2, 4, 8, 16, 32)}


def pick_verify_direct(res, rounds=20):
    """rgn_lm_pick_verify by itself at the real vocabulary, R = 1, 8, 32 rows of z = 4 randn over a map of 300 seen ids and random drafts,
    beside rgn_lm_pick_wide on the same rows (one map per row there): median us per launch of `rounds` event-timed launches per arm, the
    arms alternating."""
    from regione_amd import _lib
    lib = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    V, R = 152064, 32
    g = torch.Generator(device="cuda").manual_seed(7)
    z = (4 * torch.randn(R, V, device="cuda", generator=g)).float()
    seen = torch.zeros(R, V, dtype=torch.uint8, device="cuda")
    ids = torch.randint(0, V, (300,), device="cuda", generator=g)
    for b in range(R):
        _lib.check(lib.rgn_lm_seen_mark(ids.data_ptr(), 300, seen[b].data_ptr(), V, st), "rgn_lm_seen_mark")
    seen0 = seen.clone()
    drafts = torch.randint(0, V, (R - 1,), device="cuda", generator=g)
    uni = torch.rand(R, device="cuda", generator=g)
    tok = torch.empty(R, dtype=torch.int64, device="cuda")
    ws = torch.empty(R, V, dtype=torch.float32, device="cuda")
    nb = lib.rgn_lm_pick_workspace_bytes(V)
    skw = SAMPLED["s20"]
    pen, T, k, p = skw["repetition_penalty"], skw["temperature"], skw["top_k"], skw["top_p"]
    arms = {}
    for B in (1, 8, 32):
        arms[f"verify_r{B}"] = lambda B=B: lib.rgn_lm_pick_verify(z.data_ptr(), V, B, V, seen.data_ptr(), drafts.data_ptr(), pen, 1, T, k, p,
                                                                  uni.data_ptr(), tok.data_ptr(), 1, None, V, ws.data_ptr(), B * nb, st)
        arms[f"wide_b{B}"] = lambda B=B: lib.rgn_lm_pick_wide(z.data_ptr(), V, B, V, seen.data_ptr(), V, pen, 1, T, k, p, uni.data_ptr(),
                                                              tok.data_ptr(), 1, None, V, ws.data_ptr(), B * nb, st)
    ts = {name: [] for name in arms}
    for r in range(rounds + 2):                                                  # two warm rounds
        for name, fn in arms.items():
            seen.copy_(seen0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn()
            e1.record()
            e1.synchronize()
            _lib.check(rc, name)
            if r >= 2:
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    out = {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in ts.items()}
    res["pick_verify_direct"] = dict(V=V, rounds=rounds, config="s20", stat="event-timed single launches (launch overhead included), arms alternating",
                                     **out)
    print("pick_verify_direct", json.dumps(out), flush=True)


def half_guess(G, K, T):
    """A guess of the T greedy tokens G of which every step accepts half of its drafts (rounded down and up in turn): the loop is
    simulated and the draft after the accepted ones is made wrong."""
    g, k, up = G.clone(), 1, False
    while k < T:
        kd = max(0, min(K, T - k - 1))
        a = (kd + up) // 2
        up = not up
        if a < kd:
            g[k + a] = (g[k + a] + 1) % 151000
        k += a + 1
    return g


def lookup(a, res):
    """The `--lookup` legs: per kernel family, weight format and length, the plain generate (greedy, or sampled under --sampling) and the
    speculative loop under forced drafts, alternating in one process."""
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import qwen_text_encoder as QT
    cfg = full_size_config()
    torch.manual_seed(0)
    with torch.device("cuda"):
        mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    mod = mod.to(torch.bfloat16)
    torch.cuda.empty_cache()
    res["weights"] = "both"
    g = torch.Generator().manual_seed(1)
    prompts = {L: torch.randint(0, 151000, (1, L), generator=g).cuda() for L in LENGTHS}
    # under --sampling every generate of a leg carries the s20 configuration and the leg's uniforms (indexed by new-token position)
    uni = {n: torch.rand(NEW, generator=torch.Generator().manual_seed(2))[:n].contiguous().cuda() for n in (1, NEW)}
    adopt = dict(sampling=True, lookup_sampling=True) if a.sampling else {}
    if a.sampling:
        res["sampled_leg"] = SAMPLED["s20"]

    class Sampled:
        """The adoption with the sampled arguments of a call filled in (uniforms of the call's max_new_tokens)."""

        def __init__(self, enc):
            self.enc = enc

        def generate(self, ids, max_new_tokens, **kw):
            extra = dict(SAMPLED["s20"], uniforms=uni[max_new_tokens]) if a.sampling else {}
            return self.enc.generate(ids, max_new_tokens=max_new_tokens, **kw, **extra)

        @property
        def last_lookup_stats(self):
            return self.enc.last_lookup_stats
    for fmt in ("bf16", "fp8"):
        for fam in ("fma", "mfma"):
            enc = Sampled(QT.HipQwen25VLTextEncoder(mod, weights=fmt, batch_kernels=fam, lookup=True, **adopt))
            for L in LENGTHS:
                ids = prompts[L]
                G = enc.generate(ids, max_new_tokens=NEW, eos_token_id=[])[0, L:]
                wrong = (G + 1) % 151000
                top = LOOKUP_ROWS[fam][-1]
                arms = {"plain_1": lambda: enc.generate(ids, max_new_tokens=1, eos_token_id=[]),
                        "plain_64": lambda: enc.generate(ids, max_new_tokens=NEW, eos_token_id=[]),
                        "look_1": lambda: enc.generate(ids, max_new_tokens=1, eos_token_id=[], draft_tokens=G[:1]),
                        "r1_64": lambda: enc.generate(ids, max_new_tokens=NEW, eos_token_id=[], draft_tokens=G[:1])}
                for R in LOOKUP_ROWS[fam]:
                    arms[f"r{R}_acc0_64"] = lambda R=R: enc.generate(ids, max_new_tokens=NEW, eos_token_id=[], prompt_lookup_num_tokens=R - 1,
                                                                     draft_tokens=wrong)
                for R in sorted({8, top}):
                    half = half_guess(G, R - 1, NEW)
                    arms[f"r{R}_acc50_64"] = lambda R=R, half=half: enc.generate(ids, max_new_tokens=NEW, eos_token_id=[],
                                                                                 prompt_lookup_num_tokens=R - 1, draft_tokens=half)
                    arms[f"r{R}_acc100_64"] = lambda R=R: enc.generate(ids, max_new_tokens=NEW, eos_token_id=[], prompt_lookup_num_tokens=R - 1,
                                                                       draft_tokens=G)
                ts, stats = {k: [] for k in arms}, {}
                with torch.no_grad():
                    for k, fn in arms.items():                                   # warm; every leg must give the greedy tokens
                        out = fn()
                        assert torch.equal(out[0, L:], G[:out.shape[1] - L]), k
                        stats[k] = enc.last_lookup_stats
                    for _ in range(a.iters):
                        for k, fn in arms.items():                               # the legs alternate
                            ts[k].append(_ms(fn))
                r = {"L": L, "weights": fmt, "batch_kernels": fam, **{k: _stat(v) for k, v in ts.items()}}
                med = {k: r[k]["median_ms"] for k in arms}
                plain = (med["plain_64"] - med["plain_1"]) / (NEW - 1)
                rows = [dict(leg="plain", ms_per_step=plain, ms_per_token=plain)]
                for k in arms:
                    if k.endswith("_64") and k != "plain_64":
                        st = stats[k]
                        dt = med[k] - med["look_1"]
                        rows.append(dict(leg=k[:-3], steps=st["steps"], drafted=st["drafted"], accepted=st["accepted"],
                                         accepted_share=st["accepted"] / st["drafted"] if st["drafted"] else None,
                                         ms_per_step=dt / st["steps"], ms_per_token=dt / (NEW - 1), plain_steps=dt / (NEW - 1) / plain))
                r["table"] = rows
                r["host_read_ms_per_step"] = rows[1]["ms_per_step"] - plain      # the R = 1 step of the speculative loop against the plain step
                res[f"{fmt}_{fam}_L{L}"] = r
                print(f"{fmt} {fam} L{L}", json.dumps(rows), flush=True)
            del enc
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="only the HIP calls (for a kernel-trace run)")
    ap.add_argument("--no-ab", action="store_true", help="skip the GEMV A/B")
    ap.add_argument("--no-generate", action="store_true", help="only the GEMV A/B")
    ap.add_argument("--weights", choices=("bf16", "fp8", "both"), default="bf16", help="format of the layers' projection matrices")
    ap.add_argument("--sampling", action="store_true", help="adopt with sampling=True and time two sampled legs beside the greedy one")
    ap.add_argument("--batch", action="store_true", help="time a max_batch=8 adoption at B = 1, 2, 4, 8 beside a default one (bf16 and fp8)")
    ap.add_argument("--pick-only", action="store_true", help="with --batch --sampling: only the direct rgn_lm_pick_rows launches (for a kernel trace)")
    ap.add_argument("--wide", action="store_true", help="with --batch: batch_kernels=\"mfma\" at B = 1, 8, 16, 32 beside the default kernels at "
                    "B = 1, 8 (bf16 and fp8); with --sampling also the sampled legs at B = 16, 32")
    ap.add_argument("--wide-kernels", action="store_true", help="only the kernel table of the MFMA row GEMM beside the GEMV entries (--ab-out)")
    ap.add_argument("--lookup", action="store_true", help="lookup=True adoptions under forced drafts beside their own plain greedy generate; with --sampling: "
                    "lookup_sampling=True adoptions beside their own plain sampled generate, and rgn_lm_pick_verify by itself")
    a = ap.parse_args()
    from regione_amd import build
    sha = build.csrc_hash()
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": sha, "iters": a.iters, "new_tokens": NEW,
           "stat": "median and min / max of warm, synchronised runs, the two sides alternating; ms per new token = (t64 - t1) / 63 of the medians",
           "model": "Qwen2.5-VL-7B language model, seeded init, text-only ids, no EOS", "hbm_bytes_per_s": HBM_BYTES_PER_S}
    if a.lookup:
        res["stat"] = ("median and min / max of warm, synchronised runs, every leg alternating with the same adoption's plain "
                       + ("sampled" if a.sampling else "greedy") + " generate; "
                       "ms per step = (t64 - t1) / steps, ms per token = (t64 - t1) / 63 of the medians")
        if a.sampling:
            pick_verify_direct(res)
        if not a.pick_only:
            lookup(a, res)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if a.wide_kernels or (a.batch and a.wide):
        res["stat"] = ("median and min / max of warm, synchronised runs, every leg alternating; ms per step = (t64 - t1) / 63 of the medians; "
                       "tokens per second = B / that")
        wide_kernels(a, res) if a.wide_kernels else wide(a, res)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    if not a.no_ab and a.weights != "bf16":
        rows = gemv_w8_ab()
        res["gemv_w8_ab"] = rows
        lines = [f"# rgn_lm_gemv_w8 (fp8 e4m3fn weights, per-channel scale) against rgn_lm_gemv_bf16 on the four layer shapes: median us per GEMV of 7",
                 f"# alternating rounds, each format over its own ring of weight copies >= {RING_BYTES >> 20} MiB; A/A = |median(fp8) - median(fp8 again)|.",
                 f"# csrc_sha16 {sha}  {res['device']}",
                 f"{'N':>7} {'K':>6} {'fp8 us':>9} {'[min':>8} {'max]':>8} {'bf16 us':>9} {'[min':>8} {'max]':>8} {'fp8 again':>10} {'A/A us':>7} {'fp8 TB/s':>9} "
                 f"{'bf16 TB/s':>10} {'fp8/bf16':>9}  not_slower"]
        for r in rows:
            lines.append(f"{r['N']:>7} {r['K']:>6} {r['fp8_us']:>9.2f} {r['fp8_min_us']:>8.2f} {r['fp8_max_us']:>8.2f} {r['bf16_us']:>9.2f} "
                         f"{r['bf16_min_us']:>8.2f} {r['bf16_max_us']:>8.2f} {r['fp8_again_us']:>10.2f} {r['aa_spread_us']:>7.2f} "
                         f"{r['fp8_tb_per_s']:>9.2f} {r['bf16_tb_per_s']:>10.2f} {r['fp8_over_bf16']:>9.3f}  {r['not_slower']}")
        print("\n".join(lines), flush=True)
        if a.ab_out:
            with open(a.ab_out, "w") as f:
                f.write("\n".join(lines) + "\n")
    elif not a.no_ab:
        rows = gemv_ab()
        res["gemv_ab"] = rows
        lines = [f"# rgn_lm_gemv_bf16 (new) against rgn_gemv_bf16 B = 1 (parent): median us per GEMV of 7 alternating rounds, each pass over a",
                 f"# ring of weight copies >= {RING_BYTES >> 20} MiB; A/A = |median(new) - median(new again)|.  csrc_sha16 {sha}  {res['device']}",
                 f"{'N':>7} {'K':>6} {'copies':>6} {'new us':>9} {'parent us':>10} {'new again':>10} {'A/A us':>8} {'new TB/s':>9} {'parent TB/s':>11}  not_slower"]
        for r in rows:
            lines.append(f"{r['N']:>7} {r['K']:>6} {r['copies']:>6} {r['new_us']:>9.2f} {r['parent_us']:>10.2f} {r['new_again_us']:>10.2f} "
                         f"{r['aa_spread_us']:>8.2f} {r['new_tb_per_s']:>9.2f} {r['parent_tb_per_s']:>11.2f}  {r['not_slower']}")
        lines.append("# why one row per wave and non-temporal weight loads (variant builds, not reproducible from this tree): profiles/r14_qwen_generate_notes.md")
        print("\n".join(lines), flush=True)
        if a.ab_out:
            with open(a.ab_out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.batch and a.sampling:
        res["stat"] = ("median and min / max of warm, synchronised runs, the greedy and the sampled legs alternating; ms per step = "
                       "(t64 - t1) / 63 of the medians; tokens per second = B / that; pick_adds = the sampled step minus the greedy step at that B")
        pick_rows_direct(res)
        if not a.pick_only:
            batched_sampling(a, res)
    elif a.batch:
        res["stat"] = ("median and min / max of warm, synchronised runs, every leg alternating; ms per step = (t64 - t1) / 63 of the medians; "
                       "tokens per second = B / that")
        batched(a, res)
    elif not a.no_generate:
        from transformers import Qwen2_5_VLForConditionalGeneration
        from regione_amd import qwen_text_encoder as QT
        cfg = full_size_config()
        tc = cfg.text_config
        torch.manual_seed(0)
        with torch.device("cuda"):
            mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
        mod = mod.to(torch.bfloat16)
        torch.cuda.empty_cache()
        # the encoders by key prefix: "hip" is the bf16 adoption (today's keys), "hip_fp8" the fp8 one; both read the one module
        encs = {}
        if a.weights in ("bf16", "both"):
            encs["hip"] = QT.HipQwen25VLTextEncoder(mod, sampling=a.sampling)
        if a.weights in ("fp8", "both"):
            encs["hip_fp8"] = QT.HipQwen25VLTextEncoder(mod, weights="fp8", sampling=a.sampling)
        uni = {n: torch.rand(n, generator=torch.Generator().manual_seed(2)).cuda() for n in (1, NEW)}
        if a.sampling:
            res["sampled_legs"] = SAMPLED
        fmt = {"hip": "bf16", "hip_fp8": "fp8"}
        res["weights"] = a.weights
        hip = next(iter(encs.values()))
        g = torch.Generator().manual_seed(1)
        for L in LENGTHS:
            ids = torch.randint(0, 151000, (1, L), generator=g).cuda()
            kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids))
            arms = {}
            for name, enc in encs.items():
                arms[f"{name}_1"] = lambda enc=enc: enc.generate(**kw, max_new_tokens=1, eos_token_id=[])
                arms[f"{name}_64"] = lambda enc=enc: enc.generate(**kw, max_new_tokens=NEW, eos_token_id=[])
                if a.weights != "bf16":
                    arms[f"{name}_call"] = lambda enc=enc: enc(**kw)             # the encoder call: the prefill alone
                for leg, skw in (SAMPLED.items() if a.sampling else ()):
                    for n in (1, NEW):
                        arms[f"{name}_{leg}_{n}"] = lambda enc=enc, skw=skw, n=n: enc.generate(**kw, max_new_tokens=n, eos_token_id=[], uniforms=uni[n],
                                                                                           **skw)
            if not a.hip_only:
                ek = dict(do_sample=False, eos_token_id=None, pad_token_id=0)
                arms["eager_1"] = lambda: mod.generate(**kw, max_new_tokens=1, min_new_tokens=1, **ek)
                arms["eager_64"] = lambda: mod.generate(**kw, max_new_tokens=NEW, min_new_tokens=NEW, **ek)
            ts = {k: [] for k in arms}
            with torch.no_grad():
                for k, fn in arms.items():
                    fn()                                                         # warm
                for _ in range(a.iters):
                    for k, fn in arms.items():                                   # the sides alternate
                        ts[k].append(_ms(fn))
                r = {"L": L, **{k: _stat(v) for k, v in ts.items()}}
                assert hip.generate(**kw, max_new_tokens=NEW, eos_token_id=[]).shape[1] == L + NEW
                if not a.hip_only:
                    he, ee = hip.generate(**kw, max_new_tokens=NEW, eos_token_id=[]), mod.generate(**kw, max_new_tokens=NEW, min_new_tokens=NEW, **ek)
                    assert he.shape[1] == ee.shape[1] == L + NEW, "both sides must decode the full length"
                    r["tokens_equal_to_eager"] = int((he[0, L:] == ee[0, L:he.shape[1]]).sum())
                    r["tokens_equal_to_eager_note"] = ("of 64; informative only: the logits of a seeded-init model over 152064 words are near-ties that "
                                                       "bf16 rounding decides, and after the first difference the two sides decode different "
                                                       "sequences (tests/test_gpu_qwen_generate.py bounds the logits against fp32 instead)")
            for name in list(encs)[1:]:
                assert encs[name].generate(**kw, max_new_tokens=NEW, eos_token_id=[]).shape[1] == L + NEW
            bytes_of = {side: step_bytes(tc, L + NEW // 2, fmt.get(side, "bf16")) for side in (*encs, "eager")}
            b = bytes_of[next(iter(encs))]                                       # the printed floor: fp8's when fp8 is what runs
            r["step_bytes"] = dict(b, total=sum(b.values()))
            r["streaming_floor_ms"] = sum(b.values()) / HBM_BYTES_PER_S * 1e3
            for side in (*encs, "eager"):
                if f"{side}_64" in r:
                    sb = sum(bytes_of[side].values())
                    per = (r[f"{side}_64"]["median_ms"] - r[f"{side}_1"]["median_ms"]) / (NEW - 1)
                    r[f"{side}_ms_per_new_token"], r[f"{side}_prefill_ms"] = per, r[f"{side}_1"]["median_ms"]
                    r[f"{side}_share_of_hbm_bw"] = sb / (per * 1e-3) / HBM_BYTES_PER_S
                    if a.weights != "bf16":
                        r[f"{side}_step_bytes"], r[f"{side}_streaming_floor_ms"] = sb, sb / HBM_BYTES_PER_S * 1e3
                        r[f"{side}_ms_per_new_token_over_its_floor"] = per / (sb / HBM_BYTES_PER_S * 1e3)
            for name in encs:
                for leg in (SAMPLED if a.sampling else ()):
                    per = (r[f"{name}_{leg}_{NEW}"]["median_ms"] - r[f"{name}_{leg}_1"]["median_ms"]) / (NEW - 1)
                    r[f"{name}_{leg}_ms_per_new_token"] = per
                    r[f"{name}_{leg}_over_greedy_ms_per_new_token"] = per / r[f"{name}_ms_per_new_token"]
            if len(encs) == 2:
                r["fp8_over_bf16_ms_per_new_token"] = r["hip_fp8_ms_per_new_token"] / r["hip_ms_per_new_token"]
                r["fp8_over_bf16_call"] = r["hip_fp8_call"]["median_ms"] / r["hip_call"]["median_ms"]
            res[f"L{L}"] = r
            print(f"L{L}", json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
