"""Hosted Step1X-Edit, the VLM stages: the adopted HIP Qwen2.5-VL encoder (language model + vision tower, regione_amd/qwen_text_encoder.py,
qwen_vision.py) against the host's eager bf16 module under the SAME hosted call (`pipe._regione_hip_text = False`), one process, the two
legs alternating.

The module is Qwen2.5-VL-7B at full size - the language model of tools/qwen_text_encoder_bench.py (hidden 3584, 28 layers, vocab 152064)
with the vision tower of tools/qwen_vision_bench.py (hidden 1280, depth 32) - seeded init on the device, the way
tools/qwen_generate_bench.py builds it.  It sits under the v1p2 Step1X stand-in of tests/host_step1x_text_pipeline.py at the real
embedder's scale (a 217-token template prefix that is dropped, padding to 640) on the tiny trunk of tests/host_standins.py: the trunk, the
toy VAE and a linear stand-in connector are the same on both legs and small beside the VLM.  The processor stand-in cuts the reference
image into the (1, G, G) patch grid of its size (1024^2 area: G = 74, 512^2 area: G = 36) with torch ops on the device, so the VLM image
processor kernels are NOT in these numbers.

Per reference image size and leg: the median (min / max) of `--iters` warm hosted calls' `timing["encode_s"]` - encode_image, the positive
and the negative `encode_prompt`, prepare_latents - and of the vision tower called by itself on the same patches; `vision_share` =
2 x tower / encode (the two encode_prompt calls of an edit run the tower on the same image twice).  `think`: the hosted call's thinker
(`Retry(...).thinker.think`, a ToyThinker whose `generate` asks for 64 new tokens, no EOS) on the 1024^2-area image, seconds as the
hosted call's `timing["think_s"]` counts them.  `hip_beats_host_in_every_row` is the default-on condition of the adoption.

    python tools/step1x_vlm_bench.py [--iters 5] [--out profiles/r33_step1x_vlm_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import host_qwen_text_pipeline as HQ  # noqa: E402
import host_standins as HS  # noqa: E402
import host_step1x_text_pipeline as H1  # noqa: E402
import qwen_text_encoder_bench as TB  # noqa: E402
import qwen_vision_bench as VB  # noqa: E402

SIZES = {"area_1024": 1024, "area_512": 512}
PROMPT = "replace the cloudy sky with a clear sunset and keep the people in the foreground unchanged"
NEGATIVE = "blurry, low quality, watermark"
PREFIX, NEW = 217, 64


def full_size_config():
    from transformers import Qwen2_5_VLConfig
    return Qwen2_5_VLConfig(text_config=TB.full_size_config().text_config.to_dict(), vision_config=VB.full_size_config().to_dict())


class Processor(HQ.ToyProcessor):
    """The toy processor at the real scale: a PREFIX-token template prefix, one vision run of (G / 2)^2 image tokens for a picture of
    side S (G = 2 round(S / 28) patches of 14 pixels a side), the caption's words, the template suffix; the config's own token ids."""

    def __init__(self, cfg):
        self.start, self.image, self.end = cfg.vision_start_token_id, cfg.image_token_id, cfg.vision_end_token_id
        self.prefix = torch.randint(0, 151000, (PREFIX,), generator=torch.Generator().manual_seed(4)).tolist()

    def pixels(self, img, k):
        g = 2 * round(img.shape[-1] / 28)
        x = torch.nn.functional.interpolate(img.reshape(1, 3, *img.shape[-2:]).float(), size=(g * 14, g * 14), mode="bilinear")[0]
        p = x.unfold(1, 14, 14).unfold(2, 14, 14).permute(1, 2, 0, 3, 4).reshape(g * g, 3, 1, 14, 14)
        return p.expand(-1, -1, 2, -1, -1).reshape(g * g, 1176), (1, g, g)

    def __call__(self, text, images=None, padding=True, return_tensors="pt"):
        (t,), images = text, list(images or [])
        pv, grids, ids, k = [], [], list(self.prefix), 0
        for w in t.split():
            if w == "<image>":
                p, g = self.pixels(images[k], k)
                pv.append(p)
                grids.append(g)
                ids += [self.start] + [self.image] * (g[1] * g[2] // 4) + [self.end]
                k += 1
            else:
                ids += HQ.words_to_ids(w)
        ids += [151645, 198, 151644, 77091, 198]            # <|im_end|> \n <|im_start|> assistant \n
        return HQ.ModelInputs(input_ids=torch.tensor([ids]), attention_mask=torch.ones(1, len(ids), dtype=torch.int64),
                              pixel_values=torch.cat(pv), image_grid_thw=torch.tensor(grids, dtype=torch.int64))


class Connector(torch.nn.Module):
    """[1, L, 3584] embeddings to the tiny trunk's 256-wide context and 64-wide pooled vector; timestep dependent, like the real one."""

    def __init__(self, width):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.down, self.pool = torch.nn.Linear(width, 256), torch.nn.Linear(width, 64)
        with torch.no_grad():
            self.down.weight.copy_(0.01 * torch.randn(256, width, generator=g))
            self.pool.weight.copy_(0.01 * torch.randn(64, width, generator=g))

    def forward(self, x, t, mask):
        m = mask.unsqueeze(-1).to(x.dtype)
        return self.down(x) * (1.0 + t.to(x.dtype).view(-1, 1, 1)), self.pool((x * m).sum(1) / m.sum(1))


class Step1XEditPipelineV1P2(H1.Step1XEditPipelineV1P2):    # the adapter dispatches on the class NAME
    DROP, MAX_LENGTH = PREFIX, 640
    _execution_device = torch.device("cuda")

    def __init__(self, trunk, text_encoder):
        super().__init__(trunk, text_encoder)
        self.processor = Processor(text_encoder.config)
        object.__setattr__(trunk, "connector", Connector(text_encoder.config.text_config.hidden_size).to("cuda", torch.bfloat16))
        trunk.__dict__["text_token_mapping"] = trunk.__dict__["text_token_mapping"].to("cuda")

    def encode_prompt(self, ref_image=None, prompt=None, device=None, num_images_per_prompt=1):
        r = super().encode_prompt(ref_image=ref_image, prompt=prompt, device=device, num_images_per_prompt=num_images_per_prompt)
        r.text_embeds, r.text_masks = r.text_embeds.to(r.embedding.device), r.text_masks.to(r.embedding.device)
        self.encoded.clear()                                # a bench keeps no record
        return r


class Thinker(H1.ToyThinker):
    new_tokens = NEW


def install_thinker():
    path = "diffusers.pipelines.step1x_edit.pipeline_step1x_edit_thinker".split(".")
    for i in range(1, len(path) + 1):
        name = ".".join(path[:i])
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
    sys.modules[".".join(path)].Step1XEditThinker = Thinker


def _stat(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def _ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from transformers import Qwen2_5_VLForConditionalGeneration
    from regione_amd import RegionEHelper, build
    from regione_amd.adapters import thinking
    cfg = full_size_config()
    torch.manual_seed(0)
    with torch.device("cuda"):
        mod = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    mod = mod.to(torch.bfloat16)
    mod.generation_config.eos_token_id = None                 # no EOS: both legs decode the 64 tokens
    mod.generation_config.pad_token_id = 0
    torch.cuda.empty_cache()
    install_thinker()
    pipes = {}
    for leg, attrs in (("hip", {}), ("host", {"_regione_hip_text": False})):
        pipe = Step1XEditPipelineV1P2(HS.stub_trunk("step1x"), mod)
        for k, v in attrs.items():
            setattr(pipe, k, v)
        helper = RegionEHelper(pipe)
        helper.set_params(threshold=0.5)
        helper.enable()
        pipes[leg] = pipe
    enc = pipes["hip"]._regione_hip_qwen_text
    assert enc is not None and enc.vision is not None and pipes["host"].__dict__.get("_regione_hip_qwen_text") is None
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha16": build.csrc_hash(), "iters": a.iters, "new_tokens": NEW,
           "stat": "median and min / max of warm, synchronised runs, the host-eager and the HIP leg alternating in one process",
           "model": "Qwen2.5-VL-7B (language model and vision tower at full size), seeded init, under the v1p2 Step1X stand-in on the tiny trunk",
           "prompt_tokens": len(HQ.words_to_ids(PROMPT)), "prefix_tokens": PREFIX}
    beats = []
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, side in SIZES.items():
            image = torch.rand(1, 3, side, side, generator=gen).cuda()
            kw = dict(image=image, prompt=PROMPT, negative_prompt=NEGATIVE, output_type="latent", enable_thinking_mode=False,
                      enable_reflection_mode=False)
            mi = pipes["hip"].processor(text=["<image> " + PROMPT], images=[image]).to("cuda")
            pv, grid = mi.pixel_values, mi.image_grid_thw
            tower = {"hip": lambda: enc.vision(pv, grid), "host": lambda: mod.get_image_features(pv.to(torch.bfloat16), grid)}
            ts = {f"{leg}_{k}": [] for leg in pipes for k in ("encode", "loop", "tower")}
            for it in range(a.iters + 1):                                        # one warm round
                for leg, pipe in pipes.items():                                  # the legs alternate
                    t = pipe(generator=torch.Generator().manual_seed(1), **kw).timing
                    tw = _ms(tower[leg])
                    if it:
                        ts[f"{leg}_encode"].append(t["encode_s"] * 1e3)
                        ts[f"{leg}_loop"].append(t["loop_s"] * 1e3)
                        ts[f"{leg}_tower"].append(tw)
            r = {"image": [side, side], "grid_thw": grid[0].tolist(), "L": int(mi.input_ids.shape[1]), **{k: _stat(v) for k, v in ts.items()}}
            for leg in pipes:
                r[f"{leg}_vision_share"] = 2 * r[f"{leg}_tower"]["median_ms"] / r[f"{leg}_encode"]["median_ms"]
            r["host_over_hip_encode"] = r["host_encode"]["median_ms"] / r["hip_encode"]["median_ms"]
            beats.append(r["hip_encode"]["median_ms"] < r["host_encode"]["median_ms"])
            res[name] = r
            print(name, json.dumps(r), flush=True)
        # think: the hosted call's own thinker object per leg (the adopted encoder's generate, or the host module's with its warning)
        image = torch.rand(1, 3, 1024, 1024, generator=gen).cuda()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            thinkers = {leg: thinking.Retry(pipe, torch.device("cuda"), "enable_thinking_mode").thinker for leg, pipe in pipes.items()}
            assert thinkers["hip"].thinker.model is enc and thinkers["host"].thinker.model is mod
            ts = {leg: [] for leg in pipes}
            for it in range(a.iters + 1):
                for leg, th in thinkers.items():
                    before = th.seconds["think_s"]
                    words = th.think(image, PROMPT)
                    assert len(words.split()) == NEW, "both legs must decode the full length"
                    if it:
                        ts[leg].append((th.seconds["think_s"] - before) * 1e3)
        r = {"image": [1024, 1024], **{f"{leg}_think": _stat(v) for leg, v in ts.items()}}
        r["host_over_hip_think"] = r["host_think"]["median_ms"] / r["hip_think"]["median_ms"]
        beats.append(r["hip_think"]["median_ms"] < r["host_think"]["median_ms"])
        res["think_64"] = r
        print("think_64", json.dumps(r), flush=True)
    res["hip_beats_host_in_every_row"] = bool(all(beats))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
