"""Shared by the batched-generate tests of the Qwen2.5-VL prompt encoder (test_qwen_batched_generate_host_logic.py, test_gpu_qwen_batched_generate.py):
a left-padded batch of toy prompts, and transformers' batched greedy-search rule restated plainly; and by the GPU tests of generate:
the seeded module, the device arguments of a prompt, corrupted guesses and the kernel names of a warm call.  Test infrastructure only."""
import functools

import torch

import host_qwen_text_pipeline as HQ

ONE = "make the square red and keep the rest of the picture as it is"
PROMPTS = ("<image> make the square red and keep the rest",               # 4 image placeholders: 25 tokens
           " ".join([ONE] * 4),                                           # 63 tokens: its cache crosses 64 rows while decoding
           "red")                                                         # 12 tokens


def rows(prompts=PROMPTS, seed=3):
    """One ModelInputs per prompt (B = 1, unpadded); a prompt with an `<image>` mark gets one seeded image."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p in prompts:
        images = [torch.rand(1, 3, 64, 96, generator=g) for _ in range(p.split().count("<image>"))]
        out.append(HQ.ToyProcessor()(text=[p], images=images or None))
    return out


def left_padded(singles, pad=HQ.PAD):
    """input_ids [B, L] and attention_mask [B, L] with the rows right-aligned (zeros, then ones); the images' grids in row order."""
    L = max(s.input_ids.shape[1] for s in singles)
    ids = torch.stack([torch.cat([torch.full((L - s.input_ids.shape[1],), pad, dtype=torch.int64), s.input_ids[0]]) for s in singles])
    mask = torch.stack([torch.cat([torch.zeros(L - s.input_ids.shape[1], dtype=torch.int64), torch.ones(s.input_ids.shape[1], dtype=torch.int64)])
                        for s in singles])
    grids = [s.image_grid_thw for s in singles if s.image_grid_thw is not None]
    pixels = [s.pixel_values for s in singles if s.pixel_values is not None]
    return ids, mask, (torch.cat(grids) if grids else None), (torch.cat(pixels) if pixels else None)


# ---- shared by the GPU tests of generate (test_gpu_qwen_*.py); nothing below touches the GPU before it is called ----------------------
def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def cuda(single):
    """The generate arguments of one ModelInputs on the device (without image embeddings)."""
    kw = dict(input_ids=single.input_ids.cuda(), attention_mask=single.attention_mask.cuda())
    if single.image_grid_thw is not None:
        kw.update(image_grid_thw=single.image_grid_thw.cuda(), mm_token_type_ids=(kw["input_ids"] == HQ.IMAGE).int())
    return kw


@functools.lru_cache(maxsize=None)
def module():
    """The seeded two-layer module on the device; adoptions read it, no test writes to it."""
    torch.manual_seed(0)
    return HQ.tiny_qwen25vl(layers=2).cuda()


@functools.lru_cache(maxsize=None)
def prompts():
    """The image prompt (25 tokens) and the repetitive text prompt (63 tokens: its cache crosses 64 rows while decoding)."""
    out = []
    for s in rows(PROMPTS[:2]):
        kw = cuda(s)
        if s.image_grid_thw is not None:
            kw.update(image_embeds=torch.randn(4, 256, device="cuda", generator=gen(11)).bfloat16())
        out.append(kw)
    return out


def corrupt(G, every):
    g = G.clone()
    g[every - 1::every] = (g[every - 1::every] + 1) % HQ.VOCAB
    return g


def kernels(fn):
    """(fn()'s result, the device kernel names of that call) for a warm call: fn runs once before the profiled run (buffers, lm_head, the
    pick's LDS attribute)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]


def kernel_names(fn):
    return kernels(fn)[1]


def greedy_search_rule(prompt_ids, step_ids, eos, pad):
    """transformers' `_sample` loop for do_sample=False over the tokens `step_ids` [T, B] a model would pick at each step:
    `next = next * unfinished + pad * (1 - unfinished)`, a row is finished once its token is an EOS, stop when every row is finished."""
    B = prompt_ids.shape[0]
    seq = prompt_ids.clone()
    unfinished = torch.ones(B, dtype=torch.int64)
    for t in range(step_ids.shape[0]):
        nxt = step_ids[t]
        if eos:
            nxt = nxt * unfinished + pad * (1 - unfinished)
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        if eos:
            unfinished = unfinished * (~torch.isin(nxt, torch.tensor(eos))).long()
            if int(unfinished.max()) == 0:
                break
    return seq
