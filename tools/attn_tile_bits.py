"""sha256 digests of what the three tile-core attention entry points (rgn_text_attention_bf16, rgn_lm_attention_bf16,
rgn_vae_attention_bf16) and the models on top of them write for seeded inputs: one `case digest` line each.

Run it once per library build, each in a fresh process (RGN_LIB selects the library), and diff the two listings: a change that claims to
move no bit of these kernels has to give the same digest in every line.  The fp64-reference tests would not see a one-ulp drift.

    python tools/attn_tile_bits.py > new.txt;  RGN_LIB=/path/to/other/libregione_hip.so python tools/attn_tile_bits.py > old.txt
    python tools/attn_tile_bits.py --no-models     # the kernel cases only
"""
import argparse
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from regione_amd import _lib, ops  # noqa: E402

_p, _stream = ops._p, ops._stream


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        torch.cuda.synchronize()
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def emit(case, *ts):
    print(f"{case:<44s} {digest(*ts)}", flush=True)


def randn(shape, seed, mul=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * mul).bfloat16().cuda()


def stress_qkv(L, cols, d, q_at, k_at, seed):
    """Logits (after the 1 / sqrt(d) scale) spread over [-30, 30]: q_i = +-a u, k_j = c_j a u with u a vector of signs, c_j uniform in
    [-1, 1] and c = 1 at the LAST key, so an even query's maximum sits in the last tile and every earlier running max is overtaken; an
    odd query (-a u) sees the mirror image."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, cols, generator=g)
    u = torch.sign(torch.randn(d, generator=g)) * math.sqrt(30.0 / math.sqrt(d))
    c = torch.rand(L, generator=g) * 2 - 1
    c[L - 1] = 1.0
    x[:, q_at:q_at + d] = u
    x[1::2, q_at:q_at + d] = -u
    x[:, k_at:k_at + d] = c[:, None] * u
    return x.bfloat16().cuda()


def text_cases(lib):
    for L in (1, 7, 77, 129, 512, 1000):
        for H in (1, 12, 64):
            qkv = randn((L, 3 * H * 64), 1000 * L + H)
            bias = randn((H, 2 * 1024 - 1), 7 * L + H, 2.0)
            for mode in ("bias", "causal", "neither"):
                o = torch.full((L, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
                rc = lib.rgn_text_attention_bf16(_p(qkv), _p(o), L, H, 0.125 if mode != "bias" else 1.0, int(mode == "causal"),
                                                 _p(bias) if mode == "bias" else None, 1024, _stream())
                _lib.check(rc, "rgn_text_attention_bf16")
                emit(f"text L={L} H={H} {mode}", o)
    L, H = 1000, 2
    qkv = stress_qkv(L, 3 * H * 64, 64, 0, H * 64, 5)
    for causal in (0, 1):
        o = torch.full((L, H * 64), float("nan"), dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.rgn_text_attention_bf16(_p(qkv), _p(o), L, H, 0.125, causal, None, 0, _stream()), "rgn_text_attention_bf16")
        emit(f"text stress L={L} causal={causal}", o)


def lm_cases(lib):
    for L in (1, 7, 129, 512, 1500, 4096):
        for hq, hkv in ((2, 1), (4, 4), (28, 4)):
            qkv = randn((L, (hq + 2 * hkv) * 128), 100 * L + hq)
            o = torch.full((L, hq * 128), float("nan"), dtype=torch.bfloat16, device="cuda")
            _lib.check(lib.rgn_lm_attention_bf16(_p(qkv), _p(o), L, hq, hkv, 128 ** -0.5, _stream()), "rgn_lm_attention_bf16")
            emit(f"lm L={L} Hq={hq} Hkv={hkv}", o)
    L = 1500
    qkv = stress_qkv(L, 4 * 128, 128, 0, 2 * 128, 6)
    o = torch.full((L, 2 * 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.rgn_lm_attention_bf16(_p(qkv), _p(o), L, 2, 1, 128 ** -0.5, _stream()), "rgn_lm_attention_bf16")
    emit(f"lm stress L={L}", o)


def vae_cases(lib):
    for H, W, C in ((1, 1, 512), (1, 1, 384), (7, 11, 512), (37, 53, 384), (61, 3, 512), (128, 128, 512), (128, 128, 384)):
        Hp, Wp = H + 2, W + 2
        q, k, v = (randn((Hp * Wp, C), 10 * H + W + s, 0.3) for s in (1, 2, 3))
        bv = randn((C,), H + W)
        for b in (None, bv):
            o = torch.zeros(Hp * Wp, C, dtype=torch.bfloat16, device="cuda")
            rc = lib.rgn_vae_attention_bf16(_p(q), _p(k), _p(v), _p(b), _p(o), Hp, Wp, C, C ** -0.5, _stream())
            _lib.check(rc, "rgn_vae_attention_bf16")
            emit(f"vae H={H} W={W} C={C} b_v={'no' if b is None else 'yes'}", o)
    H, W, C = 37, 27, 512                              # 999 pixels: the stress rows as a 37 x 27 image, the maximum in the last tile
    x = stress_qkv(H * W, 2 * C, C, 0, C, 8)
    Hp, Wp = H + 2, W + 2
    q, k = (torch.zeros(Hp, Wp, C, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    q[1:-1, 1:-1] = x[:, :C].view(H, W, C)
    k[1:-1, 1:-1] = x[:, C:].view(H, W, C)
    v = randn((Hp * Wp, C), 9)
    o = torch.zeros(Hp * Wp, C, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.rgn_vae_attention_bf16(_p(q), _p(k), _p(v), None, _p(o), Hp, Wp, C, C ** -0.5, _stream()), "rgn_vae_attention_bf16")
    emit(f"vae stress H={H} W={W} C={C}", o)


def model_cases():
    from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel, Qwen2_5_VLForConditionalGeneration
    import host_qwen_text_pipeline as HQ
    import host_vae
    from regione_amd import qwen_text_encoder as QT, text_encoders as TE, vae as V
    from text_encoder_bench import clip_cfg, t5_cfg
    from qwen_text_encoder_bench import full_size_config

    def built(make, cfg):
        torch.manual_seed(0)
        with torch.device("cuda"):
            m = make(cfg).eval()
        return m.to(torch.bfloat16)

    def ids(n, L, seed):
        return torch.randint(3, n - 3, (1, L), generator=torch.Generator().manual_seed(seed)).cuda()

    tiny_clip = CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2,
                               max_position_embeddings=77, bos_token_id=998, eos_token_id=2, pad_token_id=999)
    tiny_t5 = T5Config(vocab_size=500, d_model=256, d_kv=64, d_ff=640, num_layers=3, num_heads=4, feed_forward_proj="gated-gelu",
                       is_encoder_decoder=False)
    for name, make, cfg, L in (("clip tiny", CLIPTextModel, tiny_clip, 77), ("clip-l", CLIPTextModel, clip_cfg(), 77),
                               ("t5 tiny", T5EncoderModel, tiny_t5, 129), ("t5-xxl", T5EncoderModel, t5_cfg(), 512)):
        mod = built(make, cfg)
        hip = TE.HipClipTextModel(mod) if make is CLIPTextModel else TE.HipT5EncoderModel(mod, max_length=L)
        out = hip(ids(cfg.vocab_size, L, 11))
        emit(f"model {name} L={L}", *[t for t in (out.last_hidden_state, out.pooler_output) if t is not None])
        del mod, hip
        torch.cuda.empty_cache()
    tiny = HQ.tiny_qwen25vl(dtype=torch.bfloat16, layers=3).cuda()
    i = ids(HQ.VOCAB, 200, 12).clamp_(max=min(HQ.IMAGE, HQ.VIDEO, HQ.VISION_START, HQ.VISION_END) - 1)
    emit("model qwen2.5-vl lm tiny L=200", QT.HipQwen25VLTextEncoder(tiny)(input_ids=i, attention_mask=torch.ones_like(i)).last_hidden_state)
    del tiny
    mod = built(Qwen2_5_VLForConditionalGeneration, full_size_config())
    i = ids(151000, 1500, 13)
    emit("model qwen2.5-vl lm full L=1500", QT.HipQwen25VLTextEncoder(mod)(input_ids=i, attention_mask=torch.ones_like(i)).last_hidden_state)
    del mod
    torch.cuda.empty_cache()
    dec = V.HipVaeDecoder(host_vae.seeded(5).state_dict(), "cuda")
    dec.attention = "fused"
    z = torch.randn(1, 16, 160, 160, generator=torch.Generator().manual_seed(1)).cuda()    # (160 + 2)^2 > 24576: the fused kernel
    emit("model vae decode 1280x1280 fused", dec.decode(z))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-models", action="store_true")
    a = ap.parse_args()
    lib = _lib.lib()
    print(f"# library: {os.path.basename(_lib.LIB_PATH)}  device: {torch.cuda.get_device_name(0)}", flush=True)
    text_cases(lib)
    lm_cases(lib)
    vae_cases(lib)
    if not a.no_models:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        model_cases()


if __name__ == "__main__":
    main()
