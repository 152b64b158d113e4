"""sha256 digests of what rgn_attention_bounded / rgn_attention write for seeded inputs: one `case digest` line each.

The 64-query-row, one-wave-per-SIMD kernel (attention_asm64_kernel) claims the bits of the 8-wave kernel it replaces on unsplit static-shift
launches.  Run this once per library build, each in a fresh process (RGN_LIB selects the library), and diff the listings: every line has to
carry the same digest.  tests/test_gpu_attn_w64_bits.py compares the in-tree library with the listing of the parent library kept under
tests/golden/.

    python tools/attn_w64_bits.py > new.txt;  RGN_LIB=/path/to/parent/libregione_hip.so python tools/attn_w64_bits.py > parent.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from regione_amd import _lib, ops  # noqa: E402

H = 24
D = H * 128
BOUND_U = 1.25                                  # |q_d| = |k_d| = 1.25 (exact in bf16): q . k / sqrt(128) = +-128 * 1.5625 / sqrt(128)
BOUND = 17.68                                   # >= 17.6777 = the largest |score| of the adversarial rows


def force(knobs):
    _lib.lib().rgn_plan_override(None, 0)
    for k, v in knobs.items():
        _lib.check(_lib.lib().rgn_plan_override(k.encode(), int(v)), k)


def randn(shape, seed, mul=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * mul).bfloat16().cuda()


def adversarial(Sq, Skv, seed):
    """Every score of head 0 sits in [-score_bound, +score_bound] and reaches both ends: q_i = +-1.25 u (sign by row parity), k_j = c_j 1.25 u
    with c_j uniform in [-1, 1], c = +1 at the first and the last key and -1 at key 1.  The other heads are random."""
    g = torch.Generator().manual_seed(seed)
    q, k = torch.randn(Sq, D, generator=g), torch.randn(Skv, D, generator=g)
    u = torch.sign(torch.randn(128, generator=g)) * BOUND_U
    c = torch.rand(Skv, generator=g) * 2 - 1
    c[0], c[1], c[Skv - 1] = 1.0, -1.0, 1.0
    q[:, :128] = u
    q[1::2, :128] = -u
    k[:, :128] = c[:, None] * u
    return q.bfloat16().cuda(), k.bfloat16().cuda()


# (name, Sq, Skv, score_bound, plan knobs, adversarial).  Launch classes that moved to the 64-row kernel: the whole rounds in front of a split
# or stream-K remainder (816 items), a launch that is one partial round (144 / 240 items), and - attn_split = 0 - rounds plus an unsplit tail.
CASES = [
    ("full step 8704^2", 8704, 8704, 20.0, {}, False),
    ("full step 8704^2 no split", 8704, 8704, 20.0, dict(attn_split=0), False),
    ("full step 8704^2 adversarial", 8704, 8704, BOUND, {}, True),
    ("region Sq=1536 Skv=8704", 1536, 8704, 20.0, {}, False),
    ("region Sq=1536 Skv=8704 adversarial", 1536, 8704, BOUND, {}, True),
    ("region Sq=1536 Skv=8704 no split", 1536, 8704, 20.0, dict(attn_split=0), False),
    ("region Sq=708 Skv=8704", 708, 8704, 20.0, {}, False),
    ("region Sq=708 Skv=8704 8 waves", 708, 8704, 20.0, dict(attn_waves=8), False),
    ("region Sq=708 Skv=8704 8 waves no split adversarial", 708, 8704, BOUND, dict(attn_waves=8, attn_split=0), True),
    ("region Sq=1536 Skv=2560", 1536, 2560, 20.0, {}, False),
    ("region Sq=708 Skv=2560 8 waves no split", 708, 2560, 20.0, dict(attn_waves=8, attn_split=0), False),
    ("ragged rows Sq=2500 Skv=4160 (65 tiles)", 2500, 4160, 20.0, dict(attn_waves=8, attn_split=0), False),
    ("ragged rows Sq=2821 Skv=4160 stream-K", 2821, 4160, 20.0, dict(attn_waves=8, attn_streamk=1), False),
    ("one tile Sq=300 Skv=64", 300, 64, 20.0, dict(attn_waves=8, attn_split=0), False),
    ("two tiles Sq=300 Skv=128", 300, 128, 20.0, dict(attn_waves=8, attn_split=0), True),
    ("three tiles Sq=257 Skv=192", 257, 192, 20.0, dict(attn_waves=8, attn_split=0), False),
    ("running max 8704^2 (unchanged kernels)", 8704, 8704, 0.0, {}, False),
    ("ragged KV Sq=1536 Skv=8700 (unchanged kernels)", 1536, 8700, 20.0, {}, False),
]


def run_case(name, Sq, Skv, bound, knobs, adv, seed):
    skv_pad = (Skv + 63) // 64 * 64
    if adv:
        q, k = adversarial(Sq, Skv, seed)
    else:
        q, k = randn((Sq, D), seed), randn((Skv, D), seed + 1)
    v = randn((Skv, D), seed + 2)
    k_slab = torch.zeros(skv_pad, D, dtype=torch.bfloat16, device="cuda")
    k_slab[:Skv] = k
    vt_slab = torch.zeros(D, skv_pad, dtype=torch.bfloat16, device="cuda")
    vt_slab[:, :Skv] = v.t()
    # the V^T slab keeps the kv index permuted inside 16-groups exactly as rgn_qk_norm_rope_store writes it; for a digest comparison between
    # two libraries any fixed content serves, the plain transpose included
    out = torch.full((Sq, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    force(knobs)
    try:
        ops.attention(q, k_slab, vt_slab, out, Skv, H, score_bound=bound)
        plan = _lib.lib().rgn_attention_last_plan()
    finally:
        force({})
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any(), name
    h = hashlib.sha256(out.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
    return f"{name:<56s} plan=0x{plan:02x} {h}"


def listing():
    return [run_case(*c, seed=100 + 10 * i) for i, c in enumerate(CASES)]


def main():
    _lib.lib()
    print(f"# library: {os.path.basename(_lib.LIB_PATH)}  device: {torch.cuda.get_device_name(0)}", flush=True)
    for i, c in enumerate(CASES):
        print(run_case(*c, seed=100 + 10 * i), flush=True)


if __name__ == "__main__":
    main()
