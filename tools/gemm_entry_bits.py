"""sha256 digests of what the GEMM entry points write for seeded inputs: one `case plan digest...` line each.

Every way a caller reaches the GEMM kernel - ops.gemm / gemm_pair / gemm_qkv / gemm_qkv_pair / gemm_group and, with the C++ registration,
torch.ops.regione_mi.kv_partial_update_ / _pair_ - is host code in front of one dispatcher.  A change to that host code claims the same
launches and therefore the same bits.  Run this on both trees (it uses the public op names only, so it runs unmodified on either) and diff
the listings: every line has to be equal, the launch plan word included.  tests/test_gpu_gemm_entry_bits.py compares the tree with the
listing of the parent commit kept under tests/golden/.

    python tools/gemm_entry_bits.py > listing.txt

Inputs are drawn on the CPU with a fixed seed and copied to the device.  Shapes are the smallest at which each entry can go wrong: K = 128,
two heads (k | v | q blocks of 256 columns, N = 768), N = 1024 with a 256-column GELU half, skv_pad = 576; M = 8 / 200 / 520 (520 = three row
tiles of 256 with a ragged tail)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from regione_amd import _lib, ops, torch_ops  # noqa: E402

K, H, NQ, NMLP, SKV = 128, 2, 768, 1024, 576
HD = H * 128
CPP = torch_ops.REGISTRATION == "cpp"
CPP_PREFIX = "torch.ops "                       # the cases that need the C++ registration start with this


class Draw:
    """Seeded CPU draws, copied to the device."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def bf16(self, *shape, mul=1.0, add=0.0):
        return (torch.randn(shape, generator=self.g) * mul + add).bfloat16().cuda()

    def f32(self, *shape):
        return (torch.rand(shape, generator=self.g) * 2 - 1).cuda()

    def perm(self, n):
        return torch.randperm(n, generator=self.g).cuda()

    def weight(self, N, fp8, ldw=K):
        """[N, K] bf16 or fp8 (quantised on the CPU); ldw > K: a column slice of a wider matrix."""
        w = (torch.randn(N, ldw, generator=self.g) * 0.05).bfloat16()
        if not fp8:
            return w.cuda()[:, :K]
        q = ops.quantize_w8(w[:, :K])
        big = torch.zeros(N, ldw, dtype=ops.FP8).cuda()
        big.view(torch.uint8)[:, :K] = q.view(torch.uint8).cuda()
        v = big[:, :K]
        v._rgn_scale = q._rgn_scale.cuda()
        return v


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:32]


def fmt(fp8):
    return "fp8" if fp8 else "bf16"


# ---- plain epilogues ----------------------------------------------------------------------------------------------------------------
def single(d, M, fp8, epi, ldw=K, scatter=False):
    N = NMLP if epi == "gelu" else NQ
    A, W, b = d.bf16(M, K), d.weight(N, fp8, ldw), d.bf16(N)
    out = d.bf16(256 if scatter else M, N)
    kw = {}
    if epi == "gelu":
        kw = dict(epilogue=ops.EPI_GELU, gelu_from_col=NQ)
    elif epi == "gate":
        kw = dict(epilogue=ops.EPI_GATE_RESID, gate=d.bf16(N), resid=out)         # the residual aliases C
    if scatter:
        kw["out_rows"] = d.perm(256)[:M].contiguous()
    ops.gemm(A, W, b, out, **kw)
    return [out]


def pair(d, M0, M1, fp8, epi):
    W0, W1, b0, b1 = d.weight(NQ, fp8), d.weight(NQ, fp8), d.bf16(NQ), d.bf16(NQ)
    A0, A1, o0, o1 = d.bf16(M0, K), d.bf16(M1, K), d.bf16(M0, NQ), d.bf16(M1, NQ)
    kw = {}
    if epi == "gate":
        kw = dict(epilogue=ops.EPI_GATE_RESID, gate0=d.bf16(NQ), resid0=o0, gate1=d.bf16(NQ), resid1=o1)
    ops.gemm_pair(A0, W0, b0, o0, A1, W1, b1, o1, **kw)
    return [o0, o1]


def group4(d, fp8):
    """(image, text) x (cond, uncond): the branches of a stream share W."""
    Wi, Wt = d.weight(NQ, fp8), d.weight(NQ, fp8)
    probs, outs = [], []
    for M, W in ((200, Wi), (8, Wt), (200, Wi), (8, Wt)):
        o = d.bf16(M, NQ)
        probs.append(ops.Problem(d.bf16(M, K), W, d.bf16(NQ), o, gate=d.bf16(NQ), resid=o))
        outs.append(o)
    ops.gemm_group(probs, epilogue=ops.EPI_GATE_RESID)
    return outs


# ---- fused Q/K/V epilogue -----------------------------------------------------------------------------------------------------------
class Cache:
    """Rotary tables, per-head RMSNorm weights, cache-row list and zeroed K / V^T slabs of one joint [text | image] sequence."""

    def __init__(self, d, permute):
        self.cos_q, self.sin_q, self.cos_k, self.sin_k = (d.f32(SKV, 128) for _ in range(4))
        self.kv_rows = d.perm(SKV) if permute else None
        self.k_slab = torch.zeros(SKV, HD, dtype=torch.bfloat16, device="cuda")
        self.vt_slab = torch.zeros(HD, SKV, dtype=torch.bfloat16, device="cuda")

    def epi(self, d, M, row_base, rt):
        wq, wk = d.bf16(128, mul=0.1, add=1.0), d.bf16(128, mul=0.1, add=1.0)
        return wq, wk, ops.qkv_epilogue(wq=wq, wk=wk, rope_q=(self.cos_q, self.sin_q), rope_k=(self.cos_k, self.sin_k), k_slab=self.k_slab,
                                        vt_slab=self.vt_slab, H=H, k_col=0, v_col=HD, q_col=2 * HD, kv_rows=self.kv_rows, row_base=row_base,
                                        fp16_roundtrip=rt, rows=M)


def qkv_single(d, M, fp8, mlp, permute, rt, cpp=False):
    N = NMLP if mlp else NQ
    c = Cache(d, permute)
    A, W, b, out = d.bf16(M, K), d.weight(N, fp8), d.bf16(N), torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    wq, wk, e = c.epi(d, M, 0, rt)
    if cpp:
        torch_ops.R.kv_partial_update_(A, W, b, out, wq, wk, c.cos_q, c.sin_q, c.cos_k, c.sin_k, c.kv_rows, c.k_slab, c.vt_slab, H, 0, 1e-6, rt,
                                       NQ if mlp else -1)
    else:
        ops.gemm_qkv(A, W, b, out, e, gelu_from_col=NQ if mlp else None)
    return [out, c.k_slab, c.vt_slab]


def qkv_pair(d, M_img, M_txt, fp8, cpp=False):
    """Image rows sit behind the text rows of the joint sequence (row_base = M_txt), cache rows permuted, fp16 round trip on the image."""
    c = Cache(d, True)
    Wi, Wt, bi, bt = d.weight(NQ, fp8), d.weight(NQ, fp8), d.bf16(NQ), d.bf16(NQ)
    Ai, At = d.bf16(M_img, K), d.bf16(M_txt, K)
    oi, ot = (torch.zeros(M, NQ, dtype=torch.bfloat16, device="cuda") for M in (M_img, M_txt))
    wqi, wki, ei = c.epi(d, M_img, M_txt, True)
    wqt, wkt, et = c.epi(d, M_txt, 0, False)
    if cpp:
        torch_ops.R.kv_partial_update_pair_(Ai, Wi, bi, oi, wqi, wki, At, Wt, bt, ot, wqt, wkt, c.cos_q, c.sin_q, c.cos_k, c.sin_k, c.kv_rows,
                                            c.k_slab, c.vt_slab, H, M_txt, 1e-6, True)
    else:
        ops.gemm_qkv_pair(Ai, Wi, bi, oi, ei, At, Wt, bt, ot, et)
    return [oi, ot, c.k_slab, c.vt_slab]


def cases():
    out = []
    for fp8 in (False, True):
        f = fmt(fp8)
        for M in (8, 200, 520):
            out.append((f"single {f} M={M} bias", lambda d, M=M, fp8=fp8: single(d, M, fp8, "bias")))
        for epi in ("gelu", "gate"):
            out.append((f"single {f} M=520 {epi}", lambda d, fp8=fp8, epi=epi: single(d, 520, fp8, epi)))
        out.append((f"single {f} M=200 row scatter", lambda d, fp8=fp8: single(d, 200, fp8, "bias", scatter=True)))
        out.append((f"single {f} M=200 ldw=192", lambda d, fp8=fp8: single(d, 200, fp8, "bias", ldw=192)))
        for M0, M1 in ((520, 8), (200, 0), (0, 8)):
            for epi in ("bias", "gate"):
                out.append((f"pair {f} M=({M0},{M1}) {epi}", lambda d, M0=M0, M1=M1, fp8=fp8, epi=epi: pair(d, M0, M1, fp8, epi)))
        for M in (8, 520):
            for mlp in (False, True):
                for permute in (False, True):
                    for rt in (False, True):
                        out.append((f"qkv {f} M={M} mlp={int(mlp)} perm={int(permute)} rt={int(rt)}",
                                    lambda d, M=M, fp8=fp8, mlp=mlp, permute=permute, rt=rt: qkv_single(d, M, fp8, mlp, permute, rt)))
        out.append((f"qkv pair {f} M=(520,8)", lambda d, fp8=fp8: qkv_pair(d, 520, 8, fp8)))
        out.append((f"group of four {f}", lambda d, fp8=fp8: group4(d, fp8)))
        out.append((f"{CPP_PREFIX}kv_partial_update_ {f} M=520 mlp", lambda d, fp8=fp8: qkv_single(d, 520, fp8, True, True, True, cpp=True)))
        out.append((f"{CPP_PREFIX}kv_partial_update_ {f} M=8", lambda d, fp8=fp8: qkv_single(d, 8, fp8, False, False, False, cpp=True)))
        out.append((f"{CPP_PREFIX}kv_partial_update_pair_ {f} M=(520,8)", lambda d, fp8=fp8: qkv_pair(d, 520, 8, fp8, cpp=True)))
    return out


CASES = cases()


def run_case(name, fn, seed):
    outs = fn(Draw(seed))
    plan = _lib.lib().rgn_gemm_last_plan()
    torch.cuda.synchronize()
    return f"{name:<44s} plan=0x{plan:03x} " + " ".join(digest(t) for t in outs)


def listing():
    """One line per case; the cases of the C++ registration only when this process holds it."""
    return [run_case(name, fn, 1000 + 7 * i) for i, (name, fn) in enumerate(CASES) if CPP or not name.startswith(CPP_PREFIX)]


def main():
    _lib.lib()
    print(f"# library ABI {_lib.lib().rgn_version()}  registration: {torch_ops.REGISTRATION}  device: {torch.cuda.get_device_name(0)}", flush=True)
    for line in listing():
        print(line, flush=True)


if __name__ == "__main__":
    main()
