"""Launch records and sha256 digests of what the four HIP VAE objects compute for seeded inputs: one `case launches record output` line each.

regione_amd/vae.py and regione_amd/qwen_vae.py are host code in front of the `rgn_` entry points.  A change to that host code claims the same
launches, in the same order with the same arguments, the same bits and the same device memory.  Run this on both trees (it uses the public
surface of the two modules only, so it runs unmodified on either) and diff the listings: every line has to be equal.
tests/test_gpu_vae_bits.py compares the tree with the listing of the parent commit kept under tests/golden/.

    python tools/vae_bits.py > listing.txt

The library handle is wrapped in a recorder that notes, per call of an entry that takes a stream, the entry's name and every argument
declared as int / float / double / size_t (pointers are skipped; for rgn_gemm_group each problem's M, lda, ldc, ldw too).  Weights are
tests/host_vae.seeded(3) and tests/host_qwen_vae.seeded(4); inputs are drawn on the CPU with a seed fixed by the size.  Each object is adopted
once (per pixel_groups / out_dtype, which are constructor arguments) and its switches are flipped.  The last lines walk one decoder and
one encoder per family through the sizes of tests/test_gpu_vae_reuse.py and print the device bytes the objects and their pools hold."""
import contextlib
import ctypes as C
import gc
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from regione_amd import _lib, qwen_vae as Q, vae as V  # noqa: E402
from tests import host_qwen_vae, host_vae  # noqa: E402

_SCALARS = (C.c_int, C.c_float, C.c_double, C.c_size_t)
LATENTS = [(8, 8), (16, 16), (8, 16), (5, 7)]
IMAGES = [(64, 64), (128, 128), (64, 128)]
WALK = [(8, 8), (16, 16), (8, 8), (8, 16)]


class Recorder:
    """The ctypes handle with every stream-taking entry noted in `calls` as (name, {argument index: value}, ...)."""

    def __init__(self, handle):
        self._h, self.calls = handle, []

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        types = _lib.SIGNATURES.get(name)
        if not types or types[-1] is not C.c_void_p:               # queries and settings: no stream, no launch
            return fn

        def call(*args):
            rec = [name] + [f"{i}={a!r}" for i, (a, t) in enumerate(zip(args, types)) if t in _SCALARS]
            if name == "rgn_gemm_group":
                rec += [f"p{i}=({args[0][i].M},{args[0][i].lda},{args[0][i].ldc},{args[0][i].ldw})" for i in range(args[1])]
            self.calls.append(tuple(rec))
            return fn(*args)
        return call

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


@contextlib.contextmanager
def recording():
    """Wrap the loaded library handle for the duration of the block; yields the Recorder."""
    h = _lib.lib()
    rec = _lib._lib = Recorder(h)
    try:
        yield rec
    finally:
        _lib._lib = h


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:32]


def latent(h, w):
    g = torch.Generator().manual_seed(h * 100 + w)
    return torch.randn(1, 16, h, w, generator=g).to("cuda", torch.bfloat16)


def image(H, W):
    g = torch.Generator().manual_seed(H * 100 + W + 1)
    return (torch.rand(1, 3, H, W, generator=g) * 2 - 1).to("cuda", torch.bfloat16)


def line(name, fn):
    with recording() as rec:
        out = fn()
        torch.cuda.synchronize()
    record = hashlib.sha256("\n".join(" ".join(c) for c in rec.calls).encode()).hexdigest()[:32]
    return f"{name:<64s} launches={len(rec.calls):<4d} record={record} out={digest(out)}"


def _tf(b):
    return "T" if b else "F"


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj


def kl_lines(sd):
    out = []
    dec = {pg: V.HipVaeDecoder(sd, "cuda", pixel_groups=pg) for pg in (True, False)}
    enc = {pg: V.HipVaeEncoder(sd, "cuda", pixel_groups=pg) for pg in (True, False)}
    for h, w in LATENTS:
        for gn, up in ((True, True), (False, False), (True, False)):
            for pg in (True, False):
                for att in ("materialized", "fused"):
                    d = _set(dec[pg], fuse_gn=gn, fuse_upsample=up, attention=att)
                    out.append(line(f"kl decode {h}x{w} gn={_tf(gn)} up={_tf(up)} pg={_tf(pg)} {att}", lambda: d.decode(latent(h, w))))
    for H, W in IMAGES:
        for gn in (True, False):
            for pg in (True, False):
                for att in ("materialized", "fused"):
                    e = _set(enc[pg], fuse_gn=gn, attention=att)
                    out.append(line(f"kl encode {H}x{W} gn={_tf(gn)} pg={_tf(pg)} {att}", lambda: e.encode(image(H, W))))
    d, e = _set(dec[True], fuse_gn=True, fuse_upsample=True, attention="auto"), _set(enc[True], fuse_gn=True, attention="auto")
    with _lib.plan_override(gemm_geometry=256):
        out.append(line("kl decode 16x16 geometry=256", lambda: d.decode(latent(16, 16))))
        out.append(line("kl encode 128x128 geometry=256", lambda: e.encode(image(128, 128))))
    return out


def qwen_lines(sd):
    out = []
    dts = ((torch.bfloat16, "bf16"), (torch.float32, "fp32"))
    dec = {(pg, n): Q.HipQwenVaeDecoder(sd, "cuda", out_dtype=dt, pixel_groups=pg) for pg in (True, False) for dt, n in dts}
    enc = {(pg, n): Q.HipQwenVaeEncoder(sd, "cuda", out_dtype=dt, pixel_groups=pg) for pg in (True, False) for dt, n in dts}
    for objs, sizes, what, call, draw in ((dec, LATENTS, "decode", lambda o, x: o.decode(x[:, :, None]), latent),
                                          (enc, IMAGES, "encode", lambda o, x: o.encode(x[:, :, None]), image)):
        for a, b in sizes:
            for att in ("materialized", "fused"):
                for pg in (True, False):
                    for _, n in dts:
                        o = _set(objs[(pg, n)], attention=att)
                        out.append(line(f"qwen {what} {a}x{b} pg={_tf(pg)} {att} {n}", lambda: call(o, draw(a, b))))
    d, e = _set(dec[(True, "bf16")], attention="auto"), _set(enc[(True, "bf16")], attention="auto")
    with _lib.plan_override(gemm_geometry=256):
        out.append(line("qwen decode 16x16 geometry=256", lambda: d.decode(latent(16, 16)[:, :, None])))
        out.append(line("qwen encode 128x128 geometry=256", lambda: e.encode(image(128, 128)[:, :, None])))
    return out


def walk_lines(kind, sd):
    """The reuse walk of tests/test_gpu_vae_reuse.py: one decoder and one encoder interleaved on one stream, then the bytes they hold."""
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    if kind == "qwen":
        dec, enc = Q.HipQwenVaeDecoder(sd, "cuda"), Q.HipQwenVaeEncoder(sd, "cuda")
        decode, encode = (lambda z: dec.decode(z[:, :, None])), (lambda x: enc.encode(x[:, :, None]))
    else:
        fuse = kind == "kl_fused"
        dec, enc = _set(V.HipVaeDecoder(sd, "cuda"), fuse_gn=fuse, fuse_upsample=fuse), _set(V.HipVaeEncoder(sd, "cuda"), fuse_gn=fuse)
        decode, encode = dec.decode, enc.encode
    out = []
    for i, (h, w) in enumerate(WALK):
        out.append(line(f"walk {kind} #{i} decode {h}x{w}", lambda: decode(latent(h, w))))
        out.append(line(f"walk {kind} #{i} encode {8 * h}x{8 * w}", lambda: encode(image(8 * h, 8 * w))))
    torch.cuda.synchronize()
    out.append(f"{'walk ' + kind + ' bytes held':<64s} {torch.cuda.memory_allocated() - before}")
    return out


def listing():
    kl, qw = host_vae.seeded(3).state_dict(), host_qwen_vae.seeded(4).state_dict()
    out = kl_lines(kl) + qwen_lines(qw)               # the walks come last: every per-stream workspace exists by then
    for kind, sd in (("kl_fused", kl), ("kl_unfused", kl), ("qwen", qw)):
        out += walk_lines(kind, sd)
    return out


def main():
    print(f"# library ABI {_lib.lib().rgn_version()}  device: {torch.cuda.get_device_name(0)}", flush=True)
    for ln in listing():
        print(ln, flush=True)


if __name__ == "__main__":
    main()
