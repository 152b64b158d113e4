"""CPU: hazard checks on the 64-query-row attention loop (RGN_ATTN_LOOP_W64_ASM) and the kernel built around it.

1. The generated statement keeps its MFMA results away from the VALU: nothing the hardware does orders a VALU read (or overwrite) of an asm
   MFMA's destination behind that MFMA, so every such instruction must sit behind two later MFMAs (64 matrix-pipe cycles) or 32 wait states.
2. The statement stays inside the registers it declares (v32-v239, a0-a191), uses no packed-fp32 / dot2 VALU, and never issues an LDS-DMA
   straight behind its m0 write.
3. The committed .inc is what tools/gen_attn_loop.py generates.
4. The compiler parks nothing in a0-a191 of attention_asm64_kernel, which runs with 0 scratch at one wave per SIMD.  ~40 s of hipcc."""
import importlib.util
import os
import re
import subprocess

import pytest

from regione_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "regione_amd", "csrc", "attn_loop_asm.inc")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_attn_loop", os.path.join(ROOT, "tools", "gen_attn_loop.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _macro(name):
    txt = open(INC).read()
    m = re.search(r"#define " + name + r" \\\n(.*?)\n    \"\"", txt, re.S)
    return [l.strip()[1:].split("\\n")[0] for l in m.group(1).split("\n") if l.strip().startswith('"')]


def test_committed_loop_is_the_generated_one():
    gen = _gen()
    assert _macro("RGN_ATTN_LOOP_W64_ASM") == gen.w_emit()


def test_mfma_results_keep_their_distance_from_the_valu():
    gen = _gen()
    lines = _macro("RGN_ATTN_LOOP_W64_ASM")
    found = gen.mfma_valu_distances(lines)
    # the first VALU touch of each of the 64 S elements per lane, in the prologue's S(0) and the three bodies that compute an S(t+1): always
    # the scale-and-shift fma; the loop never reads O back
    assert len(found) == 4 * 64
    for between, states, l in found:
        assert between >= 2 or states >= 32, (between, states, l)
        assert l.split()[0] == "v_fma_f32", l


def test_the_distance_checker_sees_a_close_read():
    gen = _gen()
    lines = ["v_mfma_f32_32x32x16_bf16 v[32:47], v[192:195], a[128:131], 0", "v_mfma_f32_32x32x16_bf16 a[0:15], v[192:195], v[160:163], a[0:15]",
             "v_fma_f32 v33, v33, s0, v224", "s_nop 15", "s_nop 15", "v_accvgpr_read_b32 v1, a3"]
    assert [(b, s) for b, s, _ in gen.mfma_valu_distances(lines)] == [(1, 1), (0, 33)]


def test_every_body_label_waits_for_the_prologues_reads():
    """Each body label (loop top 31, remainder 32, last tile 33) can be reached straight from the prologue, whose last instructions request K
    fragments 0-3: the first MFMA behind each label that reads a fragment slot must have an lgkmcnt wait between the label and itself."""
    lines = _macro("RGN_ATTN_LOOP_W64_ASM")
    for label in ("31:", "32:", "33:"):
        i = lines.index(label)
        j = next(k for k in range(i, len(lines)) if lines[k].startswith("v_mfma"))
        assert any(l.startswith("s_waitcnt lgkmcnt") for l in lines[i:j]), label


def test_statement_stays_inside_its_registers():
    gen = _gen()
    lines = _macro("RGN_ATTN_LOOP_W64_ASM")
    gen.w_selfcheck(lines)
    txt = open(INC).read()
    clob = re.search(r"#define RGN_ATTN_LOOP_W64_CLOBBERS (.*)", txt).group(1)
    assert {f'"a{n}"' for n in range(192)} | {f'"v{n}"' for n in range(32, 240)} <= set(c.strip() for c in clob.split(","))
    with pytest.raises(AssertionError):
        gen.w_selfcheck(lines + ["v_mov_b32 v240, v32"])


def test_kernel_resources_and_no_parked_accumulator(tmp_path):
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "attn.s")
    cmd = [build.HIPCC, *build.FLAGS, *build.EXTRA.get("attn.hip", []), "--cuda-device-only", "-S", "-o", out, os.path.join(build.CSRC, "attn.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    m = re.search(r"^(_ZN3rgn22attention_asm64_kernel\w+):", asm, re.M)
    assert m
    name = m.group(1)
    end = asm.find(".Lfunc_end", m.end())
    own, inside = [], False
    for line in asm[m.end():end].split("\n"):
        if "ASMSTART" in line:
            inside = True
        elif "ASMEND" in line:
            inside = False
        elif not inside:
            own.append(line.split(";")[0].strip())
    bad = [l for l in own if re.match(r"(?!global_store|buffer_store|scratch_store|ds_write|flat_store)\S+\s+a(\d+|\[\d+:\d+\])\s*,", l)]
    assert not bad, bad[:4]
    def meta(key):
        return int(re.search(r"\.set " + re.escape(name) + r"\." + key + r", (\d+)", asm).group(1))
    assert meta("private_seg_size") == 0
    assert meta("num_vgpr") <= 256 and meta("num_agpr") == 192
    assert meta("num_vgpr") + meta("num_agpr") > 256            # more than half the file: one wave per SIMD
