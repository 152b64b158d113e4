#!/usr/bin/env python3
"""Issue-slot budget of the hand-scheduled attention KV loop ("a profiles/ instruction-slot budget - issue cycles
per tile by unit, from the generated loop - proving the floor").

Parses the steady-state loop body of the shipped `RGN_ATTN_LOOP_SM_ASM` (static-shift softmax: the pipeline's path) and of
`RGN_ATTN_LOOP_ASM` (running max) in regione_amd/csrc/attn_loop_asm.inc - the body between the loop label and its back branch covers TWO KV
tiles (the two S-register parities) - classifies every instruction and prices it with the issue / occupancy costs of
/opt/skills/guides/MI355X_MICROARCH.md (wave64 on a SIMD16):

    v_mfma_f32_32x32x16_bf16   8 passes x 4 cycles = 32 cycles of the matrix pipe (32768 FLOP at 1024 FLOP / clk / SIMD = 2.5 PFLOP/s chip-wide), 4 issue cycles
    VALU fp32 / int / cvt_pk    4 cycles (one wave64 instruction on 16 lanes)
    v_exp_f32 (transcendental) ~5/3 of a plain VALU instruction beside MFMAs = 6.7 cycles (MI355X_MICROARCH.md, two-wave pairing section)
    ds_read_b128                issue 4 cycles; LDS array 4 cycles per wave-instruction (256 B/clk/CU, MI355X_MICROARCH.md LDS table),
                                one array per CU shared by its four SIMDs
    buffer_load ... lds         issue 4 cycles (+ ~60-185 cycles of address work on the issuing wave, measured in the microarch guide)
    SALU / waitcnt / barrier    4 cycles issue (scalar pipe, overlaps VALU issue of the OTHER wave)

A SIMD runs TWO waves of the workgroup; the matrix pipe is shared by them: per tile and SIMD it is busy 2 x 32 x 32 = 2048 cycles.  The measured tile time comes from the kernel-trace profile (us per launch / KV tiles per workgroup).

    python tools/attn_issue_budget.py [--clock-mhz 1817] [--tile-us 1.69] > profiles/r06_attn_issue_budget.txt
"""
import argparse
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def body(macro):
    txt = open(os.path.join(ROOT, "regione_amd", "csrc", "attn_loop_asm.inc")).read()
    m = re.search(r"#define " + macro + r" \\\n(.*?)\n    \"\"", txt, re.S)
    lines = [l.strip()[1:].split("\\n")[0] for l in m.group(1).split("\n") if l.strip().startswith('"')]
    start = next(i for i, l in enumerate(lines) if re.match(r"^\d+:$", l))
    end = next(i for i, l in enumerate(lines) if i > start and l.startswith("s_cbranch") and l.endswith("b"))
    return lines[start + 1:end + 1]


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_exp") or op.startswith("v_rcp") or op.startswith("v_log"):
        return "valu_trans"
    if op.startswith("ds_read") or op.startswith("ds_write"):
        return "lds"
    if op.startswith("buffer_load") or op.startswith("global_load"):
        return "vmem_dma"
    if op.startswith("v_accvgpr"):
        return "valu_acc"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    return "other"


def w64(ns):
    """RGN_ATTN_LOOP_W64_ASM: ONE wave per SIMD, 64 query rows (64 MFMAs per tile and wave).  Priced per MFMA gap with the one-wave constants of the
    microarchitecture guide: the MFMA holds vector issue for 8 of its 32 cycles, v_exp_f32 8, other VALU / ds_read 4, costs add; up to ~24 cycles of
    fillers hide in a gap."""
    b = body("RGN_ATTN_LOOP_W64_ASM")
    cnt = collections.Counter(classify(i) for i in b)
    tiles = cnt["mfma"] / 64.0
    per = {k: v / tiles for k, v in cnt.items()}
    issue = {"mfma": 8, "valu": 4, "valu_acc": 4, "valu_trans": 8, "lds": 4, "vmem_dma": 4, "salu": 4, "waitcnt": 4, "barrier": 4, "other": 4}
    print("## RGN_ATTN_LOOP_W64_ASM: static shift, 4 waves x 64 query rows, one wave per SIMD")
    print(f"loop body = {len(b)} instructions over {tiles:.0f} KV tiles (64 keys each) for one wave (64 query rows)")
    print(f"{'class':<12} {'per tile':>9} {'issue cyc':>10} {'per gap':>8}")
    vec = 0.0
    for k in ("mfma", "valu", "valu_trans", "lds", "vmem_dma", "salu", "waitcnt", "barrier"):
        if k in per:
            c = per[k] * issue[k]
            print(f"{k:<12} {per[k]:9.1f} {c:10.0f} {c / 64:8.1f}")
            if k in ("valu", "valu_trans", "lds", "vmem_dma"):
                vec += c
    gaps, cur = [], None
    for i in b:                                                   # issue cycles of the fillers behind each MFMA
        k = classify(i)
        if k == "mfma":
            if cur is not None:
                gaps.append(cur)
            cur = 0.0
        elif cur is not None and k in ("valu", "valu_trans", "lds", "vmem_dma"):
            cur += issue[k]
    gaps.append(cur)
    valu_busy = per.get("valu", 0) * 4 + per.get("valu_trans", 0) * 8
    cyc = ns.w64_tile_us * ns.clock_mhz
    print("per SIMD (ONE wave) and KV tile:")
    print(f"  matrix pipe busy      {per['mfma'] * 32:7.0f} cycles   ({per['mfma']:.0f} MFMAs x 32)")
    print(f"  VALU issue            {valu_busy:7.0f} cycles   (fp32 / cvt at 4, exp2 at 8 cycles per wave64 instruction, one wave alone)")
    print(f"  LDS array (CU-wide)   {per.get('lds', 0) * 4 * 4 + 256:7.0f} cycles   ({per.get('lds', 0):.0f} ds_read_b128 x 4 waves x 4 cycles + 32 KiB of LDS-DMA writes at 128 B/clk)")
    print(f"  vector fillers        {vec:7.0f} cycles   = {vec / 64:.1f} of the 24 a 32-cycle MFMA gap hides; per gap min {min(gaps):.0f} / max {max(gaps):.0f}, "
          f"{sum(g > 24 for g in gaps)} of {len(gaps)} gaps above 24")
    print(f"  ... + scalar / waits  {vec + sum(per.get(k, 0) * 4 for k in ('salu', 'waitcnt', 'barrier')):7.0f} cycles   (SALU, s_waitcnt, barrier at 4 each: one wave has no partner to issue them beside)")
    print(f"  LDS-DMA pieces        {per.get('vmem_dma', 0):7.0f}          (x 60-185 cycles of address work each on the issuing wave: 480-1480 cycles, the same per SIMD as in the 8-wave loop)")
    print(f"  measured tile time    {cyc:7.0f} cycles   ({ns.w64_tile_us} us at {ns.clock_mhz:.0f} MHz)")
    print(f"  => matrix pipe {per['mfma'] * 32 / cyc:.2f} of the tile time, VALU {valu_busy / cyc:.2f}, LDS array {(per.get('lds', 0) * 16 + 256) / cyc:.2f}")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-mhz", type=float, default=1817.0, help="sustained clock of the attention kernel (profiles/r05_clock_probe.json)")
    ap.add_argument("--tile-us", type=float, default=1.69, help="measured time per KV tile of a full-round launch (DESIGN 4.3 cost model c_t)")
    ap.add_argument("--w64-tile-us", type=float, default=1.60, help="measured time per KV tile of a full-round launch of the 64-row kernel")
    ns = ap.parse_args()
    for macro, label in (("RGN_ATTN_LOOP_SM_ASM", "static-shift softmax (the pipeline's path)"), ("RGN_ATTN_LOOP_ASM", "running max")):
        b = body(macro)
        cnt = collections.Counter(classify(i) for i in b)
        tiles = cnt["mfma"] / 32.0                       # 16 QK + 16 PV MFMAs per tile and wave
        per = {k: v / tiles for k, v in cnt.items()}
        issue = {"mfma": 4, "valu": 4, "valu_acc": 4, "valu_trans": 20.0 / 3.0, "lds": 4, "vmem_dma": 4, "salu": 4, "waitcnt": 4, "barrier": 4, "other": 4}
        print(f"## {macro}: {label}")
        print(f"loop body = {len(b)} instructions over {tiles:.0f} KV tiles (64 keys each) for one wave (32 query rows)")
        print(f"{'class':<12} {'per tile':>9} {'issue cyc':>10}")
        tot_vec = 0.0
        for k in ("mfma", "valu", "valu_trans", "valu_acc", "lds", "vmem_dma", "salu", "waitcnt", "barrier", "other"):
            if k in per:
                c = per[k] * issue[k]
                print(f"{k:<12} {per[k]:9.1f} {c:10.0f}")
                if k in ("mfma", "valu", "valu_trans", "valu_acc", "lds", "vmem_dma"):
                    tot_vec += c
        mfma_pipe = per["mfma"] * 32
        valu_busy = per.get("valu", 0) * 4 + per.get("valu_trans", 0) * 20.0 / 3.0 + per.get("valu_acc", 0) * 4
        lds_port = per.get("lds", 0) * 8 * 8 / 4.0        # 8 waves' reads through one CU port, seen from one SIMD's share of time: x 8 waves / 4 SIMDs
        print(f"per SIMD (TWO waves) and KV tile:")
        print(f"  matrix pipe busy      {2 * mfma_pipe:7.0f} cycles   (2 waves x {per['mfma']:.0f} MFMAs x 32)")
        print(f"  VALU pipe busy        {2 * valu_busy:7.0f} cycles   (fp32 / cvt at 4, exp2 at 6.7 cycles per wave64 instruction)")
        print(f"  LDS array (CU-wide)   {per.get('lds', 0) * 8 * 4 + 256:7.0f} cycles   ({per.get('lds', 0):.0f} ds_read_b128 x 8 waves x 4 cycles + 32 KiB of LDS-DMA writes at 128 B/clk)")
        tot_all = tot_vec + sum(per.get(k, 0) * 4 for k in ("salu", "waitcnt", "barrier", "other"))
        print(f"  vector issue slots    {2 * tot_vec:7.0f} cycles   (every MFMA / VALU / LDS / VMEM instruction of both waves, 4 cycles each, exp2 6.7)")
        print(f"  ... + scalar / waits  {2 * tot_all:7.0f} cycles   (SALU, s_waitcnt, barrier: 4 each; upper bound - they can issue beside the other wave's vector op)")
        cyc = ns.tile_us * ns.clock_mhz
        print(f"  measured tile time    {cyc:7.0f} cycles   ({ns.tile_us} us at {ns.clock_mhz:.0f} MHz)")
        print(f"  => matrix pipe {2 * mfma_pipe / cyc:.2f} of the tile time, vector issue {2 * tot_vec / cyc:.2f}, VALU {2 * valu_busy / cyc:.2f}, LDS array {(per.get('lds', 0) * 32 + 256) / cyc:.2f}")
        print()
    w64(ns)
    print("Reading (static shift): per KV tile a SIMD owes 2048 cycles to the matrix pipe, ~1300 to the CU's LDS array, ~1200 to the VALU and")
    print("~1750-2200 issue cycles to its two waves; measured 3071 = 1.5 x the largest single-unit bound: NO single unit explains the tile time, so")
    print("this budget does not prove a floor.  What it shows: (i) MFMA busy = 2048 / 3071 = 0.67 (PMC: 0.686 on full rounds) - the matrix pipe idles a")
    print("third of the time although every other unit has slack on paper; (ii) the slack is lost in the PAIRING of the two waves of a SIMD, which the")
    print("microarchitecture guide measures (VALU issue arbitrated by priority then age, a wave that loses VALU slots mid-stream also loses the MFMA")
    print("cover those instructions provided; moving work between the two waves is zero- or negative-sum) and which rounds 1-5 met as: dephased roles")
    print("-2 %, packed fp32 -3 %, v_dot2 row sums -1...-3.5 %, 4 waves x 64 rows slower, MFMA 16x16x32 in the QK product slower, static shift (45 %")
    print("fewer VALU instructions) +3.7 % only; (iii) each K / V^T fragment read (32 ds_read_b128 per tile and wave) feeds exactly ONE MFMA - 8 waves")
    print("read the same 32 KiB tile 8 times (64 reads in flight per SIMD and tile next to 64 MFMAs): the structural change left is a wave tile of 64")
    print("query rows on ONE wave per SIMD with 512 registers (halves the reads per MFMA), whose first attempt (round 3, 4 waves x 64 rows, compiler-")
    print("scheduled) lost to the 8-wave loop; the hand-scheduled version of it is RGN_ATTN_LOOP_W64_ASM above, shipped on unsplit static-shift launches.")
    print()
    print("Reading (W64): one wave per SIMD, so nothing issues beside it.  The matrix pipe is owed 2048 cycles per tile; the measured tile is ~630 cycles")
    print("longer (isolated whole rounds, same box: 8-wave ~2840, W64 ~2680 cycles).  The vector fillers average 21.8 of the 24 cycles a 32-cycle MFMA gap")
    print("hides, but 25 of the 128 gaps of the two-tile body carry more than 24 (the gaps that also hold a ds_read_b128, its v_add_u32 and an LDS-DMA")
    print("piece): each such gap runs past its MFMA by its excess, ~4-12 cycles, ~200 per tile.  The ~56 SALU / s_waitcnt / barrier instructions per tile")
    print("(224 cycles at 4 each) now take issue slots of the same wave instead of a partner's.  And the 8 LDS-DMA pieces per wave and tile cost their issuing")
    print("wave 60-185 cycles each by the guide's price list, 480-1480 cycles of which only the issue slot is in the filler count: the same DMA work per")
    print("SIMD as in the 8-wave loop, but no second wave computes while this one is held.  These three account for the gap on paper; which dominates")
    print("is not measured (that needs in-loop stamps).  Levers left: fewer, larger fillers in the read / DMA gaps (move VALU out of them), the stage")
    print("advances as one s_cselect per tile, and the DMA pieces behind the MFMAs whose gaps carry the fewest fillers.")


if __name__ == "__main__":
    main()
