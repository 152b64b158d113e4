#!/usr/bin/env python3
"""Generate the hand-scheduled KV loop of the 8-wave region attention kernel (regione_amd/csrc/attn_loop_asm.inc).

    python tools/gen_attn_loop.py            # rewrites the .inc (committed; the build does not run this script)

What the compiler-scheduled kernel (attention_kernel, attn.hip) does per KV tile and wave: 16 MFMAs (S^T = K Q^T), then
~150 VALU instructions of softmax with the matrix pipe idle, then 16 MFMAs (O^T += V^T P^T).  Both waves of a SIMD pass the
same barrier every tile, so their softmax phases coincide: a SIMD spends ~3780 cycles on 2048 cycles of MFMA work
(DESIGN.md section 4.7).  hipcc cannot be made to software-pipeline this (round 1 tried).  Here the loop is ONE asm
statement in which each wave overlaps its OWN phases:

    X(t):  MFMA  S(t+1) = K(t+1) Q^T            ||  VALU  P(t) = exp2(S(t) * c - m),  P -> bf16 (pf)
    Y(t):  MFMA  O += V^T(t) P(t)^T            ||  VALU  row sums of P(t),  max of S(t+1),  defer-max decision

Two S register sets alternate (tile parity), so the loop body exists in two parities.  K / V^T fragments stream through an
8-slot window (32 registers), each fragment requested 4 MFMAs before its use, with counted lgkmcnt waits.  K / V^T tiles
arrive by LDS-DMA into a ring of FIVE 32 KiB stages (all 160 KiB): when a wave passes the tile barrier of body t every
wave's pieces of tiles <= t+2 have landed, tile t+3 may be in flight and tile t+4 is issued right behind the barrier
(two tiles of lead; the fragment prefetch may run across the barrier).  Past the last tile the DMA re-fetches the last tile
(clamped offset), which keeps every `vmcnt` count uniform.  Online softmax with deferred max exactly like the C++ kernel
(running max raised - and O, l rescaled - only when some row's tile max exceeds it by > 2^8); the rescale sits at the head of
X(t+1), after PV(t) has drained.

Registers (per wave; 2 waves per SIMD -> 256 in total):
    a[0:63]    O^T accumulator (4 d-blocks x 16)          a[64:95]  Q fragments (B operand of S^T), 8 k-steps x 4
    v[32:63]   S set 0 (s0 = kv rows 0..31, s1 = 32..63)   v[64:95]  S set 1
    v[96:111]  pf: P packed to bf16 (B operand of PV)      v[112:143] fragment window, 8 slots x 4
    v[144:159] temporaries                                 v[0:31]   operands (compiler-allocated)
Named operands: see attn.hip (attention_asm_kernel).
"""
import os
import re

S_BASE = (32, 64)
PF, FR, TMP = 96, 112, 144
T_NEGM, T_MX, T_MXB, T_KA, T_VA, T_A, T_B, T_ALPHA = (TMP + i for i in range(8))
ACC = [TMP + 8 + i for i in range(4)]           # row-sum accumulators
T_R = [TMP + 12 + i for i in range(4)]          # rescale temporaries
K_TILE, STAGE, NSTAGE = 16384, 32768, 5
LDS_END = STAGE * NSTAGE
CFG = dict(D=4, novalu=False, noread=False, prio=False, pkfma=False, pkadd=False, dot2sum=False, dephase=False, dmaspread=False,
           staticmax=False)      # generator knobs (main() emits several variants)


def v(n, w=1):
    return f"v{n}" if w == 1 else f"v[{n}:{n + w - 1}]"


def a(n, w=1):
    return f"a{n}" if w == 1 else f"a[{n}:{n + w - 1}]"


def slot(i):
    return v(FR + 4 * (i % 8), 4)


class Stream:
    """Instruction list with LDS-read bookkeeping for counted lgkmcnt waits."""

    def __init__(self):
        self.ins = []
        self.pending = []            # fragment tags of ds_reads issued and not yet known complete (in issue order)

    def emit(self, s):
        self.ins.append(s)

    def read(self, tag, dst, addr, off):
        if CFG["noread"]:
            return
        self.ins.append(f"ds_read_b128 {dst}, {addr} offset:{off}")
        self.pending.append(tag)

    def need(self, tag):
        """make sure the read `tag` has completed: LDS reads return in order"""
        if tag in self.pending:
            i = self.pending.index(tag)
            n = len(self.pending) - 1 - i
            self.ins.append(f"s_waitcnt lgkmcnt({n})")
            self.pending = self.pending[i + 1:]


def k_addr(st, ks):
    st.emit(f"v_add_u32 {v(T_KA)}, %[stg_k], %[krel{ks}]")


def v_addr(st, kb4):
    st.emit(f"v_add_u32 {v(T_VA)}, %[stg_v], %[vrel{kb4}]")


def k_read(st, f):                 # K fragment f = 2*ks + b  (b = kv half of the tile)
    ks, b = divmod(f, 2)
    if b == 0:
        k_addr(st, ks)
    st.read(("K", f), slot(f), v(T_KA), b * 8192)


def v_read(st, g):                 # V^T fragment g = 4*kb4 + db
    kb4, db = divmod(g, 4)
    if db == 0:
        v_addr(st, kb4)
    st.read(("V", g), slot(g), v(T_VA), K_TILE + db * 4096)


def qk_mfma(st, f, q):
    ks, b = divmod(f, 2)
    d = v(S_BASE[q] + 16 * b, 16)
    c = "0" if ks == 0 else d
    st.need(("K", f))
    st.emit(f"v_mfma_f32_32x32x16_bf16 {d}, {slot(f)}, {a(64 + 4 * ks, 4)}, {c}")


def pv_mfma(st, g):
    kb4, db = divmod(g, 4)
    st.need(("V", g))
    st.emit(f"v_mfma_f32_32x32x16_bf16 {a(16 * db, 16)}, {slot(g)}, {v(PF + 4 * kb4, 4)}, {a(16 * db, 16)}")


def exp_ops(p):
    """VALU of X(t) on S set p, in place: P = exp2(S * c - m); pf[k] = bf16x2(P[2k], P[2k+1]).  Ordered so that an op never
    follows its producer closely.  ATTN_PKFMA=1 / ATTN_PKADD=1 (measurement builds): scale-and-shift / row sums on the
    packed-fp32 instructions (two elements each; 35 VALU instructions fewer per tile) - measured SLOWER on MI355X (full step
    1175 -> 1136 / 1148 / 1113 TFLOP/s with pk_fma / pk_add / both, same box), so the shipped loop keeps the scalar forms."""
    b = S_BASE[p]
    if not CFG["pkfma"]:
        return exp_ops_scalar(p)
    assert T_NEGM % 2 == 0 and b % 2 == 0
    fma = lambda i: f"v_pk_fma_f32 {v(b + 2 * i, 2)}, {v(b + 2 * i, 2)}, %[sl2e2], {v(T_NEGM, 2)} op_sel_hi:[1,1,0]"
    exp = lambda i: f"v_exp_f32 {v(b + i)}, {v(b + i)}"
    cvt = lambda k: f"v_cvt_pk_bf16_f32 {v(PF + k)}, {v(b + 2 * k)}, {v(b + 2 * k + 1)}"
    ops = [fma(i) for i in range(4)]
    for i in range(32 + 12):
        if i < 32:
            ops.append(exp(i))
        if i % 2 == 1 and (i + 8) // 2 < 16:
            ops.append(fma((i + 8) // 2))              # elements i+7, i+8: needed by exp(i+7) six or more ops later
        j = i - 10
        if 0 <= j < 32 and j % 2 == 1:
            ops.append(cvt(j // 2))
    assert sum(o.startswith("v_cvt") for o in ops) == 16 and sum(o.startswith("v_pk_fma") for o in ops) == 16
    # every element is scaled before its exp
    seen = set()
    for o in ops:
        if o.startswith("v_pk_fma"):
            r = int(o.split("v[")[1].split(":")[0])
            seen |= {r, r + 1}
        elif o.startswith("v_exp"):
            assert int(o.split()[1].strip("v,")) in seen, o
    return ops


def rowsum_ops(p):
    """l_run += sum of the 32 P values of this lane: two packed accumulators (4 running sums), 17 instructions"""
    b = S_BASE[p]
    if CFG["dot2sum"]:
        # ATTN_DOT2SUM=1 (measurement build): row sum of the bf16-ROUNDED P (the values the PV product uses) with
        # v_dot2_f32_bf16 against (1, 1): 16 + 4 instructions instead of 36
        ops = [f"v_dot2_f32_bf16 {v(ACC[i % 4])}, {v(PF + i)}, %[ones2], " + ("0" if i < 4 else v(ACC[i % 4])) for i in range(16)]
        ops += [f"v_add_f32 {v(ACC[0])}, {v(ACC[0])}, {v(ACC[1])}", f"v_add_f32 {v(ACC[2])}, {v(ACC[2])}, {v(ACC[3])}",
                f"v_add_f32 {v(ACC[0])}, {v(ACC[0])}, {v(ACC[2])}", f"v_add_f32 %[l_run], %[l_run], {v(ACC[0])}"]
        return ops
    if not CFG["pkadd"]:
        return rowsum_ops_scalar(p)
    assert ACC[0] % 2 == 0
    acc = [v(ACC[0], 2), v(ACC[2], 2)]
    ops = [f"v_pk_add_f32 {acc[0]}, {v(b, 2)}, {v(b + 2, 2)}", f"v_pk_add_f32 {acc[1]}, {v(b + 4, 2)}, {v(b + 6, 2)}"]
    ops += [f"v_pk_add_f32 {acc[(i // 2) % 2]}, {acc[(i // 2) % 2]}, {v(b + i, 2)}" for i in range(8, 32, 2)]
    ops += [f"v_pk_add_f32 {acc[0]}, {acc[0]}, {acc[1]}", f"v_add_f32 {v(ACC[0])}, {v(ACC[0])}, {v(ACC[1])}",
            f"v_add_f32 %[l_run], %[l_run], {v(ACC[0])}"]
    return ops


def exp_ops_scalar(p):
    b = S_BASE[p]
    fma = lambda i: f"v_fma_f32 {v(b + i)}, {v(b + i)}, %[sl2e], {v(T_NEGM)}"
    exp = lambda i: f"v_exp_f32 {v(b + i)}, {v(b + i)}"
    cvt = lambda k: f"v_cvt_pk_bf16_f32 {v(PF + k)}, {v(b + 2 * k)}, {v(b + 2 * k + 1)}"
    ops = [fma(i) for i in range(8)]
    for i in range(32 + 12):
        if i < 32:
            ops.append(exp(i))
        if i + 8 < 32:
            ops.append(fma(i + 8))
        j = i - 10
        if 0 <= j < 32 and j % 2 == 1:
            ops.append(cvt(j // 2))
    return ops


def rowsum_ops_scalar(p):
    b = S_BASE[p]
    ops = [f"v_mov_b32 {v(ACC[i])}, {v(b + i)}" for i in range(4)]
    ops += [f"v_add_f32 {v(ACC[i % 4])}, {v(ACC[i % 4])}, {v(b + i)}" for i in range(4, 32)]
    ops += [f"v_add_f32 {v(ACC[0])}, {v(ACC[0])}, {v(ACC[1])}", f"v_add_f32 {v(ACC[2])}, {v(ACC[2])}, {v(ACC[3])}",
            f"v_add_f32 {v(ACC[0])}, {v(ACC[0])}, {v(ACC[2])}", f"v_add_f32 %[l_run], %[l_run], {v(ACC[0])}"]
    return ops


def max_ops(q):
    """tile max of S set q (two chains), across the two half-waves, scaled; vcc = rows whose max exceeds m_run + 8"""
    b = S_BASE[q]
    ops = [f"v_max_f32 {v(T_MX)}, {v(b)}, {v(b + 1)}", f"v_max_f32 {v(T_MXB)}, {v(b + 16)}, {v(b + 17)}"]
    for i in range(1, 8):
        ops.append(f"v_max3_f32 {v(T_MX)}, {v(T_MX)}, {v(b + 2 * i)}, {v(b + 2 * i + 1)}")
        ops.append(f"v_max3_f32 {v(T_MXB)}, {v(T_MXB)}, {v(b + 16 + 2 * i)}, {v(b + 17 + 2 * i)}")
    ops += [f"v_max_f32 {v(T_MX)}, {v(T_MX)}, {v(T_MXB)}",
            f"v_mov_b32 {v(T_A)}, {v(T_MX)}", f"v_mov_b32 {v(T_B)}, {v(T_MX)}", "s_nop 1",
            f"v_permlane32_swap_b32 {v(T_A)}, {v(T_B)}",               # lanes 32-63 of A <-> lanes 0-31 of B
            f"v_max_f32 {v(T_MX)}, {v(T_A)}, {v(T_B)}",
            f"v_mul_f32 {v(T_MX)}, %[sl2e], {v(T_MX)}",
            f"v_add_f32 {v(T_A)}, 0x41000000, %[m_run]",                  # m_run + 8.0 (DEFER_THR)
            f"v_cmp_gt_f32 vcc, {v(T_MX)}, {v(T_A)}"]
    return ops


def rescale_block(st, tag):
    """head of X: if any row's new tile max exceeds the running max by more than 2^8 (vcc from the previous Y), raise the
    running max and rescale l and O.  PV of the previous tile has issued; its results need ~20 wait states."""
    st.emit(f"s_cbranch_vccz 9{tag}f")
    st.emit("s_nop 15")
    st.emit("s_nop 15")
    st.emit(f"v_max_f32 {v(T_A)}, %[m_run], {v(T_MX)}")                 # m_new
    st.emit(f"v_sub_f32 {v(T_ALPHA)}, %[m_run], {v(T_A)}")
    st.emit(f"v_exp_f32 {v(T_ALPHA)}, {v(T_ALPHA)}")                    # alpha = 2^(m_old - m_new)
    st.emit(f"v_mov_b32 %[m_run], {v(T_A)}")
    st.emit(f"v_sub_f32 {v(T_NEGM)}, 0, {v(T_A)}")
    st.emit(f"v_mul_f32 %[l_run], %[l_run], {v(T_ALPHA)}")
    for i in range(0, 64, 4):
        for k in range(4):
            st.emit(f"v_accvgpr_read_b32 {v(T_R[k])}, {a(i + k)}")
        for k in range(4):
            st.emit(f"v_mul_f32 {v(T_R[k])}, {v(T_R[k])}, {v(T_ALPHA)}")
        for k in range(4):
            st.emit(f"v_accvgpr_write_b32 {a(i + k)}, {v(T_R[k])}")
    st.emit(f"9{tag}:")


def advance(st, reg):
    st.emit(f"s_add_u32 %[{reg}], %[{reg}], {STAGE}")
    st.emit(f"s_cmp_ge_u32 %[{reg}], {LDS_END}")
    st.emit(f"s_cselect_b32 %[stmp], {LDS_END}, 0")
    st.emit(f"s_sub_u32 %[{reg}], %[{reg}], %[stmp]")


def dma_issue(st):
    """4 pieces of the next tile (clamped to the last one) into stage stg_d; advance the tile offsets and stg_d"""
    st.emit("s_min_u32 %[stmp], %[tk], %[tk_last]")
    st.emit("s_min_u32 %[stmp2], %[tv], %[tv_last]")
    st.emit("s_add_u32 %[sdst], %[stg_d], %[wdst]")
    for p in range(2):
        st.emit(f"s_add_u32 m0, %[sdst], {p * 1024}")
        st.emit("s_nop 0")
        st.emit(f"buffer_load_dwordx4 %[dk{p}], %[rk], %[stmp] offen lds")
    for p in range(2):
        st.emit(f"s_add_u32 m0, %[sdst], {K_TILE + p * 1024}")
        st.emit("s_nop 0")
        st.emit(f"buffer_load_dwordx4 %[dv{p}], %[rv], %[stmp2] offen lds")
    st.emit("s_add_u32 %[tk], %[tk], %[kadv]")
    st.emit("s_add_u32 %[tv], %[tv], 128")
    advance(st, "stg_d")


def dma_split():
    """dma_issue cut into a prologue (scalar set-up), the four pieces (callables) and an epilogue (offset / stage advance): the
    pieces are issued one at a time behind QK MFMAs 0, 2, 4, 6 of phase X (ATTN_DMA_AT) instead of back to back behind the tile
    barrier, where nothing is queued on the matrix pipe yet (an LDS-DMA piece costs the issuing wave ~60 cycles among MFMAs already
    queued, more otherwise).  Round 3, same box: full step 1202 -> 1212 TFLOP/s, region 25 % 965 -> 982, v1p2 2048^2 region 1203 -> 1220;
    placements 1,5,9,13 / 3,7,11,15 / 9,11,13,15 within 0.5 % of it.  ATTN_DMA_SPREAD=0 regenerates the round-2 schedule."""
    def pro(st):
        st.emit("s_min_u32 %[stmp], %[tk], %[tk_last]")
        st.emit("s_min_u32 %[stmp2], %[tv], %[tv_last]")
        st.emit("s_add_u32 %[sdst], %[stg_d], %[wdst]")

    def piece(kind, p):
        def f(st):
            st.emit(f"s_add_u32 m0, %[sdst], {(K_TILE if kind == 'v' else 0) + p * 1024}")
            st.emit("s_nop 0")
            st.emit(f"buffer_load_dwordx4 %[d{kind}{p}], %[r{kind}], %[{'stmp2' if kind == 'v' else 'stmp'}] offen lds")
        return f

    def epi(st):
        st.emit("s_add_u32 %[tk], %[tk], %[kadv]")
        st.emit("s_add_u32 %[tv], %[tv], 128")
        advance(st, "stg_d")
    return pro, [piece("k", 0), piece("k", 1), piece("v", 0), piece("v", 1)], epi


def interleave(st, mfmas, fillers, per_gap):
    """emit the MFMA callbacks with `per_gap[i]` fillers behind MFMA i (fillers: strings or callables(st))"""
    fi = 0
    for i, m in enumerate(mfmas):
        m(st)
        for _ in range(per_gap[i] if i < len(per_gap) else 0):
            if fi < len(fillers):
                f = fillers[fi]
                fi += 1
                f(st) if callable(f) else st.emit(f)
    while fi < len(fillers):
        f = fillers[fi]
        fi += 1
        f(st) if callable(f) else st.emit(f)


def spread(n_fill, n_gaps, first=0):
    """distribute n_fill fillers over n_gaps gaps as evenly as possible, none before gap `first`"""
    gaps = [0] * n_gaps
    live = n_gaps - first
    for k in range(n_fill):
        gaps[first + (k * live) // max(n_fill, 1)] += 1
    return gaps


def phase_x(st, p, full, dma=None):
    """X(t), S(t) in set p: exp of tile t; with `full` also the QK MFMAs of tile t+1 into set 1-p.
    Entry: K fragments 0..D-1 of tile t+1 requested (slots 0..D-1).  Exit: V fragments 0..D-1 of tile t requested.
    Fragment i of a phase lives in slot i % 8; it is requested D MFMAs before its use: behind MFMA i-D-1... i.e. read(i + D)
    follows MFMA i - 1 / precedes MFMA i; the first D fragments of the NEXT phase are requested behind this phase's
    MFMA j + 8 (the last user of slot j)."""
    D = CFG["D"]
    q = 1 - p
    vops = [] if CFG["novalu"] else exp_ops(p)
    if not full:
        for o in vops:
            st.emit(o)
        for g in range(D):
            v_read(st, g)
        return
    mf = []
    at = [int(x) for x in os.environ.get("ATTN_DMA_AT", "0,2,4,6").split(",")]
    for f in range(16):
        def m(st, f=f):
            if f + D < 16:
                k_read(st, f + D)
            qk_mfma(st, f, q)
            if f >= 8 and f - 8 < D:                       # slot f-8 is free now: V prefetch for Y(t)
                v_read(st, f - 8)
            if dma is not None and f in at:                # one LDS-DMA piece of tile t+4 behind this MFMA
                pieces, epi = dma
                pieces[at.index(f)](st)
                if f == at[-1]:
                    epi(st)
        mf.append(m)
    gaps = spread(len(vops), 16)
    interleave(st, mf, vops, gaps)


def phase_y(st, p, full, prefetch_k):
    """Y(t): PV MFMAs of tile t (P in set p / pf); row sums of P(t); with `full` the max + defer decision of S(t+1) (set 1-p);
    with `prefetch_k` the first D K fragments of tile t+2 for the next X.  Entry: V fragments 0..D-1 requested."""
    D = CFG["D"]
    q = 1 - p
    vops = [] if CFG["novalu"] else rowsum_ops(p)
    mops = max_ops(q) if (full and not CFG["staticmax"]) else []
    if CFG["novalu"] and mops:
        mops = mops[-1:]                                    # keep vcc defined
    mf = []
    for g in range(16):
        def m(st, g=g):
            if g + D < 16:
                v_read(st, g + D)
            pv_mfma(st, g)
            if prefetch_k and g >= 8 and g - 8 < D:         # slot g-8 is free now: K prefetch for X(t+1)
                k_read(st, g - 8)
        mf.append(m)
    # the max reads S(t+1), written by the last QK MFMA of X(t): keep it behind the 4th PV MFMA
    fill = vops[:8] + mops + vops[8:] if mops else vops
    gaps = spread(len(fill), 16, first=3 if mops else 0)
    interleave(st, mf, fill, gaps)


def body(st, p, full, tag, role="A"):
    """One KV tile.  Role A: tile barrier + DMA issue at the HEAD of the body (before X); role B: between X and Y.  Both roles
    execute the same phase sequence and one barrier per tile, so when all waves meet at barrier t the role-A waves are about to
    start X(t) and the role-B waves have just finished it: behind the barrier A runs X (80 VALU instructions, 2/3 of them
    quarter-rate exp) while B runs Y (61 cheap ones), then the other way round.  Two waves of one SIMD with different roles
    therefore never want the VALU for their exp phases at the same time.  ATTN_DEPHASE=1 (measurement build; the kernel picks the
    roles, waves 4..7 or the odd waves in role B): correct, and within +-0.5 % of the single-role loop on
    every shape (MI355X) - the waves of a SIMD evidently do not stay phase-locked behind the barrier anyway - so the shipped loop
    has one role.  Ring safety is unchanged: at barrier t every wave has
    finished Y(t-1) (the stage tile t+4 overwrites), and role B's early X(t) reads K(t+1), which landed by barrier t-1."""
    if not CFG["staticmax"]:
        rescale_block(st, tag)

    spread_dma = CFG.get("dmaspread") and role == "A"
    dma = None

    def tile_barrier():
        nonlocal dma
        st.emit("s_waitcnt vmcnt(4)")                      # tile t+2 has landed (t+3 may be in flight)
        st.emit("s_barrier")
        if spread_dma:
            pro, pieces, epi = dma_split()
            pro(st)
            dma = (pieces, epi)                            # issued one by one inside phase X
        else:
            dma_issue(st)                                  # tile t+4 -> the stage of tile t-1
    if full and role == "A":
        tile_barrier()
    phase_x(st, p, full, dma)
    if full:
        advance(st, "stg_k")                               # next X reads K of tile t+2
    if full and role == "B":
        tile_barrier()
    phase_y(st, p, full, prefetch_k=full)
    advance(st, "stg_v")
    # a trailing full body's K prefetch reads (t+2) are harmless when tile t+2 does not exist: the clamped DMA re-fetched
    # the last tile into that stage


def prologue(st):
    # Q fragments -> fragment window (plain loads), then the first four tiles
    for ks in range(8):
        st.emit(f"global_load_dwordx4 {slot(ks)}, %[qptr], off offset:{ks * 32}")
    for _ in range(4):
        dma_issue(st)
    for n in range(64):
        st.emit(f"v_accvgpr_write_b32 {a(n)}, 0")
    st.emit("s_waitcnt vmcnt(16)")                         # Q landed (the 16 DMA pieces may be in flight)
    for ks in range(8):
        for k in range(4):
            st.emit(f"v_accvgpr_write_b32 {a(64 + 4 * ks + k)}, {v(FR + 4 * ks + k)}")
    st.emit(f"v_sub_f32 {v(T_NEGM)}, 0, %[m_run]")
    st.emit("s_waitcnt vmcnt(8)")                          # tiles 0, 1 landed
    st.emit("s_barrier")
    # S(0) = K(0) Q^T into set 0 (stage 0: stg_v), not overlapped
    st.emit("s_mov_b32 %[stmp], %[stg_k]")
    st.emit("s_mov_b32 %[stg_k], %[stg_v]")
    D = CFG["D"]
    for f in range(D):
        k_read(st, f)
    for f in range(16):
        if f + D < 16:
            k_read(st, f + D)
        qk_mfma(st, f, 0)
    st.emit("s_mov_b32 %[stg_k], %[stmp]")
    st.emit("s_nop 15")
    st.emit("s_nop 15")
    if not CFG["staticmax"]:
        for o in max_ops(0):
            st.emit(o)
    for f in range(D):                                      # K prefetch of tile 1 for X(0)
        k_read(st, f)


def emit_loop(st, entry, role, L):
    """the tile loop for one role; L = label base (numeric local labels L+1 .. L+4, rescale labels 9<tag>)"""
    t = lambda k: str(L + k)
    st.pending = list(entry)
    st.emit("s_cmp_eq_u32 %[cnt], 0")
    st.emit(f"s_cbranch_scc1 {L + 2}f")
    st.emit(f"{L + 1}:")
    body(st, 0, True, t(1), role)
    body(st, 1, True, t(2), role)
    assert set(st.pending) <= set(entry)                 # the loop head assumed at least these reads in flight: conservative
    st.emit("s_sub_u32 %[cnt], %[cnt], 1")
    st.emit("s_cmp_lg_u32 %[cnt], 0")
    st.emit(f"s_cbranch_scc1 {L + 1}b")
    st.emit(f"{L + 2}:")
    st.emit("s_cmp_eq_u32 %[rem], 0")
    st.emit(f"s_cbranch_scc1 {L + 3}f")
    body(st, 0, True, t(3), role)
    body(st, 1, False, t(4), role)
    st.emit(f"s_branch {L + 4}f")
    st.emit(f"{L + 3}:")
    st.pending = list(entry)
    body(st, 0, False, t(5), role)
    st.emit(f"{L + 4}:")


def emit():
    st = Stream()
    prologue(st)
    entry = [] if CFG["noread"] else [("K", f) for f in range(CFG["D"])]      # LDS reads in flight at every body entry
    assert st.pending == entry
    if CFG["dephase"]:
        st.emit("s_cmp_lg_u32 %[role], 0")
        st.emit("s_cbranch_scc1 50f")
    emit_loop(st, entry, "A", 10)
    if CFG["dephase"]:
        st.emit("s_branch 60f")
        st.emit("50:")
        emit_loop(st, entry, "B", 20)
        st.emit("60:")
    st.emit("s_waitcnt vmcnt(0)")
    st.emit("s_waitcnt lgkmcnt(0)")
    st.emit("s_barrier")
    st.emit("s_nop 15")
    st.emit("s_nop 15")
    return st.ins


# ------------------------------------------------------------------------------------------------------------------------------------
# Second loop (RGN_ATTN_LOOP_W64_ASM): 4 waves, ONE per SIMD, each owning 64 query rows as two 32-row q-blocks j = 0, 1 of the same
# 256-row item.  Static-shift softmax only.  Same MFMA, same swapped products, same 64-key tile, same five-stage ring, same swizzles as
# the loop above - and per output row the same arithmetic in the same order (MFMA k order, fma / exp2 / RNE packing of P, the four-chain
# row sum, tile order), so the results are bit-identical.  What changes: every K / V^T fragment is read from LDS ONCE and feeds the MFMAs
# of both q-blocks (32 ds_read_b128 per tile for 64 MFMAs instead of 32 for 32), and the one wave of a SIMD has the VALU to itself.
#
#     X(t):  32 MFMA  S(t+1)[j] = K(t+1) Q[j]^T       ||  E2(t): exp2 of the s1 halves of S(t), all 32 bf16 packings of P(t); 8 DMA pieces
#     Y(t):  32 MFMA  O[j] += V^T(t) P(t)[j]^T        ||  R(t): row sums of P(t);  E1(t+1): exp2 of the s0 halves of S(t+1)
#
# so every MFMA gap carries about one v_exp_f32 and two or three plain VALU instructions (weights 5/3 and 1 when spacing), one ds_read
# every second gap, and no phase opens with a VALU block.  Registers (512 per wave):
#     a[0:127]    O^T, q-block j at 64 j (4 d-blocks x 16)      a[128:191]  Q fragments, q-block j at 128 + 32 j (8 k-steps x 4)
#     v[32:95]    S set 0 (q-block j at 32 + 32 j)               v[96:159]   S set 1
#     v[160:191]  pf: P packed to bf16, q-block j at 160 + 16 j  v[192:223]  fragment window, 8 slots x 4
#     v[224:239]  temporaries                                    v[0:31]     operands (compiler-allocated)
# ------------------------------------------------------------------------------------------------------------------------------------
W_S = ((32, 64), (96, 128))                        # [set][q-block]
W_PF = (160, 176)
W_FR, W_NEGM, W_KA, W_VA = 192, 224, 225, 226
W_ACC = ((228, 229, 230, 231), (232, 233, 234, 235))
W_O, W_Q = (0, 64), (128, 160)
W_NV, W_NA = 240, 192                              # registers the statement owns: v32..v239, a0..a191
W_D = 4                                            # fragment prefetch distance (fragments; two MFMAs each)
W_DMA_AT = (1, 5, 9, 13, 17, 21, 25, 29)           # MFMA index of X behind which each of the wave's 8 LDS-DMA pieces is issued
W_MFMA_TO_VALU = 3                                 # a VALU instruction touches an MFMA result only behind this many later MFMAs


def wslot(i):
    return v(W_FR + 4 * (i % 8), 4)


def w_k_read(st, f):
    ks, b = divmod(f, 2)
    if b == 0:
        st.emit(f"v_add_u32 {v(W_KA)}, %[stg_k], %[krel{ks}]")
    st.read(("K", f), wslot(f), v(W_KA), b * 8192)


def w_v_read(st, g):
    kb4, db = divmod(g, 4)
    if db == 0:
        st.emit(f"v_add_u32 {v(W_VA)}, %[stg_v], %[vrel{kb4}]")
    st.read(("V", g), wslot(g), v(W_VA), K_TILE + db * 4096)


def w_qk_mfma(st, f, q, j):
    ks, b = divmod(f, 2)
    d = v(W_S[q][j] + 16 * b, 16)
    st.need(("K", f))
    st.emit(f"v_mfma_f32_32x32x16_bf16 {d}, {wslot(f)}, {a(W_Q[j] + 4 * ks, 4)}, {'0' if ks == 0 else d}")


def w_pv_mfma(st, g, j):
    kb4, db = divmod(g, 4)
    st.need(("V", g))
    st.emit(f"v_mfma_f32_32x32x16_bf16 {a(W_O[j] + 16 * db, 16)}, {wslot(g)}, {v(W_PF[j] + 4 * kb4, 4)}, {a(W_O[j] + 16 * db, 16)}")


def w_fma(p, j, i):
    return f"v_fma_f32 {v(W_S[p][j] + i)}, {v(W_S[p][j] + i)}, %[sl2e], {v(W_NEGM)}"


def w_exp(p, j, i):
    return f"v_exp_f32 {v(W_S[p][j] + i)}, {v(W_S[p][j] + i)}"


def w_cvt(p, j, k):
    return f"v_cvt_pk_bf16_f32 {v(W_PF[j] + k)}, {v(W_S[p][j] + 2 * k)}, {v(W_S[p][j] + 2 * k + 1)}"


def w_e1_ops(p):
    """E1 on S set p: scale-and-shift and exp2 of the s0 halves (registers 0..15: the P operands of PV k-blocks 0, 1) of both q-blocks;
    a fma runs eight elements ahead of its exp"""
    el = [(j, i) for i in range(16) for j in range(2)]
    ops = [w_fma(p, j, i) for j, i in el[:8]]
    for n, (j, i) in enumerate(el):
        ops.append(w_exp(p, j, i))
        if n + 8 < len(el):
            ops.append(w_fma(p, *el[n + 8]))
    return ops


def w_e2_ops(p):
    """E2 on S set p: the s1 halves (registers 16..31) of both q-blocks, and every packing: those of the s0 halves (exp'd by E1 in the
    previous Y) first - PV starts with them - then each s1 pair ten or more exps behind its second element"""
    el = [(j, i) for i in range(16, 32) for j in range(2)]
    early = [(j, k) for k in range(8) for j in range(2)]
    ops = [w_fma(p, j, i) for j, i in el[:8]]
    for n in range(len(el) + 12):
        if n < len(el):
            ops.append(w_exp(p, *el[n]))
        if n + 8 < len(el):
            ops.append(w_fma(p, *el[n + 8]))
        if n % 2 == 1 and early:
            ops.append(w_cvt(p, *early.pop(0)))
        m = n - 10
        if 0 <= m < len(el) and el[m][1] % 2 == 1:
            ops.append(w_cvt(p, el[m][0], el[m][1] // 2))
    assert not early and sum(o.startswith("v_cvt") for o in ops) == 32 and sum(o.startswith("v_exp") for o in ops) == 32
    return ops


def w_rowsum_ops(p):
    """row sums of P (S set p), each q-block with the four chains and the final order of rowsum_ops_scalar; the two q-blocks alternate"""
    per = []
    for j in range(2):
        b, acc = W_S[p][j], W_ACC[j]
        ops = [f"v_mov_b32 {v(acc[i])}, {v(b + i)}" for i in range(4)]
        ops += [f"v_add_f32 {v(acc[i % 4])}, {v(acc[i % 4])}, {v(b + i)}" for i in range(4, 32)]
        ops += [f"v_add_f32 {v(acc[0])}, {v(acc[0])}, {v(acc[1])}", f"v_add_f32 {v(acc[2])}, {v(acc[2])}, {v(acc[3])}",
                f"v_add_f32 {v(acc[0])}, {v(acc[0])}, {v(acc[2])}", f"v_add_f32 %[l_run{j}], %[l_run{j}], {v(acc[0])}"]
        per.append(ops)
    return [o for pair in zip(*per) for o in pair]


def w_weight(o):
    return 5.0 / 3.0 if isinstance(o, str) and o.startswith("v_exp") else 1.0


def w_spread(fillers, n_gaps, first=0, pre=None):
    """fillers per gap so that every gap from `first` on carries about the same WEIGHT (v_exp_f32 5/3, anything else 1; `pre[i]` =
    weight gap i carries already: its LDS-DMA piece)"""
    pre = pre or [0.0] * n_gaps
    total = sum(w_weight(o) for o in fillers) + sum(pre[first:])
    avg = total / (n_gaps - first)
    gaps, cum, fi = [0] * n_gaps, 0.0, 0
    for g in range(first, n_gaps):
        cum += pre[g]
        target = avg * (g - first + 1)
        while fi < len(fillers) and (g == n_gaps - 1 or cum + w_weight(fillers[fi]) / 2 <= target):
            cum += w_weight(fillers[fi])
            gaps[g] += 1
            fi += 1
    assert fi == len(fillers)
    return gaps


def w_merge(xs, ys):
    """xs and ys interleaved evenly, each in its own order"""
    out, i, j = [], 0, 0
    while i < len(xs) or j < len(ys):
        if j >= len(ys) or (i < len(xs) and i * len(ys) <= j * len(xs)):
            out.append(xs[i]); i += 1
        else:
            out.append(ys[j]); j += 1
    return out


def w_dma_split():
    def pro(st):
        st.emit("s_min_u32 %[stmp], %[tk], %[tk_last]")
        st.emit("s_min_u32 %[stmp2], %[tv], %[tv_last]")
        st.emit("s_add_u32 %[sdst], %[stg_d], %[wdst]")

    def piece(kind, p):                    # (set m0, issue): one instruction at least has to sit between the two
        def m0(st):
            st.emit(f"s_add_u32 m0, %[sdst], {(K_TILE if kind == 'v' else 0) + p * 1024}")

        def load(st):
            st.emit(f"buffer_load_dwordx4 %[d{kind}{p}], %[r{kind}], %[{'stmp2' if kind == 'v' else 'stmp'}] offen lds")
        return m0, load

    def epi(st):
        st.emit("s_add_u32 %[tk], %[tk], %[kadv]")
        st.emit("s_add_u32 %[tv], %[tv], 128")
        advance(st, "stg_d")
    return pro, [piece("k", p) for p in range(4)] + [piece("v", p) for p in range(4)], epi


def w_dma_issue(st):
    pro, pieces, epi = w_dma_split()
    pro(st)
    for m0, load in pieces:
        m0(st)
        st.emit("s_nop 0")
        load(st)
    epi(st)


def w_phase_x(st, p, full, dma=None):
    """X(t), S(t) in set p.  Entry: K fragments 0..D-1 of tile t+1 requested.  Exit: V^T fragments 0..D-1 of tile t requested.
    Fragment f lives in slot f % 8 and is requested D fragments (2 D MFMAs) before its first use."""
    q = 1 - p
    vops = w_e2_ops(p)
    if not full:
        for o in vops:
            st.emit(o)
        for g in range(W_D):
            w_v_read(st, g)
        return
    mf = []
    for n in range(32):
        def m(st, n=n):
            f, j = divmod(n, 2)
            if j == 0 and f + W_D < 16:
                w_k_read(st, f + W_D)
            if n in W_DMA_AT:                                # m0 in front of the MFMA: the MFMA is the wait state the DMA needs behind it
                dma[0][W_DMA_AT.index(n)][0](st)
            w_qk_mfma(st, f, q, j)
            if j == 1 and f >= 8 and f - 8 < W_D:            # both users of slot f % 8 have issued: V^T prefetch for Y(t)
                w_v_read(st, f - 8)
            if n in W_DMA_AT:
                dma[0][W_DMA_AT.index(n)][1](st)
                if n == W_DMA_AT[-1]:
                    dma[1](st)
        mf.append(m)
    pre = [2.0 if n in W_DMA_AT else 0.0 for n in range(32)]
    interleave(st, mf, vops, w_spread(vops, 32, pre=pre))


def w_phase_y(st, p, full):
    """Y(t): PV MFMAs of tile t; row sums of P(t); with `full` E1 of S(t+1) (set 1-p, written by the last MFMAs of X(t): not before
    MFMA W_MFMA_TO_VALU of this phase) and the first D K fragments of tile t+2."""
    rs = w_rowsum_ops(p)
    mf = []
    for n in range(32):
        def m(st, n=n):
            g, j = divmod(n, 2)
            if j == 0 and g + W_D < 16:
                w_v_read(st, g + W_D)
            w_pv_mfma(st, g, j)
            if full and j == 1 and g >= 8 and g - 8 < W_D:
                w_k_read(st, g - 8)
        mf.append(m)
    if full:
        e1 = w_e1_ops(1 - p)
        n0 = 4 * W_MFMA_TO_VALU + 2
        fill = rs[:n0] + w_merge(rs[n0:], e1)
        gaps = w_spread(rs[:n0], W_MFMA_TO_VALU + 1)
        rest = w_spread(fill[n0:], 32, first=W_MFMA_TO_VALU + 1)
        gaps = gaps + rest[W_MFMA_TO_VALU + 1:]
    else:
        fill, gaps = rs, w_spread(rs, 32)
    interleave(st, mf, fill, gaps)


def w_body(st, p, full):
    dma = None
    if full:
        st.emit("s_waitcnt vmcnt(8)")                      # tile t+2 has landed (the 8 pieces of t+3 may be in flight)
        st.emit("s_barrier")
        pro, pieces, epi = w_dma_split()
        pro(st)                                            # tile t+4 -> the stage of tile t-1, piece by piece inside X
        dma = (pieces, epi)
    w_phase_x(st, p, full, dma)
    if full:
        advance(st, "stg_k")
    w_phase_y(st, p, full)
    advance(st, "stg_v")


def w_prologue(st):
    for j in range(2):                                     # Q fragments -> S set 1 (free until X(0)), then into a[128:191]
        for ks in range(8):
            st.emit(f"global_load_dwordx4 {v(W_S[1][j] + 4 * ks, 4)}, %[qptr{j}], off offset:{ks * 32}")
    for _ in range(4):
        w_dma_issue(st)
    for n in range(128):
        st.emit(f"v_accvgpr_write_b32 {a(n)}, 0")
    st.emit("s_waitcnt vmcnt(32)")                         # Q landed (the 32 DMA pieces may be in flight)
    for j in range(2):
        for k in range(32):
            st.emit(f"v_accvgpr_write_b32 {a(W_Q[j] + k)}, {v(W_S[1][j] + k)}")
    st.emit(f"v_sub_f32 {v(W_NEGM)}, 0, %[m_run]")
    st.emit("s_waitcnt vmcnt(16)")                         # tiles 0, 1 landed
    st.emit("s_barrier")
    st.emit("s_mov_b32 %[stmp], %[stg_k]")                 # S(0) = K(0) Q^T into set 0 (stage 0: stg_v), not overlapped
    st.emit("s_mov_b32 %[stg_k], %[stg_v]")
    for f in range(W_D):
        w_k_read(st, f)
    for f in range(16):
        if f + W_D < 16:
            w_k_read(st, f + W_D)
        for j in range(2):
            w_qk_mfma(st, f, 0, j)
    st.emit("s_mov_b32 %[stg_k], %[stmp]")
    st.emit("s_nop 15")
    st.emit("s_nop 15")
    for o in w_e1_ops(0):
        st.emit(o)
    for f in range(W_D):                                   # K prefetch of tile 1 for X(0)
        w_k_read(st, f)


def w_entry_check(st, entry):
    """A body label is reachable from the prologue (cnt == 0) as well as from the body in front of it: the bookkeeping there has to assume
    at least the prologue's K prefetch in flight, or the first MFMAs would be emitted without their lgkmcnt waits."""
    assert st.pending[-len(entry):] == list(entry), st.pending
    st.entry_checks = getattr(st, "entry_checks", 0) + 1


def w_emit():
    st = Stream()
    w_prologue(st)
    entry = [("K", f) for f in range(W_D)]
    assert st.pending == entry
    L = 30
    st.emit("s_cmp_eq_u32 %[cnt], 0")
    st.emit(f"s_cbranch_scc1 {L + 2}f")
    st.emit(f"{L + 1}:")
    w_entry_check(st, entry)
    w_body(st, 0, True)
    w_body(st, 1, True)
    assert set(st.pending) <= set(entry)
    st.emit("s_sub_u32 %[cnt], %[cnt], 1")
    st.emit("s_cmp_lg_u32 %[cnt], 0")
    st.emit(f"s_cbranch_scc1 {L + 1}b")
    st.emit(f"{L + 2}:")
    st.emit("s_cmp_eq_u32 %[rem], 0")
    st.emit(f"s_cbranch_scc1 {L + 3}f")
    st.pending = list(entry)                             # reached from the prologue too (two tiles): its K reads are still in flight
    w_entry_check(st, entry)
    w_body(st, 0, True)
    w_body(st, 1, False)
    st.emit(f"s_branch {L + 4}f")
    st.emit(f"{L + 3}:")
    st.pending = list(entry)
    w_entry_check(st, entry)
    w_body(st, 0, False)
    st.emit(f"{L + 4}:")
    st.emit("s_waitcnt vmcnt(0)")
    st.emit("s_waitcnt lgkmcnt(0)")
    st.emit("s_barrier")
    st.emit("s_nop 15")
    st.emit("s_nop 15")
    assert st.entry_checks == 3                          # every label a body starts at: the loop top, the remainder, the last tile
    w_selfcheck(st.ins)
    return st.ins


def regs(tok):
    """('v' | 'a', lo, hi) of a register operand token, else None"""
    m = re.fullmatch(r"([va])(\d+)", tok) or re.fullmatch(r"([va])\[(\d+):(\d+)\]", tok)
    if not m:
        return None
    return m.group(1), int(m.group(2)), int(m.group(m.lastindex))


def mfma_valu_distances(lines):
    """For every non-MFMA instruction of a straight-line listing that names a register an earlier MFMA wrote: (MFMAs issued in between,
    wait states in between with s_nop N = N + 1 and anything else 1, the line).  Only the LAST writer of a register counts."""
    last = {}                                            # (file, n) -> (mfma ordinal, position in wait states)
    out, n_mfma, pos = [], 0, 0
    for l in lines:
        op = l.split()[0] if l.split() else ""
        toks = [t.strip(",") for t in l.split()[1:]]
        if op.startswith("v_mfma"):
            n_mfma += 1
            pos += 1
            f, lo, hi = regs(toks[0])
            for r in range(lo, hi + 1):
                last[(f, r)] = (n_mfma, pos)
            continue
        if op.endswith(":") or not op:
            continue
        hit = None
        for t in toks:
            r = regs(t)
            if r:
                for k in range(r[1], r[2] + 1):
                    if (r[0], k) in last:
                        w = last.pop((r[0], k))
                        hit = w if hit is None or w[1] > hit[1] else hit
        if hit:
            out.append((n_mfma - hit[0], pos - hit[1], l))
        m = re.fullmatch(r"s_nop (\d+)", l)
        pos += int(m.group(1)) + 1 if m else 1
    return out


def w_selfcheck(lines):
    n_read = sum(l.startswith("ds_read") for l in lines)
    n_mfma = sum(l.startswith("v_mfma") for l in lines)
    for l in lines:
        assert not l.startswith(("v_pk_", "v_dot2")), l
        for t in l.split()[1:]:
            r = regs(t.strip(","))
            if r:
                assert r[2] < (W_NV if r[0] == "v" else W_NA) and (r[0] == "a" or r[1] >= 32), l
    # three full bodies (64 MFMAs, 32 fragment reads), two last-tile bodies (32 PV MFMAs, 16 reads); the prologue's S(0): 32 MFMAs, 16 + D reads
    assert n_mfma == 3 * 64 + 2 * 32 + 32, n_mfma
    assert n_read == 3 * 32 + 2 * 16 + 16 + W_D, n_read
    for x, y in zip(lines, lines[1:]):
        assert not (x.startswith("s_add_u32 m0") and y.startswith("buffer_load")), (x, y)
    for between, states, l in mfma_valu_distances(lines):
        assert between >= W_MFMA_TO_VALU - 1 or states >= 32, (between, states, l)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    out = os.path.join(here, "..", "regione_amd", "csrc", "attn_loop_asm.inc")
    # RGN_ATTN_LOOP_SM_ASM ("static max", round 3): the caller guarantees a bound on every score (rgn_attention_bounded), so the
    # softmax needs no running max: P = exp2(S * c - m0) with a CONSTANT m0 - no tile max (25 VALU instructions + a cross-half
    # exchange per tile), no defer decision, no rescale block; everything else is the same loop
    variants = [("RGN_ATTN_LOOP_ASM", dict(D=4)), ("RGN_ATTN_LOOP_SM_ASM", dict(D=4, staticmax=True))]
    if os.environ.get("ATTN_GEN_EXPERIMENTS"):       # measurement builds only: prefetch distance 6 / 7, and two
        # timing-only ablations that compute WRONG results (no softmax VALU / no LDS fragment reads)
        variants += [("RGN_ATTN_LOOP_ASM_V1", dict(D=6)), ("RGN_ATTN_LOOP_ASM_V2", dict(D=7)),
                     ("RGN_ATTN_LOOP_ASM_V3", dict(D=4, novalu=True)), ("RGN_ATTN_LOOP_ASM_V4", dict(D=4, noread=True))]
    with open(out, "w") as f:
        f.write("// GENERATED by tools/gen_attn_loop.py - do not edit.  Hand-scheduled KV loop of attention_asm_kernel.\n")
        for name, kw in variants:
            CFG.update(dict(D=4, novalu=False, noread=False, prio=False, staticmax=False, pkfma=os.environ.get("ATTN_PKFMA", "0") == "1",
                            pkadd=os.environ.get("ATTN_PKADD", "0") == "1", dot2sum=os.environ.get("ATTN_DOT2SUM", "0") == "1",
                            dephase=os.environ.get("ATTN_DEPHASE", "0") == "1",
                            dmaspread=os.environ.get("ATTN_DMA_SPREAD", "1") == "1"))
            CFG.update(kw)
            lines = emit()
            n_mfma = sum(1 for l in lines if l.startswith("v_mfma"))
            f.write(f"// {name}: {len(lines)} instructions, {n_mfma} MFMAs\n")
            f.write(f"#define {name} \\\n")
            for l in lines:
                f.write(f'    "{l}\\n\\t" \\\n')
            f.write('    ""\n')
        lines = w_emit()
        n_mfma = sum(1 for l in lines if l.startswith("v_mfma"))
        f.write(f"// RGN_ATTN_LOOP_W64_ASM: {len(lines)} instructions, {n_mfma} MFMAs (4 waves x 64 query rows, static shift)\n")
        f.write("#define RGN_ATTN_LOOP_W64_ASM \\\n")
        for l in lines:
            f.write(f'    "{l}\\n\\t" \\\n')
        f.write('    ""\n')
        clob = [f'"a{n}"' for n in range(W_NA)] + [f'"v{n}"' for n in range(32, W_NV)] + ['"memory"', '"scc"', '"vcc"']
        f.write("#define RGN_ATTN_LOOP_W64_CLOBBERS " + ", ".join(clob) + "\n")
        clob = [f'"a{n}"' for n in range(96)] + [f'"v{n}"' for n in range(32, 160)] + ['"memory"', '"scc"', '"vcc"']
        f.write("#define RGN_ATTN_LOOP_CLOBBERS " + ", ".join(clob) + "\n")
    print(f"wrote {os.path.normpath(out)}")


if __name__ == "__main__":
    main()
