"""A model of the region attention kernels (regione_amd/csrc/attn.hip: rgn_attention / rgn_attention_bounded) and the probes that pin
every launch path of attention_schedule.  Plain torch, CPU or GPU tensors.  The fp64 reference, the bound, the seeded generators and the
two-value rule of the counting probe are the ones of tests/attn_tile_model.py.

  emulate_region     the scheme of the attn.hip header comment and of attention_kernel: 64-key tiles from key 0, a pad slot of the last
                     tile exactly -inf, a running max in scaled-log2 units that is raised (and o, l rescaled) only when a row's tile max
                     exceeds it by more than 8, l summed over the UNROUNDED fp32 p, P rounded to bf16 for the PV product, fp32
                     accumulation, out = bf16(o * (1 / l)); the keys dealt out as one launch, as equal pieces (attention_combine_kernel)
                     or as stream-K runs (attention_combine_sk_kernel); with named defects.  A model of the scheme, not of any
                     kernel's instruction order;
  *_case             probe inputs whose correct output is known EXACTLY (counting, spike, wrong head) and the random / stress inputs of
                     the bound check; a case carries q [H, Sq, 128], k, v [H, Skv, 128], scale and, where it applies, a score_bound;
  check_*            the checks.  tests/test_gpu_region_attn_probes.py applies them to the kernels, tests/test_region_attn_model.py
                     applies the same functions to `emulate_region` and shows that each defect fails at least one of them.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from attn_tile_model import BF16, _f32, _gen, _ints, bound, probe_mismatches, psnr, ref64, two_roundings  # noqa: F401 (re-exported)

KV_T = 64                                                           # keys per tile
DEFER_THR = 8.0                                                     # log2 units (DEFER_THR of attn.hip)
M_INIT = -1e30                                                      # the running max before the first tile (attn.hip: m_run = -1e30f)
FAMILIES = ["randn", "late_max", "first_max", "staircase"]
STRESS_LOGIT = 60.0
SCORE_BOUND = 66.0                                                  # 66 log2(e) = 95.2 <= 96: the static shift is legal
REGION_DEFECTS = ("drop_last_key", "count_one_padded_key", "no_rescale", "piece_last_tile_dropped", "run_boundary_tile_twice",
                  "stale_accumulator_in_second_segment", "merge_ignores_piece_max", "vt_group_permutation_missing", "wrong_head",
                  "ragged_q_block_reads_row_plus_one")


def kvpos(r):
    """Column of the V^T slab that holds key r (include/regione_hip.h: bits 2 and 3 of the key index swapped)."""
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


def padded(n, m=KV_T):
    return (n + m - 1) // m * m


def sl2e_of(scale):
    """scale * log2(e) as rgn_attention_bounded computes it: an fp32 product."""
    return float(np.float32(scale) * np.float32(1.4426950408889634))


# ---- how the keys of one item are dealt out ---------------------------------------------------------------------------------------------
def run_bound(w, total, G):
    return w * total // G


def item_segments(plan, u, nt):
    """The partial results that are merged into item u (index inside the split launch) of `nt` KV tiles: a list of
    (first tile, tile count, run, segment of the run, the run's last segment?).  Unsplit: one segment, run None."""
    if plan is None or plan == "unsplit":
        return [(0, nt, None, 0, True)]
    if plan[0] == "pieces":
        S = plan[1]
        per = (nt + S - 1) // S
        segs = [(s * per, max(0, min(per, nt - s * per)), s, 0, True) for s in range(S)]
        assert all(n > 0 for _, n, _, _, _ in segs), "attention_schedule never makes an empty piece"
        return segs
    assert plan[0] == "streamk"
    _, nitems, G = plan
    total, lo, hi = nitems * nt, u * nt, (u + 1) * nt
    out = []
    for w in range(G):
        a, b = run_bound(w, total, G), run_bound(w + 1, total, G)
        if b <= a or b <= lo or a >= hi:
            continue
        assert b - a <= nt, "a run crosses at most one item boundary"
        s, e = max(a, lo), min(b, hi)
        out.append((s - lo, e - s, w, 0 if a >= lo else 1, b <= hi))
    return out


def streamk_boundary(nitems, nt, G):
    """A run whose boundary falls mid-item: (item of the first segment, its last tile, item of the second, its first tile = 0, and the
    tile counts of the two segments), the first such run with at least two tiles on either side where there is one."""
    total, best = nitems * nt, None
    for w in range(G):
        a, b = run_bound(w, total, G), run_bound(w + 1, total, G)
        u = a // nt
        if b > (u + 1) * nt and a > u * nt:
            n0, n1 = (u + 1) * nt - a, b - (u + 1) * nt
            best = best or (u, nt - 1, u + 1, 0, n0, n1)
            if n0 >= 2 and n1 >= 2:
                return (u, nt - 1, u + 1, 0, n0, n1)
    return best


def streamk_run_edges(nitems, nt, G, u):
    """(last tile of the run that ends inside item u, first tile of the run that starts there): a run boundary strictly inside item u."""
    total = nitems * nt
    for w in range(1, G):
        a = run_bound(w, total, G)
        if u * nt < a < (u + 1) * nt:
            return a - u * nt - 1, a - u * nt
    return None


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
def _tiles(t, vf, first, count, state, any_row, static_shift, no_rescale, extra=()):
    """Tiles [first, first + count) (then the tiles of `extra`) of scaled-log2 scores t [G, 32, ntiles * 64] against vf [ntiles * 64, 128],
    from state (m, l, o)."""
    m, l, o = state
    for tt in list(range(first, first + count)) + list(extra):
        sc = t[..., tt * KV_T:(tt + 1) * KV_T]
        if not static_shift:
            mx = sc.amax(-1)
            need = mx > m + DEFER_THR
            if any_row:
                need = need.any(-1, keepdim=True).expand_as(mx)
            m_new = torch.where(need, torch.maximum(m, mx), m)
            alpha = torch.ones_like(m) if no_rescale else torch.exp2(m - m_new)
            l, o, m = l * alpha, o * alpha[..., None], m_new
        p = torch.exp2(sc - m[..., None])
        l = l + p.sum(-1)
        o = o + p.to(BF16).float() @ vf[tt * KV_T:(tt + 1) * KV_T]
    return m, l, o


def _zero_state(t, static_shift):
    G = t.shape[0]
    m = torch.full((G, 32), 0.0 if static_shift else M_INIT, device=t.device)
    return m, torch.zeros(G, 32, device=t.device), torch.zeros(G, 32, 128, device=t.device)


def group_rows(Sq, groups=None):
    """Query rows of the 32-row groups `groups` (all of them by default), as the kernel addresses them: [n, 32], clamped to Sq - 1."""
    ng = (Sq + 31) // 32
    g = torch.arange(ng) if groups is None else torch.as_tensor(sorted(set(int(x) for x in groups)))
    return g, (g[:, None] * 32 + torch.arange(32)[None, :])


def emulate_region(q, k, v, scale, plan=None, defect=None, static_shift=False, any_row=True, groups=None, heads=None, first_item=0, QB=256):
    """The region scheme on q [H, Sq, 128], k, v [H, Skv, 128] (bf16).  Returns (rows, out): the query rows evaluated (whole 32-row
    groups - one wave's rows, the unit of the deferred-max decision; all of them unless `groups` names some) and bf16
    [len(heads), len(rows), 128] (every head unless `heads` names some).

    plan            None / "unsplit"; ("pieces", S); ("streamk", nitems, G) - see item_segments.  Items (head h, block of QB query rows:
                    item = h * nQ + block) below `first_item` run unsplit (the whole rounds of attention_schedule); item
                    `first_item + u` is item u of the split launch.
    static_shift    m = 0 throughout, no rescale (rgn_attention_bounded on the hand-scheduled kernels).
    any_row         a raise of the running max is decided for the 32-row group (the kernels: __any over the wave) / per row.
    defect          one of REGION_DEFECTS:
      drop_last_key                         the last key is never counted
      count_one_padded_key                  the first pad key of the last tile (K = 0, V = 0) gets score 0 instead of -inf
      no_rescale                            alpha is forced to 1
      piece_last_tile_dropped               the last tile of every piece or run is never counted
      run_boundary_tile_twice               the first tile of a run's second segment (KV tile 0) is also counted by the first
      stale_accumulator_in_second_segment   the second stream-K segment starts from the first's m, o and l
      merge_ignores_piece_max               the merge weights are 1
      vt_group_permutation_missing          V is read at key index r where kvpos(r) is meant
      wrong_head                            head h reads V of head (h + 1) % H
      ragged_q_block_reads_row_plus_one     the rows of the last, partial query block take q of the next row, clamped"""
    assert defect is None or defect in REGION_DEFECTS, defect
    H, Sq, D = q.shape
    Skv = k.shape[1]
    assert D == 128 and k.shape == v.shape and k.shape[0] == H
    dev = q.device
    nt, nQ = (Skv + KV_T - 1) // KV_T, (Sq + QB - 1) // QB
    pad = nt * KV_T - Skv
    c = sl2e_of(scale)
    gidx, rows2 = group_rows(Sq, groups)
    rows2 = rows2.to(dev)
    valid = rows2 < Sq
    src = rows2.clamp(max=Sq - 1)
    if defect == "ragged_q_block_reads_row_plus_one" and Sq % QB:
        src = torch.where(rows2 >= (nQ - 1) * QB, (src + 1).clamp(max=Sq - 1), src)
    blocks = (gidx * 32 // QB).tolist()
    heads = list(range(H)) if heads is None else list(heads)
    out = torch.empty(len(heads), rows2.shape[0], 32, 128, dtype=BF16, device=dev)
    no_rescale = defect == "no_rescale"

    def scores(h, src_rows):
        t = (q[h][src_rows].float() @ k[h].float().T) * c                     # [G, 32, Skv]
        if defect == "drop_last_key":
            t[..., Skv - 1] = float("-inf")
        t = F.pad(t, (0, pad), value=float("-inf"))
        if defect == "count_one_padded_key" and pad:
            t[..., Skv] = 0.0
        return t

    for hi, h in enumerate(heads):
        vh = v[(h + 1) % H if defect == "wrong_head" else h].float()
        vh = F.pad(vh, (0, 0, 0, pad))
        if defect == "vt_group_permutation_missing":
            r = torch.arange(nt * KV_T, device=dev)
            vh = vh[kvpos(r)]
        t_all = scores(h, src)
        for b in sorted(set(blocks)):
            sel = torch.tensor([i for i, bb in enumerate(blocks) if bb == b], device=dev)
            t = t_all[sel]
            item = h * nQ + b
            u = item - first_item
            segs = item_segments(plan if u >= 0 else None, u, nt)
            parts = []
            for first, count, run, sg, run_ends in segs:
                state = _zero_state(t, static_shift)
                extra = ()
                if plan is not None and plan != "unsplit" and u >= 0 and plan[0] == "streamk":
                    if defect == "stale_accumulator_in_second_segment" and sg == 1:
                        # the run's first segment: the tail of the item before, for the same lanes (the same rows of its own block)
                        pi = item - 1
                        ph, pb = pi // nQ, pi % nQ
                        prow = (rows2[sel] - b * QB + pb * QB).clamp(max=Sq - 1)
                        pv = F.pad(v[ph].float(), (0, 0, 0, pad))
                        pf, pc = [s for s in item_segments(plan, u - 1, nt) if s[2] == run][0][:2]
                        state = _tiles(scores(ph, prow), pv, pf, pc, state, any_row, static_shift, no_rescale)
                    if defect == "run_boundary_tile_twice" and sg == 0 and not run_ends:
                        extra = (0,)
                if defect == "piece_last_tile_dropped" and run_ends:
                    count -= 1
                parts.append(_tiles(t, vh, first, count, state, any_row, static_shift, no_rescale, extra))
            if len(parts) == 1 and (plan is None or plan == "unsplit" or u < 0):
                m, l, o = parts[0]
            else:                                                   # attention_combine[_sk]_kernel
                mstar = torch.full_like(parts[0][0], M_INIT)
                for m_s, _, _ in parts:
                    mstar = torch.maximum(mstar, m_s)
                l, o = torch.zeros_like(parts[0][1]), torch.zeros_like(parts[0][2])
                for m_s, l_s, o_s in parts:
                    w = torch.ones_like(m_s) if defect == "merge_ignores_piece_max" else torch.exp2(m_s - mstar)
                    l, o = l + l_s * w, o + o_s * w[..., None]
            out[hi, sel] = (o * (1.0 / l)[..., None]).to(BF16)
    return rows2[valid], out[:, valid]


def defect_applies(defect, plan, Sq, Skv, H, QB=256):
    """False where the defect provably cannot change the output of the shape and plan."""
    split = plan is not None and plan != "unsplit"
    if defect == "count_one_padded_key":
        return Skv % KV_T != 0
    if defect in ("run_boundary_tile_twice", "stale_accumulator_in_second_segment"):
        return split and plan[0] == "streamk"
    if defect == "merge_ignores_piece_max":
        return split
    if defect == "wrong_head":
        return H > 1
    if defect == "ragged_q_block_reads_row_plus_one":
        return Sq % QB != 0 and Sq > 1
    if defect == "vt_group_permutation_missing":
        return Skv > 4
    return True


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _case(q, k, v, scale, **extra):
    return SimpleNamespace(q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), scale=scale, **extra)


def to_device(case, device):
    c = SimpleNamespace(**vars(case))
    c.q, c.k, c.v = c.q.to(device), c.k.to(device), c.v.to(device)
    return c


def sub_case(case, heads=None, rows=None):
    """The case restricted to some heads and query rows (what a sampled emulation or reference looks at)."""
    c = SimpleNamespace(**vars(case))
    if heads is not None:
        c.q, c.k, c.v = c.q[list(heads)], c.k[list(heads)], c.v[list(heads)]
    if rows is not None:
        c.q = c.q[:, rows]
    return c


def counting_case(Sq, Skv, H):
    """q = 0: every key has weight exactly 1 and the row sum is exactly Skv.  V holds integers of [-4, 4], so every sum is exact in fp32
    in any order for Skv <= 2^20 (|sum| <= 4 Skv < 2^24); K is N(0, 1) and must not matter.  Every query row of head h returns one of
    the two roundings of sum / Skv of that head."""
    g = _gen(11, Sq, Skv, H)
    k, v = torch.randn(H, Skv, 128, generator=g), _ints(g, (H, Skv, 128))
    return _case(torch.zeros(H, Sq, 128), k, v, 128 ** -0.5, kind="counting", score_bound=SCORE_BOUND)


SPIKE_SCALE = 0.043321698904037476                                  # the fp32 number whose fp32 product with log2(e) is exactly 2^-4
SPIKE_GAINS = (1.0, 1.25, 1.5)


def spike_case(Sq, Skv, H, j):
    """Key j scores 40 above every other key for every query, built as the decode-attention spike of tests/test_gpu_qwen_generate.py:
    k_j = 8 u per head, the other keys 0.01 N(0, 1), q = gain_i u with the gains cycling over {1, 1.25, 1.5}.  u holds +-1 in 120
    channels and 0 in 8, and scale * log2(e) is exactly 2^-4 in fp32: the spike score is exactly 60 gain in log2 units (41.6, 52.0, 62.4
    nats), so its weight is exactly 1 under the running max and an exact power of two under the static shift - P rounded to bf16 for the
    PV product and the unrounded P of the row sum are then the same number, and the row returns V[j] bit for bit.  (With a spike weight
    that bf16 rounds, the static shift legitimately returns bf16(V[j] (1 + e)), |e| <= 2^-8: not a probe.)  The other weights total at
    most Skv e^-40 < 2e-13 relative, far inside a bf16 step.  V is N(0, 1) in bf16."""
    assert 0 <= j < Skv
    assert sl2e_of(SPIKE_SCALE) == 2.0 ** -4
    g = _gen(12, Sq, Skv, H, j)
    u = (2.0 * torch.randint(0, 2, (H, 128), generator=g).float() - 1.0)
    u[:, torch.randperm(128, generator=g)[:8]] = 0.0
    gain = torch.tensor(SPIKE_GAINS)[torch.arange(Sq) % 3]
    q = gain[None, :, None] * u[:, None, :]
    k = 0.01 * torch.randn(H, Skv, 128, generator=g)
    k[:, j] = 8.0 * u
    c = _case(q, k, torch.randn(H, Skv, 128, generator=g), SPIKE_SCALE, kind="spike", j=j, score_bound=SCORE_BOUND)
    check_spike_shape(c, rows=slice(0, 3))
    return c


def check_spike_shape(c, rows=slice(None)):
    """In fp64: the gap is >= 40 and max |s| <= 64."""
    s = _f32(c.scale) * (c.q[:, rows].double() @ c.k.double().transpose(1, 2))
    assert float(s.abs().max()) <= 64.0, float(s.abs().max())
    if s.shape[-1] > 1:
        rest = s.clone()
        rest[..., c.j] = float("-inf")
        assert float((s[..., c.j] - rest.amax(-1)).min()) >= 40.0


def wrong_head_case(Sq, Skv, H):
    """V of head h is h + 1 everywhere, q and k are N(0, 1): head h returns h + 1 exactly.  (o = (h + 1) sum bf16(p), l = sum p: the
    quotient is (h + 1)(1 + e) with e the p-weighted mean of the bf16 rounding errors of the weights; for a value up to 24 to leave its
    bf16 cell |e| would have to exceed 0.53 * 2^-8, more than the largest single error 2^-8 / (1 + 2^-8) allows the mean of 63 or more
    weights of scattered mantissas - and one key has p = 1 exactly.)"""
    g = _gen(13, Sq, Skv, H)
    q, k = torch.randn(H, Sq, 128, generator=g), torch.randn(H, Skv, 128, generator=g)
    v = (torch.arange(H).float() + 1)[:, None, None].expand(H, Skv, 128).clone()
    return _case(q, k, v, 128 ** -0.5, kind="wrong_head", score_bound=SCORE_BOUND)


def bound_case(family, Sq, Skv, H):
    """Inputs of the fp64 bound check.  randn: q, k, v of N(0, 1).  The stress families steer the logits through channel 0, per 64-key
    tile (the other channels are N(0, 0.4^2), a logit noise of sigma 0.16):
      late_max    scale q.k climbs from -60 in the first key tile to +60 in the last: the running maximum moves in every tile where the
                  step exceeds the deferral threshold and the largest score of every row lies in the last tile;
      first_max   key 0 at +60, the tiles falling from +56 to -60: the maximum never moves after the first tile;
      staircase   the logit rises by 5 nats (7.2 log2 units, under the threshold of 8) every third tile, centred on 0: the kernel keeps a
                  stale maximum, P exceeds 1 (up to 2^8) before the next raise.
    Every family keeps max |s| <= 64 (check_stress_shape), so the same inputs are legal for score_bound = 66."""
    assert family in FAMILIES
    g = _gen(14, Sq, Skv, H, FAMILIES.index(family))
    scale = 128 ** -0.5
    if family == "randn":
        q, k = torch.randn(H, Sq, 128, generator=g), torch.randn(H, Skv, 128, generator=g)
    else:
        q, k = 0.4 * torch.randn(H, Sq, 128, generator=g), 0.4 * torch.randn(H, Skv, 128, generator=g)
        tile = (torch.arange(Skv) // KV_T).float()
        nt = int(tile[-1]) + 1
        if family == "late_max":
            t = -STRESS_LOGIT + 2 * STRESS_LOGIT * tile / (nt - 1) if nt > 1 else torch.full((Skv,), STRESS_LOGIT)
        elif family == "first_max":
            t = (STRESS_LOGIT - 4) - (2 * STRESS_LOGIT - 4) * tile / (nt - 1) if nt > 1 else torch.full((Skv,), -STRESS_LOGIT)
            t[0] = STRESS_LOGIT
        else:
            steps = torch.floor(tile / 3)
            # 5 nats a step while that stays inside +-55 (23 steps = 69 tiles); beyond, the steps shrink to fit
            t = (steps - steps[-1] / 2) * min(5.0, 110.0 / max(float(steps[-1]), 1.0))
        q[..., 0] = 8.0
        k[..., 0] = t[None, :] / (_f32(scale) * 8.0)
    return _case(q, k, torch.randn(H, Skv, 128, generator=g), scale, kind="bound", family=family, score_bound=SCORE_BOUND)


def check_stress_shape(case, rows=None):
    """The promises of bound_case, on the fp64 logits of query rows `rows` (all by default): max |s| <= 64 - and <= score_bound - for
    every family; late_max: the largest logit of a row lies in the last key tile; first_max: on key 0; staircase: under the deferred rule every row
    meets a tile whose maximum lies more than 6 log2 units above the running maximum it keeps (P > 2^6), wherever there are 4 tiles."""
    q = case.q if rows is None else case.q[:, rows]
    s = _f32(case.scale) * (q.double() @ case.k.double().transpose(1, 2))
    smax = float(s.abs().max())
    assert smax <= 64.0 and smax <= case.score_bound, smax
    if case.family == "randn":
        return
    Skv = s.shape[-1]
    nt = (Skv + KV_T - 1) // KV_T
    arg = s.argmax(-1)
    if case.family == "late_max":
        assert bool((arg // KV_T == nt - 1).all()), "the largest logit of a row is not in its last key tile"
    elif case.family == "first_max":
        assert bool((arg == 0).all()), "the largest logit of a row is not on its first key"
    else:
        tm = F.pad(s, (0, nt * KV_T - Skv), value=float("-inf")).view(*s.shape[:-1], nt, KV_T).amax(-1) * 1.4426950408889634
        m, stale = tm[..., 0].clone(), torch.zeros_like(tm[..., 0])           # the deferred rule, per row, on the fp64 tile maxima
        for tt in range(1, nt):
            m = torch.where(tm[..., tt] > m + DEFER_THR, tm[..., tt], m)
            stale = torch.maximum(stale, tm[..., tt] - m)
        if nt >= 4:
            assert float(stale.min()) > 6.0, "a row never computes P > 2^6 under a stale maximum"
        assert float(stale.max()) <= DEFER_THR


# ---- expected outputs and checks -------------------------------------------------------------------------------------------------------
def counting_allowed(case):
    """The two values of the counting probe, bf16 [H, 1, 128] each: one row per head, no Sq x Skv reference."""
    total = case.v.double().sum(1, keepdim=True)
    return two_roundings(total, torch.full_like(total, float(case.v.shape[1])))


def check_counting(case, out):
    a, b = counting_allowed(case)
    return probe_mismatches(out, a.expand_as(out), b.expand_as(out))


def check_spike(case, out):
    want = case.v[:, case.j][:, None, :].expand_as(out)
    return int((out != want).sum())


def check_wrong_head(case, out):
    return int((out != case.v[:, :1, :1].expand_as(out)).sum())


CHECKS = {"counting": check_counting, "spike": check_spike, "wrong_head": check_wrong_head}


def bound_rows(Sq, n=192):
    """The query rows of a sampled fp64 reference: row 0, the last row, both rows around every 256-row block edge, seeded others."""
    if Sq <= n:
        return torch.arange(Sq)
    must = {0, Sq - 1}
    for e in range(256, Sq, 256):
        must |= {e - 1, e}
    assert len(must) <= n
    perm = torch.randperm(Sq, generator=_gen(15, Sq)).tolist()
    for r in perm:
        if len(must) == n:
            break
        must.add(r)
    return torch.tensor(sorted(must))


def bound_ratio(case, out, rows=None):
    """max |out - O_ref| / bound over the query rows `rows` of out [H, Sq, 128] (all by default); a NaN counts as infinite."""
    q, o = (case.q, out) if rows is None else (case.q[:, rows], out[:, rows])
    O_ref, A_ref = ref64(q, case.k, case.v, case.scale)
    assert bool(torch.isfinite(O_ref).all()) and bool(torch.isfinite(A_ref).all()), "the fp64 reference itself must be finite"
    r = (o.double() - O_ref).abs() / bound(O_ref, A_ref)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


# ---- the launch paths of attention_schedule (tests/test_gpu_region_attn_probes.py runs every row, tests/test_region_attn_model.py ------
# confirms the plans on the CPU through rgn_attention_plan_query) ----------------------------------------------------------------------
WS_ALL = 128 << 20


def _row(name, Sq, Skv, H, knobs, waves8, pieces, streamk=False, ws=WS_ALL, asm=False, bounded=(False,), left=None):
    """One launch path.  ws: workspace bytes; asm: the hand-scheduled kernels (whole KV tiles); bounded: the score-bound settings the
    row runs with (True = score_bound 66: the static shift, on the hand-scheduled kernels only); left: the items of the split launch
    (the remainder after the whole rounds; every item by default)."""
    QB = 256 if waves8 else 128
    nitems = H * ((Sq + QB - 1) // QB)
    slots = 256 if waves8 else 512
    left = nitems - nitems // slots * slots if left is None else left
    return SimpleNamespace(name=name, Sq=Sq, Skv=Skv, H=H, knobs=knobs, waves8=waves8, pieces=pieces, streamk=streamk, ws=ws, asm=asm,
                           bounded=bounded, QB=QB, nitems=nitems, left=left, first_item=nitems - left, slots=slots)


def _table():
    rows = []
    for Sq in (1, 127, 128, 129, 200):
        for Skv in (1, 63, 64, 65, 127, 129, 1000):
            rows.append(_row(f"c4-unsplit-{Sq}x{Skv}", Sq, Skv, 3, dict(attn_waves=4, attn_split=0), False, 1))
    for S, ws in ((2, 4 * 2 * 128 * 130 * 4), (3, 4 * 3 * 128 * 130 * 4), (6, WS_ALL)):
        rows.append(_row(f"c4-split{S}", 129, 1664, 2, dict(attn_waves=4), False, S, ws=ws))
    for Sq in (1, 255, 256, 257, 300):
        rows.append(_row(f"c8-ragged-unsplit-{Sq}", Sq, 1000, 2, dict(attn_waves=8, attn_split=0), True, 1))
    rows.append(_row("c8-ragged-split8", 300, 2533, 2, dict(attn_waves=8), True, 8))
    for n in (1, 2, 3, 4, 5, 6, 7, 10, 11):
        rows.append(_row(f"asm-unsplit-{n}t", 300, 64 * n, 2, dict(attn_waves=8, attn_split=0), True, 1, asm=True, bounded=(False, True)))
    rows.append(_row("asm-split8", 300, 2560, 2, dict(attn_waves=8, attn_streamk=0), True, 8, asm=True, bounded=(False, True)))
    rows.append(_row("asm-split7", 300, 2624, 2, dict(attn_waves=8, attn_streamk=0), True, 7, asm=True, bounded=(False, True)))
    rows.append(_row("asm-streamk", 1100, 3328, 8, dict(attn_waves=8, attn_streamk=1), True, 1, True, asm=True, bounded=(False, True)))
    rows.append(_row("rounds+split4", 2900, 1024, 24, dict(attn_streamk=0), True, 4, asm=True))
    rows.append(_row("rounds+ragged-split4", 2900, 1000, 24, dict(), True, 4))
    rows.append(_row("rounds+streamk", 2900, 4096, 24, dict(attn_streamk=1), True, 1, True, asm=True))
    rows.append(_row("rounds+unsplit-tail", 2900, 512, 24, dict(), True, 1, asm=True))
    return rows


TABLE = _table()
TABLE_BY_NAME = {r.name: r for r in TABLE}
# one row per kernel class (the wrong-head probe and the O-aliases-Q repeat of the spike probe run on these)
CLASS_ROWS = ["c4-unsplit-129x129", "c4-split3", "c8-ragged-unsplit-300", "c8-ragged-split8", "asm-unsplit-5t", "asm-split7", "asm-streamk"]


def _wrong_head_table():
    """The rows of the wrong-head probe: one per kernel class, with H = 3 and H = 24, the whole workspace.  (Stream-K needs 8 steps per
    workgroup slot: with H = 3, 15 items of 137 tiles.)"""
    W4, W8 = dict(attn_waves=4), dict(attn_waves=8)
    rows = []
    for H in (3, 24):
        rows += [_row(f"c4-unsplit-H{H}", 129, 129, H, dict(attn_waves=4, attn_split=0), False, 1),
                 _row(f"c4-split-H{H}", 129, 1664, H, W4, False, 6),
                 _row(f"c8-ragged-unsplit-H{H}", 300, 1000, H, dict(attn_waves=8, attn_split=0), True, 1),
                 _row(f"c8-ragged-split-H{H}", 300, 2533, H, W8, True, 8 if H == 3 else 5),
                 _row(f"asm-unsplit-H{H}", 300, 320, H, dict(attn_waves=8, attn_split=0), True, 1, asm=True, bounded=(False, True)),
                 _row(f"asm-split-H{H}", 300, 2624, H, dict(attn_waves=8, attn_streamk=0), True, 7 if H == 3 else 5, asm=True,
                      bounded=(False, True)),
                 _row(f"asm-streamk-H{H}", 1100, 8768 if H == 3 else 3328, H, dict(attn_waves=8, attn_streamk=1), True, 1, True, asm=True,
                      bounded=(False, True))]
    return rows


WRONG_HEAD_TABLE = _wrong_head_table()
ALL_ROWS = {r.name: r for r in TABLE + WRONG_HEAD_TABLE}


def plan_of(row):
    """The `plan` of emulate_region for a row of the table."""
    if row.streamk:
        return ("streamk", row.left, row.slots)
    return ("pieces", row.pieces) if row.pieces > 1 else None


def expected_plan_bits(row):
    return (1 if row.streamk else row.pieces) | (0x10 if row.streamk else 0) | (0x20 if row.waves8 else 0)


def spike_keys(row):
    """The keys of the spike probe for a row: 0, 63, 64, Skv - 1 (the last real key of a ragged tail); the first and last key of a split
    piece; for stream-K the last key of one run's first segment and the first key of its second, in an item whose boundary falls
    mid-item (with the item, so that the test can look at its rows); on Skv = 64 the keys kvpos moves."""
    Skv, nt = row.Skv, (row.Skv + KV_T - 1) // KV_T
    js = {0, min(63, Skv - 1), min(64, Skv - 1), Skv - 1}
    if Skv == 64:
        js |= {4, 8, 12, 20}
    if row.pieces > 1:
        per = (nt + row.pieces - 1) // row.pieces
        js |= {per * KV_T - 1, per * KV_T, (row.pieces - 1) * per * KV_T - 1, (row.pieces - 1) * per * KV_T}
    if row.streamk:
        b = streamk_boundary(row.left, nt, row.slots)             # None: every run ends where an item ends (32 items x 64 tiles / 256)
        last, first = streamk_run_edges(row.left, nt, row.slots, b[0] if b else 0)
        js |= {last * KV_T + KV_T - 1, first * KV_T}
    return sorted(j for j in js if 0 <= j < Skv)
