// block.hip - one masked MMDiT block per call (rgn_mmdit_double_block / rgn_mmdit_single_block, include/regione_hip.h).  Host code only:
// every launch goes through the library's own entry points, in the order and with the arguments of the harness blocks
// (regione_amd/harness/flux.py: FluxTransformerBlock.__call__, FluxSingleTransformerBlock.__call__, FluxAttnProcessor.__call__ with
// FUSE_QKV), so a block run through one call is bit-identical to the same block run launch by launch.
#include <math.h>

#include "common.h"

using namespace rgn;

namespace {

constexpr float kEps = 1e-6f;

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline const void* chunk(const void* vec, int d, int i) { return (const uint16_t*)vec + (size_t)i * d; }

bool bad_weight(const rgn_block_weight& w) { return !w.W || misaligned(w.W) || misaligned(w.wscale) || misaligned(w.bias); }

// everything both kinds share; nothing is launched before this returns 0
int validate(const rgn_mmdit_block* b, bool single) {
    if (!b) return fail(RGN_E_BADARG, "mmdit_block: null descriptor");
    if (!b->x || !b->nrm || !b->wide) return fail(RGN_E_BADARG, "mmdit_block: null activation buffer (x / nrm / wide)");
    if (b->T < 0 || b->M <= 0) return fail(RGN_E_BADARG, "mmdit_block: T must be >= 0 and M > 0");
    if (b->d <= 0 || (b->d % 64) || b->d_ff <= 0 || (b->d_ff % 64)) return fail(RGN_E_BADARG, "mmdit_block: d and d_ff must be positive multiples of 64");
    if (b->heads <= 0 || (long long)b->heads * 128 != b->d) return fail(RGN_E_BADARG, "mmdit_block: heads * 128 must equal d");
    if ((b->ldx % 8) || (b->ldnrm % 8) || (b->ldwide % 8) || b->ldx < b->d || b->ldnrm < b->d || b->ldwide < 3 * b->d + b->d_ff)
        return fail(RGN_E_BADARG, "mmdit_block: row strides must be multiples of 8 and cover d / 3 d + d_ff columns");
    if (b->skv <= 0 || b->skv_pad < b->skv || (b->skv_pad % 64)) return fail(RGN_E_BADARG, "mmdit_block: skv_pad must be a multiple of 64 and >= skv >= 1");
    if (!b->kv_rows && (long long)b->T + b->M > b->skv_pad) return fail(RGN_E_BADARG, "mmdit_block: identity cache rows exceed skv_pad");
    if (!b->k_slab || !b->vt_slab || !b->cos_q || !b->sin_q || !b->cos_k || !b->sin_k) return fail(RGN_E_BADARG, "mmdit_block: null K / V^T slab or rotary table");
    if (!b->adaln || (!single && !b->adaln_txt)) return fail(RGN_E_BADARG, "mmdit_block: null AdaLN vector");
    if (!b->norm_q || !b->norm_k || (!single && (!b->norm_added_q || !b->norm_added_k))) return fail(RGN_E_BADARG, "mmdit_block: null RMSNorm weights");
    if ((b->gemm_ws_bytes && !b->gemm_ws) || (b->attn_ws_bytes && !b->attn_ws)) return fail(RGN_E_BADARG, "mmdit_block: workspace size without a workspace");
    const rgn_block_weight* ws2[] = {&b->w_kvq, &b->w_add_kvq, &b->w_out, &b->w_add_out, &b->ff_w1, &b->ffc_w1, &b->ff_w2, &b->ffc_w2};
    const rgn_block_weight* ws1[] = {&b->w_kvqm, &b->w_po};
    bool any8 = false, all8 = true;
    for (int i = 0; i < (single ? 2 : 8); ++i) {
        const rgn_block_weight& w = single ? *ws1[i] : *ws2[i];
        if (bad_weight(w)) return fail(RGN_E_BADARG, "mmdit_block: a weight is NULL or W / wscale / bias is not 16-byte aligned");
        any8 = any8 || w.wscale; all8 = all8 && w.wscale;
    }
    const void* ptrs[] = {b->x, b->nrm, b->wide, b->adaln, b->adaln_txt, b->norm_q, b->norm_k, b->norm_added_q, b->norm_added_k, b->k_slab,
                          b->vt_slab, b->cos_q, b->sin_q, b->cos_k, b->sin_k, b->gemm_ws, b->attn_ws};
    for (const void* p : ptrs)
        if (misaligned(p)) return fail(RGN_E_BADARG, "mmdit_block: pointers must be 16-byte aligned");
    if (b->kv_rows && ((uintptr_t)b->kv_rows & 7)) return fail(RGN_E_BADARG, "mmdit_block: kv_rows must be 8-byte aligned");
    if (b->rowbands != 0 && b->rowbands != 1) return fail(RGN_E_BADARG, "mmdit_block: rowbands is 0 or 1");
    if (b->heads % 2) return fail(RGN_E_UNSUPPORTED, "mmdit_block: an odd head count takes the non-fused path (the fused Q/K/V epilogue works on two-head blocks)");
    if (b->out_rows != 0) return fail(RGN_E_UNSUPPORTED, "mmdit_block: the row-skipping last block (out_rows) is not covered");
    if (b->branches != 1) return fail(RGN_E_UNSUPPORTED, "mmdit_block: several CFG branches in one call (multi) are not covered");
    if (any8 && !all8) return fail(RGN_E_UNSUPPORTED, "mmdit_block: all weight matrices must have the same format");
    return 0;
}

inline uint16_t* at(void* base, int ld, int row, int col = 0) { return (uint16_t*)base + (size_t)row * ld + col; }

rgn_gemm_problem problem(const void* A, int lda, const rgn_block_weight& w, void* C, int ldc, int M, const void* gate = nullptr,
                         const void* resid = nullptr, const rgn_qkv_epilogue* e = nullptr) {
    rgn_gemm_problem p;
    p.A = A; p.W = w.W; p.wscale = w.wscale; p.bias = w.bias; p.C = C; p.gate = gate; p.resid = resid; p.qkv = e; p.out_rows = nullptr;
    p.lda = lda; p.ldc = ldc; p.M = M; p.ldw = 0; p.ascale = nullptr;      // bf16 activations: the block entries have no fp8-activation form
    return p;
}

// image problem first, text problem second (the order of ops.gemm_pair in the harness); empty problems are dropped as ops._launch drops them
int launch(const rgn_mmdit_block* b, rgn_gemm_problem p0, const rgn_gemm_problem* p1, int N, int K, int epilogue, int gelu_from_col, void* stream) {
    rgn_gemm_problem ps[2];
    int n = 0;
    if (p0.M > 0) ps[n++] = p0;
    if (p1 && p1->M > 0) ps[n++] = *p1;
    if (n == 0) return 0;
    return rgn_gemm_group(ps, n, N, K, epilogue, gelu_from_col, b->gemm_ws, b->gemm_ws_bytes, stream);
}

rgn_qkv_epilogue epilogue(const rgn_mmdit_block* b, const void* wq, const void* wk, int row_base, int fp16_roundtrip) {
    rgn_qkv_epilogue e;
    e.wq = wq; e.wk = wk; e.cos_q = b->cos_q; e.sin_q = b->sin_q; e.cos_k = b->cos_k; e.sin_k = b->sin_k;
    e.kv_rows = b->kv_rows; e.k_slab = b->k_slab; e.vt_slab = b->vt_slab;
    e.row_base = row_base; e.skv_pad = b->skv_pad; e.k_col = 0; e.v_col = b->d; e.q_col = 2 * b->d; e.heads = b->heads;
    e.eps = kEps; e.fp16_roundtrip = fp16_roundtrip;
    return e;
}

// FluxAttnProcessor._attention: attention reads every row - the bands of the stages before it join here and fork again behind it
int attention(const rgn_mmdit_block* b, void* stream) {
    const int R = b->T + b->M;
    int rc = rgn_rowband_join(stream);
    if (rc) return rc;
    uint16_t* q = at(b->wide, b->ldwide, 0, 2 * b->d);
    rc = rgn_attention_bounded(q, b->ldwide, b->k_slab, b->vt_slab, b->skv_pad, q, b->ldwide, R, b->skv, b->heads, (float)(1.0 / sqrt(128.0)),
                               b->score_bound, b->attn_ws, b->attn_ws_bytes, stream);
    if (rc) return rc;
    return b->rowbands ? rgn_rowband_fork(stream) : 0;
}

}  // namespace

extern "C" {

size_t rgn_mmdit_block_bytes(void) { return sizeof(rgn_mmdit_block); }

int rgn_mmdit_double_block(const rgn_mmdit_block* b, void* stream) {
    int rc = validate(b, false);
    if (rc) return rc;
    const int T = b->T, M = b->M, R = T + M, d = b->d, ff = b->d_ff;
    const int partial = b->kv_rows != nullptr;
    const void* ai = b->adaln; const void* at_ = b->adaln_txt;
    uint16_t *x_img = at(b->x, b->ldx, T), *x_txt = at(b->x, b->ldx, 0);
    uint16_t *n_img = at(b->nrm, b->ldnrm, T), *n_txt = at(b->nrm, b->ldnrm, 0);
    // norm1 / norm1_context: rows < T take the text stream's (shift_msa, scale_msa)
    if ((rc = rgn_ln_modulate(b->x, b->ldx, b->nrm, b->ldnrm, R, d, kEps, T, T > 0 ? chunk(at_, d, 0) : nullptr, T > 0 ? chunk(at_, d, 1) : nullptr,
                              chunk(ai, d, 0), chunk(ai, d, 1), stream)))
        return rc;
    // Q/K/V of both streams, RMSNorm + RoPE + K / V^T placement in the epilogue: one launch; only the image rows are ever partial
    {
        rgn_qkv_epilogue e_img = epilogue(b, b->norm_q, b->norm_k, T, partial);
        rgn_qkv_epilogue e_txt = epilogue(b, b->norm_added_q, b->norm_added_k, 0, 0);
        rgn_gemm_problem p_txt = problem(n_txt, b->ldnrm, b->w_add_kvq, at(b->wide, b->ldwide, 0), b->ldwide, T, nullptr, nullptr, &e_txt);
        if ((rc = launch(b, problem(n_img, b->ldnrm, b->w_kvq, at(b->wide, b->ldwide, T), b->ldwide, M, nullptr, nullptr, &e_img), &p_txt, 3 * d, d,
                         RGN_EPI_QKV, 0, stream)))
            return rc;
    }
    if ((rc = attention(b, stream))) return rc;
    // to_out / to_add_out with the gated residual (gate_msa)
    {
        rgn_gemm_problem p_txt = problem(at(b->wide, b->ldwide, 0, 2 * d), b->ldwide, b->w_add_out, x_txt, b->ldx, T, chunk(at_, d, 2), x_txt);
        if ((rc = launch(b, problem(at(b->wide, b->ldwide, T, 2 * d), b->ldwide, b->w_out, x_img, b->ldx, M, chunk(ai, d, 2), x_img), &p_txt, d, d,
                         RGN_EPI_GATE_RESID, 0, stream)))
            return rc;
    }
    // norm2 / norm2_context + feed-forward, the gated residual (gate_mlp) fused into the second GEMM
    if ((rc = rgn_ln_modulate(b->x, b->ldx, b->nrm, b->ldnrm, R, d, kEps, T, T > 0 ? chunk(at_, d, 3) : nullptr, T > 0 ? chunk(at_, d, 4) : nullptr,
                              chunk(ai, d, 3), chunk(ai, d, 4), stream)))
        return rc;
    {
        rgn_gemm_problem p_txt = problem(n_txt, b->ldnrm, b->ffc_w1, at(b->wide, b->ldwide, 0, 3 * d), b->ldwide, T);
        if ((rc = launch(b, problem(n_img, b->ldnrm, b->ff_w1, at(b->wide, b->ldwide, T, 3 * d), b->ldwide, M), &p_txt, ff, d, RGN_EPI_GELU, 0, stream)))
            return rc;
    }
    {
        rgn_gemm_problem p_txt = problem(at(b->wide, b->ldwide, 0, 3 * d), b->ldwide, b->ffc_w2, x_txt, b->ldx, T, chunk(at_, d, 5), x_txt);
        if ((rc = launch(b, problem(at(b->wide, b->ldwide, T, 3 * d), b->ldwide, b->ff_w2, x_img, b->ldx, M, chunk(ai, d, 5), x_img), &p_txt, d, ff,
                         RGN_EPI_GATE_RESID, 0, stream)))
            return rc;
    }
    return 0;
}

int rgn_mmdit_single_block(const rgn_mmdit_block* b, void* stream) {
    int rc = validate(b, true);
    if (rc) return rc;
    const int R = b->T + b->M, d = b->d, ff = b->d_ff;
    const int partial = b->kv_rows != nullptr;
    if ((rc = rgn_ln_modulate(b->x, b->ldx, b->nrm, b->ldnrm, R, d, kEps, 0, nullptr, nullptr, chunk(b->adaln, d, 0), chunk(b->adaln, d, 1), stream)))
        return rc;
    // one GEMM produces [k | v | q | gelu(mlp)] from the same normed activations; every row of a partial update takes the fp16 round trip
    {
        rgn_qkv_epilogue e = epilogue(b, b->norm_q, b->norm_k, 0, partial);
        if ((rc = launch(b, problem(b->nrm, b->ldnrm, b->w_kvqm, b->wide, b->ldwide, R, nullptr, nullptr, &e), nullptr, 3 * d + ff, d, RGN_EPI_QKV, 3 * d,
                         stream)))
            return rc;
    }
    if ((rc = attention(b, stream))) return rc;
    // proj_out over cat([attn_output, mlp_hidden]) = columns [2 d, 3 d + d_ff) of `wide`, gated residual
    return launch(b, problem(at(b->wide, b->ldwide, 0, 2 * d), b->ldwide, b->w_po, b->x, b->ldx, R, chunk(b->adaln, d, 2), b->x), nullptr, d, d + ff,
                  RGN_EPI_GATE_RESID, 0, stream);
}

}  // extern "C"
