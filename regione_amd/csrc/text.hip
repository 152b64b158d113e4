// Text encoders of FLUX.1 Kontext (`encode_prompt`, reference call sites FluxKontext/inplace.py:185-211):
// [EXT] transformers CLIPTextModel (the pooled vector) and T5EncoderModel (the 512 context tokens).  Every projection is rgn_gemm_group;
// this file holds what the two encoders add around it:
//   text_attention_kernel     self-attention read straight from the fused QKV GEMM output [L, (Hq + 2 Hkv) D] -> O [L, Hq D] on the tile
//                             core of attn_tile.h.  D = 64, Hq = Hkv: scale, causal mask (CLIP), per-head relative-position bias table (T5)
//   text_embed_kernel         token-embedding gather (+ CLIP's absolute position row); ids out of range give zero rows
//   geglu_kernel              T5 v1.1 gated-GELU product bf16(gelu(wi_0 x) * wi_1 x) from the [wi_1 ; wi_0] GEMM output
//   quick_gelu_kernel         CLIP's x * sigmoid(1.702 x), with the three roundings of the eager bf16 op sequence
//   layer_norm_rows_kernel    affine LayerNorm (gamma, beta) over rows (CLIP's layer_norm1 / layer_norm2 / final_layer_norm)
//   text_pool_row_kernel      CLIP's pooled row (argmax(input_ids) when eos_token_id == 2, else the first eos) on the device
// and what the language model of Qwen-Image-Edit's prompt encoder ([EXT] transformers Qwen2_5_VLForConditionalGeneration) adds:
//   text_attention_kernel     at D = 128: causal grouped-query self-attention from the fused QKV GEMM output [L, (Hq + 2 Hkv) 128]
//   mrope_kernel              multimodal RoPE on the q and k columns of that buffer, in place, with the eager op sequence's roundings
//   swiglu_kernel             Qwen2MLP's bf16(bf16(silu(gate)) * up) from the [gate_proj ; up_proj] GEMM output
// Row kernels round where torch's eager bf16 ops round (the file is built with -ffp-contract=off); every reduction has a fixed order.
#include "attn_tile.h"

namespace rgn {

// ---- self-attention over the fused QKV GEMM output (head width 64: CLIP / T5; 128: the Qwen2.5-VL language model) ------------------
// Block = one query head x 64 queries on the tile core of attn_tile.h.  Query head h reads the K/V columns of KV head h / (Hq / Hkv); the
// Hq / Hkv blocks of a group run side by side and share the tiles through L2 (attention is ~2 % of the LM's FLOPs; one staged tile per
// group would trade occupancy for little).
//   t = s * scale (+ bias[j - i + Lmax - 1]); masked keys (j >= L, causal j > i) are -inf
// The bias window of the head ([2 L - 1] entries around the diagonal) is staged in LDS as fp32 once per block.
// Causal: key tiles past the block's last query are never staged, and a wave skips the MFMAs of a staged tile that lies wholly above ITS
// 16 queries - every weight there would be exp2(-inf) = 0 and alpha = 1, so the skip changes no bit.  Key 0 is valid for every query.
constexpr int TA_MAX_L = 4096, LA_MAX_L = 4096;

template <int D, bool BIAS, bool CAUSAL>
__global__ __launch_bounds__(256) void text_attention_kernel(const uint16_t* __restrict__ QKV, uint16_t* __restrict__ O, int L, int Hq, int Hkv,
                                                             float scale, const uint16_t* __restrict__ bias, int Lmax) {
    using T = AttnTile<D>;
    __shared__ __attribute__((aligned(16))) uint16_t kl[T::K_LDS];
    __shared__ __attribute__((aligned(16))) uint16_t vl[T::V_LDS];
    extern __shared__ float bl[];                      // BIAS: bl[j - i + L - 1] = bias[h][j - i + Lmax - 1]
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int hk = h / (Hq / Hkv);
    const int q0 = blockIdx.x * T::BQ;
    const size_t ld = (size_t)(Hq + 2 * Hkv) * D, ldo = (size_t)Hq * D;
    const uint16_t* Qh = QKV + (size_t)h * D;
    const uint16_t* Kh = QKV + (size_t)(Hq + hk) * D;
    const uint16_t* Vh = QKV + (size_t)(Hq + Hkv + hk) * D;
    if constexpr (BIAS) {
        const uint16_t* br = bias + (size_t)h * (2 * Lmax - 1) + (Lmax - L);
        for (int i = tid; i < 2 * L - 1; i += 256) bl[i] = bf2f(br[i]);
    }
    const int wq0 = q0 + (tid >> 6) * 16;
    const int qi = wq0 + li;
    const bool qok = qi < L;
    const int qc = qok ? qi : L - 1;
    const int wq_hi = wq0 + 15 < L - 1 ? wq0 + 15 : L - 1;     // the last query this wave serves (clamped like qc)
    T tile;
    tile.init(Qh + (size_t)qc * ld, g);
    constexpr float L2E = 1.4426950408889634f;
    const int kend = CAUSAL ? (L < q0 + T::BQ ? L : q0 + T::BQ) : L;
    const int ntiles = (kend + T::BK - 1) / T::BK;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * T::BK;
        __syncthreads();                               // the previous tile is consumed (and, at t = 0, the bias window is visible)
        T::stage(kl, vl, Kh, Vh, ld, tid, [&](int kk) { return k0 + kk < L ? k0 + kk : -1; });
        __syncthreads();
        if (CAUSAL && k0 > wq_hi) continue;            // wave-uniform: the tile is above every query of this wave
        tile.step(kl, vl, li, g, L2E, [&](const float (&s)[8], float (&sc)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = k0 + T::key_of_slot(g, e);
                const bool ok = j < L && (!CAUSAL || j <= qc);
                float v = s[e] * scale;
                if constexpr (BIAS) v = ok ? v + bl[j - qc + L - 1] : v;
                sc[e] = ok ? v : -INFINITY;
            }
        });
    }
    const float l = tile.row_sum();
    if (!qok) return;
    const float inv = 1.0f / l;
    uint16_t* orow = O + (size_t)qi * ldo + (size_t)h * D + 4 * g;
#pragma unroll
    for (int ct = 0; ct < T::CT; ++ct)
        *(uint2*)(orow + ct * 16) = make_uint2(f2bf_pk(tile.o[ct][0] * inv, tile.o[ct][1] * inv), f2bf_pk(tile.o[ct][2] * inv, tile.o[ct][3] * inv));
}

// ---- embedding gather (+ position row): one block per token, one 8-element vector per thread and pass ------------------------------
__global__ __launch_bounds__(256) void text_embed_kernel(const int64_t* __restrict__ ids, const uint16_t* __restrict__ tok, long long vocab,
                                                         const uint16_t* __restrict__ pos, uint16_t* __restrict__ out, int d) {
    const int row = blockIdx.x;
    const long long id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    uint16_t* orow = out + (size_t)row * d;
    for (int c = threadIdx.x * 8; c < d; c += 256 * 8) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (ok) {
            w = *(const uint4*)(tok + (size_t)id * d + c);
            if (pos) {
                const uint4 p = *(const uint4*)(pos + (size_t)row * d + c);
                const uint32_t a[4] = {w.x, w.y, w.z, w.w}, b[4] = {p.x, p.y, p.z, p.w};
                uint32_t r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    r[e] = f2bf_pk(bf2f(a[e] & 0xffffu) + bf2f(b[e] & 0xffffu), bf2f(a[e] >> 16) + bf2f(b[e] >> 16));
                w = make_uint4(r[0], r[1], r[2], r[3]);
            }
        }
        *(uint4*)(orow + c) = w;
    }
}

// ---- y[m, f] = bf16(x[m, F + f] * x[m, f]): the gelu half times the linear half (a product of two bf16 is exact in fp32) ---------
__global__ __launch_bounds__(256) void geglu_kernel(const uint16_t* __restrict__ x, int ldx, uint16_t* __restrict__ y, int ldy, int M, int F) {
    const int vpr = F / 8;
    const size_t nv = (size_t)M * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / vpr), c = (int)(i - (size_t)m * vpr) * 8;
        const uint4 lin = *(const uint4*)(x + (size_t)m * ldx + c), gl = *(const uint4*)(x + (size_t)m * ldx + F + c);
        const uint32_t a[4] = {lin.x, lin.y, lin.z, lin.w}, b[4] = {gl.x, gl.y, gl.z, gl.w};
        uint32_t r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = f2bf_pk(bf2f(b[e] & 0xffffu) * bf2f(a[e] & 0xffffu), bf2f(b[e] >> 16) * bf2f(a[e] >> 16));
        *(uint4*)(y + (size_t)m * ldy + c) = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

// ---- quick_gelu: x * sigmoid(1.702 x) as three bf16 ops (`1.702 * x`, `sigmoid`, `x * s`), each rounded like torch's ----------------
__global__ __launch_bounds__(256) void quick_gelu_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = bf2f(x[i]);
        const float t = rbf(v * 1.702f);
        const float s = rbf(1.0f / (1.0f + expf(-t)));
        y[i] = f2bf(v * s);
    }
}

// ---- affine LayerNorm over a row: fp32 mean, then fp32 variance about it (two passes, fixed order), one bf16 rounding ---------------
__device__ __forceinline__ float block_sum4(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // red[] of a previous reduction is consumed
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void layer_norm_rows_kernel(const uint16_t* __restrict__ x, int ldx, const uint16_t* __restrict__ gamma,
                                                              const uint16_t* __restrict__ beta, uint16_t* __restrict__ out, int ldo, int d,
                                                              float eps) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const uint16_t* xr = x + (size_t)row * ldx;
    float s = 0.f;
    for (int i = tid; i < d; i += 256) s += bf2f(xr[i]);
    const float mean = block_sum4(s, red) / (float)d;
    float q = 0.f;
    for (int i = tid; i < d; i += 256) { const float c = bf2f(xr[i]) - mean; q += c * c; }
    const float rstd = 1.0f / sqrtf(block_sum4(q, red) / (float)d + eps);
    for (int i = tid; i < d; i += 256)
        out[(size_t)row * ldo + i] = f2bf(bf2f(gamma[i]) * (rstd * (bf2f(xr[i]) - mean)) + bf2f(beta[i]));
}

// ---- CLIP pooled row: index = argmax(int(ids)) (eos_token_id == 2) or argmax(int(ids) == eos) (first hit; 0 if none), then the copy --
__global__ __launch_bounds__(256) void text_pool_row_kernel(const int64_t* __restrict__ ids, int L, int eos, const uint16_t* __restrict__ x,
                                                            int ldx, int d, uint16_t* __restrict__ out) {
    __shared__ int bv[256], bi[256];
    const int tid = threadIdx.x;
    int best = 0, at = L;                              // at == L: no element yet (loses every comparison below)
    for (int j = tid; j < L; j += 256) {               // increasing j: a strict > keeps the first maximum of this thread's subset
        const int v = eos == 2 ? (int)ids[j] : ((int)ids[j] == eos ? 1 : 0);
        if (at == L || v > best) { best = v; at = j; }
    }
    bv[tid] = best;
    bi[tid] = at;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const int v2 = bv[tid + s], i2 = bi[tid + s];
            const bool take = i2 < L && (bi[tid] == L || v2 > bv[tid] || (v2 == bv[tid] && i2 < bi[tid]));
            if (take) { bv[tid] = v2; bi[tid] = i2; }
        }
        __syncthreads();
    }
    const int idx = bi[0];
    for (int c = tid; c < d; c += 256) out[c] = x[(size_t)idx * ldx + c];
}

// ---- multimodal RoPE, in place: one thread owns channels [c, c + 8) and [64 + c, 64 + c + 8) of one (row, head), the two halves that
// rotate_half exchanges.  out = bf16(bf16(x cos) + bf16(rotate_half(x) sin)); the negation of rotate_half is exact in bf16 -------------
__global__ __launch_bounds__(256) void mrope_kernel(uint16_t* __restrict__ QKV, int ld, const uint16_t* __restrict__ cosT,
                                                    const uint16_t* __restrict__ sinT, int L, int heads) {
    const size_t n = (size_t)L * heads * 8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i & 7) * 8;
        const size_t rh = i >> 3;
        const int row = (int)(rh / heads), hd = (int)(rh - (size_t)row * heads);
        uint16_t* x = QKV + (size_t)row * ld + (size_t)hd * 128 + c;
        const uint16_t* cr = cosT + (size_t)row * 128 + c;
        const uint16_t* sr = sinT + (size_t)row * 128 + c;
        const uint4 xa = *(const uint4*)x, xb = *(const uint4*)(x + 64);
        const uint4 ca = *(const uint4*)cr, cb = *(const uint4*)(cr + 64), sa = *(const uint4*)sr, sb = *(const uint4*)(sr + 64);
        const uint32_t x1[4] = {xa.x, xa.y, xa.z, xa.w}, x2[4] = {xb.x, xb.y, xb.z, xb.w};
        const uint32_t c1[4] = {ca.x, ca.y, ca.z, ca.w}, c2[4] = {cb.x, cb.y, cb.z, cb.w};
        const uint32_t s1[4] = {sa.x, sa.y, sa.z, sa.w}, s2[4] = {sb.x, sb.y, sb.z, sb.w};
        uint32_t r1[4], r2[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float lo[2], hi[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int sh = 16 * p;
                const float a = bf2f((uint16_t)(x1[e] >> sh)), b = bf2f((uint16_t)(x2[e] >> sh));
                lo[p] = rbf(a * bf2f((uint16_t)(c1[e] >> sh))) + rbf(-b * bf2f((uint16_t)(s1[e] >> sh)));
                hi[p] = rbf(b * bf2f((uint16_t)(c2[e] >> sh))) + rbf(a * bf2f((uint16_t)(s2[e] >> sh)));
            }
            r1[e] = f2bf_pk(lo[0], lo[1]);
            r2[e] = f2bf_pk(hi[0], hi[1]);
        }
        *(uint4*)x = make_uint4(r1[0], r1[1], r1[2], r1[3]);
        *(uint4*)(x + 64) = make_uint4(r2[0], r2[1], r2[2], r2[3]);
    }
}

// ---- y[m, f] = bf16(bf16(silu(x[m, f])) * x[m, F + f]): `act_fn(gate_proj(x)) * up_proj(x)` with torch's two roundings -------------
__global__ __launch_bounds__(256) void swiglu_kernel(const uint16_t* __restrict__ x, int ldx, uint16_t* __restrict__ y, int ldy, int M, int F) {
    const int vpr = F / 8;
    const size_t nv = (size_t)M * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / vpr), c = (int)(i - (size_t)m * vpr) * 8;
        const uint4 gt = *(const uint4*)(x + (size_t)m * ldx + c), up = *(const uint4*)(x + (size_t)m * ldx + F + c);
        const uint32_t a[4] = {gt.x, gt.y, gt.z, gt.w}, b[4] = {up.x, up.y, up.z, up.w};
        uint32_t r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g0 = bf2f(a[e] & 0xffffu), g1 = bf2f(a[e] >> 16);
            const float s0 = rbf(g0 / (1.0f + expf(-g0))), s1 = rbf(g1 / (1.0f + expf(-g1)));
            r[e] = f2bf_pk(s0 * bf2f(b[e] & 0xffffu), s1 * bf2f(b[e] >> 16));
        }
        *(uint4*)(y + (size_t)m * ldy + c) = make_uint4(r[0], r[1], r[2], r[3]);
    }
}

}  // namespace rgn

using namespace rgn;

extern "C" {

static inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

static inline int grid_of(size_t items, size_t cap) {
    const size_t g = (items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

int rgn_text_attention_bf16(const void* QKV, void* O, int L, int H, float scale, int causal, const void* bias, int Lmax, void* stream) {
    if (!QKV || !O || L < 1 || H < 1 || H > 1024 || !(scale > 0.f) || !(scale < INFINITY))
        return fail(RGN_E_BADARG, "text_attention: bad argument (QKV, O non-null; L >= 1; 1 <= H <= 1024; 0 < scale < inf)");
    if (L > TA_MAX_L) return fail(RGN_E_UNSUPPORTED, "text_attention: L > 4096");
    if (bias && (Lmax < L || Lmax > TA_MAX_L)) return fail(RGN_E_BADARG, "text_attention: the bias table needs L <= Lmax <= 4096");
    if (!al16(QKV) || !al16(O)) return fail(RGN_E_UNSUPPORTED, "text_attention: QKV and O must be 16-byte aligned");
    const dim3 grid((L + ATTN_BQ - 1) / ATTN_BQ, H);
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = bias ? (size_t)(2 * L - 1) * sizeof(float) : 0;
    const uint16_t* q = (const uint16_t*)QKV;
    const uint16_t* b = (const uint16_t*)bias;
    uint16_t* o = (uint16_t*)O;
    if (bias && causal) hipLaunchKernelGGL((text_attention_kernel<64, true, true>), grid, dim3(256), lds, st, q, o, L, H, H, scale, b, Lmax);
    else if (bias) hipLaunchKernelGGL((text_attention_kernel<64, true, false>), grid, dim3(256), lds, st, q, o, L, H, H, scale, b, Lmax);
    else if (causal) hipLaunchKernelGGL((text_attention_kernel<64, false, true>), grid, dim3(256), 0, st, q, o, L, H, H, scale, b, Lmax);
    else hipLaunchKernelGGL((text_attention_kernel<64, false, false>), grid, dim3(256), 0, st, q, o, L, H, H, scale, b, Lmax);
    return check_launch("text_attention_kernel");
}

int rgn_text_embed(const int64_t* ids, int L, const void* tok, int vocab, const void* pos, int npos, void* out, int d, void* stream) {
    if (!ids || !tok || !out || L < 1 || vocab < 1 || d < 8 || d % 8)
        return fail(RGN_E_BADARG, "text_embed: bad argument (ids, tok, out non-null; L >= 1; vocab >= 1; d a positive multiple of 8)");
    if (pos && L > npos) return fail(RGN_E_BADARG, "text_embed: L exceeds the position table");
    if (!al16(tok) || !al16(out) || (pos && !al16(pos))) return fail(RGN_E_UNSUPPORTED, "text_embed: tok, pos and out must be 16-byte aligned");
    hipLaunchKernelGGL(text_embed_kernel, dim3(L), dim3(256), 0, (hipStream_t)stream, ids, (const uint16_t*)tok, (long long)vocab,
                       (const uint16_t*)pos, (uint16_t*)out, d);
    return check_launch("text_embed_kernel");
}

int rgn_geglu_bf16(const void* x, int ldx, void* y, int ldy, int M, int F, void* stream) {
    if (M == 0) return 0;
    if (!x || !y || M < 0 || F < 8 || F % 8 || ldx < 2 * F || ldx % 8 || ldy < F || ldy % 8)
        return fail(RGN_E_BADARG, "geglu: bad argument (F a positive multiple of 8, ldx >= 2 F, ldy >= F, strides multiples of 8)");
    if (!al16(x) || !al16(y)) return fail(RGN_E_UNSUPPORTED, "geglu: x and y must be 16-byte aligned");
    hipLaunchKernelGGL(geglu_kernel, dim3(grid_of((size_t)M * (F / 8), 2048)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx,
                       (uint16_t*)y, ldy, M, F);
    return check_launch("geglu_kernel");
}

int rgn_quick_gelu_bf16(const void* x, void* y, size_t n, void* stream) {
    if (n == 0) return 0;
    if (!x || !y) return fail(RGN_E_BADARG, "quick_gelu: null pointer");
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid_of(n, 2048)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (uint16_t*)y, n);
    return check_launch("quick_gelu_kernel");
}

int rgn_layer_norm_rows(const void* x, int ldx, const void* gamma, const void* beta, void* out, int ldo, int M, int d, float eps,
                        void* stream) {
    if (M == 0) return 0;
    if (!x || !gamma || !beta || !out || M < 0 || d <= 0 || ldx < d || ldo < d || !(eps >= 0.f))
        return fail(RGN_E_BADARG, "layer_norm_rows: bad argument");
    hipLaunchKernelGGL(layer_norm_rows_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, (const uint16_t*)gamma,
                       (const uint16_t*)beta, (uint16_t*)out, ldo, d, eps);
    return check_launch("layer_norm_rows_kernel");
}

int rgn_text_pool_row(const int64_t* ids, int L, int eos_token_id, const void* x, int ldx, int d, void* out, void* stream) {
    if (!ids || !x || !out || L < 1 || d < 1 || ldx < d) return fail(RGN_E_BADARG, "text_pool_row: bad argument");
    hipLaunchKernelGGL(text_pool_row_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ids, L, eos_token_id, (const uint16_t*)x, ldx, d,
                       (uint16_t*)out);
    return check_launch("text_pool_row_kernel");
}

int rgn_lm_attention_bf16(const void* QKV, void* O, int L, int Hq, int Hkv, float scale, void* stream) {
    if (!QKV || !O || L < 1 || Hkv < 1 || Hq < Hkv || Hq > 1024 || Hq % Hkv || !(scale > 0.f) || !(scale < INFINITY))
        return fail(RGN_E_BADARG, "lm_attention: bad argument (QKV, O non-null; L >= 1; 1 <= Hkv <= Hq <= 1024, Hq % Hkv == 0; 0 < scale < inf)");
    if (L > LA_MAX_L) return fail(RGN_E_BADARG, "lm_attention: L > 4096");
    if (!al16(QKV) || !al16(O)) return fail(RGN_E_BADARG, "lm_attention: QKV and O must be 16-byte aligned");
    hipLaunchKernelGGL((text_attention_kernel<128, false, true>), dim3((L + ATTN_BQ - 1) / ATTN_BQ, Hq), dim3(256), 0,
                       (hipStream_t)stream, (const uint16_t*)QKV, (uint16_t*)O, L, Hq, Hkv, scale, (const uint16_t*)nullptr, 0);
    return check_launch("lm_attention_kernel");
}

int rgn_mrope_bf16(void* QKV, int ld, const void* cos, const void* sin, int L, int Hq, int Hkv, void* stream) {
    if (!QKV || !cos || !sin || L < 1 || Hq < 1 || Hkv < 1 || Hq > 1024 || Hkv > 1024 || ld < (Hq + 2 * Hkv) * 128 || ld % 8)
        return fail(RGN_E_BADARG, "mrope: bad argument (QKV, cos, sin non-null; L >= 1; 1 <= Hq, Hkv <= 1024; ld >= (Hq + 2 Hkv) 128, a multiple of 8)");
    if (!al16(QKV) || !al16(cos) || !al16(sin)) return fail(RGN_E_BADARG, "mrope: QKV, cos and sin must be 16-byte aligned");
    hipLaunchKernelGGL(mrope_kernel, dim3(grid_of((size_t)L * (Hq + Hkv) * 8, 2048)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)QKV, ld,
                       (const uint16_t*)cos, (const uint16_t*)sin, L, Hq + Hkv);
    return check_launch("mrope_kernel");
}

int rgn_swiglu_bf16(const void* x, int ldx, void* y, int ldy, int M, int F, void* stream) {
    if (M == 0) return 0;
    if (!x || !y || M < 0 || F < 8 || F % 8 || ldx < 2 * F || ldx % 8 || ldy < F || ldy % 8)
        return fail(RGN_E_BADARG, "swiglu: bad argument (F a positive multiple of 8, ldx >= 2 F, ldy >= F, strides multiples of 8)");
    if (!al16(x) || !al16(y)) return fail(RGN_E_BADARG, "swiglu: x and y must be 16-byte aligned");
    hipLaunchKernelGGL(swiglu_kernel, dim3(grid_of((size_t)M * (F / 8), 2048)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx,
                       (uint16_t*)y, ldy, M, F);
    return check_launch("swiglu_kernel");
}

}  // extern "C"
