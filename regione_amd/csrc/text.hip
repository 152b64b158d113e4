// Text encoders of FLUX.1 Kontext (`encode_prompt`, reference call sites FluxKontext/inplace.py:185-211):
// [EXT] transformers CLIPTextModel (the pooled vector) and T5EncoderModel (the 512 context tokens).  Every projection is rgn_gemm_bf16;
// this file holds what the two encoders add around it:
//   text_attention_kernel     head-dim-64 self-attention read straight from the fused QKV GEMM output [L, 3 H 64] -> O [L, H 64]:
//                             scale, causal mask (CLIP), per-head relative-position bias table (T5)
//   text_embed_kernel         token-embedding gather (+ CLIP's absolute position row); ids out of range give zero rows
//   geglu_kernel              T5 v1.1 gated-GELU product bf16(gelu(wi_0 x) * wi_1 x) from the [wi_1 ; wi_0] GEMM output
//   quick_gelu_kernel         CLIP's x * sigmoid(1.702 x), with the three roundings of the eager bf16 op sequence
//   layer_norm_rows_kernel    affine LayerNorm (gamma, beta) over rows (CLIP's layer_norm1 / layer_norm2 / final_layer_norm)
//   text_pool_row_kernel      CLIP's pooled row (argmax(input_ids) when eos_token_id == 2, else the first eos) on the device
// and what the language model of Qwen-Image-Edit's prompt encoder ([EXT] transformers Qwen2_5_VLForConditionalGeneration) adds:
//   lm_attention_kernel       head-dim-128 causal grouped-query self-attention from the fused QKV GEMM output [L, (Hq + 2 Hkv) 128]
//   mrope_kernel              multimodal RoPE on the q and k columns of that buffer, in place, with the eager op sequence's roundings
//   swiglu_kernel             Qwen2MLP's bf16(bf16(silu(gate)) * up) from the [gate_proj ; up_proj] GEMM output
// Row kernels round where torch's eager bf16 ops round (the file is built with -ffp-contract=off); every reduction has a fixed order.
#include "common.h"

namespace rgn {

// ---- head-dim-64 attention ----------------------------------------------------------------------------------------------------------
// Block = one head x 64 queries (4 waves x 16).  Key tiles of 32 keys are staged in LDS (K key-major with a padded row stride, V transposed
// to [64 channels][keys]) and shared by the four waves.  Per wave and tile (v_mfma_f32_16x16x32_bf16):
//   S^T [32 keys x 16 queries] = K Q^T   2 k-steps x 2 key blocks, Q^T held in registers for the whole key loop
//   t = s * scale (+ bias[j - i + Lmax - 1]); masked keys (j >= L, causal j > i) are -inf; online softmax in fp32 (exp2)
//   O^T [64 x 16 queries] += V^T P^T      P rounded to bf16 in the registers the next MFMA reads; key slot 8 g + e of lane group g is
//                                        key 4 g + e (e < 4), 16 + 4 g + e - 4 (e >= 4): the S^T output layout, so P needs no shuffle
// Key 0 is valid for every query, so the running max is finite after the first tile.  The bias window of the head ([2 L - 1] entries
// around the diagonal) is staged in LDS as fp32 once per block.  A repeated call is bit-identical.
constexpr int TA_BQ = 64, TA_BK = 32, TA_D = 64, TA_KLD = TA_D + 8, TA_VLD = TA_BK + 4, TA_MAX_L = 4096;

template <bool BIAS, bool CAUSAL>
__global__ __launch_bounds__(256) void text_attention_kernel(const uint16_t* __restrict__ QKV, uint16_t* __restrict__ O, int L, int H,
                                                             float scale, const uint16_t* __restrict__ bias, int Lmax) {
    __shared__ __attribute__((aligned(16))) uint16_t kl[TA_BK * TA_KLD];
    __shared__ __attribute__((aligned(16))) uint16_t vl[TA_D * TA_VLD];
    extern __shared__ float bl[];                      // BIAS: bl[j - i + L - 1] = bias[h][j - i + Lmax - 1]
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int q0 = blockIdx.x * TA_BQ;
    const size_t ld = (size_t)3 * H * TA_D, ldo = (size_t)H * TA_D;
    const uint16_t* Qh = QKV + (size_t)h * TA_D;
    const uint16_t* Kh = QKV + (size_t)(H + h) * TA_D;
    const uint16_t* Vh = QKV + (size_t)(2 * H + h) * TA_D;
    if constexpr (BIAS) {
        const uint16_t* br = bias + (size_t)h * (2 * Lmax - 1) + (Lmax - L);
        for (int i = tid; i < 2 * L - 1; i += 256) bl[i] = bf2f(br[i]);
    }
    const int qi = q0 + (tid >> 6) * 16 + li;
    const bool qok = qi < L;
    const int qc = qok ? qi : L - 1;
    bf16x8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const bf16x8*)(Qh + (size_t)qc * ld + ks * 32 + g * 8);
    f32x4 o[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr float L2E = 1.4426950408889634f;
    float m_run = -INFINITY, l_run = 0.f;
    const int kend = CAUSAL ? (L < q0 + TA_BQ ? L : q0 + TA_BQ) : L;
    const int ntiles = (kend + TA_BK - 1) / TA_BK;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * TA_BK;
        __syncthreads();                               // the previous tile is consumed (and, at t = 0, the bias window is visible)
        {
            const int kk = tid >> 3, v = tid & 7, j = k0 + kk;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (j < L) w = *(const uint4*)(Kh + (size_t)j * ld + v * 8);
            *(uint4*)(kl + kk * TA_KLD + v * 8) = w;
        }
        if (tid < (TA_BK / 2) * 8) {
            const int kp = tid >> 3, v = tid & 7, j0 = k0 + 2 * kp;
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;   // keys past the last one: V = 0 (P = 0 there; 0 x garbage could be NaN)
            if (j0 < L) a = *(const uint4*)(Vh + (size_t)j0 * ld + v * 8);
            if (j0 + 1 < L) b = *(const uint4*)(Vh + (size_t)(j0 + 1) * ld + v * 8);
            const uint32_t as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t lo = (e & 1) ? as[e >> 1] >> 16 : as[e >> 1] & 0xffffu;
                const uint32_t hi = (e & 1) ? bs[e >> 1] & 0xffff0000u : bs[e >> 1] << 16;
                *(uint32_t*)(vl + (v * 8 + e) * TA_VLD + 2 * kp) = lo | hi;
            }
        }
        __syncthreads();
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 k0f = *(const bf16x8*)(kl + li * TA_KLD + ks * 32 + g * 8);
            const bf16x8 k1f = *(const bf16x8*)(kl + (16 + li) * TA_KLD + ks * 32 + g * 8);
            s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0f, qf[ks], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1f, qf[ks], s1, 0, 0, 0);
        }
        float sc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = k0 + (e < 4 ? 4 * g + e : 16 + 4 * g + e - 4);
            const float s = e < 4 ? s0[e] : s1[e - 4];
            const bool ok = j < L && (!CAUSAL || j <= qc);
            float v = s * scale;
            if constexpr (BIAS) v = ok ? v + bl[j - qc + L - 1] : v;
            sc[e] = ok ? v : -INFINITY;
        }
        float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);          // finite from the first tile on (key 0)
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * L2E);
        const float nb = -m_new * L2E;
        uint32_t pw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            pw[e] = f2bf_pk(__builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e], L2E, nb)), __builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e + 1], L2E, nb)));
        // the row sum is taken over the bf16 P the MFMA multiplies, so the weights the output is divided by are the ones it used
        const float ps = ((bf2f(pw[0] & 0xffffu) + bf2f(pw[0] >> 16)) + (bf2f(pw[1] & 0xffffu) + bf2f(pw[1] >> 16))) +
                         ((bf2f(pw[2] & 0xffffu) + bf2f(pw[2] >> 16)) + (bf2f(pw[3] & 0xffffu) + bf2f(pw[3] >> 16)));
        l_run = __builtin_fmaf(l_run, alpha, ps);
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) o[ct] *= alpha;
        }
        const bf16x8 pf = __builtin_bit_cast(bf16x8, make_uint4(pw[0], pw[1], pw[2], pw[3]));
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const uint16_t* vr = vl + (ct * 16 + li) * TA_VLD + 4 * g;
            const uint2 va = *(const uint2*)vr, vb = *(const uint2*)(vr + 16);
            const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(va.x, va.y, vb.x, vb.y));
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[ct], 0, 0, 0);
        }
    }
    float l = l_run;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!qok) return;
    const float inv = 1.0f / l;
    uint16_t* orow = O + (size_t)qi * ldo + (size_t)h * TA_D + 4 * g;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
        *(uint2*)(orow + ct * 16) = make_uint2(f2bf_pk(o[ct][0] * inv, o[ct][1] * inv), f2bf_pk(o[ct][2] * inv, o[ct][3] * inv));
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

// ---- head-dim-128 causal grouped-query attention (Qwen2.5-VL language model) --------------------------------------------------------
// text_attention_kernel's scheme at head dim 128: block = one query head x 64 queries (4 waves x 16), key tiles of 32 keys in LDS (K
// key-major, V transposed to [128 channels][keys]); S^T = K Q^T in 4 k-steps x 2 key blocks, O^T [128 x 16] += V^T P^T in 8 channel
// tiles.  Query head h reads the K/V columns of KV head h / (Hq / Hkv); the Hq / Hkv blocks of a group run side by side and share the
// tiles through L2 (attention is ~2 % of the encoder's FLOPs; one staged tile per group would trade occupancy for little).
// Causal: key tiles past the block's last query are never staged, and a wave skips the MFMAs of a staged tile that lies wholly above ITS
// 16 queries - every weight there would be exp2(-inf) = 0 and alpha = 1, so the skip changes no bit.  Key 0 is valid for every query.
constexpr int LA_BQ = 64, LA_BK = 32, LA_D = 128, LA_KLD = LA_D + 8, LA_VLD = LA_BK + 4, LA_MAX_L = 4096;

__global__ __launch_bounds__(256) void lm_attention_kernel(const uint16_t* __restrict__ QKV, uint16_t* __restrict__ O, int L, int Hq, int Hkv,
                                                           float scale) {
    __shared__ __attribute__((aligned(16))) uint16_t kl[LA_BK * LA_KLD];
    __shared__ __attribute__((aligned(16))) uint16_t vl[LA_D * LA_VLD];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int hk = h / (Hq / Hkv);
    const int q0 = blockIdx.x * LA_BQ;
    const size_t ld = (size_t)(Hq + 2 * Hkv) * LA_D, ldo = (size_t)Hq * LA_D;
    const uint16_t* Qh = QKV + (size_t)h * LA_D;
    const uint16_t* Kh = QKV + (size_t)(Hq + hk) * LA_D;
    const uint16_t* Vh = QKV + (size_t)(Hq + Hkv + hk) * LA_D;
    const int wq0 = q0 + (tid >> 6) * 16;
    const int qi = wq0 + li;
    const bool qok = qi < L;
    const int qc = qok ? qi : L - 1;
    const int wq_hi = wq0 + 15 < L - 1 ? wq0 + 15 : L - 1;     // the last query this wave serves (clamped like qc)
    bf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(Qh + (size_t)qc * ld + ks * 32 + g * 8);
    f32x4 o[8];
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr float L2E = 1.4426950408889634f;
    float m_run = -INFINITY, l_run = 0.f;
    const int kend = L < q0 + LA_BQ ? L : q0 + LA_BQ;
    const int ntiles = (kend + LA_BK - 1) / LA_BK;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * LA_BK;
        __syncthreads();                               // the previous tile is consumed
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = tid + r * 256, kk = idx >> 4, v = idx & 15, j = k0 + kk;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (j < L) w = *(const uint4*)(Kh + (size_t)j * ld + v * 8);
            *(uint4*)(kl + kk * LA_KLD + v * 8) = w;
        }
        {
            const int kp = tid >> 4, v = tid & 15, j0 = k0 + 2 * kp;
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;   // keys past the last one: V = 0 (P = 0 there; 0 x garbage could be NaN)
            if (j0 < L) a = *(const uint4*)(Vh + (size_t)j0 * ld + v * 8);
            if (j0 + 1 < L) b = *(const uint4*)(Vh + (size_t)(j0 + 1) * ld + v * 8);
            const uint32_t as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t lo = (e & 1) ? as[e >> 1] >> 16 : as[e >> 1] & 0xffffu;
                const uint32_t hi = (e & 1) ? bs[e >> 1] & 0xffff0000u : bs[e >> 1] << 16;
                *(uint32_t*)(vl + (v * 8 + e) * LA_VLD + 2 * kp) = lo | hi;
            }
        }
        __syncthreads();
        if (k0 > wq_hi) continue;                      // wave-uniform: the tile is above every query of this wave
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 k0f = *(const bf16x8*)(kl + li * LA_KLD + ks * 32 + g * 8);
            const bf16x8 k1f = *(const bf16x8*)(kl + (16 + li) * LA_KLD + ks * 32 + g * 8);
            s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0f, qf[ks], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1f, qf[ks], s1, 0, 0, 0);
        }
        float sc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = k0 + (e < 4 ? 4 * g + e : 16 + 4 * g + e - 4);
            const float s = e < 4 ? s0[e] : s1[e - 4];
            sc[e] = j <= qc ? s * scale : -INFINITY;   // qc < L: the causal mask covers the keys past the last one too
        }
        float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);          // finite from the first tile on (key 0)
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * L2E);
        const float nb = -m_new * L2E;
        uint32_t pw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            pw[e] = f2bf_pk(__builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e], L2E, nb)), __builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e + 1], L2E, nb)));
        // the row sum is taken over the bf16 P the MFMA multiplies, so the weights the output is divided by are the ones it used
        const float ps = ((bf2f(pw[0] & 0xffffu) + bf2f(pw[0] >> 16)) + (bf2f(pw[1] & 0xffffu) + bf2f(pw[1] >> 16))) +
                         ((bf2f(pw[2] & 0xffffu) + bf2f(pw[2] >> 16)) + (bf2f(pw[3] & 0xffffu) + bf2f(pw[3] >> 16)));
        l_run = __builtin_fmaf(l_run, alpha, ps);
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) o[ct] *= alpha;
        }
        const bf16x8 pf = __builtin_bit_cast(bf16x8, make_uint4(pw[0], pw[1], pw[2], pw[3]));
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
            const uint16_t* vr = vl + (ct * 16 + li) * LA_VLD + 4 * g;
            const uint2 va = *(const uint2*)vr, vb = *(const uint2*)(vr + 16);
            const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(va.x, va.y, vb.x, vb.y));
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[ct], 0, 0, 0);
        }
    }
    float l = l_run;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!qok) return;
    const float inv = 1.0f / l;
    uint16_t* orow = O + (size_t)qi * ldo + (size_t)h * LA_D + 4 * g;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct)
        *(uint2*)(orow + ct * 16) = make_uint2(f2bf_pk(o[ct][0] * inv, o[ct][1] * inv), f2bf_pk(o[ct][2] * inv, o[ct][3] * inv));
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
    const dim3 grid((L + TA_BQ - 1) / TA_BQ, H);
    const hipStream_t st = (hipStream_t)stream;
    const size_t lds = bias ? (size_t)(2 * L - 1) * sizeof(float) : 0;
    const uint16_t* q = (const uint16_t*)QKV;
    const uint16_t* b = (const uint16_t*)bias;
    uint16_t* o = (uint16_t*)O;
    if (bias && causal) hipLaunchKernelGGL((text_attention_kernel<true, true>), grid, dim3(256), lds, st, q, o, L, H, scale, b, Lmax);
    else if (bias) hipLaunchKernelGGL((text_attention_kernel<true, false>), grid, dim3(256), lds, st, q, o, L, H, scale, b, Lmax);
    else if (causal) hipLaunchKernelGGL((text_attention_kernel<false, true>), grid, dim3(256), 0, st, q, o, L, H, scale, b, Lmax);
    else hipLaunchKernelGGL((text_attention_kernel<false, false>), grid, dim3(256), 0, st, q, o, L, H, scale, b, Lmax);
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
    hipLaunchKernelGGL(lm_attention_kernel, dim3((L + LA_BQ - 1) / LA_BQ, Hq), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV,
                       (uint16_t*)O, L, Hq, Hkv, scale);
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
