// Row kernels of the VAE decoder (reference call site FluxKontext/inplace.py:396-402 `self.vae.decode(latents)`,
// [EXT] AutoencoderKL of the public FLUX.1 / Step1X-Edit checkpoints) - HBM-streaming passes around the implicit-GEMM convolutions
// (rgn_conv_bf16, gemm.hip).
//
// Activation layout: a ZERO-BORDERED, pixel-major image [Hp * Wp, C] bf16 with Hp = H + 2, Wp = W + 2 (row = y * Wp + x of the padded
// image, channels contiguous): a 3 x 3 tap is then a constant row shift, a convolution a GEMM whose A tile moves by a byte offset per
// K step, and the zero border IS the convolution's zero padding.  Every kernel here writes zeros to the border rows it produces.
//   gn_stats_kernel + gn_finalize_kernel   GroupNorm(32 groups) statistics: per-block fp32 partial sums, one double-precision
//                                           finalize block -> (mean, rstd) per group; no atomics: bit-reproducible
//   gn_apply_kernel                         y = (x - mean) * rstd * gamma + beta, optional SiLU, border rows -> 0
//   upsample2x_kernel                       nearest-neighbour 2 x upsample into the next level's padded image
//   softmax_rows_kernel                     mid-block attention: P = softmax(scale * S) per row over the valid (non-border) key columns
//   vae_attention_kernel                    mid-block attention fused (flash-style, no S in memory, the tile core of attn_tile.h):
//                                           O = softmax(scale Q K^T) V + b_v
//   rms_norm_kernel                         channel RMS-norm (+ SiLU) per pixel: the Qwen-Image (Wan-2.1) VAE's RMS_norm
//   nchw_to_padded_kernel / padded_to_nchw_kernel   the host tensor layouts on either side of the decoder
#include "attn_tile.h"

namespace rgn {

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) { return f2bf_pk(a, b); }     // v_cvt_pk_bf16_f32 (RNE)
__device__ __forceinline__ float lo_bf(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_bf(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// ---- GroupNorm statistics -------------------------------------------------------------------------------------------------------
// One thread = one 8-channel vector of a row; 256 / (C / 8) rows per block pass, grid-stride over the rows.  A vector's two 4-channel
// halves are accumulated apart (C = 128: 4 channels per group); a block folds its threads to 32 groups x (sum, sum of squares) in LDS.
__global__ __launch_bounds__(256) void gn_stats_kernel(const uint16_t* __restrict__ X, int rows, int C, float* __restrict__ partial) {
    const int vpr = C >> 3, rpb = 256 / vpr;
    const int tid = threadIdx.x, v = tid % vpr, rl = tid / vpr;
    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
    for (int r = blockIdx.x * rpb + rl; r < rows; r += gridDim.x * rpb) {
        const uint4 w = *(const uint4*)(X + (size_t)r * C + v * 8);
        const float a0 = lo_bf(w.x), a1 = hi_bf(w.x), a2 = lo_bf(w.y), a3 = hi_bf(w.y);
        const float b0 = lo_bf(w.z), b1 = hi_bf(w.z), b2 = lo_bf(w.w), b3 = hi_bf(w.w);
        s0 += (a0 + a1) + (a2 + a3);
        q0 += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        s1 += (b0 + b1) + (b2 + b3);
        q1 += (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
    }
    // block fold in a FIXED order (no atomics: the statistics are bit-reproducible): thread t < 64 owns (group t >> 1, quantity t & 1)
    // and walks the 256 threads' values of that quantity, taking the halves that belong to its group
    __shared__ float sh[4][256];
    sh[0][tid] = s0; sh[1][tid] = q0; sh[2][tid] = s1; sh[3][tid] = q1;
    __syncthreads();
    if (tid < 64) {
        const int cpg = C >> 5, g = tid >> 1, qn = tid & 1;         // channels per group (4, 8, 16)
        float acc = 0.f;
        for (int i = 0; i < 256; ++i) {
            const int vi = i % vpr;
            if ((vi * 8) / cpg == g) acc += sh[qn][i];
            if ((vi * 8 + 4) / cpg == g) acc += sh[2 + qn][i];
        }
        partial[(size_t)blockIdx.x * 64 + tid] = acc;
    }
}

__global__ __launch_bounds__(1024) void gn_finalize_kernel(const float* __restrict__ partial, int nblocks, double count, float eps,
                                                           float* __restrict__ stats) {
    // thread: quantity t = tid & 63 (group t >> 1, sum / sum of squares t & 1), slice tid >> 6 of the blocks; 16 slices folded in a
    // fixed order in double precision (a single 64-thread block walking 1024 partials took 200 us: 30 such launches per decode)
    const int t = threadIdx.x & 63, part = threadIdx.x >> 6;
    double acc = 0.0;
    for (int b = part; b < nblocks; b += 16) acc += (double)partial[(size_t)b * 64 + t];
    __shared__ double sh[16][64];
    sh[part][t] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) tot += sh[i][t];
        const double other = __shfl_xor(tot, 1, 64);
        if ((t & 1) == 0) {
            const double mean = tot / count, var = other / count - mean * mean;
            stats[t] = (float)mean;
            stats[t + 1] = (float)(1.0 / sqrt((var > 0.0 ? var : 0.0) + (double)eps));
        }
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y, int Hp, int Wp, int C,
                                                       const float* __restrict__ stats, const uint16_t* __restrict__ gamma,
                                                       const uint16_t* __restrict__ beta, int silu) {
    const int vpr = C >> 3, rpb = 256 / vpr, rows = Hp * Wp;
    const int tid = threadIdx.x, v = tid % vpr, rl = tid / vpr;
    const int cpg = C >> 5;
    const int g0 = (v * 8) / cpg, g1 = (v * 8 + 4) / cpg;
    const float m0 = stats[g0 * 2], r0 = stats[g0 * 2 + 1], m1 = stats[g1 * 2], r1 = stats[g1 * 2 + 1];
    const uint4 gw = *(const uint4*)(gamma + v * 8), bw = *(const uint4*)(beta + v * 8);
    const uint32_t gws[4] = {gw.x, gw.y, gw.z, gw.w}, bws[4] = {bw.x, bw.y, bw.z, bw.w};
    float sc[8], sf[8];                              // y = x * sc + sf
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float ga = (e & 1) ? hi_bf(gws[e >> 1]) : lo_bf(gws[e >> 1]);
        const float be = (e & 1) ? hi_bf(bws[e >> 1]) : lo_bf(bws[e >> 1]);
        const float mean = e < 4 ? m0 : m1, rstd = e < 4 ? r0 : r1;
        sc[e] = rstd * ga;
        sf[e] = be - mean * rstd * ga;
    }
    for (int r = blockIdx.x * rpb + rl; r < rows; r += gridDim.x * rpb) {
        const int py = r / Wp, px = r - py * Wp;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (px != 0 && px != Wp - 1 && py != 0 && py != Hp - 1) {
            const uint4 w = *(const uint4*)(X + (size_t)r * C + v * 8);
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
            float y[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = (e & 1) ? hi_bf(ws[e >> 1]) : lo_bf(ws[e >> 1]);
                float t = __builtin_fmaf(x, sc[e], sf[e]);
                if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * t));
                y[e] = t;
            }
            o = make_uint4(pk_bf16(y[0], y[1]), pk_bf16(y[2], y[3]), pk_bf16(y[4], y[5]), pk_bf16(y[6], y[7]));
        }
        *(uint4*)(Y + (size_t)r * C + v * 8) = o;
    }
}

// ---- nearest-neighbour 2 x upsample: output-driven, one thread = one 16-byte vector ---------------------------------------------------
__global__ __launch_bounds__(256) void upsample2x_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y, int Hp, int Wp, int C) {
    const int Ho = 2 * (Hp - 2) + 2, Wo = 2 * (Wp - 2) + 2, vpr = C >> 3;
    const uint32_t total = (uint32_t)Ho * Wo * vpr;                   // < 2^31 (checked by the launcher)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int r = (int)(i / (uint32_t)vpr), v = (int)(i - (uint32_t)r * vpr), oy = r / Wo, ox = r - oy * Wo;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (ox != 0 && ox != Wo - 1 && oy != 0 && oy != Ho - 1)
            o = *(const uint4*)(X + ((size_t)(((oy - 1) >> 1) + 1) * Wp + ((ox - 1) >> 1) + 1) * C + v * 8);
        *(uint4*)(Y + (size_t)r * C + v * 8) = o;
    }
}

// ---- row softmax of the mid-block attention (one head of width C over every pixel: 3 GEMMs + this pass) -----------------------------
// S [rows, ld] bf16 holds q . k for every (query pixel, key pixel) of the PADDED image; key columns on the border (and the K padding
// columns [rows, ld)) get probability 0.  In place: P = softmax(scale * S) as bf16.  One block per query row.
__global__ __launch_bounds__(256) void softmax_rows_kernel(uint16_t* __restrict__ S, int ld, int Hp, int Wp, float scale_log2e) {
    const int rows = Hp * Wp, tid = threadIdx.x;
    uint16_t* row = S + (size_t)blockIdx.x * ld;
    constexpr int MAXV = 12;                          // 256 threads x 12 vectors x 8 = 24576 columns
    uint4 w[MAXV];
    uint32_t okm[MAXV];                               // bit e: column vi * 8 + e is a valid (non-border, non-padding) key
    float mx = -INFINITY;
    const int nvec = ld >> 3;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int vi = tid + j * 256;
        if (vi >= nvec) break;
        w[j] = *(const uint4*)(row + vi * 8);
        const uint32_t ws[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
        int cy = (vi * 8) / Wp, cx = vi * 8 - cy * Wp;            // one division per vector, then stepped
        uint32_t m = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool ok = vi * 8 + e < rows && cx != 0 && cx != Wp - 1 && cy != 0 && cy != Hp - 1;
            const float x = (e & 1) ? hi_bf(ws[e >> 1]) : lo_bf(ws[e >> 1]);
            if (ok) { mx = fmaxf(mx, x); m |= 1u << e; }
            if (++cx == Wp) { cx = 0; ++cy; }
        }
        okm[j] = m;
    }
    __shared__ float red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    float p[MAXV][8];
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int vi = tid + j * 256;
        if (vi >= nvec) break;
        const uint32_t ws[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = (e & 1) ? hi_bf(ws[e >> 1]) : lo_bf(ws[e >> 1]);
            p[j][e] = ((okm[j] >> e) & 1u) ? __builtin_amdgcn_exp2f((x - mx) * scale_log2e) : 0.f;
            sum += p[j][e];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
        const int vi = tid + j * 256;
        if (vi >= nvec) break;
        *(uint4*)(row + vi * 8) = make_uint4(pk_bf16(p[j][0] * inv, p[j][1] * inv), pk_bf16(p[j][2] * inv, p[j][3] * inv),
                                             pk_bf16(p[j][4] * inv, p[j][5] * inv), pk_bf16(p[j][6] * inv, p[j][7] * inv));
    }
}

// ---- fused mid-block attention: one head of width C over the valid pixels, no score matrix in memory ---------------------------------
// Queries and keys are enumerated over the H x W VALID pixels (i -> padded row (i / W + 1) * Wp + i % W + 1): border pixels are never keys,
// and border query rows are not written.  Block = 4 waves x 16 queries on the tile core of attn_tile.h (D = C), whose staging reads each
// key's padded row from a table in LDS, written one tile ahead.  The scores stay raw (scale * log2 e is folded into the exp2 multiplier);
// only the last tile masks (keys past the last pixel).  The epilogue adds b_v.
template <int C> struct VaShape {
    static constexpr size_t lds = (size_t)(AttnTile<C>::K_LDS + AttnTile<C>::V_LDS) * 2 + 2 * ATTN_BK * sizeof(long long);
};

template <int C>
__global__ __launch_bounds__(256, 2) void vae_attention_kernel(const uint16_t* Q, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
                                                                 const uint16_t* __restrict__ bv, uint16_t* O, int H, int W, float sl2e) {
    using T = AttnTile<C>;
    constexpr int BK = T::BK;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t* kl = (uint16_t*)smem;
    uint16_t* vl = kl + T::K_LDS;
    long long* krow = (long long*)(vl + T::V_LDS);     // [2][BK] padded row of each key of a tile (-1: past the last key)
    const int n = H * W, Wp = W + 2, tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int qi = blockIdx.x * T::BQ + (tid >> 6) * 16 + li;
    const bool qok = qi < n;
    const int qc = qok ? qi : n - 1;
    const size_t qrow = (size_t)(qc / W + 1) * Wp + qc % W + 1;
    T tile;
    tile.init(Q + qrow * C, g);
    const int ntiles = (n + BK - 1) / BK;
    if (tid < BK) krow[tid] = tid < n ? (long long)(tid / W + 1) * Wp + tid % W + 1 : -1;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = t * BK;
        const long long* kr = krow + (t & 1) * BK;
        __syncthreads();                               // the previous tile is consumed; this tile's key rows are visible
        T::stage(kl, vl, K, V, (size_t)C, tid, [&](int kk) { return kr[kk]; });
        if (tid < BK) {                                // the next tile's key rows (the other half of the table)
            const int j = k0 + BK + tid;
            krow[((t + 1) & 1) * BK + tid] = j < n ? (long long)(j / W + 1) * Wp + j % W + 1 : -1;
        }
        __syncthreads();
        tile.step(kl, vl, li, g, sl2e, [&](const float (&s)[8], float (&sc)[8]) {     // every tile holds at least one key
#pragma unroll
            for (int e = 0; e < 8; ++e) sc[e] = s[e];
            if (k0 + BK > n) {                         // last tile only
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (k0 + T::key_of_slot(g, e) >= n) sc[e] = -INFINITY;
            }
        });
    }
    const float l = tile.row_sum();
    if (!qok) return;
    const float inv = 1.0f / l;
    uint16_t* orow = O + qrow * C + 4 * g;
#pragma unroll
    for (int ct = 0; ct < T::CT; ++ct) {
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (bv) {
            const uint2 bw = *(const uint2*)(bv + ct * 16 + 4 * g);
            b[0] = lo_bf(bw.x); b[1] = hi_bf(bw.x); b[2] = lo_bf(bw.y); b[3] = hi_bf(bw.y);
        }
        *(uint2*)(orow + ct * 16) = make_uint2(f2bf_pk(__builtin_fmaf(tile.o[ct][0], inv, b[0]), __builtin_fmaf(tile.o[ct][1], inv, b[1])),
                                               f2bf_pk(__builtin_fmaf(tile.o[ct][2], inv, b[2]), __builtin_fmaf(tile.o[ct][3], inv, b[3])));
    }
}

// ---- channel RMS-norm of the Qwen-Image VAE: y = x / max(||x||_2, 1e-12) * sqrt(C_valid) * gamma (+ SiLU) per pixel ---------------------
// One pixel row = `lanes` threads of a wave (the power of two >= C_pad / 8; 16 / 32 / 64 for 128 / 192 / 384 channels), one 8-channel
// vector per thread; the sum of squares is folded by xor shuffles inside those lanes (fixed order, no atomics: bit-reproducible).  Channels
// >= C_valid and border rows are written as zeros.
__global__ __launch_bounds__(256) void rms_norm_kernel(const uint16_t* __restrict__ X, uint16_t* __restrict__ Y, int Hp, int Wp, int C_valid,
                                                       int C_pad, const uint16_t* __restrict__ gamma, float scale, int lanes_log2, int silu) {
    const int lanes = 1 << lanes_log2, rpb = 256 >> lanes_log2, rows = Hp * Wp, vpr = C_pad >> 3;
    const int tid = threadIdx.x, v = tid & (lanes - 1), rl = tid >> lanes_log2;
    const bool vec = v < vpr;
    float ga[8];
    {
        uint4 gw = make_uint4(0u, 0u, 0u, 0u);
        if (vec) gw = *(const uint4*)(gamma + v * 8);
        const uint32_t gws[4] = {gw.x, gw.y, gw.z, gw.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) ga[e] = (v * 8 + e < C_valid) ? ((e & 1) ? hi_bf(gws[e >> 1]) : lo_bf(gws[e >> 1])) * scale : 0.f;
    }
    for (int r0 = blockIdx.x * rpb; r0 < rows; r0 += gridDim.x * rpb) {
        const int r = r0 + rl;
        const bool in = r < rows;
        const int py = r / Wp, px = r - py * Wp;
        const bool valid = in && px != 0 && px != Wp - 1 && py != 0 && py != Hp - 1;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (valid && vec) w = *(const uint4*)(X + (size_t)r * C_pad + v * 8);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        float x[8], ss = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = (v * 8 + e < C_valid) ? ((e & 1) ? hi_bf(ws[e >> 1]) : lo_bf(ws[e >> 1])) : 0.f;   // the norm covers X[:C_valid] only
            ss = __builtin_fmaf(x[e], x[e], ss);
        }
        for (int o = lanes >> 1; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);          // every lane of the row group takes part
        const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = x[e] * inv * ga[e];
            if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * t));
            y[e] = valid ? t : 0.f;
        }
        if (in && vec)
            *(uint4*)(Y + (size_t)r * C_pad + v * 8) = make_uint4(pk_bf16(y[0], y[1]), pk_bf16(y[2], y[3]), pk_bf16(y[4], y[5]), pk_bf16(y[6], y[7]));
    }
}

// ---- host layouts ---------------------------------------------------------------------------------------------------------------
// z [Cz, H, W] (bf16, NCHW of one image) -> padded pixel-major [Hp * Wp, Cpad] with channels [Cz, Cpad) and the border zero
__global__ __launch_bounds__(256) void nchw_to_padded_kernel(const uint16_t* __restrict__ Z, uint16_t* __restrict__ Y, int Cz, int H, int W, int Cpad) {
    const int Hp = H + 2, Wp = W + 2;
    const uint32_t total = (uint32_t)Hp * Wp * Cpad;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int r = (int)(i / (uint32_t)Cpad), c = (int)(i - (uint32_t)r * Cpad), py = r / Wp, px = r - py * Wp;
        uint16_t o = 0;
        if (c < Cz && px != 0 && px != Wp - 1 && py != 0 && py != Hp - 1) o = Z[((size_t)c * H + (py - 1)) * W + (px - 1)];
        Y[i] = o;
    }
}

// padded pixel-major [Hp * Wp, ld] (first Co channels) -> [Co, H, W] bf16
__global__ __launch_bounds__(256) void padded_to_nchw_kernel(const uint16_t* __restrict__ X, int ld, uint16_t* __restrict__ O, int Co, int H, int W) {
    const int Wp = W + 2;
    const uint32_t total = (uint32_t)Co * H * W;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int t = (int)(i / (uint32_t)W), x = (int)(i - (uint32_t)t * W), c = t / H, y = t - c * H;
        O[i] = X[((size_t)(y + 1) * Wp + (x + 1)) * ld + c];
    }
}

// the same, clamped to [-1, 1] (the decoder's image) when clamp_unit != 0, stored as bf16 or fp32 (the host VAE's dtype)
template <bool F32>
__global__ __launch_bounds__(256) void padded_to_nchw_cvt_kernel(const uint16_t* __restrict__ X, int ld, void* __restrict__ O, int Co, int H, int W,
                                                                 int clamp_unit) {
    const int Wp = W + 2;
    const uint32_t total = (uint32_t)Co * H * W;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int t = (int)(i / (uint32_t)W), x = (int)(i - (uint32_t)t * W), c = t / H, y = t - c * H;
        float f = __uint_as_float((uint32_t)X[((size_t)(y + 1) * Wp + (x + 1)) * ld + c] << 16);
        if (clamp_unit && f == f) f = fminf(fmaxf(f, -1.0f), 1.0f);                      // NaN passes through, as torch.clamp keeps it
        if (F32) ((float*)O)[i] = f;
        else ((uint16_t*)O)[i] = (uint16_t)(__float_as_uint(f) >> 16);              // a clamped bf16 value is a bf16 value: no rounding
    }
}

template <int C>
int launch_vae_attention(const void* Q, const void* K, const void* V, const void* b_v, void* O, int H, int W, float scale, hipStream_t st) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)vae_attention_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)VaShape<C>::lds);
        attr = true;
    }
    const int blocks = (int)(((long long)H * W + ATTN_BQ - 1) / ATTN_BQ);
    hipLaunchKernelGGL(vae_attention_kernel<C>, dim3(blocks), dim3(256), VaShape<C>::lds, st, (const uint16_t*)Q, (const uint16_t*)K,
                       (const uint16_t*)V, (const uint16_t*)b_v, (uint16_t*)O, H, W, scale * 1.4426950408889634f);
    return check_launch("vae_attention_kernel");
}

}  // namespace rgn

using namespace rgn;

extern "C" {

static inline int grid_for(size_t work_items, int per_block, int cap) {
    const size_t g = (work_items + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

// workspace = [GN_MAX_BLOCKS][64] partial sums (the statistics kernel's blocks, or the tiles of the convolution that produced X) + 64 stats
constexpr int GN_MAX_BLOCKS = 32768;
size_t rgn_groupnorm_partial_bytes(void) { return (size_t)GN_MAX_BLOCKS * 64 * sizeof(float); }
size_t rgn_groupnorm_workspace_bytes(void) { return rgn_groupnorm_partial_bytes() + 64 * sizeof(float); }

int rgn_groupnorm_silu(const void* X, void* Y, int Hp, int Wp, int C, const void* gamma, const void* beta, float eps, int silu,
                       void* workspace, int precomputed_blocks, void* stream) {
    if (!X || !Y || !gamma || !beta || !workspace || Hp < 3 || Wp < 3 || precomputed_blocks < 0 || precomputed_blocks > GN_MAX_BLOCKS)
        return fail(RGN_E_BADARG, "groupnorm: bad argument");
    if (C != 128 && C != 256 && C != 512) return fail(RGN_E_UNSUPPORTED, "groupnorm: 32 groups over 128 / 256 / 512 channels");
    if ((((uintptr_t)X | (uintptr_t)Y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)workspace) & 15) != 0)
        return fail(RGN_E_UNSUPPORTED, "groupnorm: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int rows = Hp * Wp, rpb = 256 / (C / 8);
    float* partial = (float*)workspace;
    float* stats = partial + (size_t)GN_MAX_BLOCKS * 64;
    int nb = precomputed_blocks;
    if (nb == 0) {           // else: the convolution that wrote X left its tiles' sums in `partial` (rgn_conv_bf16 gn_partial)
        nb = grid_for((size_t)rows, rpb * 8, 1024);
        hipLaunchKernelGGL(gn_stats_kernel, dim3(nb), dim3(256), 0, st, (const uint16_t*)X, rows, C, partial);
    }
    const double count = (double)(Hp - 2) * (Wp - 2) * (C / 32);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, nb, count, eps, stats);
    const int nb2 = grid_for((size_t)rows, rpb * 4, 4096);
    hipLaunchKernelGGL(gn_apply_kernel, dim3(nb2), dim3(256), 0, st, (const uint16_t*)X, (uint16_t*)Y, Hp, Wp, C, stats,
                       (const uint16_t*)gamma, (const uint16_t*)beta, silu);
    return check_launch("groupnorm kernels");
}

int rgn_upsample2x(const void* X, void* Y, int Hp, int Wp, int C, void* stream) {
    if (!X || !Y || Hp < 3 || Wp < 3 || C <= 0 || (C % 8)) return fail(RGN_E_BADARG, "upsample2x: bad argument");
    const size_t total = (size_t)(2 * Hp - 2) * (2 * Wp - 2) * (C / 8);
    if (total >= ((size_t)1 << 31)) return fail(RGN_E_UNSUPPORTED, "upsample2x: image too large");
    hipLaunchKernelGGL(upsample2x_kernel, dim3(grid_for(total, 256 * 4, 16384)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X,
                       (uint16_t*)Y, Hp, Wp, C);
    return check_launch("upsample2x_kernel");
}

int rgn_softmax_rows(void* S, int ld, int Hp, int Wp, float scale, void* stream) {
    if (!S || Hp < 3 || Wp < 3 || (ld % 8) || ld < Hp * Wp) return fail(RGN_E_BADARG, "softmax_rows: bad argument");
    if (ld > 256 * 12 * 8) return fail(RGN_E_UNSUPPORTED, "softmax_rows: at most 24576 columns");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(Hp * Wp), dim3(256), 0, (hipStream_t)stream, (uint16_t*)S, ld, Hp, Wp,
                       scale * 1.4426950408889634f);
    return check_launch("softmax_rows_kernel");
}

int rgn_vae_attention_bf16(const void* Q, const void* K, const void* V, const void* b_v, void* O, int Hp, int Wp, int C, float scale, void* stream) {
    if (!Q || !K || !V || !O || Hp < 3 || Wp < 3 || !(scale > 0.f) || !(scale < INFINITY)) return fail(RGN_E_BADARG, "vae_attention: bad argument");
    if (C != 384 && C != 512) return fail(RGN_E_UNSUPPORTED, "vae_attention: C must be 384 or 512");
    if ((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O) & 15) != 0 || ((uintptr_t)b_v & 7) != 0)
        return fail(RGN_E_UNSUPPORTED, "vae_attention: Q, K, V, O must be 16-byte aligned, b_v 8-byte aligned");
    if ((long long)(Hp - 2) * (Wp - 2) >= (1ll << 31) - ATTN_BQ) return fail(RGN_E_UNSUPPORTED, "vae_attention: image too large");
    hipStream_t st = (hipStream_t)stream;
    return C == 512 ? launch_vae_attention<512>(Q, K, V, b_v, O, Hp - 2, Wp - 2, scale, st)
                    : launch_vae_attention<384>(Q, K, V, b_v, O, Hp - 2, Wp - 2, scale, st);
}

int rgn_nchw_to_padded(const void* Z, void* Y, int Cz, int H, int W, int Cpad, void* stream) {
    if (!Z || !Y || Cz <= 0 || H <= 0 || W <= 0 || Cpad < Cz) return fail(RGN_E_BADARG, "nchw_to_padded: bad argument");
    const size_t total = (size_t)(H + 2) * (W + 2) * Cpad;
    hipLaunchKernelGGL(nchw_to_padded_kernel, dim3(grid_for(total, 256 * 4, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)Z,
                       (uint16_t*)Y, Cz, H, W, Cpad);
    return check_launch("nchw_to_padded_kernel");
}

int rgn_padded_to_nchw(const void* X, int ld, void* O, int Co, int H, int W, void* stream) {
    if (!X || !O || Co <= 0 || H <= 0 || W <= 0 || ld < Co) return fail(RGN_E_BADARG, "padded_to_nchw: bad argument");
    const size_t total = (size_t)Co * H * W;
    hipLaunchKernelGGL(padded_to_nchw_kernel, dim3(grid_for(total, 256 * 4, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X,
                       ld, (uint16_t*)O, Co, H, W);
    return check_launch("padded_to_nchw_kernel");
}

int rgn_rms_norm_silu(const void* X, void* Y, int Hp, int Wp, int C_valid, int C_pad, const void* gamma, int silu, void* stream) {
    if (!X || !Y || !gamma || Hp < 3 || Wp < 3 || C_valid <= 0 || C_pad <= 0) return fail(RGN_E_BADARG, "rms_norm: bad argument");
    if (C_valid > C_pad) return fail(RGN_E_BADARG, "rms_norm: C_valid > C_pad");
    if ((C_pad % 64) || C_pad > 512) return fail(RGN_E_UNSUPPORTED, "rms_norm: C_pad must be a multiple of 64, at most 512");
    if ((((uintptr_t)X | (uintptr_t)Y | (uintptr_t)gamma) & 15) != 0) return fail(RGN_E_UNSUPPORTED, "rms_norm: pointers must be 16-byte aligned");
    if ((long long)Hp * Wp >= (1ll << 31)) return fail(RGN_E_UNSUPPORTED, "rms_norm: image too large");
    const int vpr = C_pad / 8;
    int lg = 0;
    while ((1 << lg) < vpr) ++lg;
    const int rows = Hp * Wp, rpb = 256 >> lg;
    hipLaunchKernelGGL(rms_norm_kernel, dim3(grid_for((size_t)rows, rpb * 4, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X,
                       (uint16_t*)Y, Hp, Wp, C_valid, C_pad, (const uint16_t*)gamma, sqrtf((float)C_valid), lg, silu);
    return check_launch("rms_norm_kernel");
}

int rgn_padded_to_nchw_cvt(const void* X, int ld, void* O, int Co, int H, int W, int clamp_unit, int out_fp32, void* stream) {
    if (!X || !O || Co <= 0 || H <= 0 || W <= 0 || ld < Co) return fail(RGN_E_BADARG, "padded_to_nchw_cvt: bad argument");
    const size_t total = (size_t)Co * H * W;
    if (total >= ((size_t)1 << 32)) return fail(RGN_E_UNSUPPORTED, "padded_to_nchw_cvt: image too large");
    const dim3 g(grid_for(total, 256 * 4, 8192));
    if (out_fp32)
        hipLaunchKernelGGL(padded_to_nchw_cvt_kernel<true>, g, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X, ld, O, Co, H, W, clamp_unit);
    else
        hipLaunchKernelGGL(padded_to_nchw_cvt_kernel<false>, g, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)X, ld, O, Co, H, W, clamp_unit);
    return check_launch("padded_to_nchw_cvt_kernel");
}

}  // extern "C"
