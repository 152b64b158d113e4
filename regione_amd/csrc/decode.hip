// Batch-1 greedy decode of the Qwen2.5-VL language model ([EXT] transformers Qwen2_5_VLForConditionalGeneration.generate, one new token per
// step against a KV cache; regione_amd/qwen_text_encoder.py: HipQwen25VLTextEncoder.generate).  Every weight is streamed once per token and
// nothing is MFMA-bound, so this file holds what the prefill kernels are the wrong shape for:
//   lm_gemv_kernel              y = W x (+ bias) (+ resid) for ONE row x: one wave per row, weights straight from global memory to VGPRs in
//                               non-temporal 16-byte vectors with 8 loads per lane in flight before the first use; no LDS for W
//   lm_gemv_kernel<ARGMAX>      the same dot products over the vocabulary in fp32 with a per-block (value, index) maximum, then
//   lm_gemv_w8_kernel           the same one-row product over OCP e4m3fn weights with one fp32 scale per row: half the bytes per row, the
//                               conversion exact in registers, the scale applied once to the fp32 sum
//   lm_head_finalize_kernel     one block that folds the per-block maxima: the LOWEST index among equal fp32 values wins
//   lm_kv_append_kernel         the k | v columns of packed QKV rows (after mRoPE) into rows of the cache, bit for bit
//   lm_decode_attention_kernel  one query token: a block takes one KV head and one slice of 64 cache rows for all Hq / Hkv query heads of
//                               that KV head (K and V are read once per group) and writes fp32 partials (m, l, o[128]) per query head
//   lm_decode_merge_kernel      folds the partials of a head in slice order and rounds O to bf16 once
// No atomics; every reduction has a fixed order (lanes: the butterfly of wave_sum; k, keys and slices: ascending), so a repeated call is
// bit-identical.
#include <math.h>

#include "common.h"

namespace rgn {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int DEC_MAX_N = 4096, DEC_SLICE = 64, DEC_MAX_GROUP = 8, DEC_PART = 130;      // partial = m, l, o[128]

__device__ __forceinline__ float dot8(const uint4 w, const uint4 x, float acc) {
    const uint32_t a[4] = {w.x, w.y, w.z, w.w}, b[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        acc = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(b[e] << 16), acc);
        acc = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(b[e] & 0xffff0000u), acc);
    }
    return acc;
}

// Block = 4 waves = 4 consecutive rows, lane = k in [8 lane, 8 lane + 8) of every 512-wide step.  The 8 weight loads of a round (and its 8
// loads of x, which stays in L2 / L1: at most 37 KB) are issued before the first fma; a lane past K loads nothing and adds 0.  W is read
// once per token and never again before 15 GB of other weights went by: its loads are non-temporal (measured against plain loads on the
// five shapes of a decode step: 3 to 11 % faster, profiles/r14_lm_gemv_ab.txt).  One row per wave, not several: at N = 152064 four rows
// per wave left a tail of idle CUs that cost more than the parent kernel's single load in flight.
constexpr int GEMV_U = 8;

template <bool ARGMAX>
__global__ __launch_bounds__(256) void lm_gemv_kernel(const uint16_t* __restrict__ W, const uint16_t* __restrict__ x,
                                                      const uint16_t* __restrict__ bias, const uint16_t* resid, uint16_t* y,
                                                      float* __restrict__ logits, float* __restrict__ part_v, int* __restrict__ part_i,
                                                      int N, int K) {
    __shared__ float bv[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    const uint16_t* wr = W + (size_t)(n < N ? n : N - 1) * (size_t)K;           // a row past N re-reads row N - 1 and writes nothing
    float acc = 0.f;
    for (int k0 = lane * 8; k0 < K; k0 += 512 * GEMV_U) {
        u32x4 wv[GEMV_U];
        uint4 xv[GEMV_U];
#pragma unroll
        for (int u = 0; u < GEMV_U; ++u) {
            const int k = k0 + 512 * u;
            const bool ok = k < K;
            xv[u] = ok ? *(const uint4*)(x + k) : make_uint4(0u, 0u, 0u, 0u);
            wv[u] = ok ? __builtin_nontemporal_load((const u32x4*)(wr + k)) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < GEMV_U; ++u) acc = dot8(make_uint4(wv[u].x, wv[u].y, wv[u].z, wv[u].w), xv[u], acc);
    }
    const float s = wave_sum(acc);
    if constexpr (ARGMAX) {
        if (lane == 0) {
            bv[wave] = s;
            if (logits && n < N) logits[n] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int base = blockIdx.x * 4;
            float best = bv[0];                                                  // row `base` exists in every block
            int at = base;
            for (int i = 1; i < 4; ++i)                                          // ascending index, strict >: the first maximum
                if (base + i < N && bv[i] > best) { best = bv[i]; at = base + i; }
            part_v[blockIdx.x] = best;
            part_i[blockIdx.x] = at;
        }
    } else if (lane == 0 && n < N) {
        const float v = s + (bias ? bf2f(bias[n]) : 0.f);
        y[n] = resid ? f2bf(rbf(v) + bf2f(resid[n])) : f2bf(v);                  // torch's `h + linear(a)`: two roundings
    }
}

// ---- the same product over fp8 weights (ops.quantize_w8: OCP e4m3fn, one fp32 scale per output channel) ------------------------------
// v_cvt_pk_f32_fp8 decodes two bytes of a word exactly (gfx950: OCP e4m3fn, not the fnuz form of gfx942); the products and the sum are fp32
// in ascending k per lane, the scale multiplies the reduced sum once.
__device__ __forceinline__ float dot16_w8(const u32x4 w, const uint4 xa, const uint4 xb, float acc) {
    const uint32_t a[4] = {w.x, w.y, w.z, w.w}, b[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[e], true);
        acc = fmaf(lo[0], __uint_as_float(b[2 * e] << 16), acc);
        acc = fmaf(lo[1], __uint_as_float(b[2 * e] & 0xffff0000u), acc);
        acc = fmaf(hi[0], __uint_as_float(b[2 * e + 1] << 16), acc);
        acc = fmaf(hi[1], __uint_as_float(b[2 * e + 1] & 0xffff0000u), acc);
    }
    return acc;
}

// Block = 4 waves, wave = W8_ROWS consecutive rows, lane = k in [16 lane, 16 lane + 16) of every 1024-wide step: a 16-byte load carries 16
// weights and meets two 16-byte loads of x (shared by the rows of the wave).  The W8_ROWS x W8_U weight loads of a round are issued before
// the first fma; a lane past K loads nothing and adds 0, a row past N re-reads row N - 1 and writes nothing.  A row is half the bytes of a
// bf16 row, so one row per wave with 8 loads in flight (the bf16 shape) keeps half of its slots empty at K = 3584 and costs 126 VGPRs:
// two rows per wave with 4 loads each (one round covers K <= 4096; 86 VGPRs) measured 6 % faster over the four layer matrices than one
// row with 4 loads, and 20 % faster than the bf16 shape; four rows per wave lost at every shape (profiles/r17_lm_gemv_w8_ab.txt).
constexpr int W8_ROWS = 2, W8_U = 4, W8_STEP = 64 * 16;

template <int ROWS, int U>
__global__ __launch_bounds__(256) void lm_gemv_w8_kernel(const uint8_t* __restrict__ W, const float* __restrict__ wscale,
                                                         const uint16_t* __restrict__ x, const uint16_t* __restrict__ bias,
                                                         const uint16_t* resid, uint16_t* y, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * ROWS;
    if (n0 >= N) return;                                                         // wave-uniform; the kernel has no barrier
    const uint8_t* wr[ROWS];
    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        wr[r] = W + (size_t)(n0 + r < N ? n0 + r : N - 1) * (size_t)K;
        acc[r] = 0.f;
    }
    for (int k0 = lane * 16; k0 < K; k0 += W8_STEP * U) {
        u32x4 wv[ROWS][U];
        uint4 xa[U], xb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + W8_STEP * u;
            const bool ok = k < K;
            xa[u] = ok ? *(const uint4*)(x + k) : make_uint4(0u, 0u, 0u, 0u);
            xb[u] = ok ? *(const uint4*)(x + k + 8) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int r = 0; r < ROWS; ++r) wv[r][u] = ok ? __builtin_nontemporal_load((const u32x4*)(wr[r] + k)) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] = dot16_w8(wv[r][u], xa[u], xb[u], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const float s = wave_sum(acc[r]);
        const int n = n0 + r;
        if (lane == 0 && n < N) {
            const float v = fmaf(s, wscale[n], bias ? bf2f(bias[n]) : 0.f);      // the scale once, on the reduced sum
            y[n] = resid ? f2bf(rbf(v) + bf2f(resid[n])) : f2bf(v);              // the two roundings of lm_gemv_kernel
        }
    }
}

__global__ __launch_bounds__(1024) void lm_head_finalize_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int nparts,
                                                                int64_t* __restrict__ out) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    const int tid = threadIdx.x;
    float best = -INFINITY;
    int at = 0x7fffffff;                                                         // no element yet
#pragma unroll 4
    for (int j = tid; j < nparts; j += 1024) {                                   // partials are in index order: strict > keeps the first
        const float v = part_v[j];
        const int i = part_i[j];
        if (at == 0x7fffffff || v > best) { best = v; at = i; }
    }
    sv[tid] = best;
    si[tid] = at;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) {
            const float v2 = sv[tid + s];
            const int i2 = si[tid + s];
            const bool take = i2 != 0x7fffffff && (si[tid] == 0x7fffffff || v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid]));
            if (take) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) out[0] = si[0] == 0x7fffffff ? 0 : (int64_t)si[0];
}

// ---- cache[row0 + i, :] = QKV[i, Hq 128 : (Hq + 2 Hkv) 128]: one 16-byte vector per thread and pass --------------------------------
__global__ __launch_bounds__(256) void lm_kv_append_kernel(const uint16_t* __restrict__ QKV, int ld, int col0, uint16_t* __restrict__ cache,
                                                           int row0, int L, int width) {
    const int vpr = width / 8;
    const size_t nv = (size_t)L * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / vpr), c = (int)(i - (size_t)r * vpr) * 8;
        *(uint4*)(cache + (size_t)(row0 + r) * width + c) = *(const uint4*)(QKV + (size_t)r * ld + col0 + c);
    }
}

// ---- one query token against the cache ----------------------------------------------------------------------------------------------
// Block = 4 waves = (slice of 64 cache rows, KV head); every load of the block is issued before its first use, so a block costs about one
// memory latency (the kernel is latency-bound: 3 MB of cache per layer against 466 MB of weights).
//   scores  thread = (key j = tid / 4, quarter c = tid % 4 of the 128 channels): 64 bytes of K in four 16-byte loads, q of the group's G
//           heads broadcast from LDS as fp32, then the four quarters of a key are added by two butterfly steps inside the quad
//   softmax every wave reduces the 64 scores of a head (max, exp, sum) the same way; p goes to LDS
//   P V     thread = (channels 2 lane, 2 lane + 1; keys 16 wave .. 16 wave + 15 in ascending order), the four waves' sums added in wave
//           order through LDS
// Rows >= n are not loaded: their score is -inf, their p and v are 0.
__global__ __launch_bounds__(256) void lm_decode_attention_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ cache, int n,
                                                                  int Hq, int Hkv, float scale, float* __restrict__ part, int nslices) {
    __shared__ __attribute__((aligned(16))) float ql[DEC_MAX_GROUP * 128];
    __shared__ float sl[DEC_MAX_GROUP * DEC_SLICE];                              // scores, then p
    __shared__ __attribute__((aligned(8))) float ol[3 * DEC_MAX_GROUP * 128];    // the P V sums of waves 1..3
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slice = blockIdx.x, hk = blockIdx.y, G = Hq / Hkv;
    const size_t width = (size_t)2 * Hkv * 128;
    const int row0 = slice * DEC_SLICE;
    // every global load of the block first: K (4 x 16 bytes of key tid / 4) and V (2 channels of 16 keys)
    const int kj = tid >> 2, kc = tid & 3;
    const bool kok = row0 + kj < n;
    uint4 kv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) kv[i] = make_uint4(0u, 0u, 0u, 0u);
    if (kok) {
        const uint16_t* kr = cache + (size_t)(row0 + kj) * width + (size_t)hk * 128 + kc * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) kv[i] = *(const uint4*)(kr + i * 8);
    }
    uint32_t vv[16];
    const uint16_t* vr = cache + (size_t)(row0 + wave * 16) * width + (size_t)(Hkv + hk) * 128 + 2 * lane;
#pragma unroll
    for (int k = 0; k < 16; ++k) vv[k] = row0 + wave * 16 + k < n ? *(const uint32_t*)(vr + (size_t)k * width) : 0u;
    for (int i = tid; i < G * 128; i += 256) ql[i] = bf2f(q[(size_t)hk * G * 128 + i]);
    __syncthreads();
    float s[DEC_MAX_GROUP];
#pragma unroll
    for (int g = 0; g < DEC_MAX_GROUP; ++g) s[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w[4] = {kv[i].x, kv[i].y, kv[i].z, kv[i].w};
        float kf[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { kf[2 * e] = __uint_as_float(w[e] << 16); kf[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
#pragma unroll
        for (int g = 0; g < DEC_MAX_GROUP; ++g) {
            if (g < G) {
                const float* qp = ql + g * 128 + kc * 32 + i * 8;
                const float4 qa = *(const float4*)qp, qb = *(const float4*)(qp + 4);
                float a = s[g];
                a = fmaf(qa.x, kf[0], a); a = fmaf(qa.y, kf[1], a); a = fmaf(qa.z, kf[2], a); a = fmaf(qa.w, kf[3], a);
                a = fmaf(qb.x, kf[4], a); a = fmaf(qb.y, kf[5], a); a = fmaf(qb.z, kf[6], a); a = fmaf(qb.w, kf[7], a);
                s[g] = a;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < DEC_MAX_GROUP; ++g) {
        if (g < G) {
            float a = s[g];
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            if (kc == 0) sl[g * DEC_SLICE + kj] = kok ? a * scale : -INFINITY;
        }
    }
    __syncthreads();
    float m[DEC_MAX_GROUP], l[DEC_MAX_GROUP], p[DEC_MAX_GROUP];
#pragma unroll
    for (int g = 0; g < DEC_MAX_GROUP; ++g) {
        if (g < G) {
            const float t = sl[g * DEC_SLICE + lane];
            float mx = t;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            p[g] = expf(t - mx);                                                 // key row0 is valid: mx is finite, exp(-inf) = 0
            m[g] = mx;
            l[g] = wave_sum(p[g]);
        }
    }
    __syncthreads();                                                             // every wave has read the scores
    if (wave == 0) {
#pragma unroll
        for (int g = 0; g < DEC_MAX_GROUP; ++g)
            if (g < G) sl[g * DEC_SLICE + lane] = p[g];
    }
    __syncthreads();
    float o0[DEC_MAX_GROUP], o1[DEC_MAX_GROUP];
#pragma unroll
    for (int g = 0; g < DEC_MAX_GROUP; ++g) o0[g] = o1[g] = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float v0 = __uint_as_float(vv[k] << 16), v1 = __uint_as_float(vv[k] & 0xffff0000u);
#pragma unroll
        for (int g = 0; g < DEC_MAX_GROUP; ++g) {
            if (g < G) {
                const float pk = sl[g * DEC_SLICE + wave * 16 + k];
                o0[g] = fmaf(pk, v0, o0[g]);
                o1[g] = fmaf(pk, v1, o1[g]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int g = 0; g < DEC_MAX_GROUP; ++g)
            if (g < G) *(float2*)(ol + ((wave - 1) * DEC_MAX_GROUP + g) * 128 + 2 * lane) = make_float2(o0[g], o1[g]);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int g = 0; g < DEC_MAX_GROUP; ++g) {
            if (g < G) {
                float a0 = o0[g], a1 = o1[g];
#pragma unroll
                for (int w = 0; w < 3; ++w) {                                    // wave order
                    const float2 t = *(const float2*)(ol + (w * DEC_MAX_GROUP + g) * 128 + 2 * lane);
                    a0 += t.x;
                    a1 += t.y;
                }
                float* pr = part + ((size_t)(hk * G + g) * nslices + slice) * DEC_PART;
                if (lane == 0) { pr[0] = m[g]; pr[1] = l[g]; }
                *(float2*)(pr + 2 + 2 * lane) = make_float2(a0, a1);
            }
        }
    }
}

// Block = one query head, thread = one output channel: M = max of the slices' maxima, then l and o folded in slice order.
__global__ __launch_bounds__(128) void lm_decode_merge_kernel(const float* __restrict__ part, int nslices, uint16_t* __restrict__ O) {
    const int h = blockIdx.x, d = threadIdx.x;
    const float* pr = part + (size_t)h * nslices * DEC_PART;
    float M = -INFINITY;
#pragma unroll 8
    for (int s = 0; s < nslices; ++s) M = fmaxf(M, pr[(size_t)s * DEC_PART]);
    float l = 0.f, o = 0.f;
#pragma unroll 8
    for (int s = 0; s < nslices; ++s) {
        const float a = expf(pr[(size_t)s * DEC_PART] - M);
        l = fmaf(pr[(size_t)s * DEC_PART + 1], a, l);
        o = fmaf(pr[(size_t)s * DEC_PART + 2 + d], a, o);
    }
    O[(size_t)h * 128 + d] = f2bf(o / l);
}

}  // namespace rgn

using namespace rgn;

extern "C" {

static inline bool dal16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int rgn_lm_gemv_bf16(const void* W, const void* x, const void* bias, const void* resid, void* y, int N, int K, void* stream) {
    if (!W || !x || !y || N < 1 || K < 64) return fail(RGN_E_BADARG, "lm_gemv: bad argument (W, x, y non-null; N >= 1; K >= 64)");
    if (K % 64) return fail(RGN_E_BADARG, "lm_gemv: K must be a multiple of 64");
    if (!dal16(W) || !dal16(x)) return fail(RGN_E_BADARG, "lm_gemv: W and x must be 16-byte aligned");
    if (((uintptr_t)y | (uintptr_t)bias | (uintptr_t)resid) & 1u) return fail(RGN_E_BADARG, "lm_gemv: y, bias and resid must be 2-byte aligned");
    hipLaunchKernelGGL((lm_gemv_kernel<false>), dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)W, (const uint16_t*)x,
                       (const uint16_t*)bias, (const uint16_t*)resid, (uint16_t*)y, (float*)nullptr, (float*)nullptr, (int*)nullptr, N, K);
    return check_launch("lm_gemv_kernel");
}

int rgn_lm_gemv_w8(const void* W8, const float* wscale, const void* x, const void* bias, const void* resid, void* y, int N, int K,
                   void* stream) {
    if (!W8 || !wscale || !x || !y || N < 1 || K < 64)
        return fail(RGN_E_BADARG, "lm_gemv_w8: bad argument (W8, wscale, x, y non-null; N >= 1; K >= 64)");
    if (K % 16) return fail(RGN_E_BADARG, "lm_gemv_w8: K must be a multiple of 16");
    if (!dal16(W8) || !dal16(wscale) || !dal16(x) || !dal16(y)) return fail(RGN_E_BADARG, "lm_gemv_w8: W8, wscale, x and y must be 16-byte aligned");
    if (((uintptr_t)bias | (uintptr_t)resid) & 1u) return fail(RGN_E_BADARG, "lm_gemv_w8: bias and resid must be 2-byte aligned");
    constexpr int rows = 4 * W8_ROWS;
    hipLaunchKernelGGL((lm_gemv_w8_kernel<W8_ROWS, W8_U>), dim3((N + rows - 1) / rows), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)W8,
                       wscale, (const uint16_t*)x, (const uint16_t*)bias, (const uint16_t*)resid, (uint16_t*)y, N, K);
    return check_launch("lm_gemv_w8_kernel");
}

static inline int head_parts(int V) { return (V + 3) / 4; }                 // lm_gemv_kernel<true>: 4 rows per block

size_t rgn_lm_head_workspace_bytes(int V) { return V < 1 ? 0 : (size_t)head_parts(V) * (sizeof(float) + sizeof(int)); }

int rgn_lm_head_argmax(const void* W, const void* x, int V, int K, void* token_out, float* logits_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!W || !x || !token_out || !workspace || V < 1 || K < 64)
        return fail(RGN_E_BADARG, "lm_head_argmax: bad argument (W, x, token_out, workspace non-null; V >= 1; K >= 64)");
    if (K % 64) return fail(RGN_E_BADARG, "lm_head_argmax: K must be a multiple of 64");
    if (!dal16(W) || !dal16(x)) return fail(RGN_E_BADARG, "lm_head_argmax: W and x must be 16-byte aligned");
    if (((uintptr_t)token_out & 7u) || ((uintptr_t)logits_out & 3u) || ((uintptr_t)workspace & 3u))
        return fail(RGN_E_BADARG, "lm_head_argmax: token_out must be 8-byte, logits_out and workspace 4-byte aligned");
    if (workspace_bytes < rgn_lm_head_workspace_bytes(V)) return fail(RGN_E_BADARG, "lm_head_argmax: workspace smaller than rgn_lm_head_workspace_bytes(V)");
    const int np = head_parts(V);
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + np);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((lm_gemv_kernel<true>), dim3(np), dim3(256), 0, st, (const uint16_t*)W, (const uint16_t*)x, (const uint16_t*)nullptr,
                       (const uint16_t*)nullptr, (uint16_t*)nullptr, logits_out, pv, pi, V, K);
    hipLaunchKernelGGL(lm_head_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)pv, (const int*)pi, np, (int64_t*)token_out);
    return check_launch("lm_head_argmax");
}

int rgn_lm_kv_append_bf16(const void* QKV, int ld, void* cache, int cap, int row0, int L, int Hq, int Hkv, void* stream) {
    if (L == 0) return 0;
    if (!QKV || !cache || L < 0 || row0 < 0 || Hq < 1 || Hkv < 1 || Hq > 1024 || Hkv > 1024 || ld < (Hq + 2 * Hkv) * 128 || ld % 8)
        return fail(RGN_E_BADARG, "lm_kv_append: bad argument (QKV, cache non-null; L, row0 >= 0; 1 <= Hq, Hkv <= 1024; ld >= (Hq + 2 Hkv) 128, a multiple of 8)");
    if (cap < 1 || cap > DEC_MAX_N || row0 > cap - L) return fail(RGN_E_BADARG, "lm_kv_append: rows [row0, row0 + L) must lie in a cache of 1 <= cap <= 4096 rows");
    if (!dal16(QKV) || !dal16(cache)) return fail(RGN_E_BADARG, "lm_kv_append: QKV and cache must be 16-byte aligned");
    const int width = 2 * Hkv * 128;
    const size_t items = (size_t)L * (width / 8), g = (items + 255) / 256;
    hipLaunchKernelGGL(lm_kv_append_kernel, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV, ld,
                       Hq * 128, (uint16_t*)cache, row0, L, width);
    return check_launch("lm_kv_append_kernel");
}

size_t rgn_lm_decode_attention_workspace_bytes(int Hq, int n) {
    if (Hq < 1 || n < 1) return 0;
    return (size_t)Hq * ((n + DEC_SLICE - 1) / DEC_SLICE) * DEC_PART * sizeof(float);
}

int rgn_lm_decode_attention_bf16(const void* q, const void* cache, void* O, int n, int Hq, int Hkv, float scale, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!q || !cache || !O || !workspace || Hkv < 1 || Hq < Hkv || Hq > 1024 || !(scale > 0.f) || !(scale < INFINITY))
        return fail(RGN_E_BADARG, "lm_decode_attention: bad argument (q, cache, O, workspace non-null; 1 <= Hkv <= Hq <= 1024; 0 < scale < inf)");
    if (Hq % Hkv || Hq / Hkv > DEC_MAX_GROUP) return fail(RGN_E_BADARG, "lm_decode_attention: Hq % Hkv != 0 or Hq / Hkv > 8");
    if (n < 1 || n > DEC_MAX_N) return fail(RGN_E_BADARG, "lm_decode_attention: n outside [1, 4096]");
    if (!dal16(q) || !dal16(cache) || !dal16(O) || !dal16(workspace))
        return fail(RGN_E_BADARG, "lm_decode_attention: q, cache, O and workspace must be 16-byte aligned");
    if (workspace_bytes < rgn_lm_decode_attention_workspace_bytes(Hq, n))
        return fail(RGN_E_BADARG, "lm_decode_attention: workspace smaller than rgn_lm_decode_attention_workspace_bytes(Hq, n)");
    const int ns = (n + DEC_SLICE - 1) / DEC_SLICE;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lm_decode_attention_kernel, dim3(ns, Hkv), dim3(256), 0, st, (const uint16_t*)q, (const uint16_t*)cache, n, Hq, Hkv, scale,
                       (float*)workspace, ns);
    hipLaunchKernelGGL(lm_decode_merge_kernel, dim3(Hq), dim3(128), 0, st, (const float*)workspace, ns, (uint16_t*)O);
    return check_launch("lm_decode_attention");
}

}  // extern "C"
