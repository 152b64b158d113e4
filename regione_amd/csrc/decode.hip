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
//   lm_seen_mark_kernel         seen[id] = 1 for the prompt ids: the byte map the repetition penalty reads
//   lm_pick_kernel              one block between lm_head and the next embedding: repetition penalty, temperature, top-k, top-p and the
//                               pick (argmax, or the inverse CDF at a uniform read from device memory) over the fp32 logits in L2
// and the same step for a batch of B <= 8 sequences, every weight streamed ONCE for all of them, row b bit-identical to the kernels above:
//   lm_gemv_rows_kernel         the three one-row products (bf16, fp8, lm_head with per-block maxima) for B rows of x: a weight vector is
//                               loaded and converted once, x sits in LDS as fp32, one accumulator per (weight row, x row)
//   lm_head_finalize_rows_kernel, lm_kv_append_rows_kernel, lm_decode_attention_rows_kernel, lm_decode_merge_rows_kernel
//                               the batch on a grid axis; per-sequence cache lengths travel by value (no device read, no upload)
//   lm_pick_rows_kernel         the block of lm_pick_kernel once per row (blockIdx.x = b), each on a CU of its own: the same device function
// That invariant is what the host side rests on: an operation is ONE implementation over 1 <= B <= 8 rows, reached through its `_rows`
// entry, which launches the one-row kernels at B == 1 and the `_rows` kernels from B = 2 on; the one-row entry is its B = 1 case.
// and, opt-in (batch_kernels="mfma"), the weight-streaming layers of that step for B <= 32 sequences on the matrix unit:
//   lm_gemm_rows_kernel         the three products as a skinny GEMM on v_mfma_f32_16x16x32_bf16: weights straight from HBM into the B operand,
//                               the rows of x in LDS as bf16, K split over the four waves and folded in wave order; row b depends on row b
//                               alone, but its sums are not the `_rows` kernels' sums in the last bits (described at the kernel)
// and, opt-in (lookup=True), a step that carries drafted tokens of ONE sequence as extra rows and keeps the prefix greedy search gives:
//   lm_verify_attention_kernel  R <= 8 queries against one cache, query r over n0 + r rows: K and V of a slice loaded once for all of
//                               them, row r bit-identical to lm_decode_attention_kernel at n0 + r
//   lm_lookup_step_kernel       one block after the head: accepts the drafts the argmaxes confirm, writes the token after them and
//                               proposes the next drafts (an n-gram match in the sequence so far, or a caller's guess)
// and, opt-in (lookup_sampling=True), that step under sampling and a repetition penalty, keeping the prefix the plain sampled loop gives:
//   lm_pick_verify_kernel       the block of lm_pick_kernel once per row of the step; row r picks under the map seen U drafts[0, r) and
//                               stores nothing to the map
//   lm_lookup_step_mark_kernel  lm_lookup_step_kernel over the picks; marks the tokens the step settles in the byte map
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

__device__ __forceinline__ void head_finalize_block(const float* __restrict__ part_v, const int* __restrict__ part_i, int nparts,
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

__global__ __launch_bounds__(1024) void lm_head_finalize_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int nparts,
                                                                int64_t* __restrict__ out) {
    head_finalize_block(part_v, part_i, nparts, out);
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
__device__ __forceinline__ void decode_attention_block(const uint16_t* __restrict__ q, const uint16_t* __restrict__ cache, int n, int Hq,
                                                       int Hkv, float scale, float* __restrict__ part, int nslices) {
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

__global__ __launch_bounds__(256) void lm_decode_attention_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ cache, int n,
                                                                  int Hq, int Hkv, float scale, float* __restrict__ part, int nslices) {
    decode_attention_block(q, cache, n, Hq, Hkv, scale, part, nslices);
}

// Block = one query head, thread = one output channel: M = max of the slices' maxima, then l and o folded in slice order.
__device__ __forceinline__ void decode_merge_head(const float* __restrict__ part, int nslices, uint16_t* __restrict__ O) {
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

__global__ __launch_bounds__(128) void lm_decode_merge_kernel(const float* __restrict__ part, int nslices, uint16_t* __restrict__ O) {
    decode_merge_head(part, nslices, O);
}

// ---- the same step for B <= 8 sequences from ONE stream of the weights (generate over a batch) ------------------------------------------
// Row b of every result is bit for bit what the one-row kernel above gives for row b alone: a lane owns the same k (8 per 512-wide step
// of a bf16 row, 16 per 1024-wide step of an fp8 row) in the same ascending order, adds them with the same fmaf chain into ONE fp32
// accumulator per (weight row, x row), and the 64 lanes are folded by the same wave_sum butterfly; the round structure of the one-row
// kernels (how many loads are in flight) is not part of that order, so it is free here.
//   block = 4 waves x ROWS_R weight rows; a weight vector is loaded once (non-temporal, 16 bytes) and converted once for all B rows
//   x     the B rows of a chunk of k (1024 wide for bf16 weights, 2048 for fp8) are widened to fp32 ONCE per block and kept in LDS
//         (B x 4 KB, B x 8 KB), laid out in planes of
//         float4 so that the lanes of a wave read consecutive 16-byte slots (ds_read_b128 without bank conflicts): both conversions are
//         exact, so hoisting them changes no bit, and the FMA phase issues one v_fma per product and nothing else
// The loads of the next chunk (x, then W) are issued before the products of the current one.
struct LmRows { int v[RGN_LM_MAX_BATCH]; };                                      // one int per sequence, passed to a kernel by value
constexpr int ROWS_R = 2;
template <bool W8> constexpr int rows_kc() { return W8 ? 2048 : 1024; }         // k per chunk: two steps of either lane layout

template <int B, bool W8, bool ARGMAX>
__global__ __launch_bounds__(256) void lm_gemv_rows_kernel(const uint8_t* __restrict__ W, const float* __restrict__ wscale,
                                                           const uint16_t* __restrict__ X, int ldx, const uint16_t* __restrict__ bias,
                                                           const uint16_t* resid, int ldr, uint16_t* Y, int ldy, float* __restrict__ logits,
                                                           int ldl, float* __restrict__ part_v, int* __restrict__ part_i, int nparts, int N, int K) {
    constexpr int VPL = W8 ? 16 : 8, ES = W8 ? 1 : 2, KC = rows_kc<W8>();        // k per lane and step; bytes per weight; k per chunk
    constexpr int U = KC / (64 * VPL), PL = VPL / 4, SL = 64 * U;                // steps per chunk; float4 planes; slots per plane
    constexpr int VR = KC / 8, RPP = 256 / VR, NP = (B + RPP - 1) / RPP;         // staging: 16-byte vectors per row, rows per pass, passes
    extern __shared__ __attribute__((aligned(16))) uint8_t rows_lds[];
    float4* xs = (float4*)rows_lds;                                              // [B][PL][SL]
    __shared__ float bv[4 * ROWS_R * RGN_LM_MAX_BATCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = (blockIdx.x * 4 + wave) * ROWS_R;
    const uint8_t* wr[ROWS_R];
    float acc[ROWS_R][B];
#pragma unroll
    for (int r = 0; r < ROWS_R; ++r) {
        wr[r] = W + (size_t)(n0 + r < N ? n0 + r : N - 1) * (size_t)K * ES;      // a row past N re-reads row N - 1 and writes nothing
#pragma unroll
        for (int b = 0; b < B; ++b) acc[r][b] = 0.f;
    }
    const int sk = (tid % VR) * 8, sb = tid / VR;                                // staging: 8 values at k = sk of rows sb, sb + RPP, ...
    const int sslot = sk / VPL, spl = (sk % VPL) / 4;
    uint4 xv[NP];
    u32x4 wv[ROWS_R][U];
    // the loads of one chunk: x first (the counter of outstanding loads is in order: waiting for x leaves W in flight)
    auto issue = [&](int kb) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int b = sb + j * RPP;
            xv[j] = b < B && kb + sk < K ? *(const uint4*)(X + (size_t)b * ldx + kb + sk) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kb + (u * 64 + lane) * VPL;
#pragma unroll
            for (int r = 0; r < ROWS_R; ++r)                                     // a lane past K loads nothing and adds 0
                wv[r][u] = k < K ? __builtin_nontemporal_load((const u32x4*)(wr[r] + (size_t)k * ES)) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    issue(0);
    for (int kb = 0; kb < K; kb += KC) {
        if (kb) __syncthreads();                                                 // every wave is done with the previous chunk
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int b = sb + j * RPP;
            if (b < B) {
                const uint32_t a[4] = {xv[j].x, xv[j].y, xv[j].z, xv[j].w};
                float4* dst = xs + (b * PL + spl) * SL + sslot;
                dst[0] = make_float4(__uint_as_float(a[0] << 16), __uint_as_float(a[0] & 0xffff0000u), __uint_as_float(a[1] << 16),
                                     __uint_as_float(a[1] & 0xffff0000u));
                dst[SL] = make_float4(__uint_as_float(a[2] << 16), __uint_as_float(a[2] & 0xffff0000u), __uint_as_float(a[3] << 16),
                                      __uint_as_float(a[3] & 0xffff0000u));
            }
        }
        __syncthreads();
        u32x4 wc[ROWS_R][U];                                                     // this chunk's weights; the next chunk's loads go out
#pragma unroll                                                                   // before its products, so they fly during them
        for (int r = 0; r < ROWS_R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) wc[r][u] = wv[r][u];
        if (kb + KC < K) issue(kb + KC);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float wf[ROWS_R][VPL];
#pragma unroll
            for (int r = 0; r < ROWS_R; ++r) {
                const uint32_t a[4] = {wc[r][u].x, wc[r][u].y, wc[r][u].z, wc[r][u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (W8) {
                        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)a[e], true);
                        wf[r][4 * e] = lo[0]; wf[r][4 * e + 1] = lo[1]; wf[r][4 * e + 2] = hi[0]; wf[r][4 * e + 3] = hi[1];
                    } else {
                        wf[r][2 * e] = __uint_as_float(a[e] << 16);
                        wf[r][2 * e + 1] = __uint_as_float(a[e] & 0xffff0000u);
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
#pragma unroll
                for (int p = 0; p < PL; ++p) {
                    const float4 x4 = xs[(b * PL + p) * SL + u * 64 + lane];
#pragma unroll
                    for (int r = 0; r < ROWS_R; ++r) {                           // ascending k: the chain of dot8 / dot16_w8
                        float a = acc[r][b];
                        a = fmaf(wf[r][4 * p], x4.x, a);
                        a = fmaf(wf[r][4 * p + 1], x4.y, a);
                        a = fmaf(wf[r][4 * p + 2], x4.z, a);
                        a = fmaf(wf[r][4 * p + 3], x4.w, a);
                        acc[r][b] = a;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS_R; ++r) {
        const int n = n0 + r;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const float s = wave_sum(acc[r][b]);
            if (lane != 0) continue;
            if constexpr (ARGMAX) {
                bv[(wave * ROWS_R + r) * B + b] = s;
                if (logits && n < N) logits[(size_t)b * ldl + n] = s;
            } else if (n < N) {
                const float bs = bias ? bf2f(bias[n]) : 0.f;
                float v;
                if constexpr (W8) v = fmaf(s, wscale[n], bs);                    // the scale once, on the reduced sum
                else v = s + bs;
                Y[(size_t)b * ldy + n] = resid ? f2bf(rbf(v) + bf2f(resid[(size_t)b * ldr + n])) : f2bf(v);   // two roundings
            }
        }
    }
    if constexpr (ARGMAX) {
        __syncthreads();
        if (tid < B) {
            const int base = blockIdx.x * 4 * ROWS_R;
            float best = bv[tid];                                                // row `base` exists in every block
            int at = base;
            for (int i = 1; i < 4 * ROWS_R; ++i)                                 // ascending index, strict >: the first maximum
                if (base + i < N && bv[i * B + tid] > best) { best = bv[i * B + tid]; at = base + i; }
            part_v[(size_t)tid * nparts + blockIdx.x] = best;
            part_i[(size_t)tid * nparts + blockIdx.x] = at;
        }
    }
}

// One block per sequence folds that sequence's per-block maxima, as lm_head_finalize_kernel does for one.
__global__ __launch_bounds__(1024) void lm_head_finalize_rows_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int nparts,
                                                                     int64_t* __restrict__ out, int out_stride) {
    const size_t b = blockIdx.x;
    head_finalize_block(part_v + b * nparts, part_i + b * nparts, nparts, out + b * out_stride);
}

// Row b of QKV [B, ld] into cache b (base + b cache_stride) at row row0[b]: one 16-byte vector per thread.
__global__ __launch_bounds__(256) void lm_kv_append_rows_kernel(const uint16_t* __restrict__ QKV, int ld, int col0, uint16_t* __restrict__ cache,
                                                                size_t cache_stride, LmRows row0, int width) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i < width / 8)
        *(uint4*)(cache + b * cache_stride + (size_t)row0.v[b] * width + i * 8) = *(const uint4*)(QKV + (size_t)b * ld + col0 + i * 8);
}

// Grid = (slices of the LONGEST cache, KV heads, sequences).  A block whose slice starts at or past n[b] has nothing to do and returns
// before the first barrier (n[b] and the slice are the same for every thread of the block); the others are lm_decode_attention_kernel.
__global__ __launch_bounds__(256) void lm_decode_attention_rows_kernel(const uint16_t* __restrict__ Q, int ldq, const uint16_t* __restrict__ cache,
                                                                       size_t cache_stride, LmRows nb, int Hq, int Hkv, float scale,
                                                                       float* __restrict__ part, size_t part_stride) {
    const int b = blockIdx.z, n = nb.v[b];
    if ((int)blockIdx.x * DEC_SLICE >= n) return;
    decode_attention_block(Q + (size_t)b * ldq, cache + b * cache_stride, n, Hq, Hkv, scale, part + b * part_stride,
                           (n + DEC_SLICE - 1) / DEC_SLICE);
}

__global__ __launch_bounds__(128) void lm_decode_merge_rows_kernel(const float* __restrict__ part, size_t part_stride, LmRows nb,
                                                                   uint16_t* __restrict__ O, int ldo) {
    const int b = blockIdx.y;
    decode_merge_head(part + b * part_stride, (nb.v[b] + DEC_SLICE - 1) / DEC_SLICE, O + (size_t)b * ldo);
}

// ---- R queries of ONE sequence against ONE cache: a step that verifies R - 1 drafted tokens -------------------------------------------
// Query r (row r of Q) sees cache rows [0, n0 + r).  Block = (slice of 64 cache rows, KV head) as in decode_attention_block, but K and V
// of the slice are loaded ONCE, masked by the LONGEST row (n0 + R - 1), and stay in registers (16 + 16 VGPRs) while the block walks the
// queries that own the slice: slice s exists for row r iff 64 s < n0 + r, so the rows from max(0, 64 s + 1 - n0) on.  Per query the
// arithmetic is decode_attention_block's at n = n0 + r, statement for statement - the same fmaf chain per (key, quarter), the same quad
// and wave folds, the same wave order in P V - so row r has the bits of the one-row kernel.  What differs is how a key in
// [n0 + r, n0 + R - 1) is kept out: it IS in registers here, so its score is replaced by -inf (as the one-row kernel does for a key it
// did not load) and its V is replaced by 0 in the product (the one-row kernel multiplies p = 0 by v = 0; p = 0 times a loaded v would
// differ in the sign of a zero sum, and in more for a non-finite v).  The LDS is reused from query to query: every array is last read
// before a barrier that precedes its next write (ql: scores phase / top of the next query; sl: P V / after the next query's first
// barrier; ol: the fold of wave 0 / four barriers later).  Partials of row r go to part + r part_stride, indexed by that row's own
// slice count, and lm_decode_merge_rows_kernel folds them per row.
__global__ __launch_bounds__(256) void lm_verify_attention_kernel(const uint16_t* __restrict__ Q, int ldq, const uint16_t* __restrict__ cache,
                                                                  int n0, int R, int Hq, int Hkv, float scale, float* __restrict__ part,
                                                                  size_t part_stride) {
    __shared__ __attribute__((aligned(16))) float ql[DEC_MAX_GROUP * 128];
    __shared__ float sl[DEC_MAX_GROUP * DEC_SLICE];                              // scores, then p
    __shared__ __attribute__((aligned(8))) float ol[3 * DEC_MAX_GROUP * 128];    // the P V sums of waves 1..3
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slice = blockIdx.x, hk = blockIdx.y, G = Hq / Hkv;
    const size_t width = (size_t)2 * Hkv * 128;
    const int row0 = slice * DEC_SLICE, nmax = n0 + R - 1;
    const int kj = tid >> 2, kc = tid & 3;
    uint4 kv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) kv[i] = make_uint4(0u, 0u, 0u, 0u);
    if (row0 + kj < nmax) {
        const uint16_t* kr = cache + (size_t)(row0 + kj) * width + (size_t)hk * 128 + kc * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) kv[i] = *(const uint4*)(kr + i * 8);
    }
    uint32_t vv[16];
    const uint16_t* vr = cache + (size_t)(row0 + wave * 16) * width + (size_t)(Hkv + hk) * 128 + 2 * lane;
#pragma unroll
    for (int k = 0; k < 16; ++k) vv[k] = row0 + wave * 16 + k < nmax ? *(const uint32_t*)(vr + (size_t)k * width) : 0u;
    const int rfirst = row0 + 1 - n0 > 0 ? row0 + 1 - n0 : 0;                    // < R: the grid has ceil(nmax / 64) slices
#pragma unroll 1
    for (int r = rfirst; r < R; ++r) {
        const int n = n0 + r, nslices = (n + DEC_SLICE - 1) / DEC_SLICE;
        const bool kok = row0 + kj < n;
        const uint16_t* q = Q + (size_t)r * ldq;
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
                p[g] = expf(t - mx);                                             // key row0 is valid for this row: mx is finite
                m[g] = mx;
                l[g] = wave_sum(p[g]);
            }
        }
        __syncthreads();                                                         // every wave has read the scores
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
            const uint32_t vk = row0 + wave * 16 + k < n ? vv[k] : 0u;           // a key this row does not see: v = 0, as if never loaded
            const float v0 = __uint_as_float(vk << 16), v1 = __uint_as_float(vk & 0xffff0000u);
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
            float* prow = part + (size_t)r * part_stride;
#pragma unroll
            for (int g = 0; g < DEC_MAX_GROUP; ++g) {
                if (g < G) {
                    float a0 = o0[g], a1 = o1[g];
#pragma unroll
                    for (int w = 0; w < 3; ++w) {                                // wave order
                        const float2 t = *(const float2*)(ol + (w * DEC_MAX_GROUP + g) * 128 + 2 * lane);
                        a0 += t.x;
                        a1 += t.y;
                    }
                    float* pr = prow + ((size_t)(hk * G + g) * nslices + slice) * DEC_PART;
                    if (lane == 0) { pr[0] = m[g]; pr[1] = l[g]; }
                    *(float2*)(pr + 2 + 2 * lane) = make_float2(a0, a1);
                }
            }
        }
    }
}

// ---- accept the verified drafts and propose the next ones: ONE block after the head of a verify step -----------------------------------
// seq is one run of int64 ids (prompt, then new tokens); seq[0, n) is settled, seq[n - 1] was row 0 of the step, seq[n, n + R - 1) are the
// drafts that were rows 1..R-1 and head[r hs] is the argmax after row r.
//   accept   a = the number of leading drafts that equal the heads before them (the FIRST mismatch ends the run); seq[n + a] = head[a],
//            the token the model gives after the last accepted row; n' = n + a + 1.  Every thread walks the <= 31 pairs itself.
//   propose  kcap = max(0, min(K, limit - n' - 1)) drafts at most.  With `guess`: draft i is guess[(n' - L) + i] while that index is inside
//            the guess.  Without: transformers' PromptLookupCandidateGenerator over seq[0, n') - n-gram sizes from min(max_ngram, n' - 1)
//            down to 1, per size the LOWEST window index idx whose window equals the trailing n-gram and whose continuation
//            [idx + size, min(idx + size + kcap, n')) is not empty (which excludes the trailing n-gram itself); thread t tries windows
//            t, t + 256, ... in ascending order, the block takes the minimum through the wave butterfly and four LDS slots.
//   result   int64 [2 + R]: a, k', then the a + 1 accepted tokens.  Plain stores, no atomics; the drafts go to seq[n', n' + k').
constexpr int LOOKUP_T = 256, LOOKUP_MAX_R = RGN_LM_MAX_WIDE_BATCH, LOOKUP_MAX_NGRAM = 8, LOOKUP_NONE = 0x7fffffff;

// MARK: the step of a sampled or penalised generate - head[r] is then the PICK after row r - also sets seen[t] = 1 for the a + 1 tokens it
// settles (the accepted drafts equal the picks before them, so these are head[0..a]); a rejected draft marks nothing, nor does an id
// outside [0, V).  Plain byte stores of the same value.
template <bool MARK>
__device__ __forceinline__ void lm_lookup_step_body(int64_t* __restrict__ seq, int n, int R, const int64_t* __restrict__ head, int hs, int limit,
                                                    int K, int max_ngram, const int64_t* __restrict__ guess, int guess_len, int L,
                                                    int64_t* __restrict__ result, uint8_t* __restrict__ seen, int V) {
    __shared__ int best[LOOKUP_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int a = 0;
    while (a < R - 1 && seq[n + a] == head[(size_t)a * hs]) ++a;
    const int n1 = n + a + 1;
    __syncthreads();                                                             // every thread has read the drafts
    if (tid <= a) result[2 + tid] = head[(size_t)tid * hs];
    if (tid == 0) seq[n + a] = head[(size_t)a * hs];
    if constexpr (MARK) {
        if (tid <= a) {
            const int64_t t = head[(size_t)tid * hs];
            if (t >= 0 && t < (int64_t)V) seen[t] = 1;
        }
    }
    __syncthreads();                                                             // the bonus token is in seq for the whole block
    int kcap = limit - n1 - 1 < K ? limit - n1 - 1 : K;
    kcap = kcap > 0 ? kcap : 0;
    int kn = 0;
    if (guess) {
        const int at = n1 - L;                                                   // the new-token position of draft 0
        kn = guess_len - at < kcap ? guess_len - at : kcap;
        kn = kn > 0 ? kn : 0;
        if (tid < kn) seq[n1 + tid] = guess[at + tid];
    } else if (kcap > 0) {
        for (int size = max_ngram < n1 - 1 ? max_ngram : n1 - 1; size >= 1; --size) {
            int64_t tail[LOOKUP_MAX_NGRAM];
#pragma unroll
            for (int j = 0; j < LOOKUP_MAX_NGRAM; ++j) tail[j] = j < size ? seq[n1 - size + j] : 0;
            int mine = LOOKUP_NONE;
            for (int idx = tid; idx + size < n1; idx += LOOKUP_T) {              // idx + size < n1: the continuation is not empty
                bool eq = true;
#pragma unroll
                for (int j = 0; j < LOOKUP_MAX_NGRAM; ++j)
                    if (j < size) eq = eq && seq[idx + j] == tail[j];
                if (eq) { mine = idx; break; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(mine, o, 64); mine = t < mine ? t : mine; }
            if (lane == 0) best[wave] = mine;
            __syncthreads();
            int idx = best[0];
#pragma unroll
            for (int w = 1; w < LOOKUP_T / 64; ++w) idx = best[w] < idx ? best[w] : idx;
            __syncthreads();                                                     // best[] is free for the next size
            if (idx != LOOKUP_NONE) {                                                // the same for every thread
                const int start = idx + size, end = start + kcap < n1 ? start + kcap : n1;
                kn = end - start;
                if (tid < kn) seq[n1 + tid] = seq[start + tid];                  // source below n1, destination from n1 on
                break;
            }
        }
    }
    if (tid == 0) { result[0] = a; result[1] = kn; }
}

__global__ __launch_bounds__(LOOKUP_T) void lm_lookup_step_kernel(int64_t* __restrict__ seq, int n, int R, const int64_t* __restrict__ head,
                                                                  int hs, int limit, int K, int max_ngram, const int64_t* __restrict__ guess,
                                                                  int guess_len, int L, int64_t* __restrict__ result) {
    lm_lookup_step_body<false>(seq, n, R, head, hs, limit, K, max_ngram, guess, guess_len, L, result, nullptr, 0);
}

__global__ __launch_bounds__(LOOKUP_T) void lm_lookup_step_mark_kernel(int64_t* __restrict__ seq, int n, int R, const int64_t* __restrict__ head,
                                                                       int hs, int limit, int K, int max_ngram,
                                                                       const int64_t* __restrict__ guess, int guess_len, int L,
                                                                       int64_t* __restrict__ result, uint8_t* __restrict__ seen, int V) {
    lm_lookup_step_body<true>(seq, n, R, head, hs, limit, K, max_ngram, guess, guess_len, L, result, seen, V);
}

// ---- repetition penalty and sampling: the pick between lm_head and the next embedding -------------------------------------------------
// seen[ids[i]] = 1: plain byte stores of the same value, so the order of the threads does not matter.  An id outside [0, V) marks nothing.
__global__ __launch_bounds__(256) void lm_seen_mark_kernel(const int64_t* __restrict__ ids, int n, uint8_t* __restrict__ seen, int V) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int64_t t = ids[i];
        if (t >= 0 && t < (int64_t)V) seen[t] = 1;
    }
}

// The stages of transformers' _get_logits_processor in its order, in ONE block of 16 waves: the 608 KB row of fp32 logits stays in L2 and
// is re-read per pass instead of sorted (11 passes with top-p alone, 19 with top-k and top-p).
//   element v belongs to thread v % 1024 in every pass (coalesced; wave w of round i holds tokens 1024 i + 64 w .. + 63 in lane order)
//   scores  s = penalty(z) / T goes to `s` (scores_out, else the workspace); the block maximum and its LOWEST index are folded on the way
//   top-k   the k-th largest value by a radix select over the order-preserving key bits of s, 4 bits a round: a thread adds 1.0 to ITS
//           OWN fp64 bin of the digit (LDS [16][1024], no atomics), wave w folds bin w in thread order, every thread walks the 16 totals
//   top-p   the same select with expf(s - max) as the weight, ascending: the smallest value x whose mass of values <= x exceeds
//           (1 - top_p) Z; tokens below x are dropped.  Equal scores share a key, so they are kept or dropped together.
//   pick    wave sums of the kept masses per 64 tokens (fp64, the butterfly), a block scan over them in token order, the first 64-token
//           segment whose cumulative mass exceeds u Z, then a scan over its 64 lanes: the lowest kept index with C(v) > u Z
// Every sum is fp64 in a fixed order; the only fp32 arithmetic is what transformers does in fp32 (the penalty, the division by T) and expf.
constexpr int PICK_T = 1024, PICK_BINS = 16, PICK_MAX_V = 1 << 20;              // 16384 64-token segments fit the bins' 128 KB of LDS
constexpr int PICK_LDS = PICK_BINS * PICK_T * (int)sizeof(double);
constexpr int PICK_NONE = 0x7fffffff;

__device__ __forceinline__ uint32_t pick_key(float f) {                          // a < b as floats  <=>  key(a) < key(b) (-0 below +0)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pick_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// A pass over the row: f(v, s[v]) for the thread's elements in ascending v, PICK_U loads issued before the first use (one block has to
// cover the L2 latency by itself).  Measured at V = 152064: 0.38 to 0.49 ms per pick, i.e. 20 to 35 us per pass, and the loads are the
// smaller part of it (batching them took 0.09 ms off a pick): ONE CU issues about a dozen instructions for each of 152064 elements per
// pass.  Spreading a pass over many CUs (per-block bins in the workspace, folded by the next launch) is the next step, not taken here.
constexpr int PICK_U = 16;
template <typename F>
__device__ __forceinline__ void pick_pass(const float* s, int V, F&& f) {
    for (int v0 = threadIdx.x; v0 < V; v0 += PICK_T * PICK_U) {
        float x[PICK_U];
#pragma unroll
        for (int u = 0; u < PICK_U; ++u) x[u] = v0 + u * PICK_T < V ? s[v0 + u * PICK_T] : 0.f;
#pragma unroll
        for (int u = 0; u < PICK_U; ++u)
            if (v0 + u * PICK_T < V) f(v0 + u * PICK_T, x[u]);
    }
}

// One radix select over the elements with s >= lo.  MASS = false: the value of the k-th largest element (target = k, weights 1, digits
// walked from the top).  MASS = true: the smallest value x with sum_{s <= x} expf(s - smax) > target * Z, Z the mass of all of them
// (digits walked from the bottom).  Every thread returns the same value.
template <bool MASS>
__device__ __forceinline__ float pick_select(const float* s, int V, double* bins, double* tot, float lo, float smax, double target) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t prefix = 0;
    double passed = 0.0;                                                         // the weight of the buckets already walked past
    for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int b = 0; b < PICK_BINS; ++b) bins[b * PICK_T + tid] = 0.0;
        const int shift = 28 - 4 * r;
        pick_pass(s, V, [&](int, float x) {
            if (x >= lo) {
                const uint32_t key = pick_key(x);
                if (r == 0 || (key >> (shift + 4)) == prefix) {
                    double* bin = bins + ((key >> shift) & 15u) * PICK_T + tid;
                    *bin += MASS ? (double)expf(x - smax) : 1.0;
                }
            }
        });
        __syncthreads();
        double acc = 0.0;                                                        // wave w folds bin w: threads ascending, then the butterfly
#pragma unroll
        for (int j = 0; j < PICK_T / 64; ++j) acc += bins[wave * PICK_T + j * 64 + lane];
        acc = wave_sum_f64(acc);
        if (lane == 0) tot[wave] = acc;
        __syncthreads();
        int d;
        if constexpr (MASS) {
            if (r == 0) {
                double Z = 0.0;
                for (int b = 0; b < PICK_BINS; ++b) Z += tot[b];
                target *= Z;
            }
            d = PICK_BINS - 1;
            for (int b = 0; b < PICK_BINS - 1; ++b) {
                if (passed + tot[b] > target) { d = b; break; }
                passed += tot[b];
            }
        } else {
            d = 0;
            for (int b = PICK_BINS - 1; b > 0; --b) {
                if (passed + tot[b] >= target) { d = b; break; }
                passed += tot[b];
            }
        }
        prefix = (prefix << 4) | (uint32_t)d;
        __syncthreads();                                                         // the totals are read before the next round's fold writes them
    }
    return pick_unkey(prefix);
}

// The pick of ONE row by the whole block: z [V] the row's logits, `seen` its byte map, uniform[0] its uniform, token_out[0] its id slot,
// s [V] its scores (scores_out or workspace).  The kernels below are this body, so a row's result does not depend on which one ran it.
// VERIFY (a row of a verification step, lm_pick_verify_kernel): an id is a member when seen[v] is set OR it is one of the nd ids of
// `drafts` (LDS; -1 where the caller's id lay outside [0, V)) - a membership, so an id is penalised once however often it occurs - and
// the picked token is NOT stored to the map, which is only read.
template <bool VERIFY>
__device__ __forceinline__ void lm_pick_row(const float* __restrict__ z, int V, uint8_t* __restrict__ seen, float penalty, int sample,
                                            float temperature, int top_k, double top_p, const float* __restrict__ uniform,
                                            int64_t* __restrict__ token_out, float* s, const int* drafts = nullptr, int nd = 0) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    double* bins = (double*)smem;
    __shared__ double tot[PICK_BINS];
    __shared__ float rv[PICK_T / 64];
    __shared__ int ri[PICK_T / 64];
    __shared__ double sh_prev;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // scores, and their maximum with its lowest index
    float best = -INFINITY;
    int at = PICK_NONE;
    const bool pen = penalty != 1.f;
    for (int v0 = tid; v0 < V; v0 += PICK_T * PICK_U) {
        float x[PICK_U];
        uint8_t m[PICK_U];
#pragma unroll
        for (int u = 0; u < PICK_U; ++u) {
            const int v = v0 + u * PICK_T;
            x[u] = v < V ? z[v] : 0.f;
            m[u] = pen && v < V ? seen[v] : (uint8_t)0;
        }
        if constexpr (VERIFY) {
            if (pen)
                for (int i = 0; i < nd; ++i) {                                   // nd <= 31, the same for the whole block
                    const int t = drafts[i];                                     // -1 equals no v
#pragma unroll
                    for (int u = 0; u < PICK_U; ++u) m[u] |= (uint8_t)(t == v0 + u * PICK_T);   // t < V: no element past the row matches
                }
        }
#pragma unroll
        for (int u = 0; u < PICK_U; ++u) {
            const int v = v0 + u * PICK_T;
            if (v < V) {
                float y = x[u];
                if (m[u]) y = y < 0.f ? y * penalty : y / penalty;
                if (sample) y = y / temperature;
                s[v] = y;
                if (at == PICK_NONE || y > best) { best = y; at = v; }           // ascending v per thread, strict >: the first maximum
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o, 64);
        const int i2 = __shfl_xor(at, o, 64);
        if (i2 != PICK_NONE && (at == PICK_NONE || v2 > best || (v2 == best && i2 < at))) { best = v2; at = i2; }
    }
    if (lane == 0) { rv[wave] = best; ri[wave] = at; }
    __syncthreads();                                                             // also: every s[v] is written before another thread reads it
    best = rv[0];
    at = ri[0];
    for (int w = 1; w < PICK_T / 64; ++w)
        if (ri[w] != PICK_NONE && (at == PICK_NONE || rv[w] > best || (rv[w] == best && ri[w] < at))) { best = rv[w]; at = ri[w]; }
    if (at == PICK_NONE) at = 0;
    __syncthreads();
    if (!sample) {                                                               // greedy: the argmax of the penalised scores
        if (tid == 0) {
            token_out[0] = (int64_t)at;
            if constexpr (!VERIFY) seen[at] = 1;
        }
        return;
    }
    const float smax = best;
    float lo = -INFINITY;                                                        // kept: s >= lo
    if (top_k > 0 && top_k < V) lo = pick_select<false>(s, V, bins, tot, lo, smax, (double)top_k);
    if (top_p < 1.0) lo = fmaxf(lo, pick_select<true>(s, V, bins, tot, lo, smax, 1.0 - top_p));
    lo = fminf(lo, smax);                                                        // the largest is never dropped
    // kept masses per 64-token segment, in token order
    const int niter = (V + PICK_T - 1) / PICK_T, nseg = niter * (PICK_T / 64);
    double* seg = bins;
    int last = -1;
    for (int i0 = 0; i0 < niter; i0 += PICK_U) {
        float x[PICK_U];
#pragma unroll
        for (int u = 0; u < PICK_U; ++u) x[u] = (i0 + u) * PICK_T + tid < V ? s[(i0 + u) * PICK_T + tid] : -INFINITY;
#pragma unroll
        for (int u = 0; u < PICK_U; ++u) {
            if (i0 + u < niter) {                                                // block-uniform
                const int v = (i0 + u) * PICK_T + tid;
                double e = 0.0;
                if (v < V && x[u] >= lo) { e = (double)expf(x[u] - smax); last = v; }
                e = wave_sum_f64(e);
                if (lane == 0) seg[(i0 + u) * (PICK_T / 64) + wave] = e;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) ri[wave] = last;
    __syncthreads();
    last = ri[0];
    for (int w = 1; w < PICK_T / 64; ++w) last = max(last, ri[w]);
    // block scan: thread t owns segments [t c, t c + c)
    const int c = (nseg + PICK_T - 1) / PICK_T;
    double local = 0.0;
    for (int j = 0; j < c; ++j)
        if (tid * c + j < nseg) local += seg[tid * c + j];
    double inc = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    double excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0.0;
    if (lane == 63) tot[wave] = inc;
    __syncthreads();                                                             // also: ri (the last kept index) is read by every thread
    double Z = 0.0;
    for (int w = 0; w < PICK_T / 64; ++w) {
        if (w == wave) excl += Z;
        Z += tot[w];
    }
    const double target = (double)uniform[0] * Z;
    int cand = PICK_NONE;
    double prev = 0.0, run = excl;
    for (int j = 0; j < c; ++j) {
        const int g = tid * c + j;
        if (g < nseg) {
            const double nx = run + seg[g];
            if (cand == PICK_NONE && nx > target) { cand = g; prev = run; }
            run = nx;
        }
    }
    int first = cand;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    if (lane == 0) ri[wave] = first;
    __syncthreads();
    first = ri[0];
    for (int w = 1; w < PICK_T / 64; ++w) first = min(first, ri[w]);
    if (cand != PICK_NONE && cand == first) sh_prev = prev;                      // segments are partitioned: one thread owns `first`
    __syncthreads();
    if (wave == 0) {
        int tok = last >= 0 ? last : at;                                         // rounding left no crossing: the last kept token
        if (first != PICK_NONE) {
            const int v = (first / (PICK_T / 64)) * PICK_T + (first % (PICK_T / 64)) * 64 + lane;
            double e = 0.0;
            bool kept = false;
            if (v < V) {
                const float x = s[v];
                if (x >= lo) { e = (double)expf(x - smax); kept = true; }
            }
            double ci = e;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double y = __shfl_up(ci, o, 64);
                if (lane >= o) ci += y;
            }
            const unsigned long long hit = __ballot(kept && sh_prev + ci > target), any = __ballot(kept);
            const int base = v - lane;
            if (hit) tok = base + (int)__ffsll((long long)hit) - 1;
            else if (any) tok = base + 63 - (int)__clzll((long long)any);
        }
        if (lane == 0) {
            token_out[0] = (int64_t)tok;
            if constexpr (!VERIFY) seen[tok] = 1;
        }
    }
    __syncthreads();
    if (lo > -INFINITY)                                                          // the processed scores: -inf where filtered
        pick_pass(s, V, [&](int v, float x) {
            if (!(x >= lo)) s[v] = -INFINITY;
        });
}

__global__ __launch_bounds__(PICK_T) void lm_pick_kernel(const float* __restrict__ z, int V, uint8_t* __restrict__ seen, float penalty,
                                                          int sample, float temperature, int top_k, double top_p,
                                                          const float* __restrict__ uniform, int64_t* __restrict__ token_out, float* s) {
    lm_pick_row<false>(z, V, seen, penalty, sample, temperature, top_k, top_p, uniform, token_out, s);
}

// One block per row (blockIdx.x = b < B), each the block of lm_pick_kernel with its own 128 KB of LDS, i.e. a CU to itself: the rows run
// side by side and never communicate.  `uniform` may be null when sample == 0 (never read then).
__global__ __launch_bounds__(PICK_T) void lm_pick_rows_kernel(const float* __restrict__ z, int ldl, int V, uint8_t* __restrict__ seen,
                                                               size_t seen_stride, float penalty, int sample, float temperature, int top_k,
                                                               double top_p, const float* __restrict__ uniform,
                                                               int64_t* __restrict__ token_out, int token_stride, float* s, size_t lds) {
    const size_t b = blockIdx.x;
    lm_pick_row<false>(z + b * (size_t)ldl, V, seen + b * seen_stride, penalty, sample, temperature, top_k, top_p,
                       sample ? uniform + b : uniform, token_out + b * (size_t)token_stride, s + b * lds);
}

// The picks of a verification step: block r (one CU, like a row of lm_pick_rows_kernel) picks for row r under the map seen U drafts[0, r) -
// the map row r has in the plain loop exactly when drafts 0..r-1 were accepted, known before the step runs, so the R picks run side by
// side.  ONE map for all rows, only read: the step's marks are lm_lookup_step_mark_kernel's.  Row 0 reads no draft.
__global__ __launch_bounds__(PICK_T) void lm_pick_verify_kernel(const float* __restrict__ z, int ldl, int V, const uint8_t* __restrict__ seen,
                                                                 const int64_t* __restrict__ drafts, float penalty, int sample,
                                                                 float temperature, int top_k, double top_p,
                                                                 const float* __restrict__ uniform, int64_t* __restrict__ token_out,
                                                                 int token_stride, float* s, size_t lds) {
    __shared__ int dr[LOOKUP_MAX_R];
    const int r = blockIdx.x;                                                    // < LOOKUP_MAX_R: the entry's range
    if ((int)threadIdx.x < r) {
        const int64_t t = drafts[threadIdx.x];
        dr[threadIdx.x] = t >= 0 && t < (int64_t)V ? (int)t : -1;
    }
    __syncthreads();
    lm_pick_row<true>(z + r * (size_t)ldl, V, const_cast<uint8_t*>(seen), penalty, sample, temperature, top_k, top_p,
                      sample ? uniform + r : uniform, token_out + r * (size_t)token_stride, s + r * lds, dr, r);
}

// ---- the wide step: 1 <= B <= 32 rows per step on the matrix unit (opt-in: batch_kernels="mfma") --------------------------------------
// Y [B, N] = X [B, K] W^T as a skinny GEMM on v_mfma_f32_16x16x32_bf16: D[b][n] += sum_k A[b][k] B[k][n] with the 16 rows of X as A and
// 16 weight rows as B, so a weight byte goes HBM -> VGPR -> matrix unit once for all rows and never through LDS.
//   block   4 waves, ONE tile of 16 weight rows n0 .. n0 + 15 (grid = ceil(N / 16)); a row past N re-reads row N - 1 and writes nothing
//   K split the block walks K in chunks of GEMM_KC = 1024; wave w owns k in [kb + 256 w, kb + 256 w + 256) of chunk kb (GEMM_KW = 256 k per
//           wave and chunk = 8 MFMAs), so the split depends on K alone and is uneven whenever K % 1024 != 0; MFMAs past K are skipped
//   W       lane l = (n = l & 15, g = l >> 4) loads row n0 + n in 16-byte non-temporal vectors, all 8 (bf16) / 4 (fp8) of the wave's next
//           chunk issued before the products of the current one
//   k map   bf16: MFMA m of a wave's 256 k reads element j of lane group g at k = 32 m + 8 g + j (vector m of the lane);
//           fp8:  a 16-byte vector holds 16 k, so MFMA m reads k = 64 (m >> 1) + 16 g + 8 (m & 1) + j (half m & 1 of vector m >> 1);
//           the A fragment of X is read from LDS at the SAME k, so each product meets its own x (the integer and one-hot probes of
//           tests/test_gpu_lm_rows_mfma.py change if the two maps differ)
//   fp8     each e4m3fn byte -> fp32 (v_cvt_pk_f32_fp8, exact) -> its upper 16 bits: e4m3fn is a subset of bf16, so the MFMA multiplies the
//           very values lm_gemv_w8_kernel multiplies; the per-channel scale multiplies the folded fp32 sum once
//   X       the chunk's rows b < B are staged once per block in LDS as bf16, [16 TM][1024], 16-byte slot s of row r at slot s ^ (r & 15)
//           (the 16 rows a ds_read_b128 of an A fragment touches land in 16 different bank groups); rows >= B are zero and never written out
//   fold    the four waves' accumulators go to LDS and are added in wave order 0, 1, 2, 3 by the thread that owns (b, n): no atomics
// Row b's result is a function of (W, scale, bias, X[b], resid[b], N, K) alone: the k split and the fold order do not read B, and an MFMA
// output element is the dot product of its own row and column.  HEAD keeps the logits fp32, writes them if asked and one (value, lowest
// index) maximum per block and row; lm_head_finalize_rows_kernel folds those per row.
constexpr int GEMM_KW = 256, GEMM_KC = 4 * GEMM_KW;

__device__ __forceinline__ bf16x8 w8_bf16x8(uint32_t a, uint32_t b) {            // 8 e4m3fn bytes (k ascending) as the 8 bf16 that equal them
    const uint32_t w[2] = {a, b};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], true);
        o[2 * e] = (__float_as_uint(lo[0]) >> 16) | (__float_as_uint(lo[1]) & 0xffff0000u);
        o[2 * e + 1] = (__float_as_uint(hi[0]) >> 16) | (__float_as_uint(hi[1]) & 0xffff0000u);
    }
    return __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
}

template <int TM, bool W8, bool HEAD>
__global__ __launch_bounds__(256) void lm_gemm_rows_kernel(const uint8_t* __restrict__ W, const float* __restrict__ wscale,
                                                           const uint16_t* __restrict__ X, int ldx, const uint16_t* __restrict__ bias,
                                                           const uint16_t* resid, int ldr, uint16_t* Y, int ldy, float* __restrict__ logits,
                                                           int ldl, float* __restrict__ part_v, int* __restrict__ part_i, int nparts, int B,
                                                           int N, int K) {
    constexpr int ROWS = 16 * TM, ES = W8 ? 1 : 2, U = W8 ? GEMM_KW / 64 : GEMM_KW / 32;   // 16-byte weight loads per lane and chunk
    constexpr int VR = GEMM_KC / 8, NP = ROWS / 2;                               // staging: 16-byte slots per row; rows per thread
    extern __shared__ __attribute__((aligned(16))) uint8_t gemm_lds[];
    uint4* xs = (uint4*)gemm_lds;                                                // [ROWS][VR], swizzled; 16 / 32 KB x 2
    float* red = (float*)gemm_lds;                                               // after the loop: [4 waves][TM][4][64]
    float* fin = red + 4 * TM * 256;                                             // HEAD: [ROWS][16] folded logits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const uint8_t* wr = W + (size_t)(n0 + ln < N ? n0 + ln : N - 1) * (size_t)K * ES;
    f32x4 acc[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sv = tid % VR, sr = tid / VR;                                      // staging: slot sv of rows sr, sr + 2, ...
    for (int i = tid; i < ROWS * VR; i += 256) xs[i] = make_uint4(0u, 0u, 0u, 0u);   // rows >= B stay zero
    uint4 xv[NP];
    u32x4 wv[U];
    auto issue = [&](int kb) {                                                   // x first: waiting for it leaves W in flight
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int b = sr + 2 * j;
            xv[j] = b < B && kb + sv * 8 < K ? *(const uint4*)(X + (size_t)b * ldx + kb + sv * 8) : make_uint4(0u, 0u, 0u, 0u);
        }
        const int kw = kb + wave * GEMM_KW;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kw + (W8 ? 64 * u + 16 * lg : 32 * u + 8 * lg);        // K % 64 == 0: a vector is inside K or past it as a whole
            wv[u] = k < K ? __builtin_nontemporal_load((const u32x4*)(wr + (size_t)k * ES)) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    issue(0);
    for (int kb = 0; kb < K; kb += GEMM_KC) {
        __syncthreads();                                                         // the zero fill / every wave is done with the previous chunk
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int b = sr + 2 * j;
            if (b < B) xs[b * VR + (sv ^ (b & 15))] = xv[j];
        }
        __syncthreads();
        u32x4 wc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) wc[u] = wv[u];
        if (kb + GEMM_KC < K) issue(kb + GEMM_KC);                               // the next chunk flies during this one's products
        const int kw = kb + wave * GEMM_KW;
#pragma unroll
        for (int m = 0; m < GEMM_KW / 32; ++m) {
            if (kw + 32 * m < K) {                                               // wave-uniform; LDS past K is stale
                bf16x8 bf;
                int kl;                                                          // this lane's first k inside the chunk
                if constexpr (W8) {
                    const u32x4 v = wc[m >> 1];
                    bf = (m & 1) ? w8_bf16x8(v.z, v.w) : w8_bf16x8(v.x, v.y);
                    kl = wave * GEMM_KW + 64 * (m >> 1) + 16 * lg + 8 * (m & 1);
                } else {
                    bf = __builtin_bit_cast(bf16x8, wc[m]);
                    kl = wave * GEMM_KW + 32 * m + 8 * lg;
                }
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    const int r = 16 * t + ln;
                    const bf16x8 af = __builtin_bit_cast(bf16x8, xs[r * VR + ((kl >> 3) ^ ln)]);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[t], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                                             // xs is read out: its memory becomes `red`
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * TM + t) * 4 + r) * 64 + lane] = acc[t][r];
    __syncthreads();
    // thread -> (b, n): accumulator element r of lane 16 g + n of tile t is row 16 t + 4 g + r, column n
#pragma unroll
    for (int o = tid; o < ROWS * 16; o += 256) {
        const int b = o >> 4, nl = o & 15, n = n0 + nl, t = b >> 4, g = (b & 15) >> 2, r = b & 3;
        const int at = (t * 4 + r) * 64 + 16 * g + nl;
        float s = red[at];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += red[w * TM * 256 + at];                // wave order
        if constexpr (HEAD) {
            fin[o] = s;
            if (logits && b < B && n < N) logits[(size_t)b * ldl + n] = s;
        } else if (b < B && n < N) {
            const float bs = bias ? bf2f(bias[n]) : 0.f;
            float v;
            if constexpr (W8) v = fmaf(s, wscale[n], bs);                        // the scale once, on the folded sum
            else v = s + bs;
            Y[(size_t)b * ldy + n] = resid ? f2bf(rbf(v) + bf2f(resid[(size_t)b * ldr + n])) : f2bf(v);   // two roundings
        }
    }
    if constexpr (HEAD) {
        __syncthreads();
        if (tid < B) {
            float best = fin[tid * 16];                                          // row n0 exists in every block
            int at = n0;
            for (int i = 1; i < 16; ++i)                                         // ascending index, strict >: the first maximum
                if (n0 + i < N && fin[tid * 16 + i] > best) { best = fin[tid * 16 + i]; at = n0 + i; }
            part_v[(size_t)tid * nparts + blockIdx.x] = best;
            part_i[(size_t)tid * nparts + blockIdx.x] = at;
        }
    }
}

}  // namespace rgn

using namespace rgn;

template <bool W8, bool ARGMAX, typename... Args>
static void launch_gemv_rows(int B, int N, hipStream_t st, Args... args) {
    const dim3 grid((N + 4 * ROWS_R - 1) / (4 * ROWS_R)), block(256);
    const size_t lds = (size_t)B * rows_kc<W8>() * sizeof(float);
    switch (B) {
#define RGN_ROWS_CASE(b) case b: hipLaunchKernelGGL((lm_gemv_rows_kernel<b, W8, ARGMAX>), grid, block, lds, st, args...); break;
        RGN_ROWS_CASE(2) RGN_ROWS_CASE(3) RGN_ROWS_CASE(4) RGN_ROWS_CASE(5) RGN_ROWS_CASE(6) RGN_ROWS_CASE(7) RGN_ROWS_CASE(8)
#undef RGN_ROWS_CASE
    }
}

// ---- the entries ------------------------------------------------------------------------------------------------------------------------
// Every operation is written once, over 1 <= B <= RGN_LM_MAX_BATCH rows, under the name of the public entry that called it (`who`, the
// prefix of its messages).  B == 1 launches the one-row kernels and reads no stride, so stride conditions bind from B = 2 on.
static inline bool dal16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static inline bool batch_ok(int B) { return B >= 1 && B <= RGN_LM_MAX_BATCH; }
static inline bool wide_ok(int B) { return B >= 1 && B <= RGN_LM_MAX_WIDE_BATCH; }      // the wide entries (batch_kernels="mfma")
static int bad(const char* who, const char* what) { snprintf(g_err, sizeof(g_err), "%s: %s", who, what); return RGN_E_BADARG; }

// The linear layer in either weight format: W8 reads e4m3fn bytes with `wscale`, else W is bf16 and wscale null.
template <bool W8>
static int gemv(const char* who, const void* W, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr,
                void* Y, int ldy, int B, int N, int K, void* stream) {
    if (!W || (W8 && !wscale) || !X || !Y || N < 1 || K < 64)
        return bad(who, W8 ? "bad argument (W8, wscale, X, Y non-null; N >= 1; K >= 64)" : "bad argument (W, X, Y non-null; N >= 1; K >= 64)");
    if (!batch_ok(B)) return bad(who, "B outside [1, 8]");
    if (K % (W8 ? 16 : 64)) return bad(who, W8 ? "K must be a multiple of 16" : "K must be a multiple of 64");
    if (B > 1 && (ldx % 8 || ldy % 8 || ldx < K || ldy < N || (resid && (ldr % 8 || ldr < N))))
        return bad(who, "strides must be multiples of 8, ldx >= K, ldy >= N, ldr >= N");
    if (!dal16(W) || !dal16(wscale) || !dal16(X) || (W8 && !dal16(Y)))
        return bad(who, W8 ? "W8, wscale, X and Y must be 16-byte aligned" : "W and X must be 16-byte aligned");
    if (((uintptr_t)Y | (uintptr_t)bias | (uintptr_t)resid) & 1u)
        return bad(who, W8 ? "bias and resid must be 2-byte aligned" : "Y, bias and resid must be 2-byte aligned");
    const uint16_t *x = (const uint16_t*)X, *bs = (const uint16_t*)bias, *rs = (const uint16_t*)resid;
    if (B > 1) {
        launch_gemv_rows<W8, false>(B, N, (hipStream_t)stream, (const uint8_t*)W, wscale, x, ldx, bs, rs, ldr, (uint16_t*)Y, ldy, (float*)nullptr, 0,
                                    (float*)nullptr, (int*)nullptr, 0, N, K);
        return check_launch("lm_gemv_rows_kernel");
    }
    if constexpr (W8) {
        constexpr int rows = 4 * W8_ROWS;
        hipLaunchKernelGGL((lm_gemv_w8_kernel<W8_ROWS, W8_U>), dim3((N + rows - 1) / rows), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)W,
                           wscale, x, bs, rs, (uint16_t*)Y, N, K);
    } else {
        hipLaunchKernelGGL((lm_gemv_kernel<false>), dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)W, x, bs, rs, (uint16_t*)Y,
                           (float*)nullptr, (float*)nullptr, (int*)nullptr, N, K);
    }
    return check_launch(W8 ? "lm_gemv_w8_kernel" : "lm_gemv_kernel");
}

// ---- the wide entries: 1 <= B <= RGN_LM_MAX_WIDE_BATCH rows on lm_gemm_rows_kernel, the same kernel at every B ------------------------------
template <bool W8, bool HEAD, typename... Args>
static void launch_gemm_rows(int B, int N, hipStream_t st, Args... args) {
    const dim3 grid((N + 15) / 16), block(256);
    if (B <= 16) hipLaunchKernelGGL((lm_gemm_rows_kernel<1, W8, HEAD>), grid, block, (size_t)16 * GEMM_KC * 2, st, args...);
    else hipLaunchKernelGGL((lm_gemm_rows_kernel<2, W8, HEAD>), grid, block, (size_t)32 * GEMM_KC * 2, st, args...);
}

template <bool W8>
static int gemm_rows(const char* who, const void* W, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr,
                     void* Y, int ldy, int B, int N, int K, void* stream) {
    if (!W || (W8 && !wscale) || !X || !Y || N < 1 || K < 64)
        return bad(who, W8 ? "bad argument (W8, wscale, X, Y non-null; N >= 1; K >= 64)" : "bad argument (W, X, Y non-null; N >= 1; K >= 64)");
    if (!wide_ok(B)) return bad(who, "B outside [1, 32]");
    if (K % 64) return bad(who, "K must be a multiple of 64");
    if (B > 1 && (ldx % 8 || ldy % 8 || ldx < K || ldy < N || (resid && (ldr % 8 || ldr < N))))
        return bad(who, "strides must be multiples of 8, ldx >= K, ldy >= N, ldr >= N");
    if (!dal16(W) || !dal16(wscale) || !dal16(X)) return bad(who, W8 ? "W8, wscale and X must be 16-byte aligned" : "W and X must be 16-byte aligned");
    if (((uintptr_t)Y | (uintptr_t)bias | (uintptr_t)resid) & 1u) return bad(who, "Y, bias and resid must be 2-byte aligned");
    launch_gemm_rows<W8, false>(B, N, (hipStream_t)stream, (const uint8_t*)W, wscale, (const uint16_t*)X, ldx, (const uint16_t*)bias,
                                (const uint16_t*)resid, ldr, (uint16_t*)Y, ldy, (float*)nullptr, 0, (float*)nullptr, (int*)nullptr, 0, B, N, K);
    return check_launch("lm_gemm_rows_kernel");
}

extern "C" {

int rgn_lm_gemv_bf16(const void* W, const void* x, const void* bias, const void* resid, void* y, int N, int K, void* stream) {
    return gemv<false>("lm_gemv", W, nullptr, x, 0, bias, resid, 0, y, 0, 1, N, K, stream);
}
int rgn_lm_gemv_bf16_rows(const void* W, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y, int ldy, int B, int N,
                          int K, void* stream) {
    return gemv<false>("lm_gemv_rows", W, nullptr, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream);
}
int rgn_lm_gemv_w8(const void* W8, const float* wscale, const void* x, const void* bias, const void* resid, void* y, int N, int K,
                   void* stream) {
    return gemv<true>("lm_gemv_w8", W8, wscale, x, 0, bias, resid, 0, y, 0, 1, N, K, stream);
}
int rgn_lm_gemv_w8_rows(const void* W8, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y,
                        int ldy, int B, int N, int K, void* stream) {
    return gemv<true>("lm_gemv_w8_rows", W8, wscale, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream);
}

static inline int head_parts(int V) { return (V + 3) / 4; }                 // lm_gemv_kernel<true>: 4 rows per block

size_t rgn_lm_head_workspace_bytes(int V) { return V < 1 ? 0 : (size_t)head_parts(V) * (sizeof(float) + sizeof(int)); }

static int head_argmax(const char* who, const void* W, const void* X, int ldx, int B, int V, int K, void* token_out, int token_stride,
                       float* logits_out, int ldl, void* workspace, size_t workspace_bytes, void* stream) {
    if (!W || !X || !token_out || !workspace || V < 1 || K < 64)
        return bad(who, "bad argument (W, X, token_out, workspace non-null; V >= 1; K >= 64)");
    if (!batch_ok(B)) return bad(who, "B outside [1, 8]");
    if (K % 64) return bad(who, "K must be a multiple of 64");
    if (B > 1 && (ldx % 8 || ldx < K || token_stride < 1 || (logits_out && ldl < V)))
        return bad(who, "ldx must be a multiple of 8 and >= K, token_stride >= 1, ldl >= V");
    if (!dal16(W) || !dal16(X)) return bad(who, "W and X must be 16-byte aligned");
    if (((uintptr_t)token_out & 7u) || ((uintptr_t)logits_out & 3u) || ((uintptr_t)workspace & 3u))
        return bad(who, "token_out must be 8-byte, logits_out and workspace 4-byte aligned");
    if (workspace_bytes < (size_t)B * rgn_lm_head_workspace_bytes(V)) return bad(who, "workspace smaller than B rgn_lm_head_workspace_bytes(V)");
    const int np = B == 1 ? head_parts(V) : (V + 4 * ROWS_R - 1) / (4 * ROWS_R);        // the blocks of the product, each with one maximum
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + (size_t)B * np);
    const hipStream_t st = (hipStream_t)stream;
    if (B == 1) {
        hipLaunchKernelGGL((lm_gemv_kernel<true>), dim3(np), dim3(256), 0, st, (const uint16_t*)W, (const uint16_t*)X, (const uint16_t*)nullptr,
                           (const uint16_t*)nullptr, (uint16_t*)nullptr, logits_out, pv, pi, V, K);
        hipLaunchKernelGGL(lm_head_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)pv, (const int*)pi, np, (int64_t*)token_out);
    } else {
        launch_gemv_rows<false, true>(B, V, st, (const uint8_t*)W, (const float*)nullptr, (const uint16_t*)X, ldx, (const uint16_t*)nullptr,
                                      (const uint16_t*)nullptr, 0, (uint16_t*)nullptr, 0, logits_out, ldl, pv, pi, np, V, K);
        hipLaunchKernelGGL(lm_head_finalize_rows_kernel, dim3(B), dim3(1024), 0, st, (const float*)pv, (const int*)pi, np, (int64_t*)token_out,
                           token_stride);
    }
    return check_launch(who);
}

int rgn_lm_head_argmax(const void* W, const void* x, int V, int K, void* token_out, float* logits_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return head_argmax("lm_head_argmax", W, x, 0, 1, V, K, token_out, 0, logits_out, 0, workspace, workspace_bytes, stream);
}
int rgn_lm_head_argmax_rows(const void* W, const void* X, int ldx, int B, int V, int K, void* token_out, int token_stride, float* logits_out,
                            int ldl, void* workspace, size_t workspace_bytes, void* stream) {
    return head_argmax("lm_head_argmax_rows", W, X, ldx, B, V, K, token_out, token_stride, logits_out, ldl, workspace, workspace_bytes, stream);
}

int rgn_lm_gemm_rows_bf16(const void* W, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y, int ldy, int B, int N,
                          int K, void* stream) {
    return gemm_rows<false>("lm_gemm_rows", W, nullptr, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream);
}
int rgn_lm_gemm_rows_w8(const void* W8, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y,
                        int ldy, int B, int N, int K, void* stream) {
    return gemm_rows<true>("lm_gemm_rows_w8", W8, wscale, X, ldx, bias, resid, ldr, Y, ldy, B, N, K, stream);
}

static inline int wide_parts(int V) { return (V + 15) / 16; }                // lm_gemm_rows_kernel: 16 rows per block

size_t rgn_lm_head_wide_workspace_bytes(int V, int B) {
    return V < 1 || !wide_ok(B) ? 0 : (size_t)B * wide_parts(V) * (sizeof(float) + sizeof(int));
}

int rgn_lm_head_argmax_wide(const void* W, const void* X, int ldx, int B, int V, int K, void* token_out, int token_stride, float* logits_out,
                            int ldl, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "lm_head_argmax_wide";
    if (!W || !X || !token_out || !workspace || V < 1 || K < 64)
        return bad(who, "bad argument (W, X, token_out, workspace non-null; V >= 1; K >= 64)");
    if (!wide_ok(B)) return bad(who, "B outside [1, 32]");
    if (K % 64) return bad(who, "K must be a multiple of 64");
    if (B > 1 && (ldx % 8 || ldx < K || token_stride < 1 || (logits_out && ldl < V)))
        return bad(who, "ldx must be a multiple of 8 and >= K, token_stride >= 1, ldl >= V");
    if (!dal16(W) || !dal16(X)) return bad(who, "W and X must be 16-byte aligned");
    if (((uintptr_t)token_out & 7u) || ((uintptr_t)logits_out & 3u) || ((uintptr_t)workspace & 3u))
        return bad(who, "token_out must be 8-byte, logits_out and workspace 4-byte aligned");
    if (workspace_bytes < rgn_lm_head_wide_workspace_bytes(V, B)) return bad(who, "workspace smaller than rgn_lm_head_wide_workspace_bytes(V, B)");
    const int np = wide_parts(V);
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + (size_t)B * np);
    const hipStream_t st = (hipStream_t)stream;
    launch_gemm_rows<false, true>(B, V, st, (const uint8_t*)W, (const float*)nullptr, (const uint16_t*)X, ldx, (const uint16_t*)nullptr,
                                  (const uint16_t*)nullptr, 0, (uint16_t*)nullptr, 0, logits_out, ldl, pv, pi, np, B, V, K);
    hipLaunchKernelGGL(lm_head_finalize_rows_kernel, dim3(B), dim3(1024), 0, st, (const float*)pv, (const int*)pi, np, (int64_t*)token_out,
                       B > 1 ? token_stride : 1);
    return check_launch(who);
}

// L rows of QKV into each of B caches from row row0[b] on.  The two public forms are its two edges: L rows into ONE cache (the prefill;
// lm_kv_append_kernel, which is also what one decoded row takes) and ONE row into each of B >= 2 caches (lm_kv_append_rows_kernel).
static int kv_append(const char* who, bool rows, const void* QKV, int ld, void* cache, size_t cache_stride, int cap, const int* row0, int B, int L,
                     int Hq, int Hkv, void* stream) {
    if (!QKV || !cache || !row0 || L < 1 || (!rows && row0[0] < 0) || Hq < 1 || Hkv < 1 || Hq > 1024 || Hkv > 1024 || ld < (Hq + 2 * Hkv) * 128 || ld % 8)
        return bad(who, rows ? "bad argument (QKV, cache, row0 non-null; 1 <= Hq, Hkv <= 1024; ld >= (Hq + 2 Hkv) 128, a multiple of 8)"
                             : "bad argument (QKV, cache non-null; L, row0 >= 0; 1 <= Hq, Hkv <= 1024; ld >= (Hq + 2 Hkv) 128, a multiple of 8)");
    if (!batch_ok(B)) return bad(who, "B outside [1, 8]");
    const int width = 2 * Hkv * 128;
    if (cap < 1 || cap > DEC_MAX_N || (B > 1 && (cache_stride % 8 || cache_stride < (size_t)cap * width)))
        return bad(who, rows ? "caches of 1 <= cap <= 4096 rows, cache_stride >= cap 2 Hkv 128 elements, a multiple of 8"
                             : "a cache of 1 <= cap <= 4096 rows");
    LmRows r{};
    for (int b = 0; b < B; ++b) {
        if (row0[b] < 0 || row0[b] > cap - L) return bad(who, rows ? "row0[b] outside [0, cap)" : "rows [row0, row0 + L) must lie in [0, cap)");
        r.v[b] = row0[b];
    }
    if (!dal16(QKV) || !dal16(cache)) return bad(who, "QKV and cache must be 16-byte aligned");
    if (B == 1) {
        const size_t items = (size_t)L * (width / 8), g = (items + 255) / 256;
        hipLaunchKernelGGL(lm_kv_append_kernel, dim3((unsigned)(g > 2048 ? 2048 : g)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV,
                           ld, Hq * 128, (uint16_t*)cache, r.v[0], L, width);
        return check_launch("lm_kv_append_kernel");
    }
    hipLaunchKernelGGL(lm_kv_append_rows_kernel, dim3((width / 8 + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)QKV, ld,
                       Hq * 128, (uint16_t*)cache, cache_stride, r, width);
    return check_launch("lm_kv_append_rows_kernel");
}

int rgn_lm_kv_append_bf16(const void* QKV, int ld, void* cache, int cap, int row0, int L, int Hq, int Hkv, void* stream) {
    if (L == 0) return 0;
    return kv_append("lm_kv_append", false, QKV, ld, cache, 0, cap, &row0, 1, L, Hq, Hkv, stream);
}
int rgn_lm_kv_append_bf16_rows(const void* QKV, int ld, void* cache, size_t cache_stride, int cap, const int* row0_host, int B, int Hq, int Hkv,
                               void* stream) {
    return kv_append("lm_kv_append_rows", true, QKV, ld, cache, cache_stride, cap, row0_host, B, 1, Hq, Hkv, stream);
}

size_t rgn_lm_decode_attention_workspace_bytes(int Hq, int n) {
    if (Hq < 1 || n < 1) return 0;
    return (size_t)Hq * ((n + DEC_SLICE - 1) / DEC_SLICE) * DEC_PART * sizeof(float);
}

static int decode_attention(const char* who, const void* Q, int ldq, const void* cache, size_t cache_stride, void* O, int ldo, const int* n_host,
                            int B, int Hq, int Hkv, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!Q || !cache || !O || !n_host || !workspace || Hkv < 1 || Hq < Hkv || Hq > 1024 || !(scale > 0.f) || !(scale < INFINITY))
        return bad(who, "bad argument (Q, cache, O, n, workspace non-null; 1 <= Hkv <= Hq <= 1024; 0 < scale < inf)");
    if (Hq % Hkv || Hq / Hkv > DEC_MAX_GROUP) return bad(who, "Hq % Hkv != 0 or Hq / Hkv > 8");
    if (!batch_ok(B)) return bad(who, "B outside [1, 8]");
    LmRows nb{};
    int nmax = 0;
    for (int b = 0; b < B; ++b) {
        if (n_host[b] < 1 || n_host[b] > DEC_MAX_N) return bad(who, "n[b] outside [1, 4096]");
        nb.v[b] = n_host[b];
        nmax = n_host[b] > nmax ? n_host[b] : nmax;
    }
    if (B > 1 && (ldq % 8 || ldo % 8 || ldq < Hq * 128 || ldo < Hq * 128 || cache_stride % 8 || cache_stride < (size_t)nmax * 2 * Hkv * 128))
        return bad(who, "strides must be multiples of 8, ldq and ldo >= Hq 128, cache_stride >= max n 2 Hkv 128");
    if (!dal16(Q) || !dal16(cache) || !dal16(O) || !dal16(workspace)) return bad(who, "Q, cache, O and workspace must be 16-byte aligned");
    const size_t one = rgn_lm_decode_attention_workspace_bytes(Hq, nmax);
    if (workspace_bytes < (size_t)B * one) return bad(who, "workspace smaller than B rgn_lm_decode_attention_workspace_bytes(Hq, max n)");
    const int ns = (nmax + DEC_SLICE - 1) / DEC_SLICE;
    const hipStream_t st = (hipStream_t)stream;
    if (B == 1) {
        hipLaunchKernelGGL(lm_decode_attention_kernel, dim3(ns, Hkv), dim3(256), 0, st, (const uint16_t*)Q, (const uint16_t*)cache, nmax, Hq, Hkv,
                           scale, (float*)workspace, ns);
        hipLaunchKernelGGL(lm_decode_merge_kernel, dim3(Hq), dim3(128), 0, st, (const float*)workspace, ns, (uint16_t*)O);
    } else {
        hipLaunchKernelGGL(lm_decode_attention_rows_kernel, dim3(ns, Hkv, B), dim3(256), 0, st, (const uint16_t*)Q, ldq, (const uint16_t*)cache,
                           cache_stride, nb, Hq, Hkv, scale, (float*)workspace, one / sizeof(float));
        hipLaunchKernelGGL(lm_decode_merge_rows_kernel, dim3(Hq, B), dim3(128), 0, st, (const float*)workspace, one / sizeof(float), nb,
                           (uint16_t*)O, ldo);
    }
    return check_launch(who);
}

int rgn_lm_decode_attention_bf16(const void* q, const void* cache, void* O, int n, int Hq, int Hkv, float scale, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return decode_attention("lm_decode_attention", q, 0, cache, 0, O, 0, &n, 1, Hq, Hkv, scale, workspace, workspace_bytes, stream);
}
int rgn_lm_decode_attention_bf16_rows(const void* Q, int ldq, const void* cache, size_t cache_stride, void* O, int ldo, const int* n_host, int B,
                                      int Hq, int Hkv, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    return decode_attention("lm_decode_attention_rows", Q, ldq, cache, cache_stride, O, ldo, n_host, B, Hq, Hkv, scale, workspace,
                            workspace_bytes, stream);
}

int rgn_lm_verify_attention_bf16(const void* Q, int ldq, const void* cache, void* O, int ldo, int n0, int R, int Hq, int Hkv, float scale,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "lm_verify_attention";
    if (!Q || !cache || !O || !workspace || Hkv < 1 || Hq < Hkv || Hq > 1024 || !(scale > 0.f) || !(scale < INFINITY))
        return bad(who, "bad argument (Q, cache, O, workspace non-null; 1 <= Hkv <= Hq <= 1024; 0 < scale < inf)");
    if (Hq % Hkv || Hq / Hkv > DEC_MAX_GROUP) return bad(who, "Hq % Hkv != 0 or Hq / Hkv > 8");
    if (R < 1 || R > RGN_LM_MAX_BATCH) return bad(who, "R outside [1, 8]");
    if (n0 < 1 || n0 > DEC_MAX_N - (R - 1)) return bad(who, "rows [n0, n0 + R) must lie in [1, 4096]: query r sees n0 + r cache rows");
    if (ldq % 8 || ldo % 8 || ldq < Hq * 128 || ldo < Hq * 128) return bad(who, "ldq and ldo must be multiples of 8 and >= Hq 128");
    if (!dal16(Q) || !dal16(cache) || !dal16(O) || !dal16(workspace)) return bad(who, "Q, cache, O and workspace must be 16-byte aligned");
    const int nmax = n0 + R - 1, ns = (nmax + DEC_SLICE - 1) / DEC_SLICE;
    const size_t one = rgn_lm_decode_attention_workspace_bytes(Hq, nmax);
    if (workspace_bytes < (size_t)R * one) return bad(who, "workspace smaller than R rgn_lm_decode_attention_workspace_bytes(Hq, n0 + R - 1)");
    LmRows nb{};
    for (int r = 0; r < R; ++r) nb.v[r] = n0 + r;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lm_verify_attention_kernel, dim3(ns, Hkv), dim3(256), 0, st, (const uint16_t*)Q, ldq, (const uint16_t*)cache, n0, R, Hq, Hkv,
                       scale, (float*)workspace, one / sizeof(float));
    hipLaunchKernelGGL(lm_decode_merge_rows_kernel, dim3(Hq, R), dim3(128), 0, st, (const float*)workspace, one / sizeof(float), nb, (uint16_t*)O,
                       ldo);
    return check_launch(who);
}

static int lookup_step(const char* who, void* seq, int n, int R, const void* head, int head_stride, int limit, int K, int max_ngram,
                       const void* guess, int guess_len, int L, void* result, void* seen, int V, void* stream) {
    if (!seq || !head || !result || head_stride < 1) return bad(who, "bad argument (seq, head, result non-null; head_stride >= 1)");
    if (R < 1 || R > LOOKUP_MAX_R) return bad(who, "R outside [1, 32]");
    if (K < 0 || K > LOOKUP_MAX_R - 1) return bad(who, "K outside [0, 31]");
    if (max_ngram < 1 || max_ngram > LOOKUP_MAX_NGRAM) return bad(who, "max_ngram outside [1, 8]");
    if (n < 1 || L < 0 || L > n || limit < n + R) return bad(who, "0 <= L <= n, n >= 1 and n + R <= limit: the step's R tokens end inside the run");
    if (guess ? guess_len < 0 : guess_len != 0) return bad(who, "guess_len >= 0 with a guess, 0 without");
    if (((uintptr_t)seq | (uintptr_t)head | (uintptr_t)result | (uintptr_t)guess) & 7u) return bad(who, "seq, head, guess and result must be 8-byte aligned");
    if (seen) {
        if (V < 1 || V > PICK_MAX_V) return bad(who, "1 <= V <= 1048576 with a byte map");
        hipLaunchKernelGGL(lm_lookup_step_mark_kernel, dim3(1), dim3(LOOKUP_T), 0, (hipStream_t)stream, (int64_t*)seq, n, R, (const int64_t*)head,
                           head_stride, limit, K, max_ngram, (const int64_t*)guess, guess_len, L, (int64_t*)result, (uint8_t*)seen, V);
        return check_launch("lm_lookup_step_mark_kernel");
    }
    hipLaunchKernelGGL(lm_lookup_step_kernel, dim3(1), dim3(LOOKUP_T), 0, (hipStream_t)stream, (int64_t*)seq, n, R, (const int64_t*)head, head_stride,
                       limit, K, max_ngram, (const int64_t*)guess, guess_len, L, (int64_t*)result);
    return check_launch("lm_lookup_step_kernel");
}

int rgn_lm_lookup_step(void* seq, int n, int R, const void* head, int head_stride, int limit, int K, int max_ngram, const void* guess,
                       int guess_len, int L, void* result, void* stream) {
    return lookup_step("lm_lookup_step", seq, n, R, head, head_stride, limit, K, max_ngram, guess, guess_len, L, result, nullptr, 0, stream);
}
int rgn_lm_lookup_step_mark(void* seq, int n, int R, const void* head, int head_stride, int limit, int K, int max_ngram, const void* guess,
                            int guess_len, int L, void* result, void* seen, int V, void* stream) {
    return lookup_step("lm_lookup_step_mark", seq, n, R, head, head_stride, limit, K, max_ngram, guess, guess_len, L, result, seen, V, stream);
}

int rgn_lm_seen_mark(const void* ids, int n, void* seen, int V, void* stream) {
    if (n == 0) return 0;
    if (!ids || !seen || n < 0 || V < 1) return fail(RGN_E_BADARG, "lm_seen_mark: bad argument (ids, seen non-null; n >= 0; V >= 1)");
    if ((uintptr_t)ids & 7u) return fail(RGN_E_BADARG, "lm_seen_mark: ids must be 8-byte aligned");
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(lm_seen_mark_kernel, dim3(g > 256 ? 256 : g), dim3(256), 0, (hipStream_t)stream, (const int64_t*)ids, n, (uint8_t*)seen, V);
    return check_launch("lm_seen_mark_kernel");
}

size_t rgn_lm_pick_workspace_bytes(int V) { return V < 1 ? 0 : (size_t)V * sizeof(float); }

// A pick block's PICK_LDS bytes of dynamic LDS are more than a kernel gets unasked: allowed once per kernel and device (of several GPUs).
static void pick_allow_lds(const void* kernel, bool (&done)[64]) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !done[dev]) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PICK_LDS);
        if (dev >= 0 && dev < 64) done[dev] = true;
    }
}

static int pick(const char* who, bool rows, bool wide, const float* logits, int ldl, int B, int V, void* seen, size_t seen_stride, float penalty,
                int sample, float temperature, int top_k, double top_p, const float* uniform, void* token_out, int token_stride,
                float* scores_out, int lds, void* workspace, size_t workspace_bytes, void* stream, bool verify = false,
                const void* drafts = nullptr) {
    if (!logits || !seen || !token_out || !workspace || V < 1 || V > PICK_MAX_V)
        return bad(who, "bad argument (logits, seen, token_out, workspace non-null; 1 <= V <= 1048576)");
    if (wide ? !wide_ok(B) : !batch_ok(B)) return bad(who, wide ? "B outside [1, 32]" : "B outside [1, 8]");
    if (B > 1 && (ldl < V || (scores_out && lds < V) || seen_stride < (size_t)V || token_stride < 1))
        return bad(who, "ldl >= V, lds >= V, seen_stride >= V, token_stride >= 1");
    if (!(penalty > 0.f) || !(penalty < INFINITY)) return bad(who, "the repetition penalty must be in (0, inf)");
    if (!(temperature > 0.f) || !(temperature < INFINITY)) return bad(who, "the temperature must be in (0, inf)");
    if (top_k < 0) return bad(who, "top_k must be >= 0 (0 = off)");
    if (!(top_p > 0.0) || !(top_p <= 1.0)) return bad(who, "top_p must be in (0, 1] (1 = off)");
    if (sample && !uniform) return bad(who, "sampling reads its uniforms from device memory (uniform non-null)");
    if (((uintptr_t)token_out & 7u) || (((uintptr_t)logits | (uintptr_t)scores_out | (uintptr_t)workspace | (uintptr_t)uniform) & 3u))
        return bad(who, "token_out must be 8-byte, logits, scores_out, workspace and uniform 4-byte aligned");
    if (scores_out) {                   // the spans [first element, last element of row B - 1] of the two matrices may not meet
        const uintptr_t z0 = (uintptr_t)logits, z1 = z0 + ((size_t)(B - 1) * ldl + V) * sizeof(float);
        const uintptr_t s0 = (uintptr_t)scores_out, s1 = s0 + ((size_t)(B - 1) * lds + V) * sizeof(float);
        if (rows && s0 < z1 && z0 < s1) return bad(who, "scores_out may not overlap the logits");
        if (s0 == z0) return bad(who, "scores_out may not be the logits");  // all rgn_lm_pick ever refused: its accepted set stays
    }
    if (workspace_bytes < (size_t)B * rgn_lm_pick_workspace_bytes(V)) return bad(who, "workspace smaller than B rgn_lm_pick_workspace_bytes(V)");
    static bool set_one[64] = {}, set_rows[64] = {}, set_verify[64] = {};
    float* s = scores_out ? scores_out : (float*)workspace;
    if (verify) {                                                                // one launch at every R; row 0 reads no draft
        if (B > 1 && (!drafts || ((uintptr_t)drafts & 7u))) return bad(who, "drafts must be non-null and 8-byte aligned when R > 1");
        pick_allow_lds((const void*)lm_pick_verify_kernel, set_verify);
        hipLaunchKernelGGL(lm_pick_verify_kernel, dim3(B), dim3(PICK_T), PICK_LDS, (hipStream_t)stream, logits, ldl, V, (const uint8_t*)seen,
                           (const int64_t*)drafts, penalty, sample ? 1 : 0, temperature, top_k, top_p, uniform, (int64_t*)token_out, token_stride, s,
                           scores_out ? (size_t)lds : (size_t)V);
        return check_launch("lm_pick_verify_kernel");
    }
    if (B == 1) {
        pick_allow_lds((const void*)lm_pick_kernel, set_one);
        hipLaunchKernelGGL(lm_pick_kernel, dim3(1), dim3(PICK_T), PICK_LDS, (hipStream_t)stream, logits, V, (uint8_t*)seen, penalty,
                           sample ? 1 : 0, temperature, top_k, top_p, uniform, (int64_t*)token_out, s);
        return check_launch("lm_pick_kernel");
    }
    pick_allow_lds((const void*)lm_pick_rows_kernel, set_rows);
    hipLaunchKernelGGL(lm_pick_rows_kernel, dim3(B), dim3(PICK_T), PICK_LDS, (hipStream_t)stream, logits, ldl, V, (uint8_t*)seen, seen_stride,
                       penalty, sample ? 1 : 0, temperature, top_k, top_p, uniform, (int64_t*)token_out, token_stride, s,
                       scores_out ? (size_t)lds : (size_t)V);
    return check_launch("lm_pick_rows_kernel");
}

int rgn_lm_pick(const float* logits, int V, void* seen, float penalty, int sample, float temperature, int top_k, double top_p,
                const float* uniform, void* token_out, float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
    return pick("lm_pick", false, false, logits, 0, 1, V, seen, 0, penalty, sample, temperature, top_k, top_p, uniform, token_out, 0, scores_out, 0, workspace,
                workspace_bytes, stream);
}
int rgn_lm_pick_rows(const float* logits, int ldl, int B, int V, void* seen, size_t seen_stride, float penalty, int sample, float temperature,
                     int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out, int lds,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return pick("lm_pick_rows", true, false, logits, ldl, B, V, seen, seen_stride, penalty, sample, temperature, top_k, top_p, uniform, token_out,
                token_stride, scores_out, lds, workspace, workspace_bytes, stream);
}
int rgn_lm_pick_wide(const float* logits, int ldl, int B, int V, void* seen, size_t seen_stride, float penalty, int sample, float temperature,
                     int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out, int lds,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return pick("lm_pick_wide", true, true, logits, ldl, B, V, seen, seen_stride, penalty, sample, temperature, top_k, top_p, uniform, token_out,
                token_stride, scores_out, lds, workspace, workspace_bytes, stream);
}
int rgn_lm_pick_verify(const float* logits, int ldl, int R, int V, const void* seen, const void* drafts, float penalty, int sample,
                       float temperature, int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out,
                       int lds, void* workspace, size_t workspace_bytes, void* stream) {
    return pick("lm_pick_verify", true, true, logits, ldl, R, V, const_cast<void*>(seen), (size_t)(V > 0 ? V : 0), penalty, sample, temperature, top_k,
                top_p, uniform, token_out, token_stride, scores_out, lds, workspace, workspace_bytes, stream, true, drafts);
}

}  // extern "C"
