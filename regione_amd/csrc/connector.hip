// Step1X-Edit's per-step `connector` ([EXT] Qwen2Connector: a two-block token refiner conditioned on the timestep, called once per CFG
// branch per computed step - Step1XEdit/inplace.py:514-516, Step1XEditV1P2/inplace.py:602-609).  Every projection is rgn_gemm_group, the
// embedders are rgn_gemv_bf16, the norms rgn_layer_norm_rows, the attention rgn_vision_attention_bf16 (Dp = 128) over a connector item
// table; this file holds the three row kernels the module adds around them:
//   masked_mean_rows_kernel   the pooled context: column means over the valid (leading) rows, rounded as the eager bf16 ops round
//   head_rms_norm_kernel      per-head RMSNorm (width 128) on the q and k columns of packed QKV rows, in place: rgn_qk_norm_rope_store
//                             without RoPE and without the slabs; bit-equal to rgn_rms_norm_rows on the heads as [L H, 128] rows
//   gate_resid_rows_kernel    y = resid + gate * p, the elementwise half of RGN_EPI_GATE_RESID: applies the per-step AdaLN gate to a
//                             projection that was computed once per edit
// All three stream HBM with 16-byte accesses, round where torch's eager ops round (the file is built with -ffp-contract=off), use no
// atomics and reduce in a fixed order: a repeated call is bit-identical.
#include "common.h"

namespace rgn {

__device__ __forceinline__ void widen8(const uint4 v, float (&f)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = __uint_as_float(w[k] << 16);
        f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}

// ---- out[c] = bf16(bf16(sum_{l < n_valid} x[l, c] / n_valid) * scale) --------------------------------------------------------------------
// Block = 64 column vectors (8 columns each) x 4 waves; wave w sums rows w, w + 4, ... in fp32, the four partials meet in LDS and are
// added as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(256) void masked_mean_rows_kernel(const uint16_t* __restrict__ x, int ldx, int d, int n_valid, float scale,
                                                               uint16_t* __restrict__ out) {
    __shared__ float part[4][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 8;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (c < d) {
#pragma unroll 4
        for (int l = wave; l < n_valid; l += 4) {
            float f[8];
            widen8(*(const uint4*)(x + (size_t)l * ldx + c), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += f[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[wave][e][lane] = s[e];
    __syncthreads();
    if (wave != 0 || c >= d) return;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = (part[0][e][lane] + part[1][e][lane]) + (part[2][e][lane] + part[3][e][lane]);
        o[e] = rbf(t / (float)n_valid) * scale;
    }
    *(uint4*)(out + c) = make_uint4(f2bf_pk(o[0], o[1]), f2bf_pk(o[2], o[3]), f2bf_pk(o[4], o[5]), f2bf_pk(o[6], o[7]));
}

// ---- per-head RMSNorm of the q and k columns, in place ------------------------------------------------------------------------------------
// One wave per row; 16 lanes hold one head (8 columns each), so a wave takes four heads per pass over the 2 H heads of q | k.  The sum of
// squares is added in the order of rms_norm_rows_kernel at d = 128 (norm.hip: two waves of 64 elements, xor butterfly 32 .. 1, then wave
// 0 + wave 1): element e = 8 lane + k of a half, so the strides 32, 16, 8 are lanes 4, 2, 1 apart and 4, 2, 1 are inside the lane; the
// halves are lanes 0-7 and 8-15.  Lanes of a pass past the last head recompute that head and store nothing.
__global__ __launch_bounds__(256) void head_rms_norm_kernel(uint16_t* __restrict__ QKV, int ld, const uint16_t* __restrict__ wq,
                                                            const uint16_t* __restrict__ wk, int L, int H, float eps) {
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= L) return;                                  // wave-uniform
    uint16_t* r = QKV + (size_t)row * ld + sub * 8;
    float fq[8], fk[8];
    widen8(*(const uint4*)(wq + sub * 8), fq);
    widen8(*(const uint4*)(wk + sub * 8), fk);
    const int nh = 2 * H;
    for (int h0 = 0; h0 < nh; h0 += 4) {
        const bool ok = h0 + grp < nh;
        const int h = ok ? h0 + grp : nh - 1;
        uint16_t* p = r + (size_t)h * 128;
        float x[8], t[8];
        widen8(*(const uint4*)p, x);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float s = x[k] * x[k];
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 1, 64);
            t[k] = s;
        }
        const float a0 = t[0] + t[4], a1 = t[1] + t[5], a2 = t[2] + t[6], a3 = t[3] + t[7];
        const float half = (a0 + a2) + (a1 + a3);
        const float other = __shfl_xor(half, 8, 64);
        const float lo = sub < 8 ? half : other, hi = sub < 8 ? other : half;
        const float rinv = 1.0f / sqrtf((lo + hi) / 128.0f + eps);
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = rbf(x[k] * rinv) * (h < H ? fq[k] : fk[k]);
        if (ok) *(uint4*)p = make_uint4(f2bf_pk(o[0], o[1]), f2bf_pk(o[2], o[3]), f2bf_pk(o[4], o[5]), f2bf_pk(o[6], o[7]));
    }
}

// ---- y[m, n] = bf16(f32(resid[m, n]) + f32(bf16(gate[n] * p[m, n]))): one thread per 8 columns; y may be resid (each thread reads its
// vector before it writes it) ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_resid_rows_kernel(const uint16_t* __restrict__ p, int ldp, const uint16_t* __restrict__ gate,
                                                              const uint16_t* resid, int ldr, uint16_t* y, int ldy, int M, int N) {
    const int vpr = N / 8;
    const size_t nv = (size_t)M * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / vpr), c = (int)(i - (size_t)m * vpr) * 8;
        float pf[8], gf[8], rf[8], o[8];
        widen8(*(const uint4*)(p + (size_t)m * ldp + c), pf);
        widen8(*(const uint4*)(gate + c), gf);
        widen8(*(const uint4*)(resid + (size_t)m * ldr + c), rf);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = rf[e] + rbf(gf[e] * pf[e]);
        *(uint4*)(y + (size_t)m * ldy + c) = make_uint4(f2bf_pk(o[0], o[1]), f2bf_pk(o[2], o[3]), f2bf_pk(o[4], o[5]), f2bf_pk(o[6], o[7]));
    }
}

}  // namespace rgn

using namespace rgn;

extern "C" {

static inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int rgn_masked_mean_rows(const void* x, int ldx, int L, int d, int n_valid, float scale, void* out, void* stream) {
    if (!x || !out || L < 1 || d < 8 || d % 8 || ldx < d || ldx % 8 || n_valid < 1 || n_valid > L || !(scale == scale) || scale == INFINITY ||
        scale == -INFINITY)
        return fail(RGN_E_BADARG, "masked_mean_rows: bad argument (x, out non-null; L >= 1; d a positive multiple of 8; ldx >= d, a multiple "
                                  "of 8; 1 <= n_valid <= L; scale finite)");
    if (!al16(x) || !al16(out)) return fail(RGN_E_BADARG, "masked_mean_rows: x and out must be 16-byte aligned");
    hipLaunchKernelGGL(masked_mean_rows_kernel, dim3((d / 8 + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, d, n_valid,
                       scale, (uint16_t*)out);
    return check_launch("masked_mean_rows_kernel");
}

int rgn_head_rms_norm_bf16(void* QKV, int ld, const void* wq, const void* wk, int L, int H, float eps, void* stream) {
    if (L == 0) return 0;
    if (!QKV || !wq || !wk || L < 0 || H < 1 || H > 1024 || ld < 3 * H * 128 || ld % 8 || !(eps >= 0.f) || eps == INFINITY)
        return fail(RGN_E_BADARG, "head_rms_norm: bad argument (QKV, wq, wk non-null; L >= 0; 1 <= H <= 1024; ld >= 3 H 128, a multiple of 8; "
                                  "0 <= eps < inf)");
    if (!al16(QKV) || !al16(wq) || !al16(wk)) return fail(RGN_E_BADARG, "head_rms_norm: QKV, wq and wk must be 16-byte aligned");
    hipLaunchKernelGGL(head_rms_norm_kernel, dim3((L + 3) / 4), dim3(256), 0, (hipStream_t)stream, (uint16_t*)QKV, ld, (const uint16_t*)wq,
                       (const uint16_t*)wk, L, H, eps);
    return check_launch("head_rms_norm_kernel");
}

int rgn_gate_resid_rows(const void* p, int ldp, const void* gate, const void* resid, int ldr, void* y, int ldy, int M, int N, void* stream) {
    if (M == 0) return 0;
    if (!p || !gate || !resid || !y || M < 0 || N < 8 || N % 8 || ldp < N || ldr < N || ldy < N || ldp % 8 || ldr % 8 || ldy % 8)
        return fail(RGN_E_BADARG, "gate_resid_rows: bad argument (p, gate, resid, y non-null; M >= 0; N a positive multiple of 8; row strides "
                                  ">= N, multiples of 8)");
    if (!al16(p) || !al16(gate) || !al16(resid) || !al16(y)) return fail(RGN_E_BADARG, "gate_resid_rows: p, gate, resid and y must be 16-byte aligned");
    const size_t g = ((size_t)M * (N / 8) + 255) / 256;
    hipLaunchKernelGGL(gate_resid_rows_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)p, ldp,
                       (const uint16_t*)gate, (const uint16_t*)resid, ldr, (uint16_t*)y, ldy, M, N);
    return check_launch("gate_resid_rows_kernel");
}

}  // extern "C"
