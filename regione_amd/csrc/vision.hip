// Vision tower of the Qwen2.5-VL prompt encoder ([EXT] transformers Qwen2_5_VisionTransformerPretrainedModel; SURVEY.md section 8 row f4:
// `encode_prompt` of Qwen-Image-Edit runs it over the condition images).  Every projection, the patch embedding included, is rgn_gemm_group,
// the norms are rgn_rms_norm_rows, the MLP product is rgn_swiglu_bf16; this file holds what the tower adds around them:
//   vision_attention_kernel   non-causal self-attention over packed segments (windows, or one segment per image), read straight from the
//                             fused QKV GEMM output [L, 3 H Dp] -> O [L, H Dp] on the tile core of attn_tile.h.  Dp = the head width
//                             padded with zero columns to a multiple of 32 (the real tower's 80 runs as 96); scale is the caller's
//   vision_rope_kernel        apply_rotary_pos_emb_vision on the q and k columns of that buffer, in place: fp32 products and sum, one
//                             rounding to bf16; pad and V columns are not written
//   gelu_erf_kernel           nn.GELU() (the exact erf form) of the patch merger, one rounding
//   cast_pad_rows_kernel      `pixel_values.to(bfloat16)` with zero columns appended, so the patch-embedding convolution is one GEMM
// Row kernels round where torch's eager ops round (the file is built with -ffp-contract=off); every reduction has a fixed order.
#include "attn_tile.h"

namespace rgn {

// ---- attention over packed segments ---------------------------------------------------------------------------------------------------
// Block = one head x one item of the host-built table items[n][4] = (q0, n_q, k_lo, k_hi): queries [q0, q0 + n_q), n_q <= 64, which all
// attend to the keys [k_lo, k_hi).  Queries and keys are related through the item alone: the vision tower names the segment of its queries
// (a window, an image), the Step1X connector the valid keys for runs of valid rows and key 0 alone for runs of padded rows.  Keys outside
// [k_lo, k_hi) are never staged; keys of the last tile past k_hi are masked to -inf.  The first tile starts at k_lo < k_hi, a key every
// query of the item attends to, so it holds a valid key for every query (the invariant of AttnTile::step).  Lanes past n_q compute on the item's last query and store nothing.  An item that does not lie inside [0, L) is
// skipped as a whole (the table is device data the launcher cannot read).
template <int D>
__global__ __launch_bounds__(256) void vision_attention_kernel(const uint16_t* __restrict__ QKV, uint16_t* __restrict__ O, int L, int H,
                                                               float scale, const int* __restrict__ items) {
    using T = AttnTile<D>;
    __shared__ __attribute__((aligned(16))) uint16_t kl[T::K_LDS];
    __shared__ __attribute__((aligned(16))) uint16_t vl[T::V_LDS];
    const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int4 it = *(const int4*)(items + 4 * (size_t)blockIdx.x);
    const int q0 = it.x, nq = it.y, klo = it.z, khi = it.w;
    if (q0 < 0 || nq < 1 || nq > T::BQ || q0 > L - nq || klo < 0 || khi > L || klo >= khi) return;      // block-uniform
    const size_t ld = (size_t)3 * H * D, ldo = (size_t)H * D;
    const uint16_t* Qh = QKV + (size_t)h * D;
    const uint16_t* Kh = QKV + (size_t)(H + h) * D;
    const uint16_t* Vh = QKV + (size_t)(2 * H + h) * D;
    const int qr = (tid >> 6) * 16 + li;
    const bool qok = qr < nq;
    const int qi = q0 + (qok ? qr : nq - 1);
    T tile;
    tile.init(Qh + (size_t)qi * ld, g);
    constexpr float L2E = 1.4426950408889634f;
    for (int k0 = klo; k0 < khi; k0 += T::BK) {
        __syncthreads();                               // the previous tile is consumed
        T::stage(kl, vl, Kh, Vh, ld, tid, [&](int kk) { return k0 + kk < khi ? k0 + kk : -1; });
        __syncthreads();
        tile.step(kl, vl, li, g, L2E, [&](const float (&s)[8], float (&sc)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sc[e] = k0 + T::key_of_slot(g, e) < khi ? s[e] * scale : -INFINITY;
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

// ---- vision RoPE, in place: one thread owns channels [c, c + 4) and [D/2 + c, D/2 + c + 4) of one (row, head), the two halves that
// rotate_half exchanges.  out = bf16(f32(x) cos + f32(rotate_half(x)) sin): two fp32 products, their fp32 sum, one rounding ------------
__global__ __launch_bounds__(256) void vision_rope_kernel(uint16_t* __restrict__ QKV, int ld, const float* __restrict__ cosT,
                                                          const float* __restrict__ sinT, int L, int heads, int D, int Dp) {
    const int half = D / 2, vph = half / 4;
    const size_t n = (size_t)L * heads * vph;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % vph) * 4;
        const size_t rh = i / vph;
        const int row = (int)(rh / heads), hd = (int)(rh - (size_t)row * heads);
        uint16_t* x = QKV + (size_t)row * ld + (size_t)hd * Dp + c;
        const float* cr = cosT + (size_t)row * D + c;
        const float* sr = sinT + (size_t)row * D + c;
        const uint2 xa = *(const uint2*)x, xb = *(const uint2*)(x + half);
        const float4 ca = *(const float4*)cr, cb = *(const float4*)(cr + half), sa = *(const float4*)sr, sb = *(const float4*)(sr + half);
        const float a[4] = {bf2f((uint16_t)xa.x), bf2f((uint16_t)(xa.x >> 16)), bf2f((uint16_t)xa.y), bf2f((uint16_t)(xa.y >> 16))};
        const float b[4] = {bf2f((uint16_t)xb.x), bf2f((uint16_t)(xb.x >> 16)), bf2f((uint16_t)xb.y), bf2f((uint16_t)(xb.y >> 16))};
        const float c1[4] = {ca.x, ca.y, ca.z, ca.w}, c2[4] = {cb.x, cb.y, cb.z, cb.w};
        const float s1[4] = {sa.x, sa.y, sa.z, sa.w}, s2[4] = {sb.x, sb.y, sb.z, sb.w};
        float lo[4], hi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = a[e] * c1[e] + (-b[e]) * s1[e];
            hi[e] = b[e] * c2[e] + a[e] * s2[e];
        }
        *(uint2*)x = make_uint2(f2bf_pk(lo[0], lo[1]), f2bf_pk(lo[2], lo[3]));
        *(uint2*)(x + half) = make_uint2(f2bf_pk(hi[0], hi[1]), f2bf_pk(hi[2], hi[3]));
    }
}

// ---- nn.GELU(): 0.5 x (1 + erf(x / sqrt 2)) in fp32, one rounding ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gelu_erf_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = bf2f(x[i]);
        y[i] = f2bf(v * 0.5f * (1.0f + erff(v * 0.70710678118654752440f)));
    }
}

// ---- y[m, :K] = bf16(x[m, :K]), y[m, K:Kp] = 0: one thread per 8 output columns --------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(256) void cast_pad_rows_kernel(const Src* __restrict__ x, int ldx, uint16_t* __restrict__ y, int M, int K, int Kp) {
    const int vpr = Kp / 8;
    const size_t nv = (size_t)M * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const int m = (int)(i / vpr), c = (int)(i - (size_t)m * vpr) * 8;
        const Src* xr = x + (size_t)m * ldx;
        uint16_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            uint16_t w = 0;
            if (c + e < K) {
                if constexpr (sizeof(Src) == 4) w = f2bf(xr[c + e]);
                else w = xr[c + e];
            }
            v[e] = w;
        }
        *(uint4*)(y + (size_t)m * Kp + c) = make_uint4(v[0] | (uint32_t)v[1] << 16, v[2] | (uint32_t)v[3] << 16, v[4] | (uint32_t)v[5] << 16,
                                                       v[6] | (uint32_t)v[7] << 16);
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

int rgn_vision_attention_bf16(const void* QKV, void* O, int L, int H, int Dp, float scale, const int* items, int n_items, void* stream) {
    if (n_items == 0) return 0;
    if (!QKV || !O || !items || L < 1 || H < 1 || H > 1024 || n_items < 0 || !(scale > 0.f) || !(scale < INFINITY))
        return fail(RGN_E_BADARG, "vision_attention: bad argument (QKV, O, items non-null; L >= 1; 1 <= H <= 1024; n_items >= 0; 0 < scale < inf)");
    if (Dp != 32 && Dp != 64 && Dp != 96 && Dp != 128) return fail(RGN_E_UNSUPPORTED, "vision_attention: Dp must be 32, 64, 96 or 128");
    if (!al16(QKV) || !al16(O) || !al16(items)) return fail(RGN_E_BADARG, "vision_attention: QKV, O and items must be 16-byte aligned");
    const dim3 grid(n_items, H);
    const hipStream_t st = (hipStream_t)stream;
    const uint16_t* q = (const uint16_t*)QKV;
    uint16_t* o = (uint16_t*)O;
    if (Dp == 32) hipLaunchKernelGGL((vision_attention_kernel<32>), grid, dim3(256), 0, st, q, o, L, H, scale, items);
    else if (Dp == 64) hipLaunchKernelGGL((vision_attention_kernel<64>), grid, dim3(256), 0, st, q, o, L, H, scale, items);
    else if (Dp == 96) hipLaunchKernelGGL((vision_attention_kernel<96>), grid, dim3(256), 0, st, q, o, L, H, scale, items);
    else hipLaunchKernelGGL((vision_attention_kernel<128>), grid, dim3(256), 0, st, q, o, L, H, scale, items);
    return check_launch("vision_attention_kernel");
}

int rgn_vision_rope_bf16(void* QKV, int ld, const float* cos, const float* sin, int L, int H, int D, int Dp, void* stream) {
    if (!QKV || !cos || !sin || L < 1 || H < 1 || H > 1024 || D < 8 || D % 8 || Dp < D || Dp % 32 || ld < 3 * H * Dp || ld % 8)
        return fail(RGN_E_BADARG, "vision_rope: bad argument (QKV, cos, sin non-null; L >= 1; 1 <= H <= 1024; D a positive multiple of 8; "
                                  "Dp >= D a multiple of 32; ld >= 3 H Dp, a multiple of 8)");
    if (!al16(QKV) || !al16(cos) || !al16(sin)) return fail(RGN_E_BADARG, "vision_rope: QKV, cos and sin must be 16-byte aligned");
    hipLaunchKernelGGL(vision_rope_kernel, dim3(grid_of((size_t)L * 2 * H * (D / 8), 4096)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)QKV,
                       ld, cos, sin, L, 2 * H, D, Dp);
    return check_launch("vision_rope_kernel");
}

int rgn_gelu_erf_bf16(const void* x, void* y, size_t n, void* stream) {
    if (n == 0) return 0;
    if (!x || !y) return fail(RGN_E_BADARG, "gelu_erf: null pointer");
    hipLaunchKernelGGL(gelu_erf_kernel, dim3(grid_of(n, 2048)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, (uint16_t*)y, n);
    return check_launch("gelu_erf_kernel");
}

int rgn_cast_pad_rows(const void* x, int x_dtype, int ldx, void* y, int M, int K, int Kp, void* stream) {
    if (M == 0) return 0;
    if (!x || !y || M < 0 || K < 1 || Kp < K || Kp % 8 || ldx < K || (x_dtype != RGN_F32 && x_dtype != RGN_BF16))
        return fail(RGN_E_BADARG, "cast_pad_rows: bad argument (x, y non-null; K >= 1; Kp >= K a multiple of 8; ldx >= K; x_dtype fp32 or bf16)");
    if (!al16(y)) return fail(RGN_E_BADARG, "cast_pad_rows: y must be 16-byte aligned");
    const dim3 grid(grid_of((size_t)M * (Kp / 8), 4096));
    if (x_dtype == RGN_F32)
        hipLaunchKernelGGL((cast_pad_rows_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, (uint16_t*)y, M, K, Kp);
    else
        hipLaunchKernelGGL((cast_pad_rows_kernel<uint16_t>), grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x, ldx, (uint16_t*)y, M, K, Kp);
    return check_launch("cast_pad_rows_kernel");
}

}  // extern "C"
