// Image pre- and post-processing around the VAEs and the vision tower (rgn_image_*): the 8-bit work a host does with Pillow, numpy and
// torch, restated so that every output BYTE / bf16 / fp32 pattern equals the host's.  Integer or table arithmetic only, except the
// bf16 -> u8 map, which rounds where torch and numpy round (the file is built with -ffp-contract=off).  No atomics, no MFMA; every
// output element is written by exactly one thread from a fixed expression: a repeated call is bit-identical.
//
//   resample_x_kernel / resample_y_kernel   one separable pass of Pillow's 8-bit resampler (22-bit fixed point, int32 accumulator)
//   u8_to_nchw_kernel                       uint8 [H, W, 3] -> bf16 [1, 3, H, W] through a 256-entry table (the VAE's input)
//   patchify_kernel                         uint8 [H, W, 3] -> the vision tower's patch rows (fp32 [N, 1176] or bf16 [N, Kp], zero-padded)
//   bf16_to_u8_kernel                       a decoded image (padded pixel-major or NCHW bf16) -> uint8 [H, W, 3]
#include "common.h"

namespace rgn {
namespace {

constexpr int IMG_PREC = 22;                      // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int IMG_MAX_KSIZE = 4096;

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> IMG_PREC;                // arithmetic shift, as Pillow's clip8
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The table is device data the launcher cannot read: an entry that does not lie inside the input (first < 0, count < 0, count > ksize,
// first + count > n) reads nothing and stores 0.
__device__ __forceinline__ bool entry_ok(int first, int count, int ksize, int n) {
    return first >= 0 && count >= 0 && count <= ksize && first <= n - count;
}

// x pass: src [H, Wi, 3] -> dst [H, Wo, 3].  One thread = one output pixel (three accumulators over `count` consecutive input pixels).
__global__ __launch_bounds__(256) void resample_x_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int Wi, int Wo,
                                                         const int* __restrict__ bounds, const int* __restrict__ weights, int ksize) {
    const size_t total = (size_t)H * Wo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (size_t)Wo), x = (int)(i - (size_t)y * Wo);
        const int2 b = *(const int2*)(bounds + 2 * x);
        int a0 = 1 << (IMG_PREC - 1), a1 = a0, a2 = a0;
        if (entry_ok(b.x, b.y, ksize, Wi)) {
            const uint8_t* p = src + ((size_t)y * Wi + b.x) * 3;
            const int* w = weights + (size_t)x * ksize;
            for (int k = 0; k < b.y; ++k) {
                const int wk = w[k];
                a0 += (int)p[3 * k] * wk;
                a1 += (int)p[3 * k + 1] * wk;
                a2 += (int)p[3 * k + 2] * wk;
            }
        } else {
            a0 = a1 = a2 = 0;
        }
        uint8_t* o = dst + i * 3;
        o[0] = clip8(a0); o[1] = clip8(a1); o[2] = clip8(a2);
    }
}

// y pass: src [Hi, W, 3] -> dst [Ho, W, 3].  A row is W * 3 bytes whatever they mean; one thread = 4 consecutive bytes of an output row
// (one dword load per tap and one dword store where the row's bytes are dword-aligned, byte accesses otherwise and in a row's tail).
__global__ __launch_bounds__(256) void resample_y_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hi, int Ho, int rowb,
                                                         const int* __restrict__ bounds, const int* __restrict__ weights, int ksize) {
    const int qpr = (rowb + 3) >> 2;
    const size_t total = (size_t)Ho * qpr;
    const bool al = (rowb & 3) == 0;              // src and dst are 16-byte aligned: every row then starts on a dword
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / (size_t)qpr), c = (int)(i - (size_t)y * qpr) * 4;
        const int n = rowb - c < 4 ? rowb - c : 4;
        const int2 b = *(const int2*)(bounds + 2 * y);
        int a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = 1 << (IMG_PREC - 1);
        if (entry_ok(b.x, b.y, ksize, Hi)) {
            const uint8_t* p = src + (size_t)b.x * rowb + c;
            const int* w = weights + (size_t)y * ksize;
            if (al) {
                for (int k = 0; k < b.y; ++k) {
                    const int wk = w[k];
                    const uint32_t v = *(const uint32_t*)(p + (size_t)k * rowb);
                    a[0] += (int)(v & 255u) * wk;
                    a[1] += (int)((v >> 8) & 255u) * wk;
                    a[2] += (int)((v >> 16) & 255u) * wk;
                    a[3] += (int)(v >> 24) * wk;
                }
            } else {
                for (int k = 0; k < b.y; ++k) {
                    const int wk = w[k];
                    const uint8_t* q = p + (size_t)k * rowb;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n) a[e] += (int)q[e] * wk;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = 0;
        }
        uint8_t* o = dst + (size_t)y * rowb + c;
        if (al) {
            *(uint32_t*)o = (uint32_t)clip8(a[0]) | (uint32_t)clip8(a[1]) << 8 | (uint32_t)clip8(a[2]) << 16 | (uint32_t)clip8(a[3]) << 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) o[e] = clip8(a[e]);
        }
    }
}

// uint8 [H, W, 3] -> bf16 [3, H * W] through tab[256].  One thread = 8 consecutive pixels: 24 input bytes (three 8-byte loads), one
// 16-byte store per channel plane.  VEC needs H * W % 8 == 0 (every plane then starts 16-byte aligned); otherwise one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(256) void u8_to_nchw_kernel(const uint8_t* __restrict__ src, uint16_t* __restrict__ dst, size_t HW,
                                                         const uint16_t* __restrict__ tab) {
    __shared__ uint16_t t[256];
    t[threadIdx.x] = tab[threadIdx.x];
    __syncthreads();
    if (VEC) {
        const size_t groups = HW >> 3;
        for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
            const uint2* p = (const uint2*)(src + g * 24);
            const uint2 v0 = p[0], v1 = p[1], v2 = p[2];
            const uint32_t w[6] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y};
            uint32_t o[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b0 = (2 * j) * 3 + c, b1 = (2 * j + 1) * 3 + c;        // byte positions of pixels 2j, 2j + 1
                    const uint32_t lo = t[(w[b0 >> 2] >> ((b0 & 3) * 8)) & 255u], hi = t[(w[b1 >> 2] >> ((b1 & 3) * 8)) & 255u];
                    o[c][j] = lo | hi << 16;
                }
#pragma unroll
            for (int c = 0; c < 3; ++c) *(uint4*)(dst + (size_t)c * HW + g * 8) = make_uint4(o[c][0], o[c][1], o[c][2], o[c][3]);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.x * 256) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[(size_t)c * HW + i] = t[src[i * 3 + c]];
        }
    }
}

// Patch rows of the Qwen2-VL image processor (patch 14, merge 2, temporal 2, the frame duplicated): row n = ((bh * (gw / 2) + bw) * 2 + ih)
// * 2 + iw is the patch at (2 bh + ih, 2 bw + iw) of the gh x gw patch grid; column ((c * 2 + t) * 14 + dy) * 14 + dx = tab[c][byte].
// One thread = V consecutive columns of a row (one 16-byte store): V = 4 fp32, V = 8 bf16 with the columns [1176, Kp) zero.
constexpr int PATCH = 14, PATCH_K = 3 * 2 * PATCH * PATCH;
template <bool BF16>
__global__ __launch_bounds__(256) void patchify_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, int W, int gw, int N, int ldo,
                                                       const float* __restrict__ tab) {
    __shared__ float t[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) t[i] = tab[i];
    __syncthreads();
    constexpr int V = BF16 ? 8 : 4;
    const int vpr = ldo / V, hw = gw >> 1;
    const size_t total = (size_t)N * vpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int n = (int)(i / (size_t)vpr), col0 = (int)(i - (size_t)n * vpr) * V;
        const int iw = n & 1, ih = (n >> 1) & 1, blk = n >> 2, bh = blk / hw, bw = blk - bh * hw;
        const int py = (2 * bh + ih) * PATCH, px = (2 * bw + iw) * PATCH;
        float v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int col = col0 + e;
            float f = 0.f;
            if (col < PATCH_K) {
                const int c = col / (2 * PATCH * PATCH), r = col - c * (2 * PATCH * PATCH), s = r % (PATCH * PATCH);
                const int dy = s / PATCH, dx = s - dy * PATCH;
                f = t[c * 256 + src[((size_t)(py + dy) * W + px + dx) * 3 + c]];
            }
            v[e] = f;
        }
        if (BF16)
            *(uint4*)((uint16_t*)dst + (size_t)n * ldo + col0) = make_uint4(f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3]), f2bf_pk(v[4 % V], v[5 % V]),
                                                                            f2bf_pk(v[6 % V], v[7 % V]));
        else
            *(float4*)((float*)dst + (size_t)n * ldo + col0) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// torch's `(x * 0.5 + 0.5).clamp(0, 1)` on bf16 (each op rounds to bf16), then numpy's `(a * 255).round().astype(uint8)` on fp32.
__device__ __forceinline__ uint32_t unit_u8(uint16_t h) {
    float t = rbf(bf2f(h) * 0.5f);
    t = rbf(t + 0.5f);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return (uint32_t)(int)__builtin_rintf(t * 255.0f);          // round half to even, as numpy's
}

// One thread = 4 consecutive pixels = 12 output bytes (three dword stores; dst is 16-byte aligned).  PADDED: pixel (y, x) is the row
// (y + 1) * (W + 2) + x + 1 of X with `ld` bf16 per row, channels 0..2 (one 8-byte load); else X is [3, H * W] and VEC (H * W % 4 == 0)
// reads four pixels of a plane with one 8-byte load.  The last H * W % 4 pixels are done by the threads past the groups, a pixel each.
template <bool PADDED>
__device__ __forceinline__ void load_px(const uint16_t* __restrict__ X, int ld, int W, size_t HW, size_t p, uint16_t* c3) {
    if (PADDED) {
        const size_t y = p / (size_t)W, x = p - y * W;
        const uint2 v = *(const uint2*)(X + ((y + 1) * (size_t)(W + 2) + x + 1) * ld);
        c3[0] = (uint16_t)v.x; c3[1] = (uint16_t)(v.x >> 16); c3[2] = (uint16_t)v.y;
    } else {
        c3[0] = X[p]; c3[1] = X[HW + p]; c3[2] = X[2 * HW + p];
    }
}

template <bool PADDED, bool VEC>
__global__ __launch_bounds__(256) void bf16_to_u8_kernel(const uint16_t* __restrict__ X, int ld, uint8_t* __restrict__ dst, int W, size_t HW) {
    const size_t groups = HW >> 2, tail = HW & 3;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups + tail; g += (size_t)gridDim.x * 256) {
        if (g >= groups) {
            const size_t p = groups * 4 + (g - groups);
            uint16_t c3[3];
            load_px<PADDED>(X, ld, W, HW, p, c3);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[p * 3 + c] = (uint8_t)unit_u8(c3[c]);
            continue;
        }
        uint32_t b[12];
        if (!PADDED && VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint2 v = *(const uint2*)(X + (size_t)c * HW + g * 4);
                b[c] = unit_u8((uint16_t)v.x); b[3 + c] = unit_u8((uint16_t)(v.x >> 16));
                b[6 + c] = unit_u8((uint16_t)v.y); b[9 + c] = unit_u8((uint16_t)(v.y >> 16));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint16_t c3[3];
                load_px<PADDED>(X, ld, W, HW, g * 4 + j, c3);
#pragma unroll
                for (int c = 0; c < 3; ++c) b[3 * j + c] = unit_u8(c3[c]);
            }
        }
        uint32_t* o = (uint32_t*)(dst + g * 12);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = b[4 * j] | b[4 * j + 1] << 8 | b[4 * j + 2] << 16 | b[4 * j + 3] << 24;
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline unsigned grid_of(size_t items, unsigned cap) {
    const size_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
constexpr long long IMG_MAX_PIXELS = 1ll << 28;      // 16384 x 16384: every byte offset of an image stays far below 2^32

}  // namespace
}  // namespace rgn

using namespace rgn;

extern "C" {

int rgn_image_resample_u8(const void* src, int in_h, int in_w, void* dst, int out_h, int out_w, const void* bounds, const void* weights,
                          int ksize, int axis, void* stream) {
    if (!src || !dst || !bounds || !weights || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || ksize < 1 || ksize > IMG_MAX_KSIZE)
        return fail(RGN_E_BADARG, "image_resample_u8: bad argument (src, dst, bounds, weights non-null; sizes >= 1; 1 <= ksize <= 4096)");
    if (axis != 0 && axis != 1) return fail(RGN_E_BADARG, "image_resample_u8: axis must be 0 (x) or 1 (y)");
    if (axis == 0 ? in_h != out_h : in_w != out_w)
        return fail(RGN_E_BADARG, "image_resample_u8: one pass changes one dimension (axis 0: out_h == in_h; axis 1: out_w == in_w)");
    if (src == dst) return fail(RGN_E_BADARG, "image_resample_u8: src and dst must differ");
    if (!al16(src) || !al16(dst) || ((uintptr_t)bounds & 7u) || ((uintptr_t)weights & 3u))
        return fail(RGN_E_BADARG, "image_resample_u8: src and dst must be 16-byte aligned, bounds 8-byte, weights 4-byte aligned");
    if ((long long)in_h * in_w > IMG_MAX_PIXELS || (long long)out_h * out_w > IMG_MAX_PIXELS)
        return fail(RGN_E_UNSUPPORTED, "image_resample_u8: more than 2^28 pixels");
    if (axis == 0) {
        hipLaunchKernelGGL(resample_x_kernel, dim3(grid_of((size_t)out_h * out_w, 16384)), dim3(256), 0, (hipStream_t)stream,
                           (const uint8_t*)src, (uint8_t*)dst, in_h, in_w, out_w, (const int*)bounds, (const int*)weights, ksize);
        return check_launch("resample_x_kernel");
    }
    const int rowb = in_w * 3;
    hipLaunchKernelGGL(resample_y_kernel, dim3(grid_of((size_t)out_h * ((rowb + 3) / 4), 16384)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src, (uint8_t*)dst, in_h, out_h, rowb, (const int*)bounds, (const int*)weights, ksize);
    return check_launch("resample_y_kernel");
}

int rgn_image_u8_to_nchw_bf16(const void* src, void* dst, int H, int W, const void* table, void* stream) {
    if (!src || !dst || !table || H < 1 || W < 1) return fail(RGN_E_BADARG, "image_u8_to_nchw_bf16: bad argument (src, dst, table non-null; H, W >= 1)");
    if (!al16(src) || !al16(dst) || ((uintptr_t)table & 1u))
        return fail(RGN_E_BADARG, "image_u8_to_nchw_bf16: src and dst must be 16-byte aligned, table 2-byte aligned");
    if ((long long)H * W > IMG_MAX_PIXELS) return fail(RGN_E_UNSUPPORTED, "image_u8_to_nchw_bf16: more than 2^28 pixels");
    const size_t HW = (size_t)H * W;
    if (HW % 8 == 0)
        hipLaunchKernelGGL(u8_to_nchw_kernel<true>, dim3(grid_of(HW / 8, 16384)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                           (uint16_t*)dst, HW, (const uint16_t*)table);
    else
        hipLaunchKernelGGL(u8_to_nchw_kernel<false>, dim3(grid_of(HW, 16384)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                           (uint16_t*)dst, HW, (const uint16_t*)table);
    return check_launch("u8_to_nchw_kernel");
}

int rgn_image_patchify_u8(const void* src, int H, int W, const void* table, void* dst, int out_bf16, int ldo, void* stream) {
    if (!src || !dst || !table || H < 28 || W < 28 || H % 28 || W % 28)
        return fail(RGN_E_BADARG, "image_patchify_u8: bad argument (src, dst, table non-null; H, W positive multiples of 28)");
    if (out_bf16 != 0 && out_bf16 != 1) return fail(RGN_E_BADARG, "image_patchify_u8: out_bf16 must be 0 (fp32 rows) or 1 (padded bf16 rows)");
    if (out_bf16 ? (ldo < PATCH_K || ldo % 8) : ldo != PATCH_K)
        return fail(RGN_E_BADARG, "image_patchify_u8: ldo must be 1176 for fp32 rows, a multiple of 8 >= 1176 for bf16 rows");
    if (ldo > 65536) return fail(RGN_E_BADARG, "image_patchify_u8: ldo > 65536");
    if (!al16(dst) || ((uintptr_t)table & 3u)) return fail(RGN_E_BADARG, "image_patchify_u8: dst must be 16-byte aligned, table 4-byte aligned");
    if ((long long)H * W > IMG_MAX_PIXELS) return fail(RGN_E_UNSUPPORTED, "image_patchify_u8: more than 2^28 pixels");
    const int gw = W / PATCH, N = (H / PATCH) * gw;
    const size_t vecs = (size_t)N * (ldo / (out_bf16 ? 8 : 4));
    if (out_bf16)
        hipLaunchKernelGGL(patchify_kernel<true>, dim3(grid_of(vecs, 16384)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, dst, W, gw,
                           N, ldo, (const float*)table);
    else
        hipLaunchKernelGGL(patchify_kernel<false>, dim3(grid_of(vecs, 16384)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, dst, W, gw,
                           N, ldo, (const float*)table);
    return check_launch("patchify_kernel");
}

int rgn_image_bf16_to_u8(const void* X, int layout, int ld, void* dst, int H, int W, void* stream) {
    if (!X || !dst || H < 1 || W < 1) return fail(RGN_E_BADARG, "image_bf16_to_u8: bad argument (X, dst non-null; H, W >= 1)");
    if (layout != RGN_IMAGE_PADDED && layout != RGN_IMAGE_NCHW)
        return fail(RGN_E_BADARG, "image_bf16_to_u8: layout must be RGN_IMAGE_PADDED or RGN_IMAGE_NCHW");
    if (layout == RGN_IMAGE_PADDED && (ld < 4 || ld % 4)) return fail(RGN_E_BADARG, "image_bf16_to_u8: a padded image needs ld >= 4, a multiple of 4");
    if (!al16(dst) || !al16(X)) return fail(RGN_E_BADARG, "image_bf16_to_u8: X and dst must be 16-byte aligned");
    if ((long long)H * W > IMG_MAX_PIXELS || (long long)(H + 2) * (W + 2) * (layout == RGN_IMAGE_PADDED ? ld : 1) >= (1ll << 40))
        return fail(RGN_E_UNSUPPORTED, "image_bf16_to_u8: image too large");
    const size_t HW = (size_t)H * W;
    const dim3 g(grid_of(HW / 4 + 3, 16384));
    hipStream_t st = (hipStream_t)stream;
    if (layout == RGN_IMAGE_PADDED)
        hipLaunchKernelGGL((bf16_to_u8_kernel<true, false>), g, dim3(256), 0, st, (const uint16_t*)X, ld, (uint8_t*)dst, W, HW);
    else if (HW % 4 == 0)
        hipLaunchKernelGGL((bf16_to_u8_kernel<false, true>), g, dim3(256), 0, st, (const uint16_t*)X, ld, (uint8_t*)dst, W, HW);
    else
        hipLaunchKernelGGL((bf16_to_u8_kernel<false, false>), g, dim3(256), 0, st, (const uint16_t*)X, ld, (uint8_t*)dst, W, HW);
    return check_launch("bf16_to_u8_kernel");
}

}  // extern "C"
