// LoRA merge into a bf16 weight (rgn_lora_merge_bf16): dst = bf16(W + sum_t scale_t * B_t A_t), adoption-time work (never on the per-step
// path).  fp32 VALU FMAs in a fixed order, one rounding to bf16; no atomics, no MFMA (the merge of a whole FLUX trunk is a second of
// fp32 FMA next to a weight stream of the same order).
//
// One workgroup of 256 threads owns a 64-row x 256-column tile of W; a thread owns 8 rows x 8 consecutive columns (one 16-byte vector
// per row), loads them once, keeps them in fp32 registers over all terms and stores them once - the in-place form (dst == W) is
// therefore safe.  A and B travel through LDS in chunks of 16 ranks: the A chunk [16, 256] is shared by the tile's 64 rows, the B chunk
// [16, 64] by its 256 columns.
#include "common.h"

namespace rgn {
namespace {

constexpr int LM_TN = 64, LM_TK = 256, LM_RC = 16;

struct LoraTerms {
    rgn_lora_term t[RGN_LORA_MAX_TERMS];
    int n;
};

__global__ __launch_bounds__(256) void lora_merge_kernel(uint16_t* dst, int ldd, const uint16_t* W, int ldw, int N, int K, LoraTerms terms) {
    __shared__ __attribute__((aligned(16))) float sA[LM_RC][LM_TK];
    __shared__ __attribute__((aligned(16))) float sB[LM_RC][LM_TN];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int k0 = blockIdx.x * LM_TK, n0 = blockIdx.y * LM_TN;
    const int k = k0 + tx * 8, nb = n0 + ty * 8;
    const bool kin = k < K;                                   // K % 8 == 0: a thread's 8 columns are all inside or all outside

    float t[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (kin && nb + i < N) v = *reinterpret_cast<const uint4*>(W + (size_t)(nb + i) * ldw + k);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[i][2 * j] = __uint_as_float(w[j] << 16);
            t[i][2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
    }

    for (int term = 0; term < terms.n; ++term) {
        const float* __restrict__ A = terms.t[term].A;
        const float* __restrict__ B = terms.t[term].B;
        const int R = terms.t[term].r;
        const float scale = terms.t[term].scale;
        float acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
        for (int rc = 0; rc < R; rc += LM_RC) {
            __syncthreads();                                  // the previous chunk has been read by every thread
#pragma unroll
            for (int j = 0; j < LM_RC * LM_TK / 4 / 256; ++j) {
                const int idx = tid + j * 256, rr = idx / (LM_TK / 4), c = (idx % (LM_TK / 4)) * 4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rc + rr < R && k0 + c < K) a = *reinterpret_cast<const float4*>(A + (size_t)(rc + rr) * K + k0 + c);
                *reinterpret_cast<float4*>(&sA[rr][c]) = a;
            }
#pragma unroll
            for (int j = 0; j < LM_RC * LM_TN / 256; ++j) {
                const int idx = tid + j * 256, rr = idx / LM_TN, nn = idx % LM_TN;
                sB[rr][nn] = (rc + rr < R && n0 + nn < N) ? B[(size_t)(n0 + nn) * R + rc + rr] : 0.f;
            }
            __syncthreads();
            const int lim = R - rc < LM_RC ? R - rc : LM_RC;
            for (int rr = 0; rr < lim; ++rr) {                // r ascending: the order of the contract
                const float4 a0 = *reinterpret_cast<const float4*>(&sA[rr][tx * 8]), a1 = *reinterpret_cast<const float4*>(&sA[rr][tx * 8 + 4]);
                const float4 b0 = *reinterpret_cast<const float4*>(&sB[rr][ty * 8]), b1 = *reinterpret_cast<const float4*>(&sB[rr][ty * 8 + 4]);
                const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fmaf(b[i], a[j], acc[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) t[i][j] = __builtin_fmaf(scale, acc[i][j], t[i][j]);
    }

    if (!kin) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (nb + i >= N) break;
        uint4 v;
        v.x = f2bf_pk(t[i][0], t[i][1]);
        v.y = f2bf_pk(t[i][2], t[i][3]);
        v.z = f2bf_pk(t[i][4], t[i][5]);
        v.w = f2bf_pk(t[i][6], t[i][7]);
        *reinterpret_cast<uint4*>(dst + (size_t)(nb + i) * ldd + k) = v;
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace rgn

using namespace rgn;

extern "C" {

int rgn_lora_merge_bf16(void* dst, int ldd, const void* W, int ldw, int N, int K, const rgn_lora_term* terms, int n_terms, void* stream) {
    if (N == 0) return 0;
    if (!dst || !W || !terms || N < 0 || K < 8 || K % 8 || ldd < K || ldw < K || ldd % 8 || ldw % 8)
        return fail(RGN_E_BADARG, "lora_merge: bad argument (dst, W, terms non-null; N >= 0; K a positive multiple of 8; ldd, ldw >= K, "
                                  "multiples of 8)");
    if (n_terms < 1 || n_terms > RGN_LORA_MAX_TERMS) return fail(RGN_E_BADARG, "lora_merge: n_terms must be 1..8");
    if (!al16(dst) || !al16(W)) return fail(RGN_E_BADARG, "lora_merge: dst and W must be 16-byte aligned");
    if (dst == W && ldd != ldw) return fail(RGN_E_BADARG, "lora_merge: the in-place form (dst == W) needs ldd == ldw");
    LoraTerms lt;
    lt.n = n_terms;
    for (int i = 0; i < n_terms; ++i) {
        if (!terms[i].A || !terms[i].B) return fail(RGN_E_BADARG, "lora_merge: a term's A and B must be non-null");
        if (terms[i].r < 1 || terms[i].r > RGN_LORA_MAX_RANK) return fail(RGN_E_BADARG, "lora_merge: a term's rank r must be 1..1024");
        if (!al16(terms[i].A) || ((uintptr_t)terms[i].B & 3u)) return fail(RGN_E_BADARG, "lora_merge: A must be 16-byte aligned, B 4-byte aligned");
        lt.t[i] = terms[i];
    }
    const long long gy = ((long long)N + LM_TN - 1) / LM_TN;
    if (gy > 65535) return fail(RGN_E_UNSUPPORTED, "lora_merge: N > 65535 * 64 rows in one call");
    hipLaunchKernelGGL(lora_merge_kernel, dim3((K + LM_TK - 1) / LM_TK, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (uint16_t*)dst, ldd,
                       (const uint16_t*)W, ldw, N, K, lt);
    return check_launch("lora_merge_kernel");
}

}  // extern "C"
