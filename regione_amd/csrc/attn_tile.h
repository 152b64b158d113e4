// The flash-attention tile core shared by the sequence kernel of text.hip (head width 64 / 128) and vae_attention_kernel of vae.hip
// (head width 384 / 512): ONE definition of the scheme, so a fix to it is made once.
// Block = 4 waves x 16 queries.  Key tiles of 32 keys are staged in LDS (K key-major with a padded row stride, V transposed to
// [D channels][keys]) and shared by the four waves.  Per wave and tile (v_mfma_f32_16x16x32_bf16):
//   S^T [32 keys x 16 queries] = K Q^T   D / 32 k-steps x 2 key blocks, Q^T held in registers for the whole key loop
//   sc = the kernel's score transform of S^T (scale, bias, masks: a masked slot is exactly -inf); online softmax in fp32 (exp2)
//   O^T [D x 16 queries] += V^T P^T      D / 16 channel tiles, one MFMA each; P rounded to bf16 in the registers that MFMA reads as its
//                                        B operand: key slot 8 g + e of lane group g is key 4 g + e (e < 4), 16 + 4 g + e - 4 (e >= 4) -
//                                        the S^T output layout, so P needs no shuffle
// The running max / sum and every reduction have a fixed order: a repeated call is bit-identical.  The first tile a wave steps through
// must hold a valid key for every query (key 0 does), so the running max is finite from then on.
// text.hip is built with -ffp-contract=off and vae.hip without it: no expression here has the shape a * b + c, every fused multiply-add
// is an explicit __builtin_fmaf, and so this file means the same in both.
#pragma once
#include "common.h"

namespace rgn {

constexpr int ATTN_BQ = 64, ATTN_BK = 32;             // queries per block, keys per tile

template <int D>
struct AttnTile {
    static constexpr int BQ = ATTN_BQ, BK = ATTN_BK, KS = D / 32, CT = D / 16, VPR = D / 8;
    static constexpr int KLD = D + 8;                  // K row stride in LDS (u16): 16-byte aligned rows, 4 banks apart
    static constexpr int VLD = BK + 4;                 // V^T row stride in LDS (u16): 8-byte aligned
    static constexpr int K_LDS = BK * KLD, V_LDS = D * VLD;    // u16 elements of the two staging buffers

    bf16x8 qf[KS];
    f32x4 o[CT];
    float m_run, l_run;

    // the key (within the tile) that slot e of lane group g holds, in sc[] and in P
    static __device__ __forceinline__ int key_of_slot(int g, int e) { return e < 4 ? 4 * g + e : 16 + 4 * g + e - 4; }

    // q: this lane's query row (D contiguous bf16, 16-byte aligned)
    __device__ __forceinline__ void init(const uint16_t* q, int g) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *(const bf16x8*)(q + ks * 32 + g * 8);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        m_run = -INFINITY;
        l_run = 0.f;
    }

    // Stage one tile (all 256 threads; barriers are the caller's).  row(kk) is the global row of key kk of the tile, negative when there is
    // none; key kk is then read at K / V + row(kk) * ld.
    template <class Row>
    static __device__ __forceinline__ void stage(uint16_t* kl, uint16_t* vl, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
                                                 size_t ld, int tid, Row row) {
        for (int i = tid; i < (BK / 2) * VPR; i += 256) {  // one item: vector v of K rows kp, kp + 16 and of V rows 2 kp, 2 kp + 1
            const int kp = i / VPR, v = i - kp * VPR;
            const auto rk0 = row(kp), rk1 = row(kp + BK / 2), r0 = row(2 * kp), r1 = row(2 * kp + 1);
            uint4 w0 = make_uint4(0u, 0u, 0u, 0u), w1 = w0, a = w0, b = w0;   // keys past the last one: K = V = 0 (P = 0 there; 0 x garbage
            if (rk0 >= 0) w0 = *(const uint4*)(K + (size_t)rk0 * ld + v * 8);   // could be NaN).  The four loads are issued before the first store
            if (rk1 >= 0) w1 = *(const uint4*)(K + (size_t)rk1 * ld + v * 8);
            if (r0 >= 0) a = *(const uint4*)(V + (size_t)r0 * ld + v * 8);
            if (r1 >= 0) b = *(const uint4*)(V + (size_t)r1 * ld + v * 8);
            *(uint4*)(kl + kp * KLD + v * 8) = w0;
            *(uint4*)(kl + (kp + BK / 2) * KLD + v * 8) = w1;
            const uint32_t as[4] = {a.x, a.y, a.z, a.w}, bs[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t lo = (e & 1) ? as[e >> 1] >> 16 : as[e >> 1] & 0xffffu;
                const uint32_t hi = (e & 1) ? bs[e >> 1] & 0xffff0000u : bs[e >> 1] << 16;
                *(uint32_t*)(vl + (v * 8 + e) * VLD + 2 * kp) = lo | hi;
            }
        }
    }

    // One staged tile.  score(s, sc) turns the raw S^T slots (s[e] at key_of_slot(g, e)) into the softmax inputs sc[8]; the weights are
    // exp2(sc * mult - max * mult), so mult is log2 e times whatever scale the transform left out.
    template <class Score>
    __device__ __forceinline__ void step(const uint16_t* kl, const uint16_t* vl, int li, int g, float mult, Score score) {
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 k0f = *(const bf16x8*)(kl + li * KLD + ks * 32 + g * 8);
            const bf16x8 k1f = *(const bf16x8*)(kl + (16 + li) * KLD + ks * 32 + g * 8);
            s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0f, qf[ks], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1f, qf[ks], s1, 0, 0, 0);
        }
        const float s[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
        float sc[8];
        score(s, sc);
        float mx = fmaxf(fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])), fmaxf(fmaxf(sc[4], sc[5]), fmaxf(sc[6], sc[7])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);          // finite from the first tile on
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * mult);
        const float nb = -m_new * mult;
        uint32_t pw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            pw[e] = f2bf_pk(__builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e], mult, nb)), __builtin_amdgcn_exp2f(__builtin_fmaf(sc[2 * e + 1], mult, nb)));
        // the row sum is taken over the bf16 P the MFMA multiplies, so the weights the output is divided by are the ones it used
        const float ps = ((bf2f(pw[0] & 0xffffu) + bf2f(pw[0] >> 16)) + (bf2f(pw[1] & 0xffffu) + bf2f(pw[1] >> 16))) +
                         ((bf2f(pw[2] & 0xffffu) + bf2f(pw[2] >> 16)) + (bf2f(pw[3] & 0xffffu) + bf2f(pw[3] >> 16)));
        l_run = __builtin_fmaf(l_run, alpha, ps);
        m_run = m_new;
        if (__any(alpha != 1.0f)) {                    // the max moved for some query of the wave (x 1 is exact: skipping it changes nothing)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) o[ct] *= alpha;
        }
        const bf16x8 pf = __builtin_bit_cast(bf16x8, make_uint4(pw[0], pw[1], pw[2], pw[3]));
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const uint16_t* vr = vl + (ct * 16 + li) * VLD + 4 * g;
            const uint2 va = *(const uint2*)vr, vb = *(const uint2*)(vr + 16);
            const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(va.x, va.y, vb.x, vb.y));
            o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[ct], 0, 0, 0);
        }
    }

    // the softmax denominator of this lane's query: o[ct][r] / row_sum() is channel ct * 16 + 4 g + r of the output
    __device__ __forceinline__ float row_sum() const {
        float l = l_run;
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        return l;
    }
};

}  // namespace rgn
