// MFMA building blocks of the per-layer coupling kernels that recompute a layer from its input (csrc/flow_train.hip: training
// mode; csrc/flow_frozen.hip: eval mode with frozen BatchNorm): the input contraction, the operand splits and the 64 x 64
// contraction in both orientations -- the arithmetic of csrc/flow.hip, product for product --, and the sums over a
// tile's points.  Anonymous namespace: each translation unit gets its own copy.
#ifndef DPF_FLOW_MFMA_H
#define DPF_FLOW_MFMA_H

#include "flow_common.h"

namespace {

__device__ __forceinline__ f32x16 zero16() {
    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// input MFMA of one branch: acc[t] = A0[br][t] . b0   (t = M tile)
__device__ __forceinline__ void input_mfma(const uint8_t *a0, int br, int lane, u32x4 b0, f32x16 (&acc)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
        acc[t] = mfma(*(const u32x4 *)(a0 + ((br * 2 + t) * 64 + lane) * 16), b0, zero16());
}

// the same with the operands swapped: acc[t] holds, in LANE pl, feature 32 t + pl of the 16 POINTS (r & 3) + 8 (r >> 2) + 4 h
__device__ __forceinline__ void input_mfma_swapped(const uint8_t *a0, int br, int lane, u32x4 b0, f32x16 (&acc)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
        acc[t] = mfma(b0, *(const u32x4 *)(a0 + ((br * 2 + t) * 64 + lane) * 16), zero16());
}

// Swapped accumulators (lane = feature, registers = points) as bf16 hi/lo operand fragments whose K dimension is the
// tile's 32 points: k-step j takes registers 8 j .. 8 j + 7 of the lane, i.e. k-slot i of lane-half kg holds point
// (i & 3) + 8 (2 j + (i >> 2)) + 4 kg -- some fixed order of the k-step's 16 points, the same for every operand built here.
// Symmetric hi/lo split of a pair: hi = bf16 round-to-nearest-even, lo = bf16(x - hi), signed.  The truncating split of the
// forward path (split_hi: the remainder has the sign of x) leaves a lo.lo term of the sign of the product out of every
// hi.hi + hi.lo + lo.hi contraction -- a bias of ~2^-18 per term that does not average out over a sum of 16 384 terms
// (r02: the cancelling bias gradients of the deeper layers).  With a zero-mean remainder on the activation side the omitted
// term is zero-mean.  Same six instructions per pair.  Backward-only operands: the forward recomputation keeps the forward
// kernel's split, bit for bit.
__device__ __forceinline__ void split_pair_sym(float v0, float v1, uint32_t &hi, uint32_t &lo) {
    hi = pack_bf16_rne(v0, v1);
    lo = pack_bf16_rne(v0 - u2f(hi << 16), v1 - u2f(hi & 0xFFFF0000u));
}

// the same for fp16 hi/lo operands (r04: the gradient contractions of an f16x3 stack): hi = fp16(x) and lo = fp16(x - hi), both
// round-to-nearest-even -- one v_cvt_pk_f16_f32 and the two v_fma_mix*_f16 of split_relu_f16 (`negone`: see there).  x must
// be scaled into fp16's range by the caller; 11 + 11 bits for |x| >= 2^-3, the absolute 2^-24 of fp16's subnormals below.
__device__ __forceinline__ void split_pair_sym_f16(float v0, float v1, float negone, uint32_t &hi, uint32_t &lo) {
    const f32x2 v = {v0, v1};
    const f16x2 h = __builtin_convertvector(v, f16x2);
    const f16x2 l = {(_Float16)__builtin_fmaf((float)h[0], negone, v0), (_Float16)__builtin_fmaf((float)h[1], negone, v1)};
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, l);
}
template <bool RELU, bool SCALE = true>
__device__ __forceinline__ void kfrags_from_swapped_f16(const f32x16 (&v)[2], float scale, float negone, u32x4 (&hi)[2][2], u32x4 (&lo)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float v0 = RELU ? relu(v[t][8 * j2 + 2 * d]) : v[t][8 * j2 + 2 * d];
                float v1 = RELU ? relu(v[t][8 * j2 + 2 * d + 1]) : v[t][8 * j2 + 2 * d + 1];
                if constexpr (SCALE) { v0 *= scale; v1 *= scale; }
                uint32_t hp, lp;
                split_pair_sym_f16(v0, v1, negone, hp, lp);
                hi[t][j2][d] = hp;
                lo[t][j2][d] = lp;
            }
}

template <bool RELU>
__device__ __forceinline__ void kfrags_from_swapped(const f32x16 (&v)[2], u32x4 (&hi)[2][2], u32x4 (&lo)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const float v0 = RELU ? relu(v[t][8 * j2 + 2 * d]) : v[t][8 * j2 + 2 * d];
                const float v1 = RELU ? relu(v[t][8 * j2 + 2 * d + 1]) : v[t][8 * j2 + 2 * d + 1];
                uint32_t hp, lp;
                split_pair_sym(v0, v1, hp, lp);
                hi[t][j2][d] = hp;
                lo[t][j2][d] = lp;
            }
}

// bf16 split (NS parts) of an accumulator fragment pair into the B fragments of the next contraction
// (register r of M tile t = element j = r&7 of k-step 2t + (r>>3)); RELU = clamp at zero first.
// Same arithmetic as branch_tile in csrc/flow.hip: the recomputed activations are bit-identical to
// the forward kernel's.
template <bool RELU, int NS, bool SYM = false, bool F16 = false>
__device__ __forceinline__ void split_fragment(const f32x16 (&v)[2], u32x4 (&bf)[NS][4], float negone = -1.0f) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const int s = 2 * t + (r >> 3), d = (r & 7) >> 1;
            if constexpr (F16) {               // the forward kernel's fp16 hi/lo split with the ReLU folded in (flow_common.h)
                static_assert(!F16 || (NS == 2 && RELU && !SYM), "f16x3: forward operands only");
                uint32_t hp, lp;
                split_relu_f16(v[t][r], v[t][r + 1], negone, hp, lp);
                bf[0][s][d] = hp;
                bf[1][s][d] = lp;
                continue;
            }
            const float v0 = RELU ? relu(v[t][r]) : v[t][r], v1 = RELU ? relu(v[t][r + 1]) : v[t][r + 1];
            if constexpr (SYM) {               // backward-only operand (NS == 2): symmetric split
                static_assert(!SYM || NS == 2, "symmetric split: hi/lo only");
                uint32_t hp, lp;
                split_pair_sym(v0, v1, hp, lp);
                bf[0][s][d] = hp;
                bf[NS - 1][s][d] = lp;
                continue;
            }
            float l0, l1;
            split_hi(v0, l0); split_hi(v1, l1);
            bf[0][s][d] = pack_bf16_trunc(v0, v1);
            if constexpr (NS == 2) {
                bf[1][s][d] = pack_bf16_rne(l0, l1);
            } else {
                float m0, m1;
                split_hi(l0, m0); split_hi(l1, m1);
                bf[1][s][d] = pack_bf16_trunc(l0, l1);
                bf[2][s][d] = pack_bf16_rne(m0, m1);
            }
        }
}

// acc[tp] += A1[br] . B  with the split terms of Terms<NS>; a1 = base of [part][br][tp][s][lane].  Same order as
// branch_tile in csrc/flow.hip (k-step major; the fragment of each part is loaded once and feeds every term that
// uses it): the recomputed pre-activations are bit-identical to the forward kernel's.
template <int NS, bool F16 = false>
__device__ __forceinline__ void chain_mfma(const uint8_t *a1, int br, int lane, const u32x4 (&bf)[NS][4], f32x16 (&acc)[2]) {
    using TT = Terms<NS>;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        u32x4 af[NS][2];
#pragma unroll
        for (int part = 0; part < NS; ++part)
#pragma unroll
            for (int tp = 0; tp < 2; ++tp)
                af[part][tp] = *(const u32x4 *)(a1 + part * P_A1_PART + (((br * 2 + tp) * 4 + s) * 64 + lane) * 16);
#pragma unroll
        for (int term = 0; term < TT::N; ++term)
#pragma unroll
            for (int tp = 0; tp < 2; ++tp)
                acc[tp] = F16 ? mfma_f16(af[TT::A[term]][tp], bf[TT::B[term]][s], acc[tp]) : mfma(af[TT::A[term]][tp], bf[TT::B[term]][s], acc[tp]);
    }
}

// The same contraction with the operands swapped (activations = A, weights = B; the two fragment layouts of the
// 32x32x16 MFMA mirror each other, so the same registers and the same packed fragments serve): the accumulator of
// M tile tp then holds, in LANE pl, feature 32*tp + pl of the 16 POINTS (r&3) + 8*(r>>2) + 4h of the tile -- sums
// over the points of a tile become in-lane adds plus one cross-half swap instead of a cross-lane butterfly.
template <int NS, bool F16 = false>
__device__ __forceinline__ void chain_mfma_swapped(const uint8_t *a1, int br, int lane, const u32x4 (&bf)[NS][4], f32x16 (&acc)[2]) {
    using TT = Terms<NS>;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        u32x4 af[NS][2];
#pragma unroll
        for (int part = 0; part < NS; ++part)
#pragma unroll
            for (int tp = 0; tp < 2; ++tp)
                af[part][tp] = *(const u32x4 *)(a1 + part * P_A1_PART + (((br * 2 + tp) * 4 + s) * 64 + lane) * 16);
#pragma unroll
        for (int term = 0; term < TT::N; ++term)
#pragma unroll
            for (int tp = 0; tp < 2; ++tp)
                acc[tp] = F16 ? mfma_f16(bf[TT::B[term]][s], af[TT::A[term]][tp], acc[tp]) : mfma(bf[TT::B[term]][s], af[TT::A[term]][tp], acc[tp]);
    }
}

// per-lane vector of a per-feature LDS array for the features this lane holds: out[t][r]
__device__ __forceinline__ void load_features(const float *vec, int h, f32x16 (&out)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = *(const f32x4 *)(vec + 32 * t + 8 * q + 4 * h);
            out[t][4 * q + 0] = v.x; out[t][4 * q + 1] = v.y; out[t][4 * q + 2] = v.z; out[t][4 * q + 3] = v.w;
        }
}

// Sum over the 32 point-lanes of a half wave, for all 32 accumulator registers at once: a
// recursive-halving butterfly (31 shuffles instead of 160).  On return lane pl holds in v[0][0] the
// total of register index R(pl) = b0*16 + b1*8 + b2*4 + b3*2 + b4 (b_k = bit k of pl), i.e. of
// feature acc_feature(R >> 4, R & 15, h).
template <int K>
__device__ __forceinline__ void reduce_stage(float (&w)[16], int pl) {
    constexpr int n2 = 8 >> (K - 1);
    const bool up = (pl >> K) & 1;
#pragma unroll
    for (int i = 0; i < n2; ++i) {
        const float keep = up ? w[i + n2] : w[i];
        const float send = up ? w[i] : w[i + n2];
        w[i] = keep + __shfl_xor(send, 1 << K);
    }
}
// gen(i), i = 0..31: element of accumulator register i (tile i >> 4, register i & 15); elements are
// produced on the fly so that a product like dh * x never exists as 32 live registers
template <typename Gen>
__device__ __forceinline__ float reduce_points_gen(Gen gen, int pl) {
    float w[16];
    const bool up = pl & 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float lo = gen(i), hi = gen(i + 16);
        const float keep = up ? hi : lo, send = up ? lo : hi;
        w[i] = keep + __shfl_xor(send, 1);
    }
    reduce_stage<1>(w, pl); reduce_stage<2>(w, pl); reduce_stage<3>(w, pl); reduce_stage<4>(w, pl);
    __builtin_amdgcn_sched_barrier(0);       // keep consecutive reductions from interleaving (register pressure)
    return w[0];
}
__device__ __forceinline__ float reduce_points(const f32x16 (&v)[2], int pl) {
    return reduce_points_gen([&](int i) { return v[i >> 4][i & 15]; }, pl);
}
__device__ __forceinline__ int reduced_feature(int pl, int h) {
    const int R = ((pl & 1) << 4) | ((pl & 2) << 2) | (pl & 4) | ((pl & 8) >> 2) | ((pl & 16) >> 4);
    return acc_feature(R >> 4, R & 15, h);
}

}  // namespace
#endif  // DPF_FLOW_MFMA_H
