// Packed layout and matrix-core tile code of the eval-mode PointNet encoder (csrc/encoder.hip), shared with the frozen
// backward's recomputation (csrc/encoder_frozen.hip): both run layers 0-2 through enc_layers012 below -- the same fragments,
// precision, k order and accumulator scheme -- so a recomputed pre-activation equals the forward's bit for bit (a point's
// MFMA column does not depend on the other points of its tile).
#ifndef DPF_ENCODER_MFMA_H
#define DPF_ENCODER_MFMA_H

#include "flow_common.h"
#include "encoder_layout.h"

namespace {

// packed: [A0 4 KiB: [t2][ks2][lane64][8] | bias 4 KiB: b1acc[4][2][16] b2acc[8][2][16] b3[512] pad | chunks]
// The fragments of layers 1-3 form one stream of 336 slots (a slot = the NS parts of one 1 KiB fragment):
// layer 1: 4 M tiles x 4 k-steps at slot 0, layer 2: 8 x 8 at slot 16, layer 3: 16 N tiles x 16 at slot 80; a tile's
// k-steps are consecutive and never straddle a chunk of e_slots(NS) slots.  Chunk: [part][slot][lane64][8].
constexpr int EP_A0 = 0, EP_BIAS = 4096, EP_CHUNKS = 8192;
constexpr int EB_1 = 0, EB_2 = 128, EB_3 = 384;                      // float offsets inside the bias block
constexpr int ES_L1 = 0, ES_L2 = 16, ES_L3 = 80, ES_TOTAL = 336;
// slots per chunk: 32 (two 64 KiB buffers at bf16x3) halves the number of workgroup barriers; bf16x6 keeps 16
__host__ __device__ constexpr int e_slots(int NS) { return NS == 3 ? 16 : 32; }
__host__ __device__ constexpr int e_nchunk(int NS) { return (ES_TOTAL + e_slots(NS) - 1) / e_slots(NS); }
__host__ __device__ constexpr int ep_chunk_bytes(int NS) { return NS * e_slots(NS) * 1024; }
__host__ __device__ constexpr size_t ep_bytes(int NS) { return EP_CHUNKS + (size_t)e_nchunk(NS) * ep_chunk_bytes(NS); }

// A workgroup covers 8 tiles (256 points) of one cloud.  TP = tiles per wave:
//   TP = 1 (default): 8 waves, two per SIMD with 256 VGPRs each (bf16x6: 4 waves, one per SIMD -- it keeps 192 VGPRs
//          of layer-3 operand fragments);
//   TP = 2 (-DDPF_ENC_TP=2; bf16, bf16x3): 4 waves, one per SIMD with 484 VGPRs; every weight fragment read from
//          LDS feeds the MFMAs of both tiles, halving the LDS->VGPR traffic.  Measured r01 at cfg-2: 56.1 us vs
//          50.5 us for TP = 1 -- a lone wave per SIMD does not hide its own LDS and MFMA latencies.
#ifndef DPF_ENC_TP
#define DPF_ENC_TP 1
#endif
__host__ __device__ constexpr int e_tp(int NS) { return NS == 3 ? 1 : DPF_ENC_TP; }
__host__ __device__ constexpr int e_waves(int NS) { return NS == 3 ? 4 : 8 / e_tp(NS); }

// K index held by element j of lane-half kg in k-step ks = the feature that register 8*(ks&1)+j of accumulator
// tile ks>>1 holds in lane-half kg (acc_feature)
__host__ __device__ constexpr int k_feature(int ks, int j, int kg) { return acc_feature(ks >> 1, 8 * (ks & 1) + j, kg); }

// relu + split of one accumulator tile into the two k-steps 2t, 2t+1 of the next layer's fragments
template <int NS>
__device__ __forceinline__ void relu_split(const f32x16 &acc, u32x4 (&dst)[NS][16], int t) {
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float v0 = relu(acc[r]), v1 = relu(acc[r + 1]);
        const int s = 2 * t + (r >> 3), d = (r & 7) >> 1;
        if (NS == 1) {
            dst[0][s][d] = pack_bf16_rne(v0, v1);
        } else if (NS == 2) {
            float l0, l1;
            split_hi(v0, l0); split_hi(v1, l1);
            dst[0][s][d] = pack_bf16_trunc(v0, v1);
            dst[1][s][d] = pack_bf16_rne(l0, l1);
        } else {
            float l0, l1, m0, m1;
            split_hi(v0, l0); split_hi(v1, l1);
            split_hi(l0, m0); split_hi(l1, m1);
            dst[0][s][d] = pack_bf16_trunc(v0, v1);
            dst[1][s][d] = pack_bf16_trunc(l0, l1);
            dst[2][s][d] = pack_bf16_rne(m0, m1);
        }
    }
}

template <int NS>
__device__ __forceinline__ void stage_chunk(const uint8_t *packed, int c, uint8_t *lds, int wave, int lane) {
    constexpr int NI = ep_chunk_bytes(NS) / 1024, EW = e_waves(NS);     // wave-instructions of 1 KiB
    const uint8_t *src = packed + EP_CHUNKS + (size_t)c * ep_chunk_bytes(NS);
#pragma unroll
    for (int i = 0; i < NI / EW; ++i) {
        const int k = wave + i * EW;
        __builtin_amdgcn_global_load_lds((glb_void *)(src + k * 1024 + lane * 16), (lds_void *)(lds + k * 1024), 16, 0, 0);
    }
}

// One output tile for each of the wave's TP point tiles: K k-steps of fragments at slots [slot0, slot0 + K) of the
// chunk at cb; every fragment read feeds the MFMAs of all TP tiles.  SWAP: the activations are the A operand and the
// weights the B operand.  NA accumulators per tile (even / odd k-steps) keep consecutive MFMAs independent.
template <int NS, int K, bool SWAP, int TP, int NA>
__device__ __forceinline__ void tile_gemm(const uint8_t *cb, int slot0, int lane, const u32x4 (&act)[TP][NS][16],
                                          f32x16 (&out)[TP]) {     // out: in = initial value, out = result
    typedef Terms<NS> TT;
    f32x16 acc[TP][NA];
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        acc[q][0] = out[q];
        if (NA == 2) acc[q][NA - 1] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
    u32x4 wf[2][NS];
    auto load = [&](int ks, u32x4 (&dst)[NS]) {
#pragma unroll
        for (int part = 0; part < NS; ++part)
            dst[part] = *(const u32x4 *)(cb + part * (e_slots(NS) * 1024) + ((slot0 + ks) * 64 + lane) * 16);
    };
    load(0, wf[0]);
#pragma unroll
    for (int ks = 0; ks < K; ++ks) {
        if (ks + 1 < K) load(ks + 1, wf[(ks + 1) & 1]);
#pragma unroll
        for (int term = 0; term < TT::N; ++term)
#pragma unroll
            for (int q = 0; q < TP; ++q) {
                const u32x4 w = wf[ks & 1][TT::A[term]], x = act[q][TT::B[term]][ks];
                f32x16 &d = acc[q][ks & (NA - 1)];
                d = SWAP ? mfma(x, w, d) : mfma(w, x, d);
            }
    }
    // (element by element through an opaque copy: a vector `+` becomes v_pk_add_f32, which the scheduler then places directly in
    // front of the next tile's first MFMA -- the one pairing tools/asm_bisect found losing a packed result in csrc/emd.hip's
    // vectorised build; tools/mfma_overlap_check.py --no-packed-before-mfma gates every object on it)
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        if (NA == 2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float hi = acc[q][NA - 1][r];
                asm volatile("" : "+v"(hi));
                out[q][r] = acc[q][0][r] + hi;
            }
        } else {
            out[q] = acc[q][0];
        }
    }
}

__device__ __forceinline__ float half_max(float x) {   // max(x(lane), x(lane ^ 32))
    const auto r = __builtin_amdgcn_permlane32_swap(f2u(x), f2u(x), false, false);
    return fmaxf(u2f(r[0]), u2f(r[1]));
}

// The fragment stream of layers 1-3 through the two LDS buffers at l_buf.  Chunk `cur` is resident in buffer cur & 1 and chunk
// cur + 1 is on its way into the other one.  Moving on to the next chunk is one barrier (it has landed; everybody is done with
// the buffer the one after it will overwrite).  start() after the prologue's barrier (chunk 0 resident).
template <int NS>
struct EncStream {
    const uint8_t *packed;
    uint8_t *l_buf;
    int wave, lane, cur;
    __device__ __forceinline__ void start() {
        cur = 0;
        stage_chunk<NS>(packed, 1, l_buf + ep_chunk_bytes(NS), wave, lane);
    }
    __device__ __forceinline__ const uint8_t *at(int slot) {       // slot: wave-uniform
        constexpr int S = e_slots(NS), NCH = e_nchunk(NS), CHB = ep_chunk_bytes(NS);
        const int c = slot / S;
        if (c != cur) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // chunk c's pieces (issued a chunk ago) have landed
            __syncthreads();
            cur = c;
            if (c + 1 < NCH) stage_chunk<NS>(packed, c + 1, l_buf + ((c + 1) & 1) * CHB, wave, lane);
        }
        return l_buf + (c & 1) * CHB;
    }
};

// accumulator-order shift of M tile mt (bias block offset off) for lane half h
__device__ __forceinline__ f32x16 enc_bias_tile(const uint8_t *l_bias, int off, int mt, int h) {
    const float *bp = (const float *)l_bias + off + (mt * 2 + h) * 16;
    f32x16 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 b = *(const f32x4 *)(bp + 4 * q);
        v[4 * q + 0] = b.x; v[4 * q + 1] = b.y; v[4 * q + 2] = b.z; v[4 * q + 3] = b.w;
    }
    return v;
}

struct EncNoTap {
    __device__ __forceinline__ void operator()(int, int, int, const f32x16 &) const {}
};

// Layers 0-2 of the wave's TP point tiles (coordinates px, py, pz of this lane's point per tile) -> the layer-3 operand
// fragments f3.  The A0 + bias block is resident at l_a0 / l_bias and chunk 0 at the stream's buffer; the stream is left where
// layer 3 picks it up.  tap(layer, q, mt, acc) sees every pre-activation tile (accumulator order: register r of M tile mt in
// lane half h = feature acc_feature(mt, r, h) of the lane's point) before its ReLU.
template <int NS, int TP, int NA12, class Tap>
__device__ __forceinline__ void enc_layers012(EncStream<NS> &st, const uint8_t *l_a0, const uint8_t *l_bias, int lane,
                                              const float (&px)[TP], const float (&py)[TP], const float (&pz)[TP],
                                              u32x4 (&f3)[TP][NS][16], const Tap &tap) {
    constexpr int S = e_slots(NS);
    const int h = lane >> 5;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // ---- layer 0: 3 -> 64 on the matrix core, fp32-accurate (3-way split of x, y | z)
    u32x4 f1[TP][NS][16];        // only k-steps 0..3 are used
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        const u32x4 b0 = input_fragment(h ? py[q] : px[q], h);
        u32x4 b1 = input_fragment(pz[q], 0);
        if (h) b1 = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const u32x4 a00 = *(const u32x4 *)(l_a0 + ((t * 2 + 0) * 64 + lane) * 16);
            const u32x4 a01 = *(const u32x4 *)(l_a0 + ((t * 2 + 1) * 64 + lane) * 16);
            f32x16 acc = mfma(a00, b0, zero16);
            acc = mfma(a01, b1, acc);
            tap(0, q, t, acc);
            relu_split<NS>(acc, f1[q], t);
        }
    }
    st.start();
    // ---- layer 1: 64 -> 128
    u32x4 f2[TP][NS][16];        // k-steps 0..7
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int slot = ES_L1 + 4 * mt;
        const uint8_t *cb = st.at(slot);
        f32x16 acc[TP];
#pragma unroll
        for (int q = 0; q < TP; ++q) acc[q] = enc_bias_tile(l_bias, EB_1, mt, h);
        tile_gemm<NS, 4, false, TP, NA12>(cb, slot % S, lane, f1, acc);
#pragma unroll
        for (int q = 0; q < TP; ++q) {
            tap(1, q, mt, acc[q]);
            relu_split<NS>(acc[q], f2[q], mt);
        }
    }
    // ---- layer 2: 128 -> 256
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const int slot = ES_L2 + 8 * mt;
        const uint8_t *cb = st.at(slot);
        f32x16 acc[TP];
#pragma unroll
        for (int q = 0; q < TP; ++q) acc[q] = enc_bias_tile(l_bias, EB_2, mt, h);
        tile_gemm<NS, 8, false, TP, NA12>(cb, slot % S, lane, f2, acc);
#pragma unroll
        for (int q = 0; q < TP; ++q) {
            tap(2, q, mt, acc[q]);
            relu_split<NS>(acc[q], f3[q], mt);
        }
    }
}

inline int e_ns_of(int precision) {
    return precision == DPF_PREC_BF16 ? 1 : precision == DPF_PREC_BF16X3 ? 2 : precision == DPF_PREC_BF16X6 ? 3 : 0;
}

}  // namespace
#endif  // DPF_ENCODER_MFMA_H
