// Fused PointNet cloud encoder + max over the points for gfx950 (MI355X), eval-mode BatchNorm.
//
// Replaces
//   PointNetCloudEncoder.forward           lib/networks/encoders.py:27-28
//     features = [SharedDot(no bias) . BatchNorm1d . ReLU] x 4,  3 -> 64 -> 128 -> 256 -> 512   (encoders.py:15-25)
//   torch.max(features, dim=2)[0]          lib/networks/models.py:85,131,175
// (12 ATen kernels writing and re-reading (B,C,N) activations: (64+128+256+512) * 4 B = 3.8 KB per point per pass,
// ~1 GB of HBM traffic at B=32, N=2048) by ONE kernel that reads 12 B per point and writes B*512 floats: the
// activations never leave the register file.
//
// A wave owns a tile of 32 points; a workgroup = 8 waves = 256 points of one cloud.  Per layer the weights are the
// MFMA A operand (rows = output features) and the points the B operand, so the accumulator fragment of one
// v_mfma_f32_32x32x16_bf16 -- each lane holds 16 features of ITS point -- becomes, after ReLU and a bf16 hi/lo split
// in registers, the B fragment of the next layer (the K-slot <-> feature permutation this implies is applied to the
// next layer's columns at pack time; same trick as csrc/flow.hip).  The LAST layer swaps the operands (activations
// = A, weights = B): then a lane holds 16 POINTS of its feature and the max over the tile is 8 v_max3 in-lane plus
// one cross-half swap, instead of a 5-step cross-lane butterfly per accumulator register.
//
// Split precision (bf16x3 default): products hi*hi + hi*lo + lo*hi of the bf16 hi/lo parts, fp32 accumulate.
// BatchNorm (running statistics) is folded: scale into the weight rows before the split, shift as the accumulator's
// initial value (layer 0: a constant-1 K slot of the input MFMA, whose 16 K slots hold the 3-way split of x, y, z).
//
// The 672 KiB (bf16x3) of layer 1-3 fragments stream through LDS in 11 chunks of 64 KiB (double-buffered,
// global_load_lds, one workgroup barrier per chunk).
#include "flow_common.h"
#include "encoder_layout.h"
#include "encoder_mfma.h"
#include "zero_fill.h"

namespace {

template <int NS>
__global__ __launch_bounds__(256) void enc_pack_kernel(const float *__restrict__ canon, uint8_t *__restrict__ packed) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    auto scale_shift = [&](int l, int f, float &s, float &t) {
        const float *c = canon + e_layer_off(l) + e_cout(l) * e_cin(l);
        const int co = e_cout(l);
        s = c[f] / sqrtf(c[3 * co + f] + BN_EPS);
        t = c[co + f] - c[2 * co + f] * s;
    };
    // A0: the three input channels over two k-steps (x, y + shift | z)
    uint16_t *a0 = (uint16_t *)(packed + EP_A0);
    for (int idx = tid; idx < 2 * 2 * 64 * 8; idx += nth) {
        const int j = idx & 7, lane = (idx >> 3) & 63, ks = (idx >> 9) & 1, t = idx >> 10;
        const int f = 32 * t + (lane & 31), h = lane >> 5;
        float s, sh;
        scale_shift(0, f, s, sh);
        const float *w = canon + e_layer_off(0) + f * EC0;
        uint32_t v;
        if (ks == 0) v = input_weight_slot(s * w[h], sh, h, j);
        else v = h == 0 ? input_weight_slot(s * w[2], 0.f, 0, j) : 0u;
        a0[idx] = (uint16_t)v;
    }
    float *bias = (float *)(packed + EP_BIAS);
    for (int idx = tid; idx < 1024; idx += nth) {
        float s, sh = 0.f;
        if (idx < EB_2) {                       // layer 1, accumulator order [mt4][h2][r16]
            scale_shift(1, acc_feature(idx >> 5, idx & 15, (idx >> 4) & 1), s, sh);
        } else if (idx < EB_3) {
            const int i = idx - EB_2;
            scale_shift(2, acc_feature(i >> 5, i & 15, (i >> 4) & 1), s, sh);
        } else if (idx < EB_3 + EC4) {
            scale_shift(3, idx - EB_3, s, sh);
        }
        bias[idx] = sh;
    }
    uint16_t *ch = (uint16_t *)(packed + EP_CHUNKS);
    constexpr int S = e_slots(NS);
    const int per_chunk = S * 64 * 8;           // elements per part
    for (int idx = tid; idx < e_nchunk(NS) * per_chunk; idx += nth) {
        const int c = idx / per_chunk, e = idx % per_chunk;
        const int j = e & 7, lane = (e >> 3) & 63, slot = c * S + (e >> 9);
        uint16_t *o = ch + (size_t)c * NS * per_chunk + e;
        if (slot >= ES_TOTAL) {                 // padding of the last chunk
            for (int part = 0; part < NS; ++part) o[part * per_chunk] = 0;
            continue;
        }
        int l, rt, ks;
        if (slot < ES_L2) { l = 1; rt = slot >> 2; ks = slot & 3; }
        else if (slot < ES_L3) { l = 2; rt = (slot - ES_L2) >> 3; ks = (slot - ES_L2) & 7; }
        else { l = 3; rt = (slot - ES_L3) >> 4; ks = (slot - ES_L3) & 15; }
        const int row = 32 * rt + (lane & 31), col = k_feature(ks, j, lane >> 5);
        float s, sh;
        scale_shift(l, row, s, sh);
        const float w = s * canon[e_layer_off(l) + row * e_cin(l) + col];
        if (NS == 1) {
            o[0] = (uint16_t)bf16_rne(w);
        } else if (NS == 2) {
            float r1;
            o[0] = (uint16_t)(split_hi(w, r1) >> 16);
            o[per_chunk] = (uint16_t)bf16_rne(r1);
        } else {
            float r1, r2;
            o[0] = (uint16_t)(split_hi(w, r1) >> 16);
            o[per_chunk] = (uint16_t)(split_hi(r1, r2) >> 16);
            o[2 * per_chunk] = (uint16_t)bf16_rne(r2);
        }
    }
}

struct EncArgs {
    const uint8_t *packed;
    const float *x;        // (B,3,N)
    float *gmax;           // (B,512), zero-initialised by the launcher; updated with integer atomicMax (values >= 0)
    float *feat;           // (B,512,N) or NULL
    int B, N;
    // ARG variant (dpf_encoder_forward_arg): gmax is NOT zero-initialised and is written once, by the cloud's last workgroup
    int *arg;                       // (B,512): lowest point attaining gmax
    unsigned long long *keys;       // (B,512) scratch, zero on entry: (value bits << 32) | (0xFFFFFFFF - point), integer atomic max
    unsigned *ticket;               // (B) scratch, zero on entry
};

// ARG: the max over the points also yields the point that attains it.  A lane tracks (value bits, 255 - point of the wave)
// of its in-lane maximum as one 64-bit key, the waves of a workgroup meet in LDS, the workgroups of a cloud in a 64-bit
// integer atomic max -- order-independent, no floating-point atomics -- and the workgroup that arrives last at the cloud's
// ticket unpacks the keys into gmax and arg.  The values are relu'd on the bit pattern (>= +0), so the keys order like the
// floats, equal values order by descending point, and gmax has the bits of the plain kernel's result.
template <int NS, bool ARG>
__global__ __launch_bounds__(e_waves(NS) * 64) void enc_kernel(EncArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int CHB = ep_chunk_bytes(NS), EW = e_waves(NS), TP = e_tp(NS);
    // accumulators per tile and layer: two where the registers allow it (one wave per SIMD has nobody else to fill
    // the gap between dependent MFMAs)
    constexpr int NA12 = (EW == 4 && TP == 1) ? 2 : 1, NA3 = TP == 2 ? 1 : 2;
    uint8_t *l_a0 = smem, *l_bias = smem + 4096, *l_buf = smem + 8192;
    float *l_wmax = (float *)(smem + 8192 + 2 * CHB);             // [EW][512]
    [[maybe_unused]] uint8_t *l_widx = smem + 8192 + 2 * CHB + EW * EC4 * 4;       // ARG: [EW][512] point of the wave's TP tiles

    const int bi = blockIdx.y;
    const int lane = threadIdx.x & 63, h = lane >> 5, pl = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N;
    const float *xc = a.x + (size_t)bi * 3 * N;
    int tile0[TP];                                                // first point of each of this wave's tiles
    float px[TP], py[TP], pz[TP];
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        tile0[q] = ((blockIdx.x * EW + wave) * TP + q) * TILE;
        const int nc = min(tile0[q] + pl, N - 1);
        px[q] = xc[nc]; py[q] = xc[N + nc]; pz[q] = xc[2 * (size_t)N + nc];
    }

    // A0 + bias block (8 KiB) and chunk 0
#pragma unroll
    for (int k = wave; k < 8; k += EW)
        __builtin_amdgcn_global_load_lds((glb_void *)(a.packed + k * 1024 + lane * 16), (lds_void *)(smem + k * 1024), 16, 0, 0);
    stage_chunk<NS>(a.packed, 0, l_buf, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA pieces have landed (explicit: __syncthreads() alone emits no vmcnt wait on gfx950)
    __syncthreads();

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int S = e_slots(NS);
    EncStream<NS> st{a.packed, l_buf, wave, lane, 0};
    u32x4 f3[TP][NS][16];
    enc_layers012<NS, TP, NA12>(st, l_a0, l_bias, lane, px, py, pz, f3, EncNoTap());
    // ---- layer 3: 256 -> 512, operands swapped: accumulator register r = point (r&3) + 8*(r>>2) + 4h of the tile,
    //      lane column = output feature; one 32-feature tile at a time.
    for (int nt = 0; nt < 16; ++nt) {
        const int slot = ES_L3 + 16 * nt;
        const uint8_t *cb = st.at(slot);
        f32x16 acc[TP];
#pragma unroll
        for (int q = 0; q < TP; ++q) acc[q] = zero16;
        tile_gemm<NS, 16, true, TP, NA3>(cb, slot % S, lane, f3, acc);
        const float shift = ((const float *)l_bias)[EB_3 + 32 * nt + pl];
        float best = -__builtin_inff();
        [[maybe_unused]] unsigned long long kbest = 255ull;       // ARG: value +0 at point 0 of the wave
#pragma unroll
        for (int q = 0; q < TP; ++q) {
            if (a.feat != nullptr) {       // optional (B,512,N) output: 4 consecutive points per 16-byte store
                float *fo = a.feat + ((size_t)bi * EC4 + 32 * nt + pl) * N + tile0[q] + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int p0 = tile0[q] + 4 * h + 8 * g;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[q][4 * g + e] + shift, 0.f);
                    if (p0 + 3 < N && (N & 3) == 0) {
                        *(f32x4 *)(fo + 8 * g) = f32x4{v[0], v[1], v[2], v[3]};
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (p0 + e < N) fo[8 * g + e] = v[e];
                    }
                }
            }
            if (ARG) {
                // the feature's VALUE per point, as the plain kernel forms it for the maximum (relu(x + shift): fp32 addition
                // is monotonic, so the largest of these is relu(max x + shift)); a missing point of a ragged tile never beats
                // the initial key, and the tile's point 0 exists whenever any of its points does
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pt = 32 * q + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const unsigned long long k = ((unsigned long long)f2u(relu(acc[q][r] + shift)) << 32) | (unsigned)(255 - pt);
                    if (tile0[q] + pt - 32 * q < N && k > kbest) kbest = k;
                }
                continue;
            }
            if (tile0[q] + TILE > N) {     // ragged or empty tile: its missing points do not take part in the max
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (tile0[q] + (r & 3) + 8 * (r >> 2) + 4 * h >= N) acc[q][r] = -__builtin_inff();
            }
            float m = fmaxf(fmaxf(acc[q][0], acc[q][1]), acc[q][2]);
#pragma unroll
            for (int r = 3; r < 15; r += 2) m = fmaxf(fmaxf(m, acc[q][r]), acc[q][r + 1]);
            best = fmaxf(best, fmaxf(m, acc[q][15]));
        }
        if (ARG) {
            const uint32_t klo = (uint32_t)kbest, khi = (uint32_t)(kbest >> 32);
            const auto rl = __builtin_amdgcn_permlane32_swap(klo, klo, false, false);
            const auto rh = __builtin_amdgcn_permlane32_swap(khi, khi, false, false);
            const unsigned long long k0 = ((unsigned long long)rh[0] << 32) | rl[0], k1 = ((unsigned long long)rh[1] << 32) | rl[1];
            const unsigned long long k = k0 > k1 ? k0 : k1;
            if (!h) {
                l_wmax[wave * EC4 + 32 * nt + pl] = u2f((uint32_t)(k >> 32));
                l_widx[wave * EC4 + 32 * nt + pl] = (uint8_t)(255u - ((uint32_t)k & 255u));
            }
            continue;
        }
        best = half_max(best);
        // max_p relu(x_p + shift) = relu(max_p x_p + shift): fp32 addition is monotonic; an all-empty wave gives 0
        if (!h) l_wmax[wave * EC4 + 32 * nt + pl] = fmaxf(best + shift, 0.f);
    }
    __syncthreads();
    if (ARG) {
        // ---- combine the waves (ascending points: a later wave wins only with a larger value; wave 0 of a workgroup is never
        // empty), then the workgroups of the cloud
        for (int f = threadIdx.x; f < EC4; f += EW * 64) {
            uint32_t m = f2u(l_wmax[f]);
            int w0 = 0;
#pragma unroll
            for (int w = 1; w < EW; ++w) {
                const uint32_t v = f2u(l_wmax[w * EC4 + f]);
                if (v > m) { m = v; w0 = w; }
            }
            const uint32_t point = (uint32_t)((blockIdx.x * EW + w0) * TP * TILE) + l_widx[w0 * EC4 + f];
            __hip_atomic_fetch_max(a.keys + (size_t)bi * EC4 + f, ((unsigned long long)m << 32) | (0xFFFFFFFFu - point),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this workgroup's keys have left the CU
        __syncthreads();
        unsigned *tk = (unsigned *)l_wmax;
        if (threadIdx.x == 0) *tk = __hip_atomic_fetch_add(a.ticket + bi, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*tk != gridDim.x - 1) return;
        for (int f = threadIdx.x; f < EC4; f += EW * 64) {
            const unsigned long long k = __hip_atomic_load(a.keys + (size_t)bi * EC4 + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.gmax[(size_t)bi * EC4 + f] = u2f((uint32_t)(k >> 32));
            a.arg[(size_t)bi * EC4 + f] = (int)(0xFFFFFFFFu - (uint32_t)k);
        }
        return;
    }
    // ---- combine the waves, one integer atomicMax per feature (all values are >= 0, so the bit patterns order)
    for (int f = threadIdx.x; f < EC4; f += EW * 64) {
        float m = l_wmax[f];
#pragma unroll
        for (int w = 1; w < EW; ++w) m = fmaxf(m, l_wmax[w * EC4 + f]);
        atomicMax((int *)(a.gmax + (size_t)bi * EC4 + f), (int)f2u(m));
    }
}

template <int NS, bool ARG>
int launch_enc(const EncArgs &a, hipStream_t s) {
    constexpr int EW = e_waves(NS), EWG_POINTS = EW * e_tp(NS) * TILE;
    const int lds = 8192 + 2 * ep_chunk_bytes(NS) + EW * EC4 * (ARG ? 5 : 4);
    static LdsLimit limit;
    if (hipError_t e = limit.ensure((const void *)enc_kernel<NS, ARG>, lds); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((enc_kernel<NS, ARG>), dim3((a.N + EWG_POINTS - 1) / EWG_POINTS, a.B), dim3(EW * 64), lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t dpf_encoder_canon_floats(void) { return (size_t)E_CANON; }

extern "C" size_t dpf_encoder_packed_bytes(int precision) {
    const int ns = e_ns_of(precision);
    return ns ? ep_bytes(ns) : 0;
}

extern "C" int dpf_encoder_pack(int precision, const float *canon, void *packed, dpf_stream_t stream) {
    const int ns = e_ns_of(precision);
    if (!ns || !canon || !packed) return DPF_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (ns == 1) hipLaunchKernelGGL(enc_pack_kernel<1>, dim3(256), dim3(256), 0, s, canon, (uint8_t *)packed);
    if (ns == 2) hipLaunchKernelGGL(enc_pack_kernel<2>, dim3(256), dim3(256), 0, s, canon, (uint8_t *)packed);
    if (ns == 3) hipLaunchKernelGGL(enc_pack_kernel<3>, dim3(256), dim3(256), 0, s, canon, (uint8_t *)packed);
    return (int)hipGetLastError();
}

extern "C" int dpf_encoder_forward(int B, int N, int precision, const void *packed, const float *x, float *gmax, float *feat,
                                   dpf_stream_t stream) {
    const int ns = e_ns_of(precision);
    if (!ns || B < 0 || N <= 0) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!packed || !x || !gmax) return DPF_EINVAL;
    if (B > 65535) return DPF_ENOSUP;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = dpf_zero_async(gmax, sizeof(float) * (size_t)B * EC4, s);
    if (e != hipSuccess) return (int)e;
    EncArgs a{(const uint8_t *)packed, x, gmax, feat, B, N, nullptr, nullptr, nullptr};
    return ns == 1 ? launch_enc<1, false>(a, s) : ns == 2 ? launch_enc<2, false>(a, s) : launch_enc<3, false>(a, s);
}

// (B,512) 64-bit keys, then B tickets
extern "C" size_t dpf_encoder_arg_scratch_bytes(int B) { return B > 0 ? (size_t)B * (EC4 * 8 + 4) : 0; }

extern "C" int dpf_encoder_forward_arg(int B, int N, int precision, const void *packed, const float *x, float *gmax, int *arg,
                                       void *scratch, dpf_stream_t stream) {
    const int ns = e_ns_of(precision);
    if (!ns || B < 0 || N <= 0) return DPF_EINVAL;
    if (ns == 1) return DPF_ENOSUP;                          // bf16x3 and bf16x6 only
    if (B == 0) return 0;
    if (!packed || !x || !gmax || !arg || !scratch || ((uintptr_t)scratch & 7)) return DPF_EINVAL;
    if (B > 65535) return DPF_ENOSUP;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = dpf_zero_async(scratch, dpf_encoder_arg_scratch_bytes(B), s);
    if (e != hipSuccess) return (int)e;
    EncArgs a{(const uint8_t *)packed, x, gmax, nullptr, B, N, arg, (unsigned long long *)scratch,
              (unsigned *)((uint8_t *)scratch + (size_t)B * EC4 * 8)};
    return ns == 2 ? launch_enc<2, true>(a, s) : launch_enc<3, true>(a, s);
}
