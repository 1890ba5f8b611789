// Farthest-point sampling: k greedy selections per cloud, each the point farthest from those already taken.  The contract (strides,
// arithmetic, tie rule, refusals, outputs) is in include/dpf_hip.h; tests/fps_ref.py restates it in numpy, round for round.
//
// One workgroup per cloud, nothing wider, no synchronisation between workgroups.  Run time is k times the latency of a round, so the
// round is what is designed:
//   * a thread keeps its points (tid + j * THREADS, j < PPT) and their mind in registers; the cloud also lies in LDS, 12 bytes a
//     point, so that the winner's coordinates are one LDS read at a wave-uniform address for every thread;
//   * update: PPT times (3 subtractions, 3 products, 2 sums, a minimum), and the thread's own best (mind's bits, lowest index);
//   * the argmax is a maximum of the packed key (bits of mind << 32 | ~index): mind >= +0 orders as an unsigned integer, and the
//     complemented index makes the plain maximum pick the LOWEST index among equal mind.  Inside a wave it runs on DPP moves, as two
//     32-bit maxima (the high half, then the low half of the lanes that hold that high half) -- six steps each, no LDS traffic;
//   * the waves meet in a double-buffered LDS slot: lane 0 of every wave writes its key into slot[t & 1], ONE barrier, every wave
//     reads the W keys (one per lane of a row) and reduces them with the same DPP steps.  Round t + 2 reuses the buffer of round t;
//     a wave can only get there through the barrier of round t + 1, which every wave passes after its reads of round t;
//   * radius2[t] is the winning key's high half: no second reduction;
//   * index / radius2 of a round are wave-uniform values: thread (t mod THREADS) keeps them in a register and the workgroup stores
//     THREADS rounds at a time, coalesced -- no global store (and no wait for one) stands in the ordinary round.
// The one-wave form has no slot and no barrier in its round.  Padding points (index >= n) hold mind = 0 for ever: their key's high
// half is 0, so they lose to every real point, and where every mind is 0 the lowest index -- 0, a real point -- wins.
//
// Bounded: the loops run over PPT, over k and over the DPP steps; nothing waits on another workgroup.
// Compiled with -ffp-contract=off: the distance is a stated sequence of separately rounded fp32 operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "lds_attr.h"

namespace {

typedef unsigned long long u64;

struct FPSArgs {
    const float *xyz;
    long sc, sp, sa;                                // floats between clouds, points, axes
    int n, k;
    const int *start;                               // (B) or NULL
    int *index;                                     // (B, k)
    float *radius2;                                 // (B, k) or NULL
    int *status;                                    // (B) or NULL
};

// DPP controls (gfx9): quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror, row_bcast15, row_bcast31
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_BCAST15 = 0x142, DPP_BCAST31 = 0x143;

// max(v, the value the DPP control brings); rows outside ROWS keep v
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned fps_dpp_max(unsigned v) {
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xf, false);
    return v > o ? v : o;
}
// the maximum over LANES (4 | 16) neighbouring lanes, in every one of them
template <int LANES>
__device__ __forceinline__ unsigned fps_row_max(unsigned v) {
    v = fps_dpp_max<DPP_XOR1, 0xf>(v);
    v = fps_dpp_max<DPP_XOR2, 0xf>(v);
    if (LANES > 4) {
        v = fps_dpp_max<DPP_HALF_MIRROR, 0xf>(v);
        v = fps_dpp_max<DPP_MIRROR, 0xf>(v);
    }
    return v;
}
// the maximum over the wave's 64 lanes, wave-uniform
__device__ __forceinline__ unsigned fps_wave_max(unsigned v) {
    v = fps_row_max<16>(v);
    v = fps_dpp_max<DPP_BCAST15, 0xa>(v);           // rows 1, 3: with the row before
    v = fps_dpp_max<DPP_BCAST31, 0xc>(v);           // rows 2, 3: with rows 0-1; lane 63 holds all
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int THREADS, int PPT>
__global__ __launch_bounds__(THREADS) void fps_kernel(FPSArgs A) {
    constexpr int W = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) float fps_cloud[];          // n points, x y z each
    __shared__ u64 slot[2][W];
    __shared__ unsigned refuse;

    const int n = A.n, k = A.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float *src = A.xyz + (long)b * A.sc;

    float px[PPT], py[PPT], pz[PPT], md[PPT];
    unsigned bad = 0;
    if (tid == 0) refuse = 0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int i = tid + j * THREADS;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (i < n) {
            const float *q = src + (long)i * A.sp;
            x = q[0]; y = q[A.sa]; z = q[2 * A.sa];
            fps_cloud[3 * i] = x; fps_cloud[3 * i + 1] = y; fps_cloud[3 * i + 2] = z;
        }
        bad |= (unsigned)((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) | (unsigned)((__float_as_uint(y) & 0x7f800000u) == 0x7f800000u) |
               (unsigned)((__float_as_uint(z) & 0x7f800000u) == 0x7f800000u);
        px[j] = x; py[j] = y; pz[j] = z;
        md[j] = i < n ? __builtin_inff() : 0.0f;
    }
    int sel = A.start ? A.start[b] : 0;
    bad |= (unsigned)(sel < 0 || sel >= n);
    __syncthreads();
    if (bad) refuse = 1;
    __syncthreads();                                                            // (the cloud's LDS copy is complete here too)
    int *index = A.index + b * (size_t)k;
    float *radius2 = A.radius2 ? A.radius2 + b * (size_t)k : nullptr;
    if (refuse) {                                                               // workgroup-uniform
        for (int t = tid; t < k; t += THREADS) {
            index[t] = -1;
            if (radius2) radius2[t] = __builtin_nanf("");
        }
        if (tid == 0 && A.status) A.status[b] = DPF_FPS_REFUSED;
        return;
    }

    int out_sel = 0;
    unsigned out_r = 0;
    for (int t = 0; t < k; ++t) {
        const float wx = fps_cloud[3 * sel], wy = fps_cloud[3 * sel + 1], wz = fps_cloud[3 * sel + 2];
        unsigned bh = 0, bi = 0;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const float dx = px[j] - wx, dy = py[j] - wy, dz = pz[j] - wz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const float m = d < md[j] ? d : md[j];
            md[j] = m;
            const unsigned bits = __float_as_uint(m);
            if (j == 0 || bits > bh) { bh = bits; bi = (unsigned)(tid + j * THREADS); }   // (ascending index: strictly greater keeps the lowest)
        }
        unsigned hi = fps_wave_max(bh);
        unsigned lo = fps_wave_max(bh == hi ? ~bi : 0u);
        if constexpr (W > 1) {
            if (lane == 0) slot[t & 1][wave] = ((u64)hi << 32) | lo;
            __syncthreads();
            const u64 s = slot[t & 1][lane & (W - 1)];
            const unsigned shi = (unsigned)(s >> 32), slo = (unsigned)s;
            hi = fps_row_max<W>(shi);
            lo = fps_row_max<W>(shi == hi ? slo : 0u);
            hi = (unsigned)__builtin_amdgcn_readfirstlane((int)hi);
            lo = (unsigned)__builtin_amdgcn_readfirstlane((int)lo);
        }
        const int r = t & (THREADS - 1);
        if (tid == r) { out_sel = sel; out_r = hi; }
        if (r == THREADS - 1 || t == k - 1) {                                   // workgroup-uniform: store the rounds since the last store
            const int t0 = t - r;
            if (tid <= r) {
                index[t0 + tid] = out_sel;
                if (radius2) radius2[t0 + tid] = __uint_as_float(out_r);
            }
        }
        sel = (int)~lo;
    }
    if (tid == 0 && A.status) A.status[b] = 0;
}

constexpr int FPS_KERNELS = 3 * 6;
LdsLimit fps_lds_limit[FPS_KERNELS];

template <int THREADS, int PPT>
int fps_launch_one(int B, const FPSArgs &A, int slot, hipStream_t s) {
    const int lds = (A.n * 12 + 15) & ~15;
    if (hipError_t e = fps_lds_limit[slot].ensure((const void *)fps_kernel<THREADS, PPT>, lds); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((fps_kernel<THREADS, PPT>), dim3((unsigned)B), dim3(THREADS), lds, s, A);
    return (int)hipGetLastError();
}

// the instantiations: every power of two up to the form's most points per thread
template <int THREADS, int MAXPPT, int PPT = 1>
int fps_launch_ppt(int B, const FPSArgs &A, int ppt, int slot, hipStream_t s) {
    if (ppt == PPT) return fps_launch_one<THREADS, PPT>(B, A, slot, s);
    if constexpr (2 * PPT <= MAXPPT) return fps_launch_ppt<THREADS, MAXPPT, 2 * PPT>(B, A, ppt, slot + 1, s);
    return DPF_ENOSUP;
}

}  // namespace

extern "C" int dpf_fps_max_points(void) { return dispatch::FPS_MAX_POINTS; }

extern "C" int dpf_fps(int B, int n, const float *xyz, long cloud_stride, long point_stride, long axis_stride, int k, const int *start,
                       int form, int *index, float *radius2, int *status, dpf_stream_t stream) {
    if (B < 0 || n < 1 || k < 1 || k > n || form < 0 || form > 3) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!xyz || !index) return DPF_EINVAL;
    const dispatch::FPSForm f = dispatch::fps_form(n, form);
    if (f.kernel == dispatch::FPSKernel::Unserved) return DPF_ENOSUP;
    const FPSArgs A{xyz, cloud_stride, point_stride, axis_stride, n, k, start, index, radius2, status};
    switch (f.kernel) {
        case dispatch::FPSKernel::Wave: return fps_launch_ppt<64, dispatch::FPS_WAVE_MAX / 64>(B, A, f.ppt, 0, (hipStream_t)stream);
        case dispatch::FPSKernel::Quad: return fps_launch_ppt<256, dispatch::FPS_QUAD_MAX / 256>(B, A, f.ppt, 6, (hipStream_t)stream);
        default: return fps_launch_ppt<1024, dispatch::FPS_MAX_POINTS / 1024>(B, A, f.ppt, 12, (hipStream_t)stream);
    }
}
