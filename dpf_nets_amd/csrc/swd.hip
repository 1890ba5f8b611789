// Sliced 2-Wasserstein distance: project every cloud on L directions, sort each projection ONCE per cloud, then a pair costs L * n
// subtract-square-adds over two sorted tables.  The contract (strides, arithmetic, order, refusals, the float64 sums, the gradient) is
// in include/dpf_hip.h; tests/swd_ref.py restates it in numpy.
//
// dpf_swd_tables -- one workgroup per (cloud, direction), nothing wider.  A key is one 64-bit value: the order-preserving integer
//   image of the projection in the high word, the point's index in the low word, so a compare-exchange is ONE comparison, every key is
//   distinct and the lowest index comes first among equal values for free.  The network is the bitonic one over THREADS * KPT keys
//   (the power-of-two class of n; a padding key has an all-ones high word, above every finite value).  Element e of wave w lies in
//   register j of lane `lane` with e = w * 64 * KPT + j * 64 + lane, so
//     strides 1 .. 32             are cross-lane moves: DPP quad permutes (1, 2), ds_swizzle xor masks (4, 8, 16), one bpermute (32);
//     strides 64 .. 32 * KPT      are compare-exchanges between two registers of one thread;
//     strides 64 * KPT and above  (between waves) go through LDS: the keys are stored once, every such stride is one pass of
//                                 conflict-free 8-byte accesses (a thread owns pair p: consecutive lanes, consecutive keys) and a barrier,
//                                 and the keys return to registers for the strides below.
//   A bitonic network and not a radix sort: at n = 2048 (KPT = 8, four waves) the network is 66 strides, 3 of them through LDS, about
//   9 VALU instructions a key and stride; a stable LSD radix sort of the 32-bit value needs 4 passes of 8 bits, each a histogram
//   (LDS atomics), a 256-bin scan and a scatter of 8-byte records through LDS with data-dependent bank conflicts, and its cost does not
//   fall with n.  The network's control flow is the same for every input, which is also what makes its time predictable.
//   Refusal needs the whole cloud's verdict in every one of its L workgroups.  Each takes the largest magnitude among the 3n
//   coordinates (it reads them anyway) and among the 3L direction components: a non-finite one refuses; a product of the two maxima
//   below 2^125 proves every projection finite (three products below 2^125 each sum to less than 2^127); only otherwise does the
//   workgroup evaluate all L * n projections -- the same verdict in every workgroup of the cloud, from the same arithmetic.
// dpf_swd_pairwise -- a workgroup owns a TILE x TILE block of the matrix and walks the flat (l, r) range in slices of 32 staged in LDS
//   (transposed: [element][cloud], so a thread's clouds are one 8-byte read); a thread owns a 2 x 2 block of pairs, so a table value
//   loaded from memory serves TILE = 32 pairs.  float64 accumulators, one owner thread per pair, no atomics.
// dpf_swd_grad -- scatter g = sa - sb through `order` into a (B, L, n) workspace (the targets are a permutation: unique), then one
//   thread per point sums over l in ascending order in float64.
//
// Bounded: every loop runs over n, log n, L or L * n.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "lds_attr.h"

namespace {

typedef unsigned long long u64;

struct SWDArgs {
    const float *xyz;
    long sc, sp, sa;                                // floats between clouds, points, axes
    int n, L;
    const float *dirs;                              // (L, 3)
    float *sorted;                                  // (B, L, n)
    int *order;                                     // (B, L, n) or NULL
    int *status;                                    // (B) or NULL
};

constexpr unsigned SWD_INF_BITS = 0x7f800000u;

// the partner's value at lane ^ S
template <int S>
__device__ __forceinline__ unsigned swd_xor32(unsigned v) {
    if constexpr (S == 1) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
    else if constexpr (S == 2) return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false); // quad_perm [2,3,0,1]
    else if constexpr (S < 32) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (S << 10));              // and 0x1f, or 0, xor S
    else return (unsigned)__shfl_xor((int)v, 32, 64);
}
template <int S>
__device__ __forceinline__ u64 swd_xor(u64 v) {
    return ((u64)swd_xor32<S>((unsigned)(v >> 32)) << 32) | swd_xor32<S>((unsigned)v);
}

__device__ __forceinline__ float swd_project(const float *q, long sa, float tx, float ty, float tz) {
    const float x = q[0], y = q[sa], z = q[2 * sa];
    return ((x * tx + y * ty) + z * tz) + 0.0f;
}

template <int THREADS, int KPT>
__global__ __launch_bounds__(THREADS) void swd_sort_kernel(SWDArgs A) {
    constexpr int W = THREADS / 64, CHUNK = 64 * KPT, N = THREADS * KPT;
    extern __shared__ __attribute__((aligned(16))) u64 swd_keys[];             // N keys where W > 1, nothing otherwise
    __shared__ unsigned red[3];                                                 // largest |coordinate| bits, |direction| bits, a flag

    const int n = A.n, L = A.L, tid = threadIdx.x, lane = tid & 63, wbase = (tid >> 6) * CHUNK;
    const unsigned b = blockIdx.x / (unsigned)L, l = blockIdx.x % (unsigned)L;
    const float *src = A.xyz + (long)b * A.sc;
    const float tx = A.dirs[3 * l], ty = A.dirs[3 * l + 1], tz = A.dirs[3 * l + 2];

    if (tid < 3) red[tid] = 0;
    __syncthreads();
    u64 r[KPT];
    unsigned cmax = 0, dmax = 0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int e = wbase + j * 64 + lane;
        unsigned hi = 0xFFFFFFFFu;
        if (e < n) {
            const float *q = src + (long)e * A.sp;
            const unsigned ax = __float_as_uint(q[0]) & 0x7fffffffu, ay = __float_as_uint(q[A.sa]) & 0x7fffffffu,
                           az = __float_as_uint(q[2 * A.sa]) & 0x7fffffffu;
            cmax = max(cmax, max(ax, max(ay, az)));
            const unsigned bits = __float_as_uint(swd_project(q, A.sa, tx, ty, tz));
            hi = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
        }
        r[j] = ((u64)hi << 32) | (unsigned)e;
    }
    for (int t = tid; t < 3 * L; t += THREADS) dmax = max(dmax, __float_as_uint(A.dirs[t]) & 0x7fffffffu);
    atomicMax(&red[0], cmax);
    atomicMax(&red[1], dmax);
    __syncthreads();
    cmax = red[0];
    dmax = red[1];
    bool refused = cmax >= SWD_INF_BITS || dmax >= SWD_INF_BITS;
    if (!refused && !(__uint_as_float(cmax) * __uint_as_float(dmax) < 0x1p125f)) {      // workgroup-uniform: the rare full check
        unsigned bad = 0;
        for (int e = tid; e < n; e += THREADS) {
            const float *q = src + (long)e * A.sp;
            for (int m = 0; m < L; ++m) {
                const unsigned bits = __float_as_uint(swd_project(q, A.sa, A.dirs[3 * m], A.dirs[3 * m + 1], A.dirs[3 * m + 2]));
                bad |= (unsigned)((bits & SWD_INF_BITS) == SWD_INF_BITS);
            }
        }
        if (bad) red[2] = 1;
        __syncthreads();
        refused = red[2] != 0;
    }
    const size_t row = ((size_t)b * L + l) * (size_t)n;
    float *sorted = A.sorted + row;
    int *order = A.order ? A.order + row : nullptr;
    if (refused) {                                                              // workgroup-uniform
        for (int e = tid; e < n; e += THREADS) {
            sorted[e] = __builtin_nanf("");
            if (order) order[e] = -1;
        }
        if (tid == 0 && l == 0 && A.status) A.status[b] = DPF_SWD_REFUSED;
        return;
    }

#pragma unroll 1
    for (int k = 2; k <= N; k <<= 1) {
        if constexpr (W > 1) {
            if (k > CHUNK) {                                                    // the strides between waves
#pragma unroll
                for (int j = 0; j < KPT; ++j) swd_keys[wbase + j * 64 + lane] = r[j];
                __syncthreads();
#pragma unroll 1
                for (int s = k >> 1; s >= CHUNK; s >>= 1) {
#pragma unroll
                    for (int q = 0; q < (KPT + 1) / 2; ++q) {
                        const int p = tid + q * THREADS;
                        if (p >= N / 2) continue;                               // (KPT == 1: half the threads own a pair)
                        const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1));
                        const u64 a = swd_keys[i], c = swd_keys[i | s];
                        if ((a > c) == ((i & k) == 0)) { swd_keys[i] = c; swd_keys[i | s] = a; }
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int j = 0; j < KPT; ++j) r[j] = swd_keys[wbase + j * 64 + lane];
            }
        }
#pragma unroll
        for (int s = CHUNK / 2; s >= 64; s >>= 1) {                             // between two registers of a thread
            if (s < k) {
#pragma unroll
                for (int j = 0; j < KPT; ++j) {
                    if (j & (s / 64)) continue;
                    const bool asc = ((wbase + j * 64 + lane) & k) == 0;
                    const u64 a = r[j], c = r[j | (s / 64)];
                    const bool sw = (a > c) == asc;
                    r[j] = sw ? c : a;
                    r[j | (s / 64)] = sw ? a : c;
                }
            }
        }
#define SWD_LANE_STRIDE(S)                                                              \
        if (S < k) {                                                                    \
            _Pragma("unroll") for (int j = 0; j < KPT; ++j) {                           \
                const u64 o = swd_xor<S>(r[j]);                                         \
                const bool keep_min = ((lane & S) == 0) == (((wbase + j * 64 + lane) & k) == 0); \
                r[j] = (keep_min ? o < r[j] : o > r[j]) ? o : r[j];                     \
            }                                                                           \
        }
        SWD_LANE_STRIDE(32) SWD_LANE_STRIDE(16) SWD_LANE_STRIDE(8) SWD_LANE_STRIDE(4) SWD_LANE_STRIDE(2) SWD_LANE_STRIDE(1)
#undef SWD_LANE_STRIDE
    }

#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int e = wbase + j * 64 + lane;
        if (e < n) {                                                            // (the padding keys sort behind every real one)
            const unsigned hi = (unsigned)(r[j] >> 32);
            sorted[e] = __uint_as_float(hi ^ ((hi >> 31) ? 0x80000000u : 0xFFFFFFFFu));
            if (order) order[e] = (int)(unsigned)r[j];
        }
    }
    if (tid == 0 && l == 0 && A.status) A.status[b] = 0;
}

constexpr int SWD_KERNELS = 3 * 6;
LdsLimit swd_lds_limit[SWD_KERNELS];

template <int THREADS, int KPT>
int swd_launch_one(long sorts, const SWDArgs &A, int slot, hipStream_t s) {
    const int lds = THREADS > 64 ? THREADS * KPT * 8 : 0;
    if (hipError_t e = swd_lds_limit[slot].ensure((const void *)swd_sort_kernel<THREADS, KPT>, lds); e != hipSuccess) return (int)e;
    // a launch holds fewer than 2^32 threads: whole clouds per launch, one launch for anything below that
    const long per = ((1L << 32) - 1) / THREADS / A.L;
    if (per < 1) return DPF_ENOSUP;
    const long B = sorts / A.L;
    for (long b0 = 0; b0 < B; b0 += per) {
        const long nb = B - b0 < per ? B - b0 : per;
        SWDArgs C = A;
        C.xyz += b0 * A.sc;
        C.sorted += (size_t)b0 * A.L * A.n;
        if (C.order) C.order += (size_t)b0 * A.L * A.n;
        if (C.status) C.status += b0;
        hipLaunchKernelGGL((swd_sort_kernel<THREADS, KPT>), dim3((unsigned)(nb * A.L)), dim3(THREADS), lds, s, C);
    }
    return (int)hipGetLastError();
}

// the instantiations: every power of two up to the form's most keys per thread
template <int THREADS, int MAXKPT, int KPT = 1>
int swd_launch_kpt(long sorts, const SWDArgs &A, int kpt, int slot, hipStream_t s) {
    if (kpt == KPT) return swd_launch_one<THREADS, KPT>(sorts, A, slot, s);
    if constexpr (2 * KPT <= MAXKPT) return swd_launch_kpt<THREADS, MAXKPT, 2 * KPT>(sorts, A, kpt, slot + 1, s);
    return DPF_ENOSUP;
}

// ---- pair sums --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_pairs_kernel(long total, const float *ta, const int *sta, long a_stride, const float *tb,
                                                         const int *stb, long b_stride, int accumulate, double *out) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float *pa = ta + b * (size_t)a_stride * (size_t)total, *pb = tb + b * (size_t)b_stride * (size_t)total;
    double acc = 0.0;
    for (long e = tid; e < total; e += 256) {
        const double d = (double)(pa[e] - pb[e]);
        acc = __builtin_fma(d, d, acc);                                         // (d * d is exact in float64: the fusion changes no bit)
    }
    part[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const bool refused = sta[b * (size_t)a_stride] != 0 || stb[b * (size_t)b_stride] != 0;
        const double v = refused ? (double)__builtin_nanf("") : part[0];
        out[b] = accumulate ? out[b] + v : v;
    }
}

constexpr int SWD_SLICE = 32, SWD_PITCH = 68;       // elements of (l, r) per staged slice; floats between two elements' cloud rows
constexpr int SWD_TM = 2;                           // pairs per thread and side: a 32 x 32 block of the matrix per workgroup

// TM x TM pairs a thread, 16 x 16 threads: a (16 TM) x (16 TM) block of the matrix per workgroup
template <int TM>
__global__ __launch_bounds__(256) void swd_pairwise_kernel(int N1, int N2, long total, const float *t1, const int *st1, const float *t2,
                                                            const int *st2, int accumulate, double *out) {
    constexpr int TILE = 16 * TM;
    __shared__ __attribute__((aligned(16))) float As[SWD_SLICE][SWD_PITCH], Bs[SWD_SLICE][SWD_PITCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    double acc[TM][TM];
#pragma unroll
    for (int u = 0; u < TM; ++u)
#pragma unroll
        for (int v = 0; v < TM; ++v) acc[u][v] = 0.0;

    for (long k0 = 0; k0 < total; k0 += SWD_SLICE) {
#pragma unroll
        for (int q = 0; q < TILE * SWD_SLICE / 256; ++q) {                      // consecutive lanes, consecutive elements of one cloud
            const int idx = tid + q * 256, c = idx / SWD_SLICE, k = idx % SWD_SLICE;
            const long e = k0 + k;
            As[k][c] = (i0 + c < N1 && e < total) ? t1[(size_t)(i0 + c) * (size_t)total + e] : 0.0f;
            Bs[k][c] = (j0 + c < N2 && e < total) ? t2[(size_t)(j0 + c) * (size_t)total + e] : 0.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SWD_SLICE; ++k) {
            float a[TM], c[TM];
#pragma unroll
            for (int u = 0; u < TM; ++u) { a[u] = As[k][ty * TM + u]; c[u] = Bs[k][tx * TM + u]; }
#pragma unroll
            for (int u = 0; u < TM; ++u)
#pragma unroll
                for (int v = 0; v < TM; ++v) {
                    const double d = (double)(a[u] - c[v]);
                    acc[u][v] = __builtin_fma(d, d, acc[u][v]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < TM; ++u) {
        const int i = i0 + ty * TM + u;
        if (i >= N1) continue;
        const bool ri = st1[i] != 0;
#pragma unroll
        for (int v = 0; v < TM; ++v) {
            const int j = j0 + tx * TM + v;
            if (j >= N2) continue;
            const double val = (ri || st2[j] != 0) ? (double)__builtin_nanf("") : acc[u][v];
            double *o = out + (size_t)i * (size_t)N2 + j;
            *o = accumulate ? *o + val : val;
        }
    }
}

// ---- gradient ---------------------------------------------------------------------------------------------------------------------
// ws[b][l][order[b][l][r]] = sa[b][l][r] - sb[b][l][r]; grid (L, B), threads over r
__global__ __launch_bounds__(256) void swd_grad_scatter_kernel(int n, const float *sa, const float *sb, const int *order, const int *sta,
                                                                const int *stb, float *ws) {
    const size_t b = blockIdx.y, row = (b * gridDim.x + blockIdx.x) * (size_t)n;
    if (sta[b] != 0 || stb[b] != 0) return;                                     // (a refused side's order is -1: nothing to scatter)
    for (int r = threadIdx.x; r < n; r += 256) {
        const int i = order[row + r];
        if ((unsigned)i < (unsigned)n) ws[row + i] = sa[row + r] - sb[row + r];
    }
}

// grad[b][i][:] = fl32(grad_cost[b] * (sign * 2 / (L n)) * sum_l g[b][l][i] * theta[l][:]); one thread per point, l ascending
__global__ __launch_bounds__(256) void swd_grad_reduce_kernel(int L, int n, const float *dirs, const float *ws, const int *sta,
                                                               const int *stb, const float *grad_cost, double sign, float *grad) {
    const size_t b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float *g = grad + (b * (size_t)n + i) * 3;
    if (sta[b] != 0 || stb[b] != 0) { g[0] = 0.0f; g[1] = 0.0f; g[2] = 0.0f; return; }
    const float *w = ws + b * (size_t)L * (size_t)n + i;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int l = 0; l < L; ++l) {
        const double v = (double)w[(size_t)l * (size_t)n];
        sx = __builtin_fma(v, (double)dirs[3 * l], sx);                          // (a float x float product is exact in float64)
        sy = __builtin_fma(v, (double)dirs[3 * l + 1], sy);
        sz = __builtin_fma(v, (double)dirs[3 * l + 2], sz);
    }
    const double scale = (double)grad_cost[b] * (sign * 2.0 / ((double)L * (double)n));
    g[0] = (float)(scale * sx);
    g[1] = (float)(scale * sy);
    g[2] = (float)(scale * sz);
}

}  // namespace

extern "C" int dpf_swd_max_points(void) { return dispatch::SWD_MAX_POINTS; }

extern "C" int dpf_swd_tables(int B, int n, const float *xyz, long cloud_stride, long point_stride, long axis_stride, int L,
                              const float *dirs, int form, float *sorted, int *order, int *status, dpf_stream_t stream) {
    if (B < 0 || n < 1 || L < 1 || form < 0 || form > 3) return DPF_EINVAL;
    if ((long)B * (long)L >= (1L << 31)) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!xyz || !dirs || !sorted) return DPF_EINVAL;
    const dispatch::SWDForm f = dispatch::swd_form(n, form);
    if (f.kernel == dispatch::SWDKernel::Unserved) return DPF_ENOSUP;
    const SWDArgs A{xyz, cloud_stride, point_stride, axis_stride, n, L, dirs, sorted, order, status};
    const long sorts = (long)B * L;
    switch (f.kernel) {
        case dispatch::SWDKernel::Wave: return swd_launch_kpt<64, dispatch::SWD_WAVE_MAX / 64>(sorts, A, f.kpt, 0, (hipStream_t)stream);
        case dispatch::SWDKernel::Quad: return swd_launch_kpt<256, dispatch::SWD_QUAD_MAX / 256>(sorts, A, f.kpt, 6, (hipStream_t)stream);
        default: return swd_launch_kpt<1024, dispatch::SWD_MAX_POINTS / 1024>(sorts, A, f.kpt, 12, (hipStream_t)stream);
    }
}

extern "C" int dpf_swd_pairs(int B, int L, int n, const float *sorted_a, const int *status_a, long a_stride, const float *sorted_b,
                             const int *status_b, long b_stride, int accumulate, double *sumsq, dpf_stream_t stream) {
    if (B < 0 || L < 1 || n < 1 || a_stride < 0 || b_stride < 0 || (accumulate != 0 && accumulate != 1)) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!sorted_a || !status_a || !sorted_b || !status_b || !sumsq) return DPF_EINVAL;
    hipLaunchKernelGGL(swd_pairs_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (long)L * n, sorted_a, status_a, a_stride,
                       sorted_b, status_b, b_stride, accumulate, sumsq);
    return (int)hipGetLastError();
}

extern "C" int dpf_swd_pairwise(int N1, int N2, int L, int n, const float *sorted1, const int *status1, const float *sorted2,
                                const int *status2, int accumulate, double *sumsq, dpf_stream_t stream) {
    if (N1 < 0 || N2 < 0 || L < 1 || n < 1 || (accumulate != 0 && accumulate != 1)) return DPF_EINVAL;
    if (N1 == 0 || N2 == 0) return 0;
    if (!sorted1 || !status1 || !sorted2 || !status2 || !sumsq) return DPF_EINVAL;
    const long total = (long)L * n;
    constexpr int TILE = 16 * SWD_TM;
    if ((N1 + TILE - 1) / TILE > 65535) return DPF_ENOSUP;
    hipLaunchKernelGGL(swd_pairwise_kernel<SWD_TM>, dim3((unsigned)((N2 + TILE - 1) / TILE), (unsigned)((N1 + TILE - 1) / TILE)), dim3(256),
                       0, (hipStream_t)stream, N1, N2, total, sorted1, status1, sorted2, status2, accumulate, sumsq);
    return (int)hipGetLastError();
}

extern "C" size_t dpf_swd_grad_workspace_bytes(int B, int L, int n) {
    if (B < 1 || L < 1 || n < 1) return 0;
    return (size_t)B * (size_t)L * (size_t)n * sizeof(float);
}

extern "C" int dpf_swd_grad(int B, int L, int n, const float *dirs, const float *sorted_a, const int *order_a, const int *status_a,
                            const float *sorted_b, const int *order_b, const int *status_b, const float *grad_cost, float *grad_a,
                            float *grad_b, void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || L < 1 || n < 1) return DPF_EINVAL;
    if (B == 0 || (!grad_a && !grad_b)) return 0;
    if (B > 65535 || L > 0x7fffffff / 2) return DPF_ENOSUP;
    if (!dirs || !sorted_a || !status_a || !sorted_b || !status_b || !grad_cost || !workspace) return DPF_EINVAL;
    if ((grad_a && !order_a) || (grad_b && !order_b)) return DPF_EINVAL;
    if (workspace_bytes < dpf_swd_grad_workspace_bytes(B, L, n)) return DPF_EINVAL;
    float *ws = (float *)workspace;
    const dim3 gs((unsigned)L, (unsigned)B), gr((unsigned)((n + 255) / 256), (unsigned)B);
    for (int side = 0; side < 2; ++side) {                                      // (the workspace serves one side after the other)
        float *grad = side ? grad_b : grad_a;
        if (!grad) continue;
        hipLaunchKernelGGL(swd_grad_scatter_kernel, gs, dim3(256), 0, (hipStream_t)stream, n, sorted_a, sorted_b, side ? order_b : order_a,
                           status_a, status_b, ws);
        hipLaunchKernelGGL(swd_grad_reduce_kernel, gr, dim3(256), 0, (hipStream_t)stream, L, n, dirs, ws, status_a, status_b, grad_cost,
                           side ? -1.0 : 1.0, grad);
    }
    return (int)hipGetLastError();
}
