// Occupancy-grid counting for the two Jensen-Shannon metrics of the reference: bin every point of (S, n, 3) clouds into a
// res^3 grid and count, per cell, the points (counts, 64-bit) and the clouds that put at least one point there
// (clouds_touching).  Integer atomics only: the result does not depend on the order the points arrive in.
//
//   mode 0 -- lib/networks/utils.py:45-80 (get_voxel_occ_dist): half-open cube bins, the voxel of x is the i with
//             edges[i] <= x < edges[i + 1], compared in double against the HOST's table of edges.
//   mode 1 -- lib/metrics/evaluation_metrics.py:241-280 (entropy_of_occupancy_grid): nearest cell centre among the KEPT
//             centres of the grid (all of them, or those inside the unit sphere).  The contract: the argmin over the kept
//             centres of (dx*dx + dy*dy) + dz*dz in double (fp32 inputs widened), lowest kept index on an exact tie.
//
// Mode 1's fast path.  Along each axis the centre nearest to x, lowest index on a tie, is found from a rounded guess and a
// walk over the double differences.  Rounding is monotone, so fl(d*d) is smallest where |d| is and the cell c* made of the
// three per-axis winners has a contract distance D* <= that of EVERY cell of the full grid; the kept centres are a subset
// of the full grid, so if c* is kept it attains the minimum.  What is left is the tie rule: a kept cell of lower index with
// the same rounded distance would have to win.  Kept indices grow with the flat index (i * res + j) * res + k, and a cell
// of lower flat index has i' < i, or i' = i and j' < j, or i' = i, j' = j and k' < k; since |x - c[i']| >= |x - c[i - 1]|
// for every i' < i (c grows, i is the argmin), its distance is >= that of (i-1, j, k), (i, j-1, k) or (i, j, k-1).  The
// fast path is taken only if those three distances are STRICTLY above D*; then no cell of lower index ties and c* is the
// contract's answer.  Every other point -- c* clipped away, or one of the three not strictly above -- goes to the slow path.
//
// Slow path: the workgroup compacts such points into an LDS list; each wave takes four of them at a time, its lanes stride
// over the kept centres (one load of a centre serves the four points), and the wave min-reduces (distance, index)
// lexicographically.  fp64 VALU; no packed fp32, no matrix cores.
//
// clouds_touching: a presence bitmap of the cloud (res^3 bits, LDS) per workgroup, flushed once at the end -- one atomic per
// set bit.  A cloud longer than OCC_SLICE points is split over several workgroups; those first OR their words into a
// bitmap of the cloud in the workspace and flush only the bits that were not set before, so the cloud still counts once.
//
// Compiled with -ffp-contract=off: every double operation of the contract rounds on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "zero_fill.h"

namespace {

constexpr int OCC_THREADS = 256;
constexpr int OCC_WAVES = OCC_THREADS / 64;
constexpr int OCC_SLICE = 4096;                    // points of one cloud per workgroup
constexpr int OCC_MAX_RES = 64;                    // bitmap: 64^3 bits = 32 KiB of LDS
constexpr int OCC_MAX_WGS = 32768;                 // workgroups per launch (the host loop chunks the clouds)
constexpr size_t OCC_MAX_WS = (size_t)64 << 20;    // bytes of per-cloud bitmaps per launch (split clouds only)
constexpr int OCC_PB = 4;                          // slow points a wave scans together

struct OccArgs {
    const float *clouds;                           // first cloud of this launch
    int n, res, slices, K;
    const double *edges;
    const float *centres;
    const int *kept;
    const float *kept_xyz;
    unsigned long long *counts;
    unsigned int *touching;
    unsigned int *flags;
    unsigned int *cloud_bits;                      // (clouds of the launch, words) or NULL when slices == 1
    float warn_bound;
};

__device__ __forceinline__ int occ_words(int res) { return (res * res * res + 31) >> 5; }

__device__ __forceinline__ void occ_commit(const OccArgs &a, unsigned int *bits, int cell) {
    atomicAdd(&a.counts[cell], 1ull);
    atomicOr(&bits[cell >> 5], 1u << (cell & 31));
}

// the index of the edge interval that holds x, or -1 (outside the cube)
__device__ __forceinline__ int occ_bin(double x, const double *e, int res) {
    double t = (x + 0.5) * (double)res;
    t = fmin(fmax(t, 0.0), (double)(res - 1));
    int i = (int)t;
    while (i > 0 && x < e[i]) --i;
    while (i < res - 1 && x >= e[i + 1]) ++i;
    return (e[i] <= x && x < e[i + 1]) ? i : -1;
}

// argmin_i |x - c[i]| over the increasing table c, lowest index on a tie
__device__ __forceinline__ int occ_nearest(double x, const double *c, int res) {
    double t = (x + 0.5) * (double)(res - 1);
    t = fmin(fmax(t, 0.0), (double)(res - 1));
    int i = (int)rint(t);
    while (i > 0 && fabs(x - c[i - 1]) <= fabs(x - c[i])) --i;
    while (i < res - 1 && fabs(x - c[i + 1]) < fabs(x - c[i])) ++i;
    return i;
}

__device__ __forceinline__ double occ_d2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

__global__ __launch_bounds__(OCC_THREADS) void occ_kernel(OccArgs a, int mode) {
    extern __shared__ double occ_lds[];
    const int res = a.res, nw = occ_words(res), tid = threadIdx.x;
    double *tab = occ_lds;                                          // res + 1 edges, or res centres widened
    unsigned int *bits = (unsigned int *)(tab + res + 1);           // nw words
    unsigned int *slow = bits + nw;                                 // OCC_THREADS point indices
    unsigned int *slow_n = slow + OCC_THREADS;

    const int cloud = blockIdx.x / a.slices, slice = blockIdx.x - cloud * a.slices;
    const float *pts = a.clouds + (size_t)cloud * (size_t)a.n * 3;
    const int p0 = slice * OCC_SLICE, p1 = min(a.n, p0 + OCC_SLICE);

    for (int i = tid; i < res + (mode == 0); i += OCC_THREADS) tab[i] = mode == 0 ? a.edges[i] : (double)a.centres[i];
    for (int w = tid; w < nw; w += OCC_THREADS) bits[w] = 0u;
    if (tid == 0) *slow_n = 0u;
    __syncthreads();

    for (int base = p0; base < p1; base += OCC_THREADS) {
        const int p = base + tid;
        if (p < p1) {
            const float fx = pts[(size_t)p * 3], fy = pts[(size_t)p * 3 + 1], fz = pts[(size_t)p * 3 + 2];
            const int nan = (fx != fx) + (fy != fy) + (fz != fz);
            const int far = (fabsf(fx) > a.warn_bound) + (fabsf(fy) > a.warn_bound) + (fabsf(fz) > a.warn_bound);
            const bool finite = fabsf(fx) <= 3.402823466e38f && fabsf(fy) <= 3.402823466e38f && fabsf(fz) <= 3.402823466e38f;
            if (!finite) atomicAdd(&a.flags[0], 1u);
            if (nan) atomicAdd(&a.flags[1], (unsigned int)nan);
            if (far) atomicOr(&a.flags[2], 1u);
            const double x = (double)fx, y = (double)fy, z = (double)fz;
            if (mode == 0) {
                if (!nan) {                                         // (an infinite coordinate is outside every interval)
                    const int i = occ_bin(x, tab, res), j = occ_bin(y, tab, res), k = occ_bin(z, tab, res);
                    if ((i | j | k) >= 0) occ_commit(a, bits, (i * res + j) * res + k);
                }
            } else if (finite) {
                const int i = occ_nearest(x, tab, res), j = occ_nearest(y, tab, res), k = occ_nearest(z, tab, res);
                const double dx = x - tab[i], dy = y - tab[j], dz = z - tab[k];
                const double best = occ_d2(dx, dy, dz);
                bool fast = true;                                   // no cell of lower index may tie (header)
                if (i > 0) fast = fast && occ_d2(x - tab[i - 1], dy, dz) > best;
                if (j > 0) fast = fast && occ_d2(dx, y - tab[j - 1], dz) > best;
                if (k > 0) fast = fast && occ_d2(dx, dy, z - tab[k - 1]) > best;
                int cell = (i * res + j) * res + k;
                if (a.kept) cell = a.kept[cell];
                if (fast && cell >= 0) occ_commit(a, bits, cell);
                else slow[atomicAdd(slow_n, 1u)] = (unsigned int)p;
            }
        }
        if (mode == 0) continue;
        __syncthreads();
        const int m = (int)*slow_n, wave = tid >> 6, lane = tid & 63;
        for (int q0 = wave * OCC_PB; q0 < m; q0 += OCC_WAVES * OCC_PB) {
            double px[OCC_PB], py[OCC_PB], pz[OCC_PB], bd[OCC_PB];
            int bi[OCC_PB];
#pragma unroll
            for (int u = 0; u < OCC_PB; ++u) {
                const size_t q = (size_t)slow[min(q0 + u, m - 1)] * 3;            // (a short last group repeats a point)
                px[u] = (double)pts[q]; py[u] = (double)pts[q + 1]; pz[u] = (double)pts[q + 2];
                bd[u] = __builtin_huge_val(); bi[u] = 0x7fffffff;
            }
            for (int c = lane; c < a.K; c += 64) {
                const double cx = (double)a.kept_xyz[(size_t)c * 3], cy = (double)a.kept_xyz[(size_t)c * 3 + 1],
                             cz = (double)a.kept_xyz[(size_t)c * 3 + 2];
#pragma unroll
                for (int u = 0; u < OCC_PB; ++u) {
                    const double d = occ_d2(px[u] - cx, py[u] - cy, pz[u] - cz);
                    if (d < bd[u]) { bd[u] = d; bi[u] = c; }                      // c grows: the lowest index of a tie stays
                }
            }
#pragma unroll
            for (int u = 0; u < OCC_PB; ++u) {
                for (int off = 32; off > 0; off >>= 1) {
                    const double od = __shfl_xor(bd[u], off);
                    const int oi = __shfl_xor(bi[u], off);
                    if (od < bd[u] || (od == bd[u] && oi < bi[u])) { bd[u] = od; bi[u] = oi; }
                }
                if (lane == u && q0 + u < m && bi[u] < a.K) occ_commit(a, bits, bi[u]);
            }
        }
        __syncthreads();
        if (tid == 0) *slow_n = 0u;
        __syncthreads();
    }

    __syncthreads();
    unsigned int *shared_bits = a.cloud_bits ? a.cloud_bits + (size_t)cloud * nw : nullptr;
    for (int w = tid; w < nw; w += OCC_THREADS) {
        unsigned int b = bits[w];
        if (b && shared_bits) b &= ~atomicOr(&shared_bits[w], b);   // another slice of this cloud was here first
        while (b) {
            const int s = __ffs(b) - 1;
            b &= b - 1;
            atomicAdd(&a.touching[w * 32 + s], 1u);
        }
    }
}

// clouds per launch and the bytes of their shared bitmaps
inline int occ_chunk(int n, int res, int *slices_out, size_t *ws_out) {
    const int slices = (n + OCC_SLICE - 1) / OCC_SLICE;
    const size_t words = ((size_t)res * res * res + 31) / 32;
    size_t chunk = (size_t)OCC_MAX_WGS / (size_t)slices;
    if (slices > 1) {
        const size_t fit = OCC_MAX_WS / (words * 4);
        if (chunk > fit) chunk = fit;
    }
    if (chunk < 1) chunk = 1;
    *slices_out = slices;
    *ws_out = slices > 1 ? chunk * words * 4 : 0;
    return (int)chunk;
}

}  // namespace

extern "C" int dpf_occupancy_max_res(void) { return OCC_MAX_RES; }

extern "C" size_t dpf_occupancy_grid_workspace_bytes(int S, int n, int res) {
    if (S < 1 || n < 1 || res < 1 || res > OCC_MAX_RES) return 0;
    int slices; size_t ws;
    const int chunk = occ_chunk(n, res, &slices, &ws);
    if (slices > 1 && S < chunk) ws = (size_t)S * (((size_t)res * res * res + 31) / 32) * 4;
    return ws;
}

extern "C" int dpf_occupancy_grid(int S, int n, const float *clouds, int res, int mode, const double *edges, const float *centres,
                                  const int *kept, const float *kept_xyz, int K, float warn_bound, unsigned long long *counts,
                                  unsigned int *clouds_touching, unsigned int *flags, void *workspace, size_t workspace_bytes,
                                  dpf_stream_t stream) {
    if (S < 1 || n < 1 || res < 1 || !clouds || !counts || !clouds_touching || !flags) return DPF_EINVAL;
    if (mode != 0 && mode != 1) return DPF_EINVAL;
    if (res > OCC_MAX_RES) return DPF_ENOSUP;
    const int cells = res * res * res;
    if (mode == 0 && (!edges || kept)) return DPF_EINVAL;
    if (mode == 1 && (res < 2 || !centres || !kept_xyz || K < 1 || K > cells || (!kept && K != cells))) return DPF_EINVAL;
    if (((uintptr_t)counts & 7) || ((uintptr_t)workspace & 3)) return DPF_EINVAL;
    const int ncells = mode == 1 ? K : cells;
    int slices; size_t ws;
    const int chunk = occ_chunk(n, res, &slices, &ws);
    if (workspace_bytes < dpf_occupancy_grid_workspace_bytes(S, n, res) || (slices > 1 && !workspace)) return DPF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = dpf_zero_async(counts, (size_t)ncells * 8, st);
    if (e == hipSuccess) e = dpf_zero_async(clouds_touching, (size_t)ncells * 4, st);
    if (e == hipSuccess) e = dpf_zero_async(flags, 16, st);
    if (e != hipSuccess) return (int)e;
    const size_t words = ((size_t)cells + 31) / 32;
    const size_t lds = (size_t)(res + 1) * 8 + words * 4 + (OCC_THREADS + 1) * 4;
    for (int c0 = 0; c0 < S; c0 += chunk) {
        const int nc = S - c0 < chunk ? S - c0 : chunk;
        if (slices > 1) {
            e = dpf_zero_async(workspace, (size_t)nc * words * 4, st);
            if (e != hipSuccess) return (int)e;
        }
        OccArgs a{clouds + (size_t)c0 * (size_t)n * 3, n, res, slices, K, edges, centres, kept, kept_xyz, counts, clouds_touching, flags,
                  slices > 1 ? (unsigned int *)workspace : nullptr, warn_bound};
        hipLaunchKernelGGL(occ_kernel, dim3((unsigned)(nc * slices)), dim3(OCC_THREADS), lds, st, a, mode);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
