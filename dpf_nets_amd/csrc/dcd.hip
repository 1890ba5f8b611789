// Density-aware Chamfer distance (dpf_dcd): from one nn_distance result per cloud -- dist1 / idx1 (n queries into m targets) and
// dist2 / idx2 (m queries into n targets) -- the counts of the queries that share a target, the bounded and count-divided terms, the
// per-cloud loss and the per-query gradient coefficients.  The contract (the term's operations, the sums' order, refusal) is in
// include/dpf_hip.h; tests/dcd_ref.py restates it in numpy.
//
// Two forms, the same bits (dispatch::dcd_form):
//   * dcd_lds_kernel -- ONE launch, one workgroup of 1024 threads a cloud.  The workgroup zeroes an int32 histogram of side 1's
//     targets in LDS, counts idx1 into it with LDS integer atomics (integer addition: the counts do not depend on the order; all n
//     queries on one target serialise on one LDS word and stay correct), meets, then walks the queries 1024 a step: a thread reads
//     count[idx[i]], forms its term and its coefficient, and the four blocks of 256 of the step run their pairwise trees in LDS
//     (stride 128, 64, ... 1; lanes past the end hold +0.0).  Thread 0 adds the block sums in ascending order.  Side 2 reuses the LDS.
//   * the workspace form -- for targets above the histogram's cap: the counts live in the workspace, cleared in-call by a kernel
//     (zero_fill.h) and filled by dcd_count_kernel with global integer atomics; dcd_term_kernel runs one workgroup of 256 per (cloud,
//     block) and writes the block's float64 sum; dcd_finish_kernel, one wave a cloud, adds the partials in ascending order.
// No floating-point atomic anywhere; nothing in the workspace has to be clear on entry; no allocation, no host synchronisation.
//
// Refusal is by cloud: an index outside its target set is never used as an address, and both forms have looked at every index of a
// cloud before they write one of its outputs.
// Compiled with -ffp-contract=off: every float64 operation rounds on its own, in the header's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "lds_attr.h"
#include "zero_fill.h"

namespace {

constexpr int DC_BLOCK = dispatch::DCD_BLOCK;
constexpr int DC_THREADS = dispatch::DCD_LDS_THREADS;
constexpr int DC_GROUPS = DC_THREADS / DC_BLOCK;     // blocks of the tree a step of the one-workgroup form

static_assert((DC_BLOCK & (DC_BLOCK - 1)) == 0 && DC_THREADS % DC_BLOCK == 0, "the tree halves a block; a step is whole blocks");
static_assert(dispatch::DCD_LDS_TARGETS * 4 + DC_THREADS * 8 <= 160 * 1024, "the histogram and the tree share the workgroup's LDS");

enum { DC_POW_ONE = 0, DC_POW_COUNT = 1, DC_POW_GENERAL = 2 };    // n_lambda == 0, == 1, anything else

struct DcdSide {
    const float *dist;      // (B, q)
    const int *idx;         // (B, q), into t targets
    int *count;             // (B, q) or NULL
    float *coef;            // (B, q) or NULL
    int *hist;              // the workspace form's counts: (B, t)
    int q, t;
    double frac;            // q / t (under non_reg at least 1)
    double h;               // (0.5 * alpha) / q
};

struct DcdArgs {
    DcdSide side[2];
    double alpha, lambda;
    int pow_kind;
    double *loss, *halves;  // (B), (B, 2) or NULL
    int *status;            // (B)
    int *bad;               // the workspace form's refusal flags: (B)
    double *partial;        //                      block sums: (B, blocks1 + blocks2)
    long blocks1, blocks2;
};

// 1 - e W and the coefficient of one query whose target c queries share (c >= 1: the query counts itself)
__device__ __forceinline__ double dc_term(const DcdArgs &A, const DcdSide &S, float d, int c, float &coef) {
    const double p = A.pow_kind == DC_POW_COUNT ? (double)c : A.pow_kind == DC_POW_ONE ? 1.0 : pow((double)c, A.lambda);
    const double W = S.frac / (p + 1e-6);
    const double e = exp(-(A.alpha * (double)d));
    const double q = e * W;
    coef = (float)(S.h * q);
    return 1.0 - q;
}

// the pairwise tree over every block of DC_BLOCK entries of red at once: the sum of block g is left in red[g * DC_BLOCK]
__device__ __forceinline__ void dc_tree(double *red, int tid) {
    const int lane = tid & (DC_BLOCK - 1);
    for (int stride = DC_BLOCK / 2; stride >= 1; stride >>= 1) {
        if (lane < stride) red[tid] = red[tid] + red[tid + stride];
        __syncthreads();
    }
}

__device__ __forceinline__ void dc_refuse_query(const DcdSide &S, size_t b, long i) {
    if (S.count) S.count[b * (size_t)S.q + (size_t)i] = -1;
    if (S.coef) S.coef[b * (size_t)S.q + (size_t)i] = __builtin_nanf("");
}

__device__ __forceinline__ void dc_finish(const DcdArgs &A, size_t b, double s1, double s2) {
    const double l1 = s1 / (double)A.side[0].q, l2 = s2 / (double)A.side[1].q;
    A.loss[b] = 0.5 * (l1 + l2);
    if (A.halves) { A.halves[b * 2] = l1; A.halves[b * 2 + 1] = l2; }
    A.status[b] = 0;
}

__device__ __forceinline__ void dc_finish_refused(const DcdArgs &A, size_t b) {
    const double nan = __builtin_nan("");
    A.loss[b] = nan;
    if (A.halves) { A.halves[b * 2] = nan; A.halves[b * 2 + 1] = nan; }
    A.status[b] = DPF_DCD_REFUSED;
}

__global__ __launch_bounds__(DC_THREADS) void dcd_lds_kernel(DcdArgs A, int b0) {
    extern __shared__ __attribute__((aligned(16))) int dc_hist[];               // max(n, m) counts
    __shared__ double red[DC_THREADS];

    const int tid = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;

    // every index of the cloud, both sides, before anything of it is written
    unsigned bad = 0;
    for (int s = 0; s < 2; ++s) {
        const DcdSide &S = A.side[s];
        const int *idx = S.idx + b * (size_t)S.q;
        for (long i = tid; i < S.q; i += DC_THREADS) bad |= (unsigned)((unsigned)idx[i] >= (unsigned)S.t);
    }
    if (__syncthreads_or((int)bad)) {
        for (int s = 0; s < 2; ++s)
            for (long i = tid; i < A.side[s].q; i += DC_THREADS) dc_refuse_query(A.side[s], b, i);
        if (tid == 0) dc_finish_refused(A, b);
        return;
    }

    double sums[2] = {0.0, 0.0};                                                // thread 0's
    for (int s = 0; s < 2; ++s) {
        const DcdSide &S = A.side[s];
        const int *idx = S.idx + b * (size_t)S.q;
        const float *dist = S.dist + b * (size_t)S.q;
        __syncthreads();                                                        // side 1's counts have been read by every thread
        for (int j = tid; j < S.t; j += DC_THREADS) dc_hist[j] = 0;
        __syncthreads();
        for (long i = tid; i < S.q; i += DC_THREADS) atomicAdd(&dc_hist[idx[i]], 1);         // (inside [0, t): checked above)
        __syncthreads();

        double acc = 0.0;
        for (long base = 0; base < S.q; base += DC_THREADS) {
            const long i = base + tid;
            double term = 0.0;
            if (i < S.q) {
                const int c = dc_hist[idx[i]];
                float coef;
                term = dc_term(A, S, dist[i], c, coef);
                if (S.count) S.count[b * (size_t)S.q + (size_t)i] = c;
                if (S.coef) S.coef[b * (size_t)S.q + (size_t)i] = coef;
            }
            __syncthreads();                                                    // the step before: thread 0 has read its block sums
            red[tid] = term;
            __syncthreads();
            dc_tree(red, tid);
            if (tid == 0) {
#pragma unroll
                for (int g = 0; g < DC_GROUPS; ++g)
                    if (base + (long)g * DC_BLOCK < S.q) acc = (base == 0 && g == 0) ? red[0] : acc + red[g * DC_BLOCK];
            }
        }
        sums[s] = acc;
    }
    if (tid == 0) dc_finish(A, b, sums[0], sums[1]);
}

// a workgroup of the workspace form's (cloud, block) launches: side 1's blocks first
__device__ __forceinline__ int dc_side_of(const DcdArgs &A, long &blk) {
    if (blk < A.blocks1) return 0;
    blk -= A.blocks1;
    return 1;
}

// launch 2 of 4: the cleared histograms are filled; an index outside its target set raises the cloud's flag instead
__global__ __launch_bounds__(DC_BLOCK) void dcd_count_kernel(DcdArgs A, int b0, long blk0) {
    const size_t b = (size_t)b0 + blockIdx.y;
    long blk = blk0 + blockIdx.x;
    const DcdSide &S = A.side[dc_side_of(A, blk)];
    const long i = blk * DC_BLOCK + threadIdx.x;
    if (i >= S.q) return;
    const int j = S.idx[b * (size_t)S.q + (size_t)i];
    if ((unsigned)j < (unsigned)S.t) atomicAdd(S.hist + b * (size_t)S.t + (size_t)j, 1);
    else atomicOr(A.bad + b, 1);
}

// launch 3 of 4: the terms of one block, their tree, the block's sum
__global__ __launch_bounds__(DC_BLOCK) void dcd_term_kernel(DcdArgs A, int b0, long blk0) {
    __shared__ double red[DC_BLOCK];
    const int tid = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    long blk = blk0 + blockIdx.x;
    const long slot = blk;
    const DcdSide &S = A.side[dc_side_of(A, blk)];
    const long i = blk * DC_BLOCK + tid;
    if (A.bad[b]) {                                                             // the same for every workgroup of the cloud
        if (i < S.q) dc_refuse_query(S, b, i);
        return;
    }
    double term = 0.0;
    if (i < S.q) {
        const int c = S.hist[b * (size_t)S.t + (size_t)S.idx[b * (size_t)S.q + (size_t)i]];     // (inside [0, t): no flag was raised)
        float coef;
        term = dc_term(A, S, S.dist[b * (size_t)S.q + (size_t)i], c, coef);
        if (S.count) S.count[b * (size_t)S.q + (size_t)i] = c;
        if (S.coef) S.coef[b * (size_t)S.q + (size_t)i] = coef;
    }
    red[tid] = term;
    __syncthreads();
    dc_tree(red, tid);
    if (tid == 0) A.partial[b * (size_t)(A.blocks1 + A.blocks2) + (size_t)slot] = red[0];
}

// launch 4 of 4: lane 0 adds side 1's block sums in ascending order, lane 1 side 2's
__global__ __launch_bounds__(64) void dcd_finish_kernel(DcdArgs A, int b0) {
    const int lane = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    if (A.bad[b]) {
        if (lane == 0) dc_finish_refused(A, b);
        return;
    }
    double acc = 0.0;
    if (lane < 2) {
        const double *part = A.partial + b * (size_t)(A.blocks1 + A.blocks2) + (lane ? (size_t)A.blocks1 : 0);
        const long nblk = lane ? A.blocks2 : A.blocks1;
        acc = part[0];
        for (long k = 1; k < nblk; ++k) acc = acc + part[k];
    }
    const double s1 = __shfl(acc, 0), s2 = __shfl(acc, 1);
    if (lane == 0) dc_finish(A, b, s1, s2);
}

// the workspace: [ (B, m) counts | (B, n) counts | (B) flags ] cleared in-call, then (8-byte aligned) the (B, blocks) partials
size_t dc_cleared_bytes(int B, int n, int m) { return (size_t)B * ((size_t)n + (size_t)m + 1) * sizeof(int); }
size_t dc_partial_offset(int B, int n, int m) { return (dc_cleared_bytes(B, n, m) + 7) & ~(size_t)7; }

LdsLimit dc_lds_limit;

}  // namespace

extern "C" size_t dpf_dcd_workspace_bytes(int B, int n, int m) {
    const dispatch::DCDForm f = dispatch::dcd_form(B, n, m, 2);
    if (f.kernel == dispatch::DCDKernel::Unserved || B < 1) return 0;
    return dc_partial_offset(B, n, m) + (size_t)B * (size_t)(f.blocks1 + f.blocks2) * sizeof(double);
}

extern "C" int dpf_dcd(int B, int n, int m, const float *dist1, const int *idx1, const float *dist2, const int *idx2, double alpha,
                       double n_lambda, int non_reg, int form, double *loss, double *halves, int *count1, int *count2, float *coef1,
                       float *coef2, int *status, void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || n < 1 || m < 1 || form < 0 || form > 2) return DPF_EINVAL;
    if (!(alpha > 0.0) || !(alpha < __builtin_inf()) || !(n_lambda >= 0.0) || !(n_lambda < __builtin_inf())) return DPF_EINVAL;
    const dispatch::DCDForm f = dispatch::dcd_form(B, n, m, form);
    if (f.kernel == dispatch::DCDKernel::Unserved) return DPF_ENOSUP;
    if (B == 0) return 0;
    if (!dist1 || !idx1 || !dist2 || !idx2 || !loss || !status || !workspace || ((uintptr_t)workspace & 7)) return DPF_EINVAL;
    if (workspace_bytes < dpf_dcd_workspace_bytes(B, n, m)) return DPF_EINVAL;
    hipStream_t s = (hipStream_t)stream;

    double frac1 = (double)n / (double)m, frac2 = (double)m / (double)n;
    if (non_reg) { frac1 = frac1 > 1.0 ? frac1 : 1.0; frac2 = frac2 > 1.0 ? frac2 : 1.0; }
    char *w = (char *)workspace;
    int *hist1 = (int *)w, *hist2 = hist1 + (size_t)B * (size_t)m, *bad = hist2 + (size_t)B * (size_t)n;
    DcdArgs A{{{dist1, idx1, count1, coef1, hist1, n, m, frac1, (0.5 * alpha) / (double)n},
               {dist2, idx2, count2, coef2, hist2, m, n, frac2, (0.5 * alpha) / (double)m}},
              alpha, n_lambda, n_lambda == 1.0 ? DC_POW_COUNT : n_lambda == 0.0 ? DC_POW_ONE : DC_POW_GENERAL,
              loss, halves, status, bad, (double *)(w + dc_partial_offset(B, n, m)), f.blocks1, f.blocks2};

    if (f.kernel == dispatch::DCDKernel::Lds) {
        const int lds = ((n > m ? n : m) * 4 + 15) & ~15;
        if (hipError_t e = dc_lds_limit.ensure((const void *)dcd_lds_kernel, lds); e != hipSuccess) return (int)e;
        return dispatch::chunk_grid(B, 1, [&](int b0, unsigned nb, long, unsigned) {
            hipLaunchKernelGGL(dcd_lds_kernel, dim3(1, nb), dim3(DC_THREADS), lds, s, A, b0);
            return (int)hipGetLastError();
        });
    }
    if (hipError_t e = dpf_zero_async(workspace, dc_cleared_bytes(B, n, m), s); e != hipSuccess) return (int)e;
    const long blocks = f.blocks1 + f.blocks2;
    if (const int e = dispatch::chunk_grid(B, blocks, [&](int b0, unsigned nb, long k0, unsigned nk) {
            hipLaunchKernelGGL(dcd_count_kernel, dim3(nk, nb), dim3(DC_BLOCK), 0, s, A, b0, k0);
            return (int)hipGetLastError();
        }))
        return e;
    if (const int e = dispatch::chunk_grid(B, blocks, [&](int b0, unsigned nb, long k0, unsigned nk) {
            hipLaunchKernelGGL(dcd_term_kernel, dim3(nk, nb), dim3(DC_BLOCK), 0, s, A, b0, k0);
            return (int)hipGetLastError();
        }))
        return e;
    return dispatch::chunk_grid(B, 1, [&](int b0, unsigned nb, long, unsigned) {
        hipLaunchKernelGGL(dcd_finish_kernel, dim3(1, nb), dim3(64), 0, s, A, b0);
        return (int)hipGetLastError();
    });
}
