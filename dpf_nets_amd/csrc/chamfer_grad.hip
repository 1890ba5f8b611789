// chamfer_grad.hip -- the DETERMINISTIC backward of the Chamfer search (include/dpf_hip.h: dpf_nndistancegrad_det,
// dpf_chamfer_cd_backward).  The atomic backward (chamfer.hip: nn_grad_scatter_kernel) adds the scattered term in whatever order
// the chip delivers it; here the order is part of the contract, per cloud and output ("target" cloud, T points; the other,
// "query" cloud has Q):
//     g[t]  = (2 * gd_t[t]) * (xt[t] - xq[idx_t[t]])                                     the direct term, as nn_grad_direct_kernel
//     g[t]  = g[t] + (-((2 * gd_q[l]) * (xq[l] - xt[t])))      for l = 0 .. Q-1 ascending, where idx_q[l] == t
// every operation a separately rounded fp32 one (the object is built with -ffp-contract=off).  No float atomics in this file.
//
// The ordering scheme: sort the keys (idx_q[l], l) -- all different -- with a bitonic network.  In sorted order every target's
// queries stand together, ascending in l.  One thread per sorted position then writes its contribution beside its key, the
// thread whose left neighbour has another target (the list's head) adds its list up, one element after the other, on top of the
// direct term.  The network's cost depends on Q alone: a collapsed cloud (every query at one target) sorts as fast as a permutation.
// What a collapsed cloud does cost is the contract's own chain of Q dependent additions; a list longer than the form's
// `long_list` goes to a whole wave, whose lanes fetch 64 contributions at a time for the one sequential sum.
//
// Two forms (dispatch::cg_form), one body (cg_merge, cg_contrib, cg_direct, cg_walk):
//   Lds        one workgroup per (cloud, output); 32-bit keys (idx << 13 | l), contributions and the long lists' queue in LDS
//   Workspace  64-bit keys (idx << 32 | l) and contributions in the caller's workspace; chunks of CG_CHUNK keys are sorted in
//              LDS, the network's wider steps run in global memory
// The workspace may come in dirty and is left dirty: every word that is read has been written by the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"
#include "dpf_hip.h"
#include "lds_attr.h"

namespace {

constexpr int CG_THREADS = 1024;       // of the LDS form's workgroup and of the chunk sorts
constexpr int CG_CHUNK = 4096;         // 64-bit keys sorted in LDS at a time (32 KB)
constexpr int CG_WALK = 256;           // sorted positions per workgroup of the workspace form's walk
constexpr int CG_LBITS = 13;           // the LDS form's key: the low bits hold l < dispatch::CG_LDS_QUERIES
static_assert((1 << CG_LBITS) == dispatch::CG_LDS_QUERIES, "the 32-bit key's query field");
static_assert((long)dispatch::CG_LDS_TARGETS << CG_LBITS <= (1l << 31), "the 32-bit key's target field; ~0u stays the padding");

// one output of one call: its gradient, the cloud it belongs to (targets) and the other one (queries)
struct Side {
    const float *xt, *xq;          // (B, T, 3), (B, Q, 3)
    const int *idx_t, *idx_q;      // (B, T) into the queries, (B, Q) into the targets
    const float *gd_t, *gd_q;      // (B, T), (B, Q) rows, or nullptr: gcd[b] / T, gcd[b] / Q
    float *g;                      // (B, T, 3)
    int T, Q;
    unsigned long long *keys;      // Workspace form: B * P keys, P = cg_pow2(Q); then B * 3Q contributions
    float *contrib;
};
struct Args { Side s[2]; const float *gcd; int long_list; };

__device__ __forceinline__ int cg_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }     // a wild index reads in bounds

struct CloudGrad { float t, q; };      // the per-cloud form's two row values
__device__ __forceinline__ CloudGrad cg_cloud_grad(const Args &A, const Side &S, int bi) {
    if (A.gcd == nullptr) return {0.f, 0.f};
    const float g = A.gcd[bi];
    return {g / (float)S.T, g / (float)S.Q};                // (correctly rounded: -fhip-fp32-correctly-rounded-divide-sqrt)
}

struct F3 { float x, y, z; };

// (2 gd_t[t]) (xt[t] - xq[idx_t[t]])
__device__ __forceinline__ F3 cg_direct(const Side &S, long bi, int t, float gscal) {
    const long u = bi * S.T + t;
    const int j2 = cg_clamp(S.idx_t[u], S.Q);
    const float g = __fmul_rn(S.gd_t ? S.gd_t[u] : gscal, 2.f);
    const float *pa = S.xt + u * 3, *pb = S.xq + (bi * S.Q + j2) * 3;
    return {__fmul_rn(g, __fsub_rn(pa[0], pb[0])), __fmul_rn(g, __fsub_rn(pa[1], pb[1])), __fmul_rn(g, __fsub_rn(pa[2], pb[2]))};
}
// -((2 gd_q[l]) (xq[l] - xt[t]))
__device__ __forceinline__ F3 cg_contrib(const Side &S, long bi, int t, int l, float gscal) {
    const long u = bi * S.Q + l;
    const float g = __fmul_rn(S.gd_q ? S.gd_q[u] : gscal, 2.f);
    const float *pa = S.xq + u * 3, *pb = S.xt + (bi * S.T + t) * 3;
    return {-__fmul_rn(g, __fsub_rn(pa[0], pb[0])), -__fmul_rn(g, __fsub_rn(pa[1], pb[1])), -__fmul_rn(g, __fsub_rn(pa[2], pb[2]))};
}

__host__ __device__ inline long cg_pow2(long q) { long p = 1; while (p < q) p <<= 1; return p; }

// the bitonic network's steps j = jstart, jstart / 2 .. 1 of stage k over a[0 .. P) (P a power of two, in LDS), element i being
// element gbase + i of the whole sequence; every thread of the workgroup calls it.  Pair x belongs to thread x % blockDim, so the
// 64 pairs of a wave's turn cover one aligned run of 128 elements when j <= 64: those steps stay inside the wave, whose LDS
// accesses execute in order, and need no workgroup barrier -- 56 of the 66 steps at 2048 keys.  The wider steps are fenced by
// barriers on both sides; the caller puts one behind the last stage before other threads read the keys.
template <typename K>
__device__ __forceinline__ void cg_merge(K *a, int P, long gbase, long k, int jstart) {
    if (jstart > 64) __syncthreads();
    for (int j = jstart; j > 0; j >>= 1) {
        for (int x = threadIdx.x; x < P / 2; x += blockDim.x) {
            const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), ixj = i | j;
            const bool up = ((gbase + i) & k) == 0;
            const K lo = a[i], hi = a[ixj];
            if ((lo > hi) == up) { a[i] = hi; a[ixj] = lo; }
        }
        if (j > 64) {
            __syncthreads();
        } else {                                // the wave's own stores before its next loads: order for the compiler, nothing to wait for
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

__device__ __forceinline__ float cg_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// The sums.  keys[0 .. Q) sorted, contrib[3p ..] the contribution of sorted position p.  The workgroup's threads take the positions
// [p0, p1): a list's head adds up to long_list elements itself; a longer list is queued (`queue`, `qcount` in LDS, qcount zero on
// entry; integer atomic: the queue's order decides nothing) and summed by one wave, 64 contributions per fetch.
template <typename K, int SHIFT>
__device__ __forceinline__ void cg_walk(const K *keys, const float *contrib, long p0, long p1, const Side &S, long bi, float gscal_t,
                                        int long_list, long *queue, int *qcount) {
    const long Q = S.Q;
    for (long p = p0 + threadIdx.x; p < p1; p += blockDim.x) {
        const int t = (int)(keys[p] >> SHIFT);
        if (p > 0 && (int)(keys[p - 1] >> SHIFT) == t) continue;                 // not a head
        F3 acc = cg_direct(S, bi, t, gscal_t);
        long i = p;
        for (int c = 0; c < long_list && i < Q && (int)(keys[i] >> SHIFT) == t; ++c, ++i) {
            acc.x = __fadd_rn(acc.x, contrib[3 * i + 0]);
            acc.y = __fadd_rn(acc.y, contrib[3 * i + 1]);
            acc.z = __fadd_rn(acc.z, contrib[3 * i + 2]);
        }
        if (i < Q && (int)(keys[i] >> SHIFT) == t) { queue[atomicAdd(qcount, 1)] = p; continue; }
        float *go = S.g + (bi * S.T + t) * 3;
        go[0] = acc.x; go[1] = acc.y; go[2] = acc.z;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, nq = *qcount;
    for (int e = threadIdx.x >> 6; e < nq; e += blockDim.x >> 6) {
        const long p = queue[e];
        const int t = (int)(keys[p] >> SHIFT);
        F3 acc = cg_direct(S, bi, t, gscal_t);                                    // (every lane the same value)
        for (long base = p;; base += 64) {
            const long i = base + lane;
            const bool mine = i < Q && (int)(keys[i] >> SHIFT) == t;              // sorted: the lanes that hold are a prefix
            const int cnt = __popcll(__ballot(mine));
            const float cx = mine ? contrib[3 * i + 0] : 0.f, cy = mine ? contrib[3 * i + 1] : 0.f, cz = mine ? contrib[3 * i + 2] : 0.f;
            for (int k = 0; k < cnt; ++k) {
                acc.x = __fadd_rn(acc.x, cg_lane(cx, k));
                acc.y = __fadd_rn(acc.y, cg_lane(cy, k));
                acc.z = __fadd_rn(acc.z, cg_lane(cz, k));
            }
            if (cnt < 64) break;
        }
        if (lane == 0) {
            float *go = S.g + (bi * S.T + t) * 3;
            go[0] = acc.x; go[1] = acc.y; go[2] = acc.z;
        }
    }
}

// ---- the LDS form: grid (B, outputs) ------------------------------------------------------------------------------------------
// dynamic LDS: P keys | 3Q contributions | the queue: Q / (long_list + 1) + 1 entries at most | its count
__host__ __device__ inline size_t cg_lds_queue(int Q, int long_list) { return (size_t)Q / (long_list + 1) + 2; }
__host__ __device__ inline size_t cg_lds_bytes(int Q, int long_list) {
    return ((size_t)cg_pow2(Q) * 4 + (size_t)Q * 12 + 7) / 8 * 8 + cg_lds_queue(Q, long_list) * 8 + 8;
}
__global__ __launch_bounds__(CG_THREADS) void cg_lds_kernel(Args A) {
    extern __shared__ __align__(8) unsigned char cg_smem[];
    const Side &S = A.s[blockIdx.y];
    const int bi = blockIdx.x, Q = S.Q, T = S.T, P = (int)cg_pow2(Q), tid = threadIdx.x;
    uint32_t *keys = (uint32_t *)cg_smem;
    float *contrib = (float *)(keys + P);
    long *queue = (long *)(cg_smem + ((size_t)P * 4 + (size_t)Q * 12 + 7) / 8 * 8);
    int *qcount = (int *)(queue + cg_lds_queue(Q, A.long_list));
    const CloudGrad cg = cg_cloud_grad(A, S, bi);
    for (int p = tid; p < P; p += CG_THREADS)
        keys[p] = p < Q ? ((uint32_t)cg_clamp(S.idx_q[(long)bi * Q + p], T) << CG_LBITS) | (uint32_t)p : ~0u;
    if (tid == 0) *qcount = 0;
    // every target's direct term; the heads write theirs again, with their sums, behind the barriers below
    for (int t = tid; t < T; t += CG_THREADS) {
        const F3 d = cg_direct(S, bi, t, cg.t);
        float *go = S.g + ((long)bi * T + t) * 3;
        go[0] = d.x; go[1] = d.y; go[2] = d.z;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) cg_merge(keys, P, 0, k, k >> 1);
    __syncthreads();
    for (int p = tid; p < Q; p += CG_THREADS) {
        const uint32_t key = keys[p];
        const F3 c = cg_contrib(S, bi, (int)(key >> CG_LBITS), (int)(key & ((1u << CG_LBITS) - 1)), cg.q);
        contrib[3 * p + 0] = c.x; contrib[3 * p + 1] = c.y; contrib[3 * p + 2] = c.z;
    }
    __syncthreads();
    cg_walk<uint32_t, CG_LBITS>(keys, contrib, 0, Q, S, bi, cg.t, A.long_list, queue, qcount);
}

// ---- the workspace form: one output per launch sequence, grid (.., B) ------------------------------------------------------------
// keys of chunk blockIdx.x, sorted as the network's stages k <= chunk length leave them
__global__ __launch_bounds__(CG_THREADS) void cg_ws_sort_kernel(Side S, int chunk) {
    __shared__ unsigned long long a[CG_CHUNK];
    const long bi = blockIdx.y, P = cg_pow2(S.Q), gbase = (long)blockIdx.x * chunk;
    for (int i = threadIdx.x; i < chunk; i += CG_THREADS) {
        const long l = gbase + i;
        a[i] = l < S.Q ? ((unsigned long long)cg_clamp(S.idx_q[bi * S.Q + l], S.T) << 32) | (unsigned long long)l : ~0ull;
    }
    __syncthreads();
    for (int k = 2; k <= chunk; k <<= 1) cg_merge(a, chunk, gbase, k, k >> 1);
    __syncthreads();
    for (int i = threadIdx.x; i < chunk; i += CG_THREADS) S.keys[bi * P + gbase + i] = a[i];
}
// step j >= chunk length of stage k: one pair per thread
__global__ __launch_bounds__(256) void cg_ws_step_kernel(Side S, long k, long j) {
    const long bi = blockIdx.y, P = cg_pow2(S.Q), x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= P / 2) return;
    const long i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), ixj = i | j;
    unsigned long long *a = S.keys + bi * P;
    const bool up = (i & k) == 0;
    const unsigned long long lo = a[i], hi = a[ixj];
    if ((lo > hi) == up) { a[i] = hi; a[ixj] = lo; }
}
// steps j < chunk length of stage k
__global__ __launch_bounds__(CG_THREADS) void cg_ws_merge_kernel(Side S, int chunk, long k) {
    __shared__ unsigned long long a[CG_CHUNK];
    const long bi = blockIdx.y, P = cg_pow2(S.Q), gbase = (long)blockIdx.x * chunk;
    for (int i = threadIdx.x; i < chunk; i += CG_THREADS) a[i] = S.keys[bi * P + gbase + i];
    __syncthreads();
    cg_merge(a, chunk, gbase, k, chunk >> 1);
    __syncthreads();
    for (int i = threadIdx.x; i < chunk; i += CG_THREADS) S.keys[bi * P + gbase + i] = a[i];
}
// the contribution of every sorted position and the direct term of every target
__global__ __launch_bounds__(256) void cg_ws_terms_kernel(Args A) {
    const Side &S = A.s[0];
    const long bi = blockIdx.y, P = cg_pow2(S.Q), u = (long)blockIdx.x * 256 + threadIdx.x;
    const CloudGrad cg = cg_cloud_grad(A, S, (int)bi);
    if (u < S.Q) {
        const unsigned long long key = S.keys[bi * P + u];
        const F3 c = cg_contrib(S, bi, (int)(key >> 32), (int)(key & 0xffffffffu), cg.q);
        float *co = S.contrib + (bi * S.Q + u) * 3;
        co[0] = c.x; co[1] = c.y; co[2] = c.z;
    }
    if (u < S.T) {
        const F3 d = cg_direct(S, bi, (int)u, cg.t);
        float *go = S.g + (bi * S.T + u) * 3;
        go[0] = d.x; go[1] = d.y; go[2] = d.z;
    }
}
__global__ __launch_bounds__(CG_WALK) void cg_ws_walk_kernel(Args A) {
    __shared__ long queue[CG_WALK + 2];
    __shared__ int qcount;
    const Side &S = A.s[0];
    const long bi = blockIdx.y, P = cg_pow2(S.Q), p0 = (long)blockIdx.x * CG_WALK, p1 = p0 + CG_WALK < S.Q ? p0 + CG_WALK : S.Q;
    const CloudGrad cg = cg_cloud_grad(A, S, (int)bi);
    if (threadIdx.x == 0) qcount = 0;
    __syncthreads();
    cg_walk<unsigned long long, 32>(S.keys + bi * P, S.contrib + bi * S.Q * 3, p0, p1, S, bi, cg.t, A.long_list, queue, &qcount);
}

size_t cg_side_ws_bytes(int b, int Q) { return (size_t)b * ((size_t)cg_pow2(Q) * 8 + (size_t)Q * 12); }

size_t cg_workspace_bytes(int b, int n, int m, const dispatch::Switches &sw) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    size_t bytes = 0;
    if (dispatch::cg_form(n, m, sw).kernel == dispatch::CGKernel::Workspace) bytes += cg_side_ws_bytes(b, m);     // grad_xyz1's
    if (dispatch::cg_form(m, n, sw).kernel == dispatch::CGKernel::Workspace) bytes += cg_side_ws_bytes(b, n);     // grad_xyz2's
    return bytes;
}

LdsLimit cg_lds_limit;

int cg_launch(int b, int n, const float *xyz1, int m, const float *xyz2, const float *gd1, const int *idx1, const float *gd2,
              const int *idx2, const float *gcd, float *g1, float *g2, void *workspace, size_t workspace_bytes, hipStream_t s) {
    if (b < 0 || n <= 0 || m <= 0) return DPF_EINVAL;
    if (b == 0) return 0;
    if (!xyz1 || !xyz2 || !idx1 || !idx2) return DPF_EINVAL;
    if ((long)n * 3 >= (1l << 31) || (long)m * 3 >= (1l << 31) || b > 65535) return DPF_ENOSUP;
    const dispatch::Switches sw = dispatch::snapshot();
    const size_t need = cg_workspace_bytes(b, n, m, sw);
    if (need && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))) return DPF_EINVAL;
    const Side sides[2] = {{xyz1, xyz2, idx1, idx2, gd1, gd2, g1, n, m, nullptr, nullptr},
                           {xyz2, xyz1, idx2, idx1, gd2, gd1, g2, m, n, nullptr, nullptr}};
    Args lds;                                            // the outputs the LDS form serves: one launch for both
    lds.gcd = gcd;
    int nlds = 0, lds_bytes = 0;
    unsigned char *ws = (unsigned char *)workspace;
    for (int o = 0; o < 2; ++o) {
        Side S = sides[o];
        const dispatch::CGForm form = dispatch::cg_form(S.T, S.Q, sw);
        unsigned char *mine = ws;
        if (form.kernel == dispatch::CGKernel::Workspace) ws += cg_side_ws_bytes(b, S.Q);      // (the layout does not depend on the NULLs)
        if (S.g == nullptr) continue;
        if (form.kernel == dispatch::CGKernel::Lds) {
            lds.s[nlds++] = S;
            lds.long_list = form.long_list;
            const int bytes = (int)cg_lds_bytes(S.Q, form.long_list);
            if (bytes > lds_bytes) lds_bytes = bytes;
            continue;
        }
        const long P = cg_pow2(S.Q);
        const int chunk = (int)(P < CG_CHUNK ? P : CG_CHUNK);
        S.keys = (unsigned long long *)mine;
        S.contrib = (float *)(mine + (size_t)b * P * 8);
        Args A;
        A.s[0] = S; A.s[1] = S; A.gcd = gcd; A.long_list = form.long_list;
        hipLaunchKernelGGL(cg_ws_sort_kernel, dim3((unsigned)(P / chunk), b), dim3(CG_THREADS), 0, s, S, chunk);
        for (long k = 2l * chunk; k <= P; k <<= 1) {
            for (long j = k >> 1; j >= chunk; j >>= 1)
                hipLaunchKernelGGL(cg_ws_step_kernel, dim3((unsigned)((P / 2 + 255) / 256), b), dim3(256), 0, s, S, k, j);
            hipLaunchKernelGGL(cg_ws_merge_kernel, dim3((unsigned)(P / chunk), b), dim3(CG_THREADS), 0, s, S, chunk, k);
        }
        const long most = S.Q > S.T ? S.Q : S.T;
        hipLaunchKernelGGL(cg_ws_terms_kernel, dim3((unsigned)((most + 255) / 256), b), dim3(256), 0, s, A);
        hipLaunchKernelGGL(cg_ws_walk_kernel, dim3((unsigned)((S.Q + CG_WALK - 1) / CG_WALK), b), dim3(CG_WALK), 0, s, A);
    }
    if (nlds) {
        if (hipError_t e = cg_lds_limit.ensure((const void *)cg_lds_kernel, lds_bytes); e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(cg_lds_kernel, dim3(b, nlds), dim3(CG_THREADS), lds_bytes, s, lds);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dpf_chamfer_grad_lds_mode(int mode) { return dispatch::set_mode(dispatch::settable().cg_lds, mode); }

extern "C" size_t dpf_nndistancegrad_det_workspace_bytes(int b, int n, int m) {
    return cg_workspace_bytes(b, n, m, dispatch::snapshot());
}

extern "C" int dpf_nndistancegrad_det(int b, int n, const float *xyz1, int m, const float *xyz2, const float *grad_dist1,
                                      const int *idx1, const float *grad_dist2, const int *idx2, float *grad_xyz1, float *grad_xyz2,
                                      void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (b > 0 && (!grad_dist1 || !grad_dist2)) return DPF_EINVAL;
    return cg_launch(b, n, xyz1, m, xyz2, grad_dist1, idx1, grad_dist2, idx2, nullptr, grad_xyz1, grad_xyz2, workspace,
                     workspace_bytes, (hipStream_t)stream);
}

extern "C" int dpf_chamfer_cd_backward(int b, int n, const float *xyz1, int m, const float *xyz2, const int *idx1, const int *idx2,
                                       const float *grad_cd, float *grad_xyz1, float *grad_xyz2, void *workspace,
                                       size_t workspace_bytes, dpf_stream_t stream) {
    if (b > 0 && !grad_cd) return DPF_EINVAL;
    return cg_launch(b, n, xyz1, m, xyz2, nullptr, idx1, nullptr, idx2, grad_cd, grad_xyz1, grad_xyz2, workspace, workspace_bytes,
                     (hipStream_t)stream);
}
