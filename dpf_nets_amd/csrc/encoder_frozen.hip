// PointNet cloud encoder, EVAL mode under autograd: the backward of  pooled = max over the points of
// [SharedDot . BatchNorm1d (running statistics) . ReLU] x 4  (lib/networks/encoders.py:15-28 + models.py:106,124 under model.eval())
// to the twelve parameter gradients and, optionally, the input.  The forward of the autograd node is encoder.hip's launch with
// the argmax switched on (dpf_encoder_forward_arg).
//
// With frozen statistics there are no batch-statistic terms, and the max-pool sends gradient to exactly one point per (cloud,
// feature): the whole backward touches B * 512 VIRTUAL POINTS -- (b, f) stands for the point x[b, :, arg[b, f]] -- whatever N is.
// The 512 virtual points of a cloud are two 256-point workgroups of the forward's geometry.
//
// Launches: FOUR for the parameter gradients, SIX with dx, whatever B and N are:
//   recompute  layers 0-2 of the virtual points on the matrix cores through encoder_mfma.h's enc_layers012 -- the forward's
//              fragments, precision, k order and accumulator scheme, so every ReLU decision is the forward's own (a point's MFMA
//              column does not depend on its neighbours); leaves the activations a0 | a1 | a2 (448 floats per virtual point);
//   chain      16 virtual points per workgroup, fp32 FMAs against the fp32 weights, folded scale s_l = gamma_l / sqrt(var_l + 1e-5):
//              d z3 is one-hot, so d a2 = g s3[f] W3[f, :] (a scaled row, not a GEMM); d a1 = (s2 dz2) W2 and d a0 = (s1 dz1) W1 with
//              the k index ascending, masked by the recomputed ReLUs; d x_v = (s0 dz0) W0;
//   partials   per slab of clouds (at most 64 slabs): M_l = sum_v dz_l[v] a_{l-1}[v]^T for l = 1, 2 as 64 x 64 register-tiled
//              products with v ascending, M_0, and the column sums of dz_l;
//   rows       one wave per output row: the slabs' partials added in slab order, dW_l = s_l M_l, dbeta_l = sum dz_l, and
//              dgamma_l = sum dz_l xhat_l formed as rstd_l (W_l[j, :] . M_l[j, :] - mean_l dbeta_l) in double -- the same sum
//              with xhat_l = (W_l a_{l-1} - mean_l) rstd_l written out, exact for gamma = 0 and gamma < 0 (nothing divides by
//              gamma); layer 3: M_3[f, :] = sum_b g[b, f] a2(b, f), a B-term sum per row in cloud order;
//   fill, dx   dx zero-filled by a kernel (zero_fill.h); then per cloud the 512 (arg, d x_v) triples in LDS: the lowest feature of
//              each group of features sharing a point sums the group in ascending feature order and writes it.
// No atomics anywhere and every sum in an order fixed by the shapes: the result is bit-reproducible.
// Workspace: 2 * 448 + 8 floats per virtual point = 1.84 MB per cloud (59 MB at B = 32) plus 166 KB per slab.  The entry accepts
// B <= 65535 as the forward does, but the caller's memory is the bound that binds: 7.5 GB at B = 4096, 120 GB at B = 65535.
// Matrix cores serve the recomputation only: the backward contractions are fp32 FMAs (2 x 41 K per virtual point, 1.3 GFMA at
// B = 32), which keeps the gradients fp32-class at both forward precisions.
#include "flow_common.h"
#include "encoder_layout.h"
#include "encoder_mfma.h"
#include "zero_fill.h"

namespace {

constexpr int EA_0 = 0, EA_1 = EC1, EA_2 = EC1 + EC2, EA_N = EC1 + EC2 + EC3;       // a0 | a1 | a2 (and dz0 | dz1 | dz2): 448
constexpr int CP = 16;                                                            // virtual points per chain workgroup
constexpr int MAX_SLABS = 64;
// a slab's partial sums: M2 [256][128] | M1 [128][64] | M0 [64][3] | column sums of dz [448]
constexpr int PM_2 = 0, PM_1 = EC3 * EC2, PM_0 = PM_1 + EC2 * EC1, PM_B = PM_0 + EC1 * EC0, PM_N = PM_B + EA_N;

struct EfArgs {
    const float *canon;
    const uint8_t *packed;
    const float *x, *pooled, *g;
    const int *arg;
    float *dcanon, *dx;
    float *act, *dz, *xv, *dxv, *part;       // workspace: (V,448), (V,448), (V,4) x y z g_live, (V,4), (slabs, PM_N)
    int B, N, slabs;
};

__device__ __forceinline__ float fold_scale(const float *canon, int l, int f) {      // enc_pack_kernel's own expression
    const float *c = canon + e_layer_off(l) + e_cout(l) * e_cin(l);
    return c[f] / sqrtf(c[3 * e_cout(l) + f] + BN_EPS);
}

template <int TP>
struct ActTap {
    float *row[TP];      // this lane's virtual point per tile
    int h;
    __device__ __forceinline__ void operator()(int l, int q, int mt, const f32x16 &acc) const {
        float *dst = row[q] + (l == 0 ? EA_0 : l == 1 ? EA_1 : EA_2) + 32 * mt + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *(f32x4 *)(dst + 8 * g) = f32x4{relu(acc[4 * g]), relu(acc[4 * g + 1]), relu(acc[4 * g + 2]), relu(acc[4 * g + 3])};
    }
};

template <int NS>
__global__ __launch_bounds__(e_waves(NS) * 64) void ef_recompute_kernel(EfArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int EW = e_waves(NS), TP = e_tp(NS);
    constexpr int NA12 = (EW == 4 && TP == 1) ? 2 : 1;
    uint8_t *l_a0 = smem, *l_bias = smem + 4096, *l_buf = smem + 8192;
    const int bi = blockIdx.y;
    const int lane = threadIdx.x & 63, h = lane >> 5, pl = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N;
    const float *xc = a.x + (size_t)bi * 3 * N;
    float px[TP], py[TP], pz[TP];
    ActTap<TP> tap;
    tap.h = h;
#pragma unroll
    for (int q = 0; q < TP; ++q) {
        const int f = ((blockIdx.x * EW + wave) * TP + q) * TILE + pl;        // < 512: the grid covers exactly the 512 features
        const size_t v = (size_t)bi * EC4 + f;
        const int nc = min(max(a.arg[v], 0), N - 1);
        px[q] = xc[nc]; py[q] = xc[N + nc]; pz[q] = xc[2 * (size_t)N + nc];
        tap.row[q] = a.act + v * EA_N;
        if (!h) {
            const float gl = a.pooled[v] > 0.f ? a.g[v] : 0.f;                // a dead feature passes no gradient
            *(f32x4 *)(a.xv + v * 4) = f32x4{px[q], py[q], pz[q], gl};
        }
    }
#pragma unroll
    for (int k = wave; k < 8; k += EW)
        __builtin_amdgcn_global_load_lds((glb_void *)(a.packed + k * 1024 + lane * 16), (lds_void *)(smem + k * 1024), 16, 0, 0);
    stage_chunk<NS>(a.packed, 0, l_buf, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    EncStream<NS> st{a.packed, l_buf, wave, lane, 0};
    u32x4 f3[TP][NS][16];
    enc_layers012<NS, TP, NA12>(st, l_a0, l_bias, lane, px, py, pz, f3, tap);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the stream's next chunk is still on its way into LDS
    __syncthreads();
}

__global__ __launch_bounds__(256) void ef_chain_kernel(EfArgs a) {
    __shared__ float u2[CP][EC3], u1[CP][EC2], u0[CP][EC1], sc[EA_N], gs3[CP];
    const int tid = threadIdx.x;
    const size_t v0 = (size_t)blockIdx.x * CP;                   // CP divides 512: one cloud per workgroup
    const float *W0 = a.canon + e_layer_off(0), *W1 = a.canon + e_layer_off(1), *W2 = a.canon + e_layer_off(2),
                *W3 = a.canon + e_layer_off(3);
    for (int e = tid; e < EA_N; e += 256)
        sc[e] = e < EA_1 ? fold_scale(a.canon, 0, e) : e < EA_2 ? fold_scale(a.canon, 1, e - EA_1) : fold_scale(a.canon, 2, e - EA_2);
    if (tid < CP) gs3[tid] = a.xv[(v0 + tid) * 4 + 3] * fold_scale(a.canon, 3, (int)((v0 + tid) & (EC4 - 1)));      // g s3[f] per point
    __syncthreads();
    // d z2 = [a2 > 0] g s3[f] W3[f, :]
    for (int e = tid; e < CP * EC3; e += 256) {
        const int p = e >> 8, k = e & 255;
        const size_t v = v0 + p;
        const int f = (int)(v & (EC4 - 1));
        const float gs = gs3[p];
        const float d = a.act[v * EA_N + EA_2 + k] > 0.f ? gs * W3[(size_t)f * EC3 + k] : 0.f;
        a.dz[v * EA_N + EA_2 + k] = d;
        u2[p][k] = d * sc[EA_2 + k];
    }
    __syncthreads();
    {   // d a1[p][j] = sum_k u2[p][k] W2[k][j], k ascending; a thread: one j, 8 points
        const int j = tid & 127, p0 = (tid >> 7) * 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = 0; k < EC3; ++k) {
            const float w = W2[k * EC2 + j];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = fmaf(u2[p0 + q][k], w, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const size_t v = v0 + p0 + q;
            const float d = a.act[v * EA_N + EA_1 + j] > 0.f ? acc[q] : 0.f;
            a.dz[v * EA_N + EA_1 + j] = d;
            u1[p0 + q][j] = d * sc[EA_1 + j];
        }
    }
    __syncthreads();
    {   // d a0[p][i] = sum_j u1[p][j] W1[j][i], j ascending; a thread: one i, 4 points
        const int i = tid & 63, p0 = (tid >> 6) * 4;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < EC2; ++j) {
            const float w = W1[j * EC1 + i];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(u1[p0 + q][j], w, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const size_t v = v0 + p0 + q;
            const float d = a.act[v * EA_N + EA_0 + i] > 0.f ? acc[q] : 0.f;
            a.dz[v * EA_N + EA_0 + i] = d;
            u0[p0 + q][i] = d * sc[EA_0 + i];
        }
    }
    if (a.dx == nullptr) return;
    __syncthreads();
    if (tid < CP * 4) {      // d x_v[c] = sum_i u0[p][i] W0[i][c], i ascending
        const int p = tid >> 2, c = tid & 3;
        float acc = 0.f;
        if (c < 3)
            for (int i = 0; i < EC1; ++i) acc = fmaf(u0[p][i], W0[i * EC0 + c], acc);
        a.dxv[(v0 + p) * 4 + c] = acc;
    }
}

// C[64][64] = sum over the slab's virtual points v (ascending) of A[v][0..64) B[v][0..64)^T; A, B: rows of EA_N floats
__device__ __forceinline__ void slab_tile(const float *A, const float *Bm, size_t v_lo, size_t v_hi, float *C, int ldc) {
    __shared__ __attribute__((aligned(16))) float As[32][64], Bs[32][64];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    float acc[4][4] = {};
    for (size_t v = v_lo; v < v_hi; v += 32) {       // a slab is a multiple of 512 points
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i, row = e >> 4, c4 = e & 15;
            *(f32x4 *)&As[row][4 * c4] = *(const f32x4 *)(A + (v + row) * EA_N + 4 * c4);
            *(f32x4 *)&Bs[row][4 * c4] = *(const f32x4 *)(Bm + (v + row) * EA_N + 4 * c4);
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
            const f32x4 av = *(const f32x4 *)&As[kk][4 * ty], bv = *(const f32x4 *)&Bs[kk][4 * tx];
            const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(ar[r], br[c], acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) C[(size_t)(4 * ty + r) * ldc + 4 * tx + c] = acc[r][c];
}

// sum over the slab's virtual points (ascending) of x[v] * y[v] (y == nullptr: of x[v]): four interleaved partial sums, one tree
__device__ __forceinline__ float slab_dot(const float *x, size_t xs, const float *y, size_t ys, size_t v_lo, size_t v_hi) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (size_t v = v_lo; v < v_hi; v += 4)          // a slab is a multiple of 512 points
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = fmaf(x[(v + q) * xs], y ? y[(v + q) * ys] : 1.f, s[q]);
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// grid (11 + PB_BLOCKS, slabs): x = 0..7 the 64 x 64 tiles of M2, 8..9 of M1, from 10 on the column sums and M0, a thread each
constexpr int PB_ITEMS = EA_N + EC1 * EC0, PB_BLOCKS = (PB_ITEMS + 255) / 256;
__global__ __launch_bounds__(256) void ef_partial_kernel(EfArgs a) {
    const int s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const size_t v_lo = (size_t)((long long)a.B * s / a.slabs) * EC4, v_hi = (size_t)((long long)a.B * (s + 1) / a.slabs) * EC4;
    float *part = a.part + (size_t)s * PM_N;
    if (t < 8) {
        const int r0 = 64 * (t >> 1), c0 = 64 * (t & 1);
        slab_tile(a.dz + EA_2 + r0, a.act + EA_1 + c0, v_lo, v_hi, part + PM_2 + (size_t)r0 * EC2 + c0, EC2);
    } else if (t < 10) {
        const int r0 = 64 * (t - 8);
        slab_tile(a.dz + EA_1 + r0, a.act + EA_0, v_lo, v_hi, part + PM_1 + (size_t)r0 * EC1, EC1);
    } else {
        const int e = (t - 10) * 256 + tid;
        if (e < EA_N) {
            part[PM_B + e] = slab_dot(a.dz + e, EA_N, nullptr, 0, v_lo, v_hi);
        } else if (e < PB_ITEMS) {
            const int i = (e - EA_N) / EC0, c = (e - EA_N) % EC0;
            part[PM_0 + i * EC0 + c] = slab_dot(a.dz + EA_0 + i, EA_N, a.xv + c, 4, v_lo, v_hi);
        }
    }
}

__device__ __forceinline__ double wave_sum(double x) {       // fixed butterfly: the same order in every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// one wave per output row (64 + 128 + 256 + 512 = 960 rows)
__global__ __launch_bounds__(64) void ef_rows_kernel(EfArgs a) {
    const int lane = threadIdx.x;
    int row = blockIdx.x, l = 0;
    while (row >= e_cout(l)) { row -= e_cout(l); ++l; }
    const int cin = e_cin(l), cout = e_cout(l), j = row;
    const float *W = a.canon + e_layer_off(l) + (size_t)j * cin;
    const float *bn = a.canon + e_layer_off(l) + (size_t)cout * cin;       // gamma | beta | running_mean | running_var
    float *dW = a.dcanon + e_layer_off(l) + (size_t)j * cin, *dbn = a.dcanon + e_layer_off(l) + (size_t)cout * cin;
    const float rstd = 1.f / sqrtf(bn[3 * cout + j] + BN_EPS), sj = fold_scale(a.canon, l, j);
    double dot = 0.0;
    float dbeta = 0.f;
    if (l < 3) {
        const int pm = l == 0 ? PM_0 : l == 1 ? PM_1 : PM_2, pb = PM_B + (l == 0 ? EA_0 : l == 1 ? EA_1 : EA_2);
        for (int i = lane; i < cin; i += 64) {
            float m = 0.f;
            for (int s = 0; s < a.slabs; ++s) m += a.part[(size_t)s * PM_N + pm + (size_t)j * cin + i];
            dW[i] = sj * m;
            dot += (double)W[i] * (double)m;
        }
        for (int s = 0; s < a.slabs; ++s) dbeta += a.part[(size_t)s * PM_N + pb + j];
    } else {
        // M3[f, :] = sum_b g[b, f] a2(b, f): four interleaved partial sums over the clouds, one fixed tree
        const size_t vs = EC4;
        for (int i = lane; i < cin; i += 64) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int b = 0;
            for (; b + 4 <= a.B; b += 4) {
                const size_t v = (size_t)b * vs + j;
                s0 = fmaf(a.xv[v * 4 + 3], a.act[v * EA_N + EA_2 + i], s0);
                s1 = fmaf(a.xv[(v + vs) * 4 + 3], a.act[(v + vs) * EA_N + EA_2 + i], s1);
                s2 = fmaf(a.xv[(v + 2 * vs) * 4 + 3], a.act[(v + 2 * vs) * EA_N + EA_2 + i], s2);
                s3 = fmaf(a.xv[(v + 3 * vs) * 4 + 3], a.act[(v + 3 * vs) * EA_N + EA_2 + i], s3);
            }
            for (; b < a.B; ++b) {
                const size_t v = (size_t)b * vs + j;
                s0 = fmaf(a.xv[v * 4 + 3], a.act[v * EA_N + EA_2 + i], s0);
            }
            const float m = (s0 + s1) + (s2 + s3);
            dW[i] = sj * m;
            dot += (double)W[i] * (double)m;
        }
        for (int b = 0; b < a.B; ++b) dbeta += a.xv[((size_t)b * vs + j) * 4 + 3];
    }
    dot = wave_sum(dot);
    if (lane == 0) {
        dbn[j] = (float)((double)rstd * (dot - (double)bn[2 * cout + j] * (double)dbeta));
        dbn[cout + j] = dbeta;
    }
}

// one workgroup per cloud, one thread per feature
__global__ __launch_bounds__(512) void ef_dx_kernel(EfArgs a) {
    __shared__ int l_arg[EC4];
    __shared__ float l_d[EC4][3];
    const int f = threadIdx.x, N = a.N;
    const size_t v = (size_t)blockIdx.x * EC4 + f;
    const int n = min(max(a.arg[v], 0), N - 1);
    l_arg[f] = n;
    l_d[f][0] = a.dxv[v * 4]; l_d[f][1] = a.dxv[v * 4 + 1]; l_d[f][2] = a.dxv[v * 4 + 2];
    __syncthreads();
    int first = -1;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int o = 0; o < EC4; ++o) {
        if (l_arg[o] == n) {
            if (first < 0) first = o;
            s0 += l_d[o][0]; s1 += l_d[o][1]; s2 += l_d[o][2];
        }
    }
    if (first == f) {
        float *d = a.dx + (size_t)blockIdx.x * 3 * N + n;
        d[0] = s0; d[N] = s1; d[2 * (size_t)N] = s2;
    }
}

inline int ef_slabs(int B) { return B < MAX_SLABS ? B : MAX_SLABS; }
inline size_t al64(size_t floats) { return (floats + 63) & ~(size_t)63; }

template <int NS>
int launch_recompute(const EfArgs &a, hipStream_t s) {
    constexpr int EW = e_waves(NS), EWG_POINTS = EW * e_tp(NS) * TILE;
    static_assert(EC4 % EWG_POINTS == 0, "the virtual points of a cloud fill whole workgroups");
    const int lds = 8192 + 2 * ep_chunk_bytes(NS);
    static LdsLimit limit;
    if (hipError_t e = limit.ensure((const void *)ef_recompute_kernel<NS>, lds); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ef_recompute_kernel<NS>, dim3(EC4 / EWG_POINTS, a.B), dim3(EW * 64), lds, s, a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" size_t dpf_encoder_frozen_workspace_bytes(int B) {
    if (B <= 0) return 0;
    const size_t V = (size_t)B * EC4;
    return sizeof(float) * (2 * al64(V * EA_N) + 2 * al64(V * 4) + al64((size_t)ef_slabs(B) * PM_N));
}

extern "C" int dpf_encoder_frozen_backward(int B, int N, int precision, const float *canon, const void *packed, const float *x,
                                           const float *pooled, const int *arg, const float *g_pooled, float *dcanon, float *dx,
                                           void *workspace, dpf_stream_t stream) {
    const int ns = e_ns_of(precision);
    if (!ns || B < 0 || N <= 0) return DPF_EINVAL;
    if (ns == 1) return DPF_ENOSUP;
    if (B == 0) return 0;
    if (!canon || !packed || !x || !pooled || !arg || !g_pooled || !workspace || ((uintptr_t)workspace & 15) || (!dcanon && !dx))
        return DPF_EINVAL;
    if (B > 65535) return DPF_ENOSUP;
    hipStream_t s = (hipStream_t)stream;
    const size_t V = (size_t)B * EC4;
    EfArgs a = {};
    a.canon = canon; a.packed = (const uint8_t *)packed; a.x = x; a.pooled = pooled; a.g = g_pooled; a.arg = arg;
    a.dcanon = dcanon; a.dx = dx; a.B = B; a.N = N; a.slabs = ef_slabs(B);
    a.act = (float *)workspace; a.dz = a.act + al64(V * EA_N); a.xv = a.dz + al64(V * EA_N); a.dxv = a.xv + al64(V * 4);
    a.part = a.dxv + al64(V * 4);
    if (dx) {
        if (hipError_t e = dpf_zero_async(dx, sizeof(float) * (size_t)B * 3 * N, s); e != hipSuccess) return (int)e;
    }
    if (int e = ns == 2 ? launch_recompute<2>(a, s) : launch_recompute<3>(a, s); e != 0) return e;
    hipLaunchKernelGGL(ef_chain_kernel, dim3((unsigned)(V / CP)), dim3(256), 0, s, a);
    if (dcanon) {
        hipLaunchKernelGGL(ef_partial_kernel, dim3(11 + PB_BLOCKS, a.slabs), dim3(256), 0, s, a);
        hipLaunchKernelGGL(ef_rows_kernel, dim3(EC1 + EC2 + EC3 + EC4), dim3(64), 0, s, a);
    }
    if (dx) hipLaunchKernelGGL(ef_dx_kernel, dim3(B), dim3(512), 0, s, a);
    return (int)hipGetLastError();
}
