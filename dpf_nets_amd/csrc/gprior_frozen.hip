// Latent prior flow, EVAL mode under autograd: the backward of the whole GlobalRNVPDecoder stack with FROZEN BatchNorm
// (running statistics; lib/networks/flows.py:198-243, decoders.py:21-38 under model.eval()) in TWO launches, whatever the
// number of steps.  The forward of the autograd node is gprior.hip's launch, unchanged.
//
// With frozen statistics a coupling step is a per-row map: no batch-statistics pass, no column kernels, B = 1 is legal.
//   rows launch    a workgroup owns one row of the batch (grid-stride over rows) and walks the steps in reverse.  Per step it
//                  recomputes the hidden activations of both nets from the step's input (gs of the step before, or g),
//                  differentiates the affine update, log(eps + exp(.)), the second map, Swish and BatchNorm
//                  (du = dy * gamma * rstd: no mean terms), carries the chain gradient in LDS, and leaves per step and row
//                  the Swish outputs, xhat, dy and d_o in the workspace.  The weights (0.13-0.5 MB per step) stream from L2.
//   params launch  one thread per element of the gradient block, spread over the whole chip: dW0, dgamma, dbeta, dW1, db1 of
//                  all 2 S nets as sums over the rows in row order (four interleaved partial sums, combined in a fixed tree).
// No atomics anywhere and every sum in an order fixed by the shapes: the result is bit-reproducible.
// fp32 FMAs, as gprior.hip and gprior_train.hip: the operands are (1 x 64..256) rows against 0.1 MB matrices, a step is a
// chain of dependent round trips to L2 and LDS -- latency-, not throughput-bound; matrix cores would buy nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "gprior_common.h"

namespace {

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int PT = 256;
constexpr int MAX_ROW_BLOCKS = 1024;

struct FArgs {
    int S, B, G, nf, inverse, nbn, parts2, parts3;
    float bn_eps, eps;
    const float *canon, *stats, *g, *gs, *mus, *lvs, *d_gs, *d_mus, *d_lvs;
    float *dg, *dcanon;
    float *w_sw, *w_xh, *w_dy, *w_do;          // workspace: (S,B,2nf) Swish outputs, xhat, dy; (S,B,2K) d_o
    StepCodes codes;
};

// running_mean [nf] | running_var [nf] of net n = 2 * step + (0 mu, 1 logvar): inside the canonical block, or the separate block
__device__ __forceinline__ const float *net_stats(const FArgs &a, int n, size_t cn, int K) {
    return a.nbn == 4 ? a.canon + (size_t)n * cn + (size_t)a.nf * K + 2 * (size_t)a.nf : a.stats + (size_t)n * 2 * a.nf;
}

// the input of step s: the output of the step the forward ran before it, or g for the forward's first step
__device__ __forceinline__ const float *step_input(const FArgs &a, int s) {
    const int t = a.inverse ? a.S - 1 - s : s;
    return t == 0 ? a.g : a.gs + (size_t)(a.inverse ? s + 1 : s - 1) * a.B * a.G;
}

__global__ __launch_bounds__(THREADS) void gprior_frozen_rows_kernel(FArgs a) {
    extern __shared__ float lds[];
    const int G = a.G, K = G >> 1, nf = a.nf, H = 2 * nf, P2 = a.parts2, P3 = a.parts3;
    float *dcur = lds;                 // [G]  the chain gradient as it stands
    float *gin = dcur + G;             // [G]  the step's input row
    float *d_o = gin + G;              // [2K] gradient of the second maps' outputs, mu net then logvar net
    float *dsdy = d_o + G;             // [H]  Swish'(y)
    float *gr = dsdy + H;              // [H]  gamma * rstd
    float *du = gr + H;                // [H]  gradient of the first maps' outputs
    float *part = du + H;              // [P2][H] partial sums of d_o W1, then [P3][K] of du W0
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t cn = net_floats(K, nf, a.nbn), BG = (size_t)a.B * G;
    for (int row = blockIdx.x; row < a.B; row += gridDim.x) {
        for (int e = tid; e < G; e += THREADS) dcur[e] = 0.f;
        __syncthreads();
        for (int t = a.S - 1; t >= 0; --t) {                     // the forward's steps, last one first
            const int s = a.inverse ? a.S - 1 - t : t;
            const auto [kmul, kadd, wadd] = step_index(step_code(a.codes, s), K);
            const float *cs = a.canon + (size_t)s * 2 * cn;
            const float *gsrc = step_input(a, s) + (size_t)row * G;
            const size_t at = (size_t)s * BG + (size_t)row * G;          // the row in the (S,B,G) blocks; G = 2K: in w_do too
            const size_t hrow = ((size_t)s * a.B + row) * H;
            // ---- the affine update and log(eps + exp(.)) backwards: one warped coordinate per thread
            for (int e = tid; e < G; e += THREADS) gin[e] = gsrc[e];
            for (int i = tid; i < K; i += THREADS) {
                const int wi = kmul * i + wadd, ki = kmul * i + kadd;
                const float dw = dcur[wi] + (a.d_gs ? a.d_gs[at + wi] : 0.f);
                const float dk = dcur[ki] + (a.d_gs ? a.d_gs[at + ki] : 0.f);
                const float lv = a.lvs[at + wi], mu = a.mus[at + wi], out = a.gs[at + wi];
                const float sc = expf(a.inverse ? -0.5f * lv : 0.5f * lv);
                const float dmu = (a.d_mus ? a.d_mus[at + wi] : 0.f) + (a.inverse ? -dw * sc : dw);
                const float dlv = (a.d_lvs ? a.d_lvs[at + wi] : 0.f) + (a.inverse ? -0.5f * dw * out : 0.5f * dw * (out - mu));
                const float dol = dlv * (1.f - a.eps * expf(-lv));       // d/do log(eps + exp(o)) = exp(o) / (eps + exp(o))
                d_o[i] = dmu;
                d_o[K + i] = dol;
                a.w_do[at + i] = dmu;
                a.w_do[at + K + i] = dol;
                dcur[wi] = dw * sc;
                dcur[ki] = dk;
            }
            __syncthreads();
            // ---- the hidden activations once more: a wave per hidden unit (the rows of W0 [nf][K] are contiguous: lanes along k,
            // then a butterfly), four units in flight; lane u of the wave finishes unit q0 + u
            for (int q0 = wave * 4; q0 < H; q0 += WAVES * 4) {
                float acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u;
                    acc[u] = 0.f;
                    if (q < H) {
                        const int net = q >= nf, j = q - net * nf;
                        const float *w = cs + net * cn + (size_t)j * K;
                        for (int k = lane; k < K; k += 64) acc[u] = fmaf(w[k], gin[kmul * k + kadd], acc[u]);
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u] += __shfl_xor(acc[u], off);
                const int q = q0 + lane;
                if (lane < 4 && q < H) {
                    const float v = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
                    const int net = q >= nf, j = q - net * nf;
                    const float *st = net_stats(a, 2 * s + net, cn, K);
                    const float rstd = 1.f / sqrtf(st[nf + j] + a.bn_eps);
                    const float gam = cs[net * cn + (size_t)nf * K + j], bet = cs[net * cn + (size_t)nf * K + nf + j];
                    const float xhat = (v - st[j]) * rstd, y = fmaf(xhat, gam, bet), sg = 1.f / (1.f + expf(-y));
                    a.w_xh[hrow + q] = xhat;
                    a.w_sw[hrow + q] = y * sg;
                    dsdy[q] = sg * (1.f + y * (1.f - sg));
                    gr[q] = gam * rstd;
                }
            }
            // ---- d hs = d_o W1 (W1 [K][nf]: lanes along the hidden unit), the warped range split into P2 parts
            for (int o = tid; o < P2 * H; o += THREADS) {
                const int p = o / H, q = o - p * H, net = q >= nf, j = q - net * nf;
                const int i0 = K * p / P2, i1 = K * (p + 1) / P2;
                const float *w = cs + net * cn + (size_t)nf * K + (size_t)a.nbn * nf + j;
                const float *x = d_o + net * K;
                float acc = 0.f;
#pragma unroll 4
                for (int i = i0; i < i1; ++i) acc = fmaf(w[(size_t)i * nf], x[i], acc);
                part[o] = acc;
            }
            __syncthreads();
            // ---- Swish and the frozen BatchNorm backwards
            for (int q = tid; q < H; q += THREADS) {
                float acc = 0.f;
                for (int p = 0; p < P2; ++p) acc += part[p * H + q];
                const float dy = acc * dsdy[q];
                a.w_dy[hrow + q] = dy;
                du[q] = dy * gr[q];
            }
            __syncthreads();
            // ---- d g_keep += sum over both nets of du W0 (lanes along k), the hidden range split into P3 parts
            for (int o = tid; o < P3 * K; o += THREADS) {
                const int p = o / K, k = o - p * K;
                const int q0 = H * p / P3, q1 = H * (p + 1) / P3;
                float acc = 0.f;
#pragma unroll 4
                for (int q = q0; q < q1; ++q) {
                    const int net = q >= nf, j = q - net * nf;
                    acc = fmaf(cs[net * cn + (size_t)j * K + k], du[q], acc);
                }
                part[o] = acc;
            }
            __syncthreads();
            for (int k = tid; k < K; k += THREADS) {
                float acc = 0.f;
                for (int p = 0; p < P3; ++p) acc += part[p * K + k];
                dcur[kmul * k + kadd] += acc;
            }
            __syncthreads();
        }
        for (int e = tid; e < G; e += THREADS) a.dg[(size_t)row * G + e] = dcur[e];
        __syncthreads();
    }
}

// sum over the B rows of x[b] * y[b] (or of x[b]) in row order: four interleaved partial sums, one fixed tree
__device__ __forceinline__ float rows_dot(const float *x, size_t xs, const float *y, size_t ys, int B) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
    for (; b + 4 <= B; b += 4) {
        s0 = fmaf(x[(size_t)b * xs], y[(size_t)b * ys], s0);
        s1 = fmaf(x[(size_t)(b + 1) * xs], y[(size_t)(b + 1) * ys], s1);
        s2 = fmaf(x[(size_t)(b + 2) * xs], y[(size_t)(b + 2) * ys], s2);
        s3 = fmaf(x[(size_t)(b + 3) * xs], y[(size_t)(b + 3) * ys], s3);
    }
    for (; b < B; ++b) s0 = fmaf(x[(size_t)b * xs], y[(size_t)b * ys], s0);
    return (s0 + s1) + (s2 + s3);
}

__device__ __forceinline__ float rows_sum(const float *x, size_t xs, int B) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int b = 0;
    for (; b + 4 <= B; b += 4) {
        s0 += x[(size_t)b * xs];
        s1 += x[(size_t)(b + 1) * xs];
        s2 += x[(size_t)(b + 2) * xs];
        s3 += x[(size_t)(b + 3) * xs];
    }
    for (; b < B; ++b) s0 += x[(size_t)b * xs];
    return (s0 + s1) + (s2 + s3);
}

// One thread per element of dcanon (the layout of canon): consecutive threads are consecutive k of a W0 row or consecutive
// hidden units of a W1 row, so the per-row operand that varies across a wave is read coalesced and the other is one address.
__global__ __launch_bounds__(PT) void gprior_frozen_params_kernel(FArgs a) {
    const int G = a.G, K = G >> 1, nf = a.nf, H = 2 * nf, B = a.B;
    const size_t cn = net_floats(K, nf, a.nbn), total = (size_t)a.S * 2 * cn;
    for (size_t e = (size_t)blockIdx.x * PT + threadIdx.x; e < total; e += (size_t)gridDim.x * PT) {
        const int n = (int)(e / cn), s = n >> 1, br = n & 1;
        size_t o = e - (size_t)n * cn;
        const float *dy = a.w_dy + (size_t)s * B * H + br * nf;        // + b H + j
        const float *dout = a.w_do + (size_t)s * B * G + br * K;       // + b G + i
        float v;
        if (o < (size_t)nf * K) {                                      // d W0 [j][k] = gamma rstd sum_b dy[b][j] g_keep[b][k]
            const int j = (int)(o / K), k = (int)(o - (size_t)j * K);
            const auto [kmul, kadd, wadd] = step_index(step_code(a.codes, s), K);
            const float *st = net_stats(a, n, cn, K);
            const float rstd = 1.f / sqrtf(st[nf + j] + a.bn_eps);
            v = a.canon[(size_t)n * cn + (size_t)nf * K + j] * rstd * rows_dot(dy + j, H, step_input(a, s) + kmul * k + kadd, G, B);
        } else if ((o -= (size_t)nf * K) < (size_t)nf) {               // d gamma
            v = rows_dot(dy + o, H, a.w_xh + (size_t)s * B * H + br * nf + o, H, B);
        } else if ((o -= nf) < (size_t)nf) {                           // d beta
            v = rows_sum(dy + o, H, B);
        } else if ((o -= nf) < (size_t)(a.nbn - 2) * nf) {             // running statistics carry no gradient
            v = 0.f;
        } else if ((o -= (size_t)(a.nbn - 2) * nf) < (size_t)K * nf) { // d W1 [i][j] = sum_b d_o[b][i] hs[b][j]
            const int i = (int)(o / nf), j = (int)(o - (size_t)i * nf);
            v = rows_dot(dout + i, G, a.w_sw + (size_t)s * B * H + br * nf + j, H, B);
        } else {                                                       // d b1
            v = rows_sum(dout + (o - (size_t)K * nf), G, B);
        }
        a.dcanon[e] = v;
    }
}

}  // namespace

extern "C" {

size_t dpf_gprior_frozen_workspace_floats(int n_steps, int B, int G, int n_features) {
    if (n_steps <= 0 || B <= 0 || G <= 0 || n_features <= 0) return 0;
    return (size_t)n_steps * B * (3 * 2 * (size_t)n_features + G);      // hs | xhat | dy | d_o
}

int dpf_gprior_frozen_backward(int n_steps, int B, int G, int n_features, int mode, const int *codes, int params_only, const float *canon,
                               const float *stats, float bn_eps, float eps, const float *g, const float *gs, const float *mus,
                               const float *lvs, const float *d_gs, const float *d_mus, const float *d_lvs, float *dg, float *dcanon,
                               float *workspace, dpf_stream_t stream) {
    if (n_steps <= 0 || n_steps > MAX_STEPS || B < 0 || G < 2 || (G & 1) || n_features <= 0 || !codes || (mode != 0 && mode != 1))
        return DPF_EINVAL;
    FArgs a = {};
    if (!pack_step_codes(n_steps, codes, a.codes)) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!canon || (params_only && !stats) || !g || !gs || !mus || !lvs || !dg || !dcanon || !workspace) return DPF_EINVAL;
    const int K = G / 2, H = 2 * n_features;
    a.S = n_steps; a.B = B; a.G = G; a.nf = n_features; a.inverse = mode; a.nbn = params_only ? 2 : 4;
    a.bn_eps = bn_eps; a.eps = eps;
    a.canon = canon; a.stats = stats; a.g = g; a.gs = gs; a.mus = mus; a.lvs = lvs; a.d_gs = d_gs; a.d_mus = d_mus; a.d_lvs = d_lvs;
    a.dg = dg; a.dcanon = dcanon;
    const size_t SBH = (size_t)n_steps * B * H;
    a.w_sw = workspace; a.w_xh = a.w_sw + SBH; a.w_dy = a.w_xh + SBH; a.w_do = a.w_dy + SBH;
    // the inner ranges of the two transposed maps are split over the threads their outputs leave idle
    a.parts2 = THREADS / H > 1 ? (THREADS / H < K ? THREADS / H : K) : 1;
    a.parts3 = THREADS / K > 1 ? (THREADS / K < H ? THREADS / K : H) : 1;
    const size_t p2 = (size_t)a.parts2 * H, p3 = (size_t)a.parts3 * K;
    const size_t lds = sizeof(float) * (3 * (size_t)G + 3 * (size_t)H + (p2 > p3 ? p2 : p3));
    if (lds > 64 * 1024) return DPF_ENOSUP;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gprior_frozen_rows_kernel, dim3(B < MAX_ROW_BLOCKS ? B : MAX_ROW_BLOCKS), dim3(THREADS), lds, st, a);
    const size_t total = (size_t)n_steps * 2 * net_floats(K, n_features, a.nbn), blocks = (total + PT - 1) / PT;
    hipLaunchKernelGGL(gprior_frozen_params_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(PT), 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
