// Backward pass of the eval-mode coupling stack (frozen BatchNorm) for gfx950 (MI355X).
//
// Under model.eval() CondRealNVPFlow3D.forward (lib/networks/flows.py:95-117) is a pure per-point map: both BatchNorm1d
// layers of a conditioner branch normalise with their running statistics, so nothing couples the points of a batch.  The
// forward is the fused stack of csrc/flow.hip (one launch, per-layer lists); this file differentiates it with respect to the
// input points, the FiLM vectors and every parameter of the conditioner stacks:
//
//   zbwd_kernel     one launch per layer, in reverse execution order, over the points.  A wave owns 32-point tiles of one
//                   cloud.  It rebuilds h0 = BN0(W0 x), its ReLU mask and the pre-activation h1 + D from the layer's input
//                   with the forward kernel's own packed fragments, FiLM block, operand split and product order (the masks are
//                   the forward's, bit for bit), differentiates the affine transform, and contracts on the matrix cores
//                   in fp32 (v_mfma_f32_32x32x2_f32: no operand split, no range limit):
//                       dh0 = W1^T dh1                 weights from LDS, dh1 straight from the accumulator registers
//                       dW1 = sum_pt dh1 (x) relu(h0)  both operands straight from SWAPPED accumulators (lane = feature,
//                                                      registers = points), accumulated over the wave's tiles
//                   The layer is recomputed in both orientations (the f16x3 recomputation costs a sixteenth of an fp32
//                   contraction) so that no activation is transposed through LDS.  The gradient of the input points is
//                   complete when the kernel ends (direct term + conditioner path of both branches); parameter and FiLM
//                   gradients leave as ONE partial row per workgroup, summed over its waves in wave order.
//   zreduce_kernel  one launch per layer: the partial rows -> dcanon (d gamma0, d beta0, dW0 in closed form from three
//                   per-feature sums) and the per-cloud d FiLM vectors, every sum in row order.
//
// Two launches per layer, none for the stack, no statistic pass, no floating-point atomics: repeated calls agree bit for bit.
// The per-cloud FiLM conditioner nets (B x 64 tensors) stay with the caller; they enter as `fm` and leave as `dfm`.
#include <stdlib.h>

#include "flow_common.h"
#include "flow_mfma.h"
#include "graph_cache.h"

namespace {

constexpr int ZW = 4;                    // waves per workgroup

// `tcanon` block per branch (include/dpf_hip.h, training mode)
constexpr int T_W0 = 0, T_G0 = 128, T_B0 = 192, T_W1 = 256, T_W2 = 4352, T_B2 = 4480, T_BR = 4484, T_LAYER = 2 * T_BR;
// frozen statistics per layer: [br][running_mean0, running_var0, running_mean1, running_var1][64]
constexpr int FS_BR = 256, FS_LAYER = 2 * FS_BR;

// a workgroup's partial row per branch (floats)
constexpr int Z_W1 = 0;          // [64][64] dW1, row = out feature
constexpr int Z_S = 4096;        // [64] sum dh0a                 (d beta0)
constexpr int Z_SA = 4160;       // [64] sum dh0a * x_a
constexpr int Z_SB = 4224;       // [64] sum dh0a * x_b
constexpr int Z_W2A = 4288;      // [64] dW2 row a
constexpr int Z_W2B = 4352;      // [64] dW2 row b
constexpr int Z_CW = 4416;       // [64] d cw of the workgroup's cloud
constexpr int Z_CB = 4480;       // [64] d cb
constexpr int Z_B2 = 4544;       // [2]  db2, then zeros
constexpr int Z_J = 4576;
constexpr int Z_GROUPS = 128 + 2 + 2 + 2 + 2 + 2 + 1;     // 32-column groups of zreduce_kernel per branch

// LDS of zbwd_kernel (bytes): 80 KiB, two workgroups per CU
constexpr int W1_STRIDE = 68;                               // floats per W1 row: the two lane halves read rows 4 apart
constexpr int L_PACK = 0;                                   // the eval layer's packed fragments (two operand parts)
constexpr int L_W1 = p_layer_bytes(2);                      // [br][64][W1_STRIDE] sd1.weight fp32; branch 0's half doubles as the dW1 reduction buffer
constexpr int L_FILM = L_W1 + 2 * 64 * W1_STRIDE * 4;       // the cloud's eval FiLM block
constexpr int L_CONS = L_FILM + FILM_BYTES;                 // [br][8][64] per-feature constants of the cloud
constexpr int L_WAVE = L_CONS + 2 * 8 * 64 * 4;             // per wave: d(o_a), d(o_b), x_a, x_b of the tile's 32 points
constexpr int L_RED = L_WAVE + ZW * 128 * 4;                // [8][64] per-feature sums across the waves
constexpr int L_END = L_RED + 8 * 64 * 4;
static_assert(L_END <= 80 * 1024, "two workgroups per CU");
static_assert(64 * 64 * 4 <= 64 * W1_STRIDE * 4, "the dW1 reduction buffer fits branch 0's W1");

struct ZArgs {
    const uint8_t *packed_l;     // p_layer_bytes(2) of this layer (dpf_flow_pack)
    const float *film_l;         // (B, 512) eval FiLM blocks of this layer (dpf_flow_film)
    const float *tcanon_l;       // T_LAYER
    const float *fstats_l;       // FS_LAYER
    const float *fm_l;           // [br][w|b][B][64]
    const float *p_in, *mu_l, *lv_l;                   // (B, 3, N): the layer's input, its mu and logvar outputs
    const float *g_chain, *g_p, *g_mu, *g_lv;          // gradients: from the layer behind / of ps, mus, logvars (any may be NULL)
    float *dp_out;               // (B, 3, N)
    float *part;                 // (B * gridDim.x, 2, Z_J)
    int B, N, ka, kb, wa, wb, mode, tpw;
    float eps, negone;
};

__device__ __forceinline__ f32x16 mfma32(float x, float y, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, c, 0, 0, 0);
}

// the power of two dpf_flow_pack gave a branch's fp16 W1 (flow_common.h w1_pow2_scale) from the largest |W1|
__device__ __forceinline__ float pow2_scale_of(float t) {
    const int e = (int)((f2u(t) >> 23) & 0xFFu) - 127;
    const bool ok = t > 0.f && e > -100 && e < 100;
    return ok ? u2f((uint32_t)(127 + 13 - e) << 23) : 1.0f;
}

__global__ __launch_bounds__(ZW * 64, 2) void zbwd_kernel(ZArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int bi = blockIdx.y, lane = threadIdx.x & 63, h = lane >> 5, pl = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int N = a.N, nk = a.kb >= 0 ? 2 : 1;
    float *w1s = (float *)(smem + L_W1);
    const float *film = (const float *)(smem + L_FILM);
    float *cons = (float *)(smem + L_CONS);
    float *red = (float *)(smem + L_RED);
    // ---- prologue: the layer's fragments, the cloud's FiLM block, W1 in fp32, the scale of the packed W1
    for (int i = threadIdx.x; i < p_layer_bytes(2) / 16; i += ZW * 64)
        *(u32x4 *)(smem + L_PACK + i * 16) = *(const u32x4 *)(a.packed_l + (size_t)i * 16);
    if (threadIdx.x < FILM_BYTES / 16)
        *(u32x4 *)(smem + L_FILM + threadIdx.x * 16) = *(const u32x4 *)((const uint8_t *)(a.film_l + (size_t)bi * 512) + threadIdx.x * 16);
    float wmax[2] = {0.f, 0.f};
#pragma unroll
    for (int br = 0; br < 2; ++br)
        for (int i = threadIdx.x; i < 4096; i += ZW * 64) {
            const float v = a.tcanon_l[br * T_BR + T_W1 + i];
            w1s[(br * 64 + (i >> 6)) * W1_STRIDE + (i & 63)] = v;
            wmax[br] = fmaxf(wmax[br], fabsf(v));
        }
    red[threadIdx.x] = wmax[0];
    red[256 + threadIdx.x] = wmax[1];
    if (threadIdx.x < 128) {
        const int br = threadIdx.x >> 6, f = threadIdx.x & 63;
        const float *cb = a.tcanon_l + br * T_BR, *fs = a.fstats_l + br * FS_BR;
        const float cw = a.fm_l[((size_t)(br * 2 + 0) * a.B + bi) * 64 + f];
        const float FA = (a.eps + expf(cw)) * (1.0f / sqrtf(fs[3 * 64 + f] + BN_EPS));
        const float w2a = cb[T_W2 + f], w2b = cb[T_W2 + 64 + f];
        const float s0 = cb[T_G0 + f] / sqrtf(fs[64 + f] + BN_EPS);
        float *c = cons + br * 512;
        c[0 * 64 + f] = FA * w2a; c[1 * 64 + f] = FA * w2b; c[2 * 64 + f] = w2a; c[3 * 64 + f] = w2b;
        c[4 * 64 + f] = s0 * cb[T_W0 + f * nk]; c[5 * 64 + f] = nk == 2 ? s0 * cb[T_W0 + f * 2 + 1] : 0.f;
    }
    __syncthreads();
    float wsc[2];
#pragma unroll
    for (int br = 0; br < 2; ++br) {
        float t = 0.f;
        for (int i = 0; i < 256; ++i) t = fmaxf(t, red[br * 256 + i]);
        wsc[br] = pow2_scale_of(t);
    }
    __syncthreads();                                        // `red` is free again
    const bool inverse = a.mode == DPF_MODE_INVERSE;
    float *pts = (float *)(smem + L_WAVE) + wave * 128;
    float *prow0 = a.part + ((size_t)bi * gridDim.x + blockIdx.x) * (2 * Z_J);
#pragma unroll 1
    for (int br = 0; br < 2; ++br) {
        const float *cbr = cons + br * 512;
        const float *w1b = w1s + br * 64 * W1_STRIDE;
        f32x16 dw[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) dw[i >> 1][i & 1] = zero16();
        float s0[2] = {0.f, 0.f}, s1[2] = {0.f, 0.f}, s3[2] = {0.f, 0.f};
        float sbeta = 0.f, sxa = 0.f, sxb = 0.f, sdoa = 0.f, sdob = 0.f;
#pragma unroll 1
        for (int tt = 0; tt < a.tpw; ++tt) {
            const int tile = (blockIdx.x * a.tpw + tt) * ZW + wave;
            if (tile * TILE >= N) break;                    // (wave-uniform; the loop holds no workgroup barrier)
            const int n = tile * TILE + pl;
            const bool valid = n < N;
            const int nc = valid ? n : N - 1;
            const size_t cloud = (size_t)bi * 3 * N;
            // ---- the affine transform and its derivative (flows.py:96-115); mu / logvar are the forward's stored outputs
            float p[3], dpc[3], doa = 0.f, dob = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t o = cloud + (size_t)c * N + nc;
                p[c] = a.p_in[o];
                float gp = (a.g_chain ? a.g_chain[o] : 0.f) + (a.g_p ? a.g_p[o] : 0.f);
                float gm = a.g_mu ? a.g_mu[o] : 0.f, gl = a.g_lv ? a.g_lv[o] : 0.f;
                if (!valid) { gp = 0.f; gm = 0.f; gl = 0.f; }
                const bool isa = c == a.wa, isb = c == a.wb;
                const float lv = (isa || isb) ? a.lv_l[o] : 0.f, mu = (isa || isb) ? a.mu_l[o] : 0.f;
                const float e = expf(lv), var = a.eps + e;
                float dmu, dlv;
                if (inverse) {
                    const float r = 1.0f / sqrtf(var);
                    dpc[c] = gp * r;
                    dmu = gm - gp * r;
                    dlv = gl + gp * (p[c] - mu) * (-0.5f * e * r * r * r);
                } else {
                    const float s = sqrtf(var);
                    dpc[c] = gp * s;
                    dmu = gm + gp;
                    dlv = gl + gp * p[c] * (0.5f * e / s);
                }
                const float dsoft = (1.0f - fabsf(lv)) * (1.0f - fabsf(lv));      // d softsign / d o = (1 - |logvar|)^2
                const float d_o = br == 0 ? dlv * dsoft : dmu;
                if (isa) doa = d_o;
                if (isb) dob = d_o;
            }
            const float xa = sel3(a.ka, p[0], p[1], p[2]), xb = a.kb >= 0 ? sel3(a.kb, p[0], p[1], p[2]) : 0.f;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                // the previous tile's reads of the scratch are done
            if (!h) { pts[pl] = doa; pts[32 + pl] = dob; }
            sdoa += h ? 0.f : doa; sdob += h ? 0.f : dob;
            const u32x4 b0 = input_fragment(h ? xb : xa, h);
            // ---- lane = point: h0, the pre-activation, dh1, dh0 = W1^T dh1
            f32x16 acc0[2], pre[2];
            u32x4 bf[2][4];
            input_mfma(smem + L_PACK + p_a0_off(2), br, lane, b0, acc0);
            split_fragment<true, 2, false, true>(acc0, bf, a.negone);
            load_features(film + br * FILM_BR_FLOATS, h, pre);
            chain_mfma<2, true>(smem + L_PACK, br, lane, bf, pre);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 k1 = *(const f32x4 *)(cbr + 0 * 64 + 32 * t + 8 * q + 4 * h);
                    const f32x4 k2 = *(const f32x4 *)(cbr + 1 * 64 + 32 * t + 8 * q + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = __builtin_fmaf(k1[j], doa, k2[j] * dob);
                        pre[t][4 * q + j] = pre[t][4 * q + j] > 0.f ? v : 0.f;
                    }
                }
            f32x16 d0[2] = {zero16(), zero16()};
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float *wrow = w1b + (32 * t + (r & 3) + 8 * (r >> 2) + 4 * h) * W1_STRIDE + pl;
                    d0[0] = mfma32(wrow[0], pre[t][r], d0[0]);
                    d0[1] = mfma32(wrow[32], pre[t][r], d0[1]);
                }
            float ua = 0.f, ub = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 c1 = *(const f32x4 *)(cbr + 4 * 64 + 32 * t + 8 * q + 4 * h);
                    const f32x4 c2 = *(const f32x4 *)(cbr + 5 * 64 + 32 * t + 8 * q + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = acc0[t][4 * q + j] > 0.f ? d0[t][4 * q + j] : 0.f;     // relu backward: dh0a
                        d0[t][4 * q + j] = v;
                        ua = __builtin_fmaf(c1[j], v, ua);
                        ub = __builtin_fmaf(c2[j], v, ub);
                    }
                }
            ua += __shfl_xor(ua, 32); ub += __shfl_xor(ub, 32);
            if (valid && !h) {                              // d(input points): direct term + the conditioner path on the kept channels
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float *o = a.dp_out + cloud + (size_t)c * N + n;
                    const float u = c == a.ka ? ua : (c == a.kb ? ub : 0.f);
                    if (br == 0) *o = dpc[c] + u;
                    else if (c == a.ka || c == a.kb) *o += u;      // (this thread wrote it in the first branch's round)
                }
            }
            sbeta += reduce_points(d0, pl);
            sxa += reduce_points_gen([&](int i) { return d0[i >> 4][i & 15] * xa; }, pl);
            if (a.kb >= 0) sxb += reduce_points_gen([&](int i) { return d0[i >> 4][i & 15] * xb; }, pl);
            // ---- lane = feature (swapped): per-feature sums over the tile's points, dW1 = dh1 (x) relu(h0)
            f32x16 hs[2], psw[2];
            input_mfma_swapped(smem + L_PACK + p_a0_off(2), br, lane, b0, hs);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float dsh = film[br * FILM_BR_FLOATS + 32 * t + pl];
#pragma unroll
                for (int r = 0; r < 16; ++r) psw[t][r] = dsh;
            }
            chain_mfma_swapped<2, true>(smem + L_PACK, br, lane, bf, psw);
            f32x4 doa4[4], dob4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { doa4[q] = *(const f32x4 *)(pts + 8 * q + 4 * h); dob4[q] = *(const f32x4 *)(pts + 32 + 8 * q + 4 * h); }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int fo = 32 * t + pl;
                const float k1 = cbr[0 * 64 + fo], k2 = cbr[1 * 64 + fo], w2a = cbr[2 * 64 + fo], w2b = cbr[3 * 64 + fo];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float da = doa4[r >> 2][r & 3], db = dob4[r >> 2][r & 3];
                    const float pv = psw[t][r], rp = relu(pv);
                    const bool m = pv > 0.f;
                    s0[t] = __builtin_fmaf(da, rp, s0[t]);
                    s1[t] = __builtin_fmaf(db, rp, s1[t]);
                    s3[t] += m ? __builtin_fmaf(w2a, da, w2b * db) : 0.f;
                    psw[t][r] = m ? __builtin_fmaf(k1, da, k2 * db) : 0.f;
                    hs[t][r] = relu(hs[t][r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    dw[i >> 1][i & 1] = mfma32(psw[i >> 1][r], hs[i & 1][r], dw[i >> 1][i & 1]);
        }
        // ---- the workgroup's row of this branch: the waves add in wave order
#pragma unroll
        for (int t = 0; t < 2; ++t) { s0[t] += __shfl_xor(s0[t], 32); s1[t] += __shfl_xor(s1[t], 32); s3[t] += __shfl_xor(s3[t], 32); }
        for (int q = 32; q > 0; q >>= 1) { sdoa += __shfl_xor(sdoa, q); sdob += __shfl_xor(sdob, q); }
        float *buf = w1s;                                   // branch 0's W1: no wave reads it once its branch-0 tiles are done
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < ZW; ++w) {
            if (wave == w) {
                const bool first = w == 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float *d = buf + (32 * (i >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h) * 64 + 32 * (i & 1) + pl;
                        *d = first ? dw[i >> 1][i & 1][r] : *d + dw[i >> 1][i & 1][r];
                    }
                const int fr = reduced_feature(pl, h);
                auto put = [&](int k, int f, float v) { red[k * 64 + f] = first ? v : red[k * 64 + f] + v; };
                put(3, fr, sbeta); put(4, fr, sxa); put(5, fr, sxb);
                if (!h) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) { put(0, 32 * t + pl, s0[t]); put(1, 32 * t + pl, s1[t]); put(2, 32 * t + pl, s3[t]); }
                }
                if (lane == 0) { put(6, 0, sdoa); put(6, 1, sdob); }
            }
            __syncthreads();
        }
        float *prow = prow0 + br * Z_J;
        for (int i = threadIdx.x; i < 4096; i += ZW * 64) prow[Z_W1 + i] = buf[i];
        if (threadIdx.x < 64) {
            const int f = threadIdx.x;
            const float *fs = a.fstats_l + br * FS_BR;
            const float cw = a.fm_l[((size_t)(br * 2 + 0) * a.B + bi) * 64 + f], cb = a.fm_l[((size_t)(br * 2 + 1) * a.B + bi) * 64 + f];
            const float ex = expf(cw), aa = a.eps + ex, sn = 1.0f / sqrtf(fs[3 * 64 + f] + BN_EPS), winv = 1.0f / wsc[br];
            const float w2a = cbr[2 * 64 + f], w2b = cbr[3 * 64 + f];
            const float S0 = red[0 * 64 + f] * winv, S1 = red[1 * 64 + f] * winv, S3 = red[2 * 64 + f];     // sums of do * relu(h1 + D)
            prow[Z_W2A + f] = aa * sn * S0;                 // relu(h2) = FA relu(h1 + D)
            prow[Z_W2B + f] = aa * sn * S1;
            const float da = sn * (w2a * S0 + w2b * S1) - (cb / aa) * S3;      // h1n = s1 (h1 + D) - cb / a
            prow[Z_CW + f] = da * ex;
            prow[Z_CB + f] = S3;
            prow[Z_S + f] = red[3 * 64 + f];
            prow[Z_SA + f] = red[4 * 64 + f];
            prow[Z_SB + f] = red[5 * 64 + f];
        } else if (threadIdx.x < 64 + Z_J - Z_B2) {
            const int i = threadIdx.x - 64;
            prow[Z_B2 + i] = i < 2 ? red[6 * 64 + i] : 0.f;
        }
        __syncthreads();
    }
}

// sum of column `col` of rows [row0, row0 + nrows) of the (.., stride) partials, rows in order within each of eight
// interleaved row groups, the groups in order: the total in the threads of row group 0.  Every thread of the block calls it.
__device__ __forceinline__ float column_total(const float *__restrict__ part, size_t stride, int row0, int nrows, int col, float (*sh)[33]) {
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    float s = 0.f;
    for (int r = rg; r < nrows; r += 8) s += part[(size_t)(row0 + r) * stride + col];
    __syncthreads();
    sh[rg][c] = s;
    __syncthreads();
    float t = 0.f;
    if (rg == 0)
        for (int i = 0; i < 8; ++i) t += sh[i][c];
    return t;
}

// the partial rows of one layer -> dcanon_l (T_LAYER, every float written) and dfm_l ([br][w|b][B][64]).  Block = 32 columns.
__global__ __launch_bounds__(256) void zreduce_kernel(int B, int nbx, int nk, int nw, const float *__restrict__ part,
                                                      const float *__restrict__ tcanon_l, const float *__restrict__ fstats_l,
                                                      float *__restrict__ dcanon_l, float *__restrict__ dfm_l) {
    __shared__ float sh[8][33];
    const int br = blockIdx.x / Z_GROUPS, grp = blockIdx.x % Z_GROUPS;
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const size_t stride = 2 * Z_J;
    const float *pb = part + br * Z_J;
    float *dc = dcanon_l + br * T_BR;
    const int nrows = B * nbx;
    if (grp < 128) {                                        // dW1
        const float t = column_total(pb, stride, 0, nrows, Z_W1 + grp * 32 + c, sh);
        if (rg == 0) dc[T_W1 + grp * 32 + c] = t;
        return;
    }
    if (grp < 130) {                                        // BN0 and the first SharedDot, features f
        const int f = (grp - 128) * 32 + c;
        const float S = column_total(pb, stride, 0, nrows, Z_S + f, sh);
        const float Sa = column_total(pb, stride, 0, nrows, Z_SA + f, sh);
        const float Sb = column_total(pb, stride, 0, nrows, Z_SB + f, sh);
        if (rg != 0) return;
        const float *cb = tcanon_l + br * T_BR, *fs = fstats_l + br * FS_BR;
        const float rstd = 1.0f / sqrtf(fs[64 + f] + BN_EPS), gamma = cb[T_G0 + f];
        const float wa = cb[T_W0 + f * nk], wb = nk == 2 ? cb[T_W0 + f * 2 + 1] : 0.f;
        dc[T_B0 + f] = S;
        dc[T_G0 + f] = rstd * (wa * Sa + wb * Sb - fs[f] * S);     // sum dh0a * xhat, xhat = rstd0 (W0 x - running_mean0)
        dc[T_W0 + f * nk] = gamma * rstd * Sa;
        if (nk == 2) dc[T_W0 + f * 2 + 1] = gamma * rstd * Sb;
        else dc[T_W0 + 64 + f] = 0.f;
        return;
    }
    if (grp < 134) {                                        // the output SharedDot's rows
        const int w = (grp - 130) >> 1, f = ((grp - 130) & 1) * 32 + c;
        const float t = column_total(pb, stride, 0, nrows, (w ? Z_W2B : Z_W2A) + f, sh);
        if (rg == 0) dc[T_W2 + w * 64 + f] = w < nw ? t : 0.f;
        return;
    }
    if (grp < 138) {                                        // d FiLM vectors: per cloud
        const int sub = (grp - 134) >> 1, f = ((grp - 134) & 1) * 32 + c;
        for (int b = 0; b < B; ++b) {
            const float t = column_total(pb, stride, b * nbx, nbx, (sub ? Z_CB : Z_CW) + f, sh);
            if (rg == 0) dfm_l[((size_t)(br * 2 + sub) * B + b) * 64 + f] = t;
        }
        return;
    }
    const float t = column_total(pb, stride, 0, nrows, Z_B2 + (c & 1), sh);      // db2
    if (rg == 0 && c < 4) dc[T_B2 + c] = c < nw ? t : 0.f;
}

struct ZTiling { int tpw, nbx; };
ZTiling z_tiling(int B, int N) {
    const long tiles = (N + TILE - 1) / TILE;
    long tpw = (B * tiles + ZW * 512 - 1) / (ZW * 512);     // aim at two workgroups per CU of the part, then grow the workgroups
    tpw = tpw < 1 ? 1 : (tpw > 8 ? 8 : tpw);
    return ZTiling{(int)tpw, (int)((tiles + ZW * tpw - 1) / (ZW * tpw))};
}

}  // namespace

extern "C" size_t dpf_flow_frozen_stats_floats(void) { return (size_t)FS_LAYER; }

extern "C" size_t dpf_flow_frozen_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (size_t)B * z_tiling(B, N).nbx * 2 * Z_J * sizeof(float);
}

extern "C" int dpf_flow_frozen_backward_lists(int n_layers, int B, int N, int mode, int precision, const int *meta_host,
                                              const float *tcanon, const float *fstats, const void *packed, const float *film,
                                              const float *fm, const float *p_in, const float *ps, const float *mus,
                                              const float *logvars, const float *const *g_ps, const float *const *g_mus,
                                              const float *const *g_lvs, float *dp_in, float *dp_tmp, float *dcanon, float *dfm,
                                              float flow_eps, void *workspace, dpf_stream_t stream) {
    if (n_layers <= 0 || B <= 0 || N <= 0 || !meta_host || !tcanon || !fstats || !packed || !film || !fm || !p_in || !ps || !mus ||
        !logvars || !dp_in || !dp_tmp || !dcanon || !dfm || !workspace)
        return DPF_EINVAL;
    if (mode != DPF_MODE_DIRECT && mode != DPF_MODE_INVERSE) return DPF_EINVAL;
    if (precision != DPF_PREC_F16X3 || B > 65535) return DPF_ENOSUP;
    const float *const *tab[3] = {g_ps, g_mus, g_lvs};
    auto direct = [&](hipStream_t s) -> int {
        static LdsLimit lim;
        if (hipError_t e = lim.ensure((const void *)zbwd_kernel, L_END); e != hipSuccess) return (int)e;
        const ZTiling tl = z_tiling(B, N);
        const size_t lst = (size_t)B * 3 * N;
        const float *chain = nullptr;
        for (int step = n_layers - 1; step >= 0; --step) {
            const int l = mode == DPF_MODE_DIRECT ? step : n_layers - 1 - step;
            const int lprev = mode == DPF_MODE_DIRECT ? step - 1 : n_layers - step;        // the layer whose output fed layer l
            const int *m = meta_host + 4 * l;
            ZArgs a = {};
            a.packed_l = (const uint8_t *)packed + (size_t)l * p_layer_bytes(2);
            a.film_l = film + (size_t)l * B * (FILM_BYTES / 4);
            a.tcanon_l = tcanon + (size_t)l * T_LAYER;
            a.fstats_l = fstats + (size_t)l * FS_LAYER;
            a.fm_l = fm + (size_t)l * 4 * B * DPF_FLOW_F;
            a.p_in = step == 0 ? p_in : ps + lprev * lst;
            a.mu_l = mus + l * lst; a.lv_l = logvars + l * lst;
            a.g_chain = chain;
            a.g_p = tab[0] ? tab[0][l] : nullptr; a.g_mu = tab[1] ? tab[1][l] : nullptr; a.g_lv = tab[2] ? tab[2][l] : nullptr;
            a.dp_out = (step & 1) ? dp_tmp : dp_in;                                        // step 0 writes dp_in
            a.part = (float *)workspace;
            a.B = B; a.N = N; a.ka = m[0]; a.kb = m[1]; a.wa = m[2]; a.wb = m[3]; a.mode = mode; a.tpw = tl.tpw;
            a.eps = flow_eps; a.negone = -1.0f;
            hipLaunchKernelGGL(zbwd_kernel, dim3(tl.nbx, B), dim3(ZW * 64), L_END, s, a);
            hipLaunchKernelGGL(zreduce_kernel, dim3(2 * Z_GROUPS), dim3(256), 0, s, B, tl.nbx, m[1] >= 0 ? 2 : 1, m[3] >= 0 ? 2 : 1,
                               (const float *)workspace, a.tcanon_l, a.fstats_l, dcanon + (size_t)l * T_LAYER,
                               dfm + (size_t)l * 4 * B * DPF_FLOW_F);
            chain = a.dp_out;
        }
        return (int)hipGetLastError();
    };
    static GraphCache cache;
    return dpf_graph_call(cache, (hipStream_t)stream, direct, [&](GraphKey &k) {
        k.vals(n_layers, B, N, mode, precision); k.add(meta_host, sizeof(int) * 4 * n_layers);
        k.vals(tcanon, fstats, packed, film, fm, p_in, ps, mus, logvars);
        for (const float *const *t : {g_ps, g_mus, g_lvs}) {                 // (named here: tests/test_graph_cache_cpu.py reads this fill)
            const int present = t != nullptr;
            k.val(present);
            if (present) k.add(t, sizeof(const float *) * n_layers);
        }
        k.vals(dp_in, dp_tmp, dcanon, dfm, flow_eps, workspace);
    });
}
