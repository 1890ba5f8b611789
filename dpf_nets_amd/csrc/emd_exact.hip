// Exact EMD of two clouds of n points each: the linear assignment problem on an integer cost grid, solved by Bertsekas' auction
// with epsilon-scaling in 64-bit integer arithmetic.  The contract (grid, refusals, tie rules, outputs, status codes) is in
// include/dpf_hip.h; tests/emd_exact_ref.py restates it in numpy, round for round.
//
// One workgroup per cloud pair, no synchronisation between workgroups.  The pair's state lives in LDS:
//   key[j]    -- (price of object j << 13 | 8191 - bidder) as an unsigned 64-bit word.  A bid is a 64-bit LDS maximum on it: the
//                highest bid wins, among equal bids the lowest bidder.  Prices only rise, so a key of an earlier round never beats a
//                new bid and the array is never cleared; the price a scan reads is key >> 13.
//   owner[j]  -- the point of `a` that holds object j in this phase (0xffff: none)
//   list[2]   -- the compacted unassigned bidders of this round and of the next (appended through an LDS counter; their order
//                decides only which wave serves whom, never a result: every bid of a round is made on the round's starting prices)
//   bidj[t], bidv[t] -- the object and the bid of the list's slot t, between the scan and the bidding step
// What the auction minimises is u_ij = (n + 1) c_ij + price_j; a bidder's best object j1 (lowest index among equal u) gets the bid
// price_j1 + (u2 - u1) + epsilon with u2 the second lowest u.
//
// A round is three steps with a barrier after each.  Scan: a wave serves a bidder, its lanes stride over the candidates, a
// butterfly of (u, index) keys gives the best and the second best.  Late rounds have one or two bidders, so while bidders * S
// fits the workgroup's waves every bidder's candidates are cut into S contiguous slices (S a power of two, slices of >= 64), one
// wave each: waves without a bidder of their own help scan.  Bid: a thread per bidder merges its slices in ascending order and
// sends the bid.  Resolve: a thread per bidder reads its object's key; the winner takes the object and sends the evicted owner
// to the next list, a loser goes there itself.  Best and second best are minima, so they do not depend on S or on the launch shape.
//
// Two forms (dispatch.h: ee_form).  Resident: the second cloud (three planes) and bidv are in LDS too -- 36 bytes a point,
// n <= 4096.  Streamed: the second cloud is read from global memory (L2 serves it: 96 KB a pair at 8192 points) and bidv lies in the
// caller's workspace -- 16 bytes a point, n <= 8192.  Same arithmetic, same bits.
//
// Bounded: every loop runs over n, over the phases (14 at most; the loop stops at EE_MAX_PHASES whatever epsilon does), or over
// rounds counted against the caller's max_rounds.
//
// Compiled with -ffp-contract=off and correctly rounded fp32 square root: the grid is a stated sequence of fp32 operations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "lds_attr.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int EE_WAVES = 16;                        // the most waves of a workgroup
constexpr int EE_TAG = 13;                          // bits of the bidder tag of a key: n <= 8192
constexpr unsigned EE_TAGMASK = (1u << EE_TAG) - 1;
constexpr i64 EE_BID_LIMIT = 1ll << 50;             // bid << 13 stays below 2^63
constexpr i64 EE_INF = 0x7fffffffffffffffll;
constexpr unsigned short EE_NONE = 0xffff;
constexpr int EE_MAX_PHASES = 32;                   // epsilon < 2^38 falls by 3 bits a phase: 14 phases at most; the loop's own bound
constexpr int EE_GRAD_THREADS = 256;

static_assert(dispatch::EE_MAX_POINTS <= (1 << EE_TAG), "the bidder tag holds a point index");

struct EEArgs {
    const float *a, *b;
    long sa_r, sa_c, sb_r, sb_c;                    // pair p = (r, c) = (p / ncols, p % ncols): a + r * sa_r + c * sa_c, b likewise
    long ncols;
    int n, bits, max_rounds;
    int *assignment, *inverse;                      // (pairs, n) each, optional
    i64 *qcost;
    float *cost;
    int *status;
    u64 *bids;                                      // the streamed form's bidv: pad8(n) words a pair
};

__host__ __device__ inline int ee_pad(int n) { return (n + 7) & ~7; }

// the fp32 distance of the contract: every operation rounded on its own, the square root correctly rounded
__device__ __forceinline__ float ee_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ int ee_cost(float d, float s) { return (int)rintf(d * s); }

// (u1, j1, u2) of two candidate sets -> of their union: the lowest u (lowest index among equals) and the second lowest
__device__ __forceinline__ void ee_merge(i64 &u1, int &j1, i64 &u2, i64 o1, int oj, i64 o2) {
    if (o1 < u1 || (o1 == u1 && oj < j1)) {
        u2 = u1 < o2 ? u1 : o2;
        u1 = o1;
        j1 = oj;
    } else {
        u2 = u2 < o1 ? u2 : o1;
    }
}

template <bool STREAMED>
__global__ __launch_bounds__(EE_WAVES * 64) void ee_kernel(EEArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ee_lds[];
    __shared__ float red[EE_WAVES][8];
    __shared__ i64 part_u1[EE_WAVES], part_u2[EE_WAVES], part_p[EE_WAVES];
    __shared__ int part_j[EE_WAVES];
    __shared__ int cnt[2];
    __shared__ int err;
    __shared__ u64 qsum;

    const int n = A.n, np = ee_pad(n);
    const int tid = threadIdx.x, threads = blockDim.x, lane = tid & 63, wave = tid >> 6, W = threads >> 6;
    const size_t p = blockIdx.x;
    const long r = (long)(p / (size_t)A.ncols), c = (long)(p % (size_t)A.ncols);
    const float *a = A.a + r * A.sa_r + c * A.sa_c;
    const float *bg = A.b + r * A.sb_r + c * A.sb_c;

    u64 *key = (u64 *)ee_lds;
    unsigned short *owner = (unsigned short *)(key + np);
    unsigned short *bidj = owner + np;
    unsigned short *list0 = bidj + np;              // list0 and list1 are contiguous: 4 bytes a point, the final distances' room
    unsigned short *list1 = list0 + np;
    u64 *bidv = STREAMED ? A.bids + p * (size_t)np : (u64 *)(list1 + np);
    const float *bl = (const float *)(bidv + np);   // resident form only: x, y, z planes of np floats
    float *dsum = (float *)list0;

    // ---- the grid: exact extents over the 2n points, refusals ---------------------------------------------------------------
    float lo0 = __builtin_inff(), lo1 = lo0, lo2 = lo0, hi0 = -lo0, hi1 = -lo0, hi2 = -lo0;
    unsigned bad = 0;
    for (int t = tid; t < 2 * n; t += threads) {
        const float *q = t < n ? a + (size_t)t * 3 : bg + (size_t)(t - n) * 3;
        const float x = q[0], y = q[1], z = q[2];
        bad |= (unsigned)((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) | (unsigned)((__float_as_uint(y) & 0x7f800000u) == 0x7f800000u) |
               (unsigned)((__float_as_uint(z) & 0x7f800000u) == 0x7f800000u);
        lo0 = fminf(lo0, x); lo1 = fminf(lo1, y); lo2 = fminf(lo2, z);
        hi0 = fmaxf(hi0, x); hi1 = fmaxf(hi1, y); hi2 = fmaxf(hi2, z);
        if (!STREAMED && t >= n) {
            float *w = (float *)bl;
            w[t - n] = x; w[np + t - n] = y; w[2 * np + t - n] = z;
        }
    }
    for (int off = 32; off; off >>= 1) {
        lo0 = fminf(lo0, __shfl_xor(lo0, off)); lo1 = fminf(lo1, __shfl_xor(lo1, off)); lo2 = fminf(lo2, __shfl_xor(lo2, off));
        hi0 = fmaxf(hi0, __shfl_xor(hi0, off)); hi1 = fmaxf(hi1, __shfl_xor(hi1, off)); hi2 = fmaxf(hi2, __shfl_xor(hi2, off));
        bad |= (unsigned)__shfl_xor((int)bad, off);
    }
    if (lane == 0) {
        red[wave][0] = lo0; red[wave][1] = lo1; red[wave][2] = lo2; red[wave][3] = hi0; red[wave][4] = hi1; red[wave][5] = hi2;
        red[wave][6] = __uint_as_float(bad);
    }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; err = 0; qsum = 0; }
    for (int j = tid; j < n; j += threads) key[j] = 0;
    __syncthreads();
    for (int w = 0; w < W; ++w) {                                           // (every thread: the result is uniform)
        lo0 = fminf(lo0, red[w][0]); lo1 = fminf(lo1, red[w][1]); lo2 = fminf(lo2, red[w][2]);
        hi0 = fmaxf(hi0, red[w][3]); hi1 = fmaxf(hi1, red[w][4]); hi2 = fmaxf(hi2, red[w][5]);
        bad |= __float_as_uint(red[w][6]);
    }
    const float E = fmaxf(fmaxf(hi0 - lo0, hi1 - lo1), hi2 - lo2);
    const float E2 = E * E;
    const unsigned e2x = (__float_as_uint(E2) >> 23) & 0xffu;               // E * E normal: exponent field neither 0 nor 255
    const bool finite3 = ((__float_as_uint(3.0f * E2) >> 23) & 0xffu) != 0xffu;
    const bool zero = !bad && E == 0.0f;
    const bool refused = bad || (!zero && (e2x == 0u || e2x == 0xffu || !finite3));
    // E = mant * 2^ex, mant in [0.5, 1): ex = exponent field - 126 (E is normal here); s = 2^(bits - 1 - ex)
    const int ex = (int)((__float_as_uint(E) >> 23) & 0xffu) - 126;
    const float s = __uint_as_float((unsigned)(127 + A.bits - 1 - ex) << 23);
    const i64 np1 = (i64)n + 1;

    int status = refused ? DPF_EMD_EXACT_REFUSED : 0;
    int rounds = 0;
    const bool run = !refused && !zero && n > 1;
    if (!run)
        for (int j = tid; j < n; j += threads) owner[j] = (unsigned short)j;    // zero extent, or a single point: the identity

    // ---- the auction ------------------------------------------------------------------------------------------------------------
    if (run) {
        i64 eps = (np1 << A.bits) >> dispatch::EE_EPS0_SHIFT;
        if (eps < 1) eps = 1;
        for (int phase = 0; phase < EE_MAX_PHASES && status == 0; ++phase) {
            __syncthreads();
            for (int j = tid; j < n; j += threads) { owner[j] = EE_NONE; list0[j] = (unsigned short)j; }
            if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
            int k = n, cur = 0;
            __syncthreads();
            while (k > 0) {
                if (rounds >= A.max_rounds) { status = DPF_EMD_EXACT_CAP; break; }
                ++rounds;
                const unsigned short *list = cur ? list1 : list0;
                unsigned short *next = cur ? list0 : list1;
                int S = 1, lgS = 0;
                while (2 * S * k <= W && n / (2 * S) >= 64) { S *= 2; ++lgS; }
                const int len = (((n + S - 1) >> lgS) + 63) & ~63;
                const int T = k << lgS;
                // scan: work item t = (bidder slot t >> lgS, slice t & (S - 1))
                for (int t = wave; t < T; t += W) {
                    const int slot = t >> lgS, sl = t & (S - 1);
                    const int i = list[slot];
                    const float ax = a[(size_t)i * 3], ay = a[(size_t)i * 3 + 1], az = a[(size_t)i * 3 + 2];
                    const int j0 = sl * len, j1 = j0 + len < n ? j0 + len : n;
                    i64 u1 = EE_INF, u2 = EE_INF;
                    int jb = 0x7fffffff;
                    for (int j = j0 + lane; j < j1; j += 64) {
                        float bx, by, bz;
                        if (STREAMED) { bx = bg[(size_t)j * 3]; by = bg[(size_t)j * 3 + 1]; bz = bg[(size_t)j * 3 + 2]; }
                        else { bx = bl[j]; by = bl[np + j]; bz = bl[2 * np + j]; }
                        const i64 u = (i64)ee_cost(ee_dist(ax, ay, az, bx, by, bz), s) * np1 + (i64)(key[j] >> EE_TAG);
                        if (u < u1) { u2 = u1; u1 = u; jb = j; }             // ascending j in a lane: strict keeps the lowest index
                        else if (u < u2) u2 = u;
                    }
                    for (int off = 32; off; off >>= 1) {
                        const i64 o1 = __shfl_xor(u1, off), o2 = __shfl_xor(u2, off);
                        const int oj = __shfl_xor(jb, off);
                        ee_merge(u1, jb, u2, o1, oj, o2);
                    }
                    if (lane == 0) {
                        const i64 price = jb < n ? (i64)(key[jb] >> EE_TAG) : 0;   // (an empty slice has no best)
                        if (S == 1) {
                            bidj[slot] = (unsigned short)jb;
                            bidv[slot] = (u64)(price + (u2 - u1) + eps);
                        } else {
                            part_u1[t] = u1; part_u2[t] = u2; part_j[t] = jb; part_p[t] = price;
                        }
                    }
                }
                __syncthreads();
                // bid: one thread per bidder, on the prices the scans read
                for (int t = tid; t < k; t += threads) {
                    i64 bid;
                    int jb;
                    if (S == 1) {
                        bid = (i64)bidv[t];
                        jb = bidj[t];
                    } else {
                        i64 u1 = EE_INF, u2 = EE_INF, price = 0;
                        jb = 0x7fffffff;
                        for (int q = t << lgS; q < (t + 1) << lgS; ++q) {
                            const int before = jb;
                            ee_merge(u1, jb, u2, part_u1[q], part_j[q], part_u2[q]);
                            price = jb != before ? part_p[q] : price;
                        }
                        bid = price + (u2 - u1) + eps;
                        bidj[t] = (unsigned short)jb;
                    }
                    if (bid >= EE_BID_LIMIT) err = 1;
                    else atomicMax(&key[jb], ((u64)bid << EE_TAG) | (u64)(EE_TAGMASK - (unsigned)list[t]));
                }
                __syncthreads();
                // resolve: the winner takes the object, the evicted owner and the losers bid again
                for (int t = tid; t < k; t += threads) {
                    const int i = list[t], j = bidj[t];
                    if ((int)(EE_TAGMASK - ((unsigned)key[j] & EE_TAGMASK)) == i) {
                        const unsigned short old = owner[j];
                        owner[j] = (unsigned short)i;
                        if (old != EE_NONE) next[atomicAdd(&cnt[cur ^ 1], 1)] = old;
                    } else {
                        next[atomicAdd(&cnt[cur ^ 1], 1)] = (unsigned short)i;
                    }
                }
                __syncthreads();
                k = cnt[cur ^ 1];
                if (tid == 0) cnt[cur] = 0;          // the list after next's counter: last read before this round's first barrier
                cur ^= 1;
                if (err) { status = DPF_EMD_EXACT_RANGE; break; }
            }
            if (eps == 1) break;
            eps >>= dispatch::EE_EPS_SHIFT;
            if (eps < 1) eps = 1;
        }
    }
    __syncthreads();

    // ---- the outputs ------------------------------------------------------------------------------------------------------------
    int *asg_out = A.assignment ? A.assignment + p * (size_t)n : nullptr;
    int *inv_out = A.inverse ? A.inverse + p * (size_t)n : nullptr;
    if (status < 0) {
        for (int j = tid; j < n; j += threads) {
            if (asg_out) asg_out[j] = -1;
            if (inv_out) inv_out[j] = -1;
        }
        if (tid == 0) { A.cost[p] = __builtin_nanf(""); A.qcost[p] = -1; A.status[p] = status; }
        return;
    }
    for (int j = tid; j < n; j += threads) {
        const int i = owner[j];
        if (i < n) bidj[i] = (unsigned short)j;                             // the assignment, point of a -> point of b
        if (inv_out) inv_out[j] = i;
    }
    __syncthreads();
    u64 q = 0;
    for (int i = tid; i < n; i += threads) {
        const int j = bidj[i];
        if (asg_out) asg_out[i] = j;
        float d = 0.0f;
        if (!zero) {
            d = ee_dist(a[(size_t)i * 3], a[(size_t)i * 3 + 1], a[(size_t)i * 3 + 2], bg[(size_t)j * 3], bg[(size_t)j * 3 + 1], bg[(size_t)j * 3 + 2]);
            q += (u64)ee_cost(d, s);
        }
        dsum[i] = d;
    }
    for (int off = 32; off; off >>= 1) q += __shfl_xor(q, off);
    if (lane == 0 && q) atomicAdd(&qsum, q);
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        for (int i = 0; i < n; ++i) sum += dsum[i];                         // ascending i: the one order of the contract
        A.cost[p] = sum;
        A.qcost[p] = (i64)qsum;
        A.status[p] = rounds;
    }
}

// one thread per index t of a pair: grad_a[t] from its match, grad_b[t] from the point matched to it
__global__ __launch_bounds__(EE_GRAD_THREADS) void ee_grad_kernel(int n, const float *__restrict__ a, const float *__restrict__ b,
                                                                  const int *__restrict__ assignment, const int *__restrict__ inverse,
                                                                  const float *__restrict__ g, float *__restrict__ grad_a,
                                                                  float *__restrict__ grad_b) {
    const unsigned nblk = (unsigned)((n + EE_GRAD_THREADS - 1) / EE_GRAD_THREADS);
    const size_t pair = blockIdx.x / nblk;
    const int t = (int)(blockIdx.x % nblk) * EE_GRAD_THREADS + threadIdx.x;
    if (t >= n) return;
    const size_t base = pair * (size_t)n;
    const float gp = g[pair];
    for (int side = 0; side < 2; ++side) {
        float *out = side ? grad_b : grad_a;
        if (!out) continue;
        const int o = (side ? inverse : assignment)[base + t];
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (o >= 0) {                                                           // (-1: the pair was not solved)
            const size_t ia = side ? base + (size_t)o : base + t, ib = side ? base + t : base + (size_t)o;
            const float dx = a[ia * 3] - b[ib * 3], dy = a[ia * 3 + 1] - b[ib * 3 + 1], dz = a[ia * 3 + 2] - b[ib * 3 + 2];
            const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (d > 0.0f) { gx = gp * (dx / d); gy = gp * (dy / d); gz = gp * (dz / d); }
            if (side) { gx = -gx; gy = -gy; gz = -gz; }
        }
        out[(base + t) * 3] = gx; out[(base + t) * 3 + 1] = gy; out[(base + t) * 3 + 2] = gz;
    }
}

LdsLimit ee_lds_limit[2];

int ee_launch(long pairs, EEArgs A, int form, void *workspace, size_t workspace_bytes, hipStream_t s) {
    if (pairs < 0 || A.n < 0 || A.bits < dispatch::EE_MIN_BITS || A.bits > dispatch::EE_MAX_BITS || A.max_rounds < 0 || form < 0 || form > 2)
        return DPF_EINVAL;
    if (pairs == 0 || A.n == 0) return 0;
    if (!A.a || !A.b || !A.qcost || !A.cost || !A.status) return DPF_EINVAL;
    if (A.n > dispatch::EE_MAX_POINTS || pairs > 0x7fffffffL) return DPF_ENOSUP;
    const dispatch::EEForm f = dispatch::ee_form(A.n, form);
    if (f.kernel == dispatch::EEKernel::Unserved) return DPF_ENOSUP;
    const bool streamed = f.kernel == dispatch::EEKernel::Streamed;
    if (streamed) {
        if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < dpf_emd_exact_workspace_bytes(pairs, A.n)) return DPF_EINVAL;
        A.bids = (u64 *)workspace;
    }
    const int lds = ee_pad(A.n) * f.lds_per_point;
    const void *fn = streamed ? (const void *)ee_kernel<true> : (const void *)ee_kernel<false>;
    if (hipError_t e = ee_lds_limit[streamed].ensure(fn, lds); e != hipSuccess) return (int)e;
    if (streamed) hipLaunchKernelGGL(ee_kernel<true>, dim3((unsigned)pairs), dim3(f.threads), lds, s, A);
    else hipLaunchKernelGGL(ee_kernel<false>, dim3((unsigned)pairs), dim3(f.threads), lds, s, A);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dpf_emd_exact_max_points(void) { return dispatch::EE_MAX_POINTS; }

extern "C" size_t dpf_emd_exact_workspace_bytes(long pairs, int n) {
    if (pairs < 1 || n < 1 || n > dispatch::EE_MAX_POINTS) return 0;
    return (size_t)pairs * (size_t)ee_pad(n) * sizeof(u64);                     // (the resident form reads none of it)
}

extern "C" int dpf_emd_exact(int B, int n, const float *a, long a_stride, const float *b, long b_stride, int bits, int max_rounds,
                             int form, int *assignment, int *inverse, long long *qcost, float *cost, int *status, void *workspace,
                             size_t workspace_bytes, dpf_stream_t stream) {
    if (a_stride < 0 || b_stride < 0) return DPF_EINVAL;
    const EEArgs A{a, b, a_stride, 0, b_stride, 0, 1, n, bits, max_rounds, assignment, inverse, qcost, cost, status, nullptr};
    return ee_launch(B, A, form, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int dpf_pairwise_emd_exact(int N1, int N2, int n, const float *clouds1, const float *clouds2, int bits, int max_rounds,
                                      int form, long long *qcost, float *cost, int *status, void *workspace, size_t workspace_bytes,
                                      dpf_stream_t stream) {
    if (N1 < 0 || N2 < 0) return DPF_EINVAL;
    const EEArgs A{clouds1, clouds2, (long)n * 3, 0, 0, (long)n * 3, N2 > 0 ? N2 : 1, n, bits, max_rounds, nullptr, nullptr, qcost, cost,
                   status, nullptr};
    return ee_launch((long)N1 * N2, A, form, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int dpf_emd_exact_grad(int B, int n, const float *a, const float *b, const int *assignment, const int *inverse,
                                  const float *grad_cost, float *grad_a, float *grad_b, dpf_stream_t stream) {
    if (B < 0 || n < 0) return DPF_EINVAL;
    if (B == 0 || n == 0 || (!grad_a && !grad_b)) return 0;
    if (!a || !b || !grad_cost || (grad_a && !assignment) || (grad_b && !inverse)) return DPF_EINVAL;
    const long nblk = dispatch::ceil_div(n, EE_GRAD_THREADS);
    if (nblk * B > 0x7fffffffL) return DPF_ENOSUP;
    hipLaunchKernelGGL(ee_grad_kernel, dim3((unsigned)(nblk * B)), dim3(EE_GRAD_THREADS), 0,
                       (hipStream_t)stream, n, a, b, assignment, inverse, grad_cost, grad_a, grad_b);
    return (int)hipGetLastError();
}
