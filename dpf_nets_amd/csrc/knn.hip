// k nearest neighbours: for every query point the k candidates of its slot's cloud with the smallest key (squared distance, index),
// ascending.  The contract (strides, arithmetic, eligibility, tie rule, refusal, outputs) is in include/dpf_hip.h; tests/knn_ref.py
// restates it in numpy.  The Chamfer scan's sibling: brute force, B * n * m distances, one query per lane, the candidates broadcast
// from LDS -- with a sorted list of KCAP (distance, index) pairs per lane in place of one running minimum.
//
// A workgroup of 4 waves holds 256 queries of one slot and walks the slot's cloud in tiles of 256 candidates, structure of arrays
// in LDS (x[], y[], z[]): one ds_read_b128 per axis brings four consecutive candidates at a wave-uniform address to every lane.
// The next tile's global loads are issued before the current tile is searched.
//
// The list is what is designed (DESIGN 4.5g has the account).  Inserting costs 5 VALU instructions per list slot (a compare, two
// selects for the distance, two for the index), 5 * KCAP a candidate, and a wave pays them whenever ANY of its 64 lanes takes the
// candidate -- while one lane takes only k * (1 + ln(m / k)) of its m candidates.  So insertion is deferred:
//   * per candidate a lane only tests d < thr (thr = its list's LAST distance as of the last drain, +inf before -- a compile-time
//     slot: a k below KCAP is searched at KCAP's price, and a run-time slot would put the list in scratch) and j != itself, and a
//     passing lane appends (d, j) to a queue of its own in LDS: KNN_QUEUE entries, entry r of thread t at queue[r * 256 + t], so a
//     wave's writes of one depth fall in distinct banks;
//   * before each group of four candidates, if any lane of the wave has fewer than four free entries, the wave DRAINS: round r
//     pops entry r of every lane that has one (the others bring +inf, which changes nothing) and runs the insertion chain once.
//     A drain's rounds are the fullest lane's entries, so the chain runs about as often as the busiest lane needs it, not as often
//     as any lane does.  The queues are drained once more after the last tile.
// A queue is first in, first out and candidates arrive in ascending index, so the chain's strict d < list[s] keeps the lowest index
// among equal distances without comparing indices.  thr is stale between drains: that only lets candidates through which the chain
// then drops.  Empty list slots hold (+inf, -1); in-range input never produces +inf (include/dpf_hip.h), and the padding of a tile's
// tail is +inf coordinates, whose distance +inf never passes d < thr.
//
// The list is indexed with compile-time indices only (fully unrolled chains; no run-time subscript): it lives in registers, and the
// Makefile refuses a build of these kernels that uses scratch.  Queue entries a lane reads beyond its count are stale LDS inside the
// queue; their values are replaced by +inf before use.
//
// Refusal is by slot, so every workgroup of a slot looks at all of the slot's coordinates: the candidates as it stages them, the n
// queries in a strided pass of their own (3 * n / 256 loads a thread, against m distances).  One __syncthreads_or at the end.
//
// Bounded: the loops run over n / 256, over m, over KNN_QUEUE and over KCAP; no workgroup waits on another.
// Compiled with -ffp-contract=off: the distance is a stated sequence of separately rounded fp32 operations, dpf_nndistance's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"

namespace {

constexpr int KNN_THREADS = dispatch::KNN_WG_QUERIES;       // queries of a workgroup, one per lane
constexpr int KNN_TILE = dispatch::KNN_TILE;                // candidates per LDS tile: one staged per thread
constexpr int KNN_QUEUE = dispatch::KNN_QUEUE;              // a lane's deferred candidates
constexpr int KNN_GROUP = 4;                                // candidates per LDS read

static_assert(KNN_TILE == KNN_THREADS, "one thread stages one candidate of a tile");
static_assert(KNN_TILE % KNN_GROUP == 0 && KNN_QUEUE >= 2 * KNN_GROUP, "a group never overflows a queue that passed the check");

struct KNNArgs {
    const float *query;
    long qsc, qsp, qsa;                             // floats between clouds, points, axes
    const float *cloud;
    long csc, csp, csa;
    int n, m, k, exclude;
    float *dist;                                    // (B, n, k)
    int *index;                                     // (B, n, k)
    int *status;                                    // (B) or NULL
};

// a coordinate the contract refuses: not finite, or larger in magnitude than 2^61 (NaN fails the comparison too)
__device__ __forceinline__ unsigned knn_out_of_range(float x, float y, float z) {
    const float lim = 0x1p61f;
    return (unsigned)!(__builtin_fabsf(x) <= lim) | (unsigned)!(__builtin_fabsf(y) <= lim) | (unsigned)!(__builtin_fabsf(z) <= lim);
}

template <int KCAP>
struct KNNList {
    float d[KCAP];
    int i[KCAP];
    // the sorted insertion of (cd, ci), from the list's end down: slot s takes its lower neighbour where the candidate goes in front of
    // that one (every pair behind the candidate's place moves up by one, equal distances in their order; the last is dropped), the
    // candidate where it goes in front of slot s only, else it stays.  Strict: an equal distance already listed stays in front.
    __device__ __forceinline__ void insert(float cd, int ci) {
        bool here = cd < d[KCAP - 1];
#pragma unroll
        for (int s = KCAP - 1; s > 0; --s) {
            const bool up = cd < d[s - 1];                                      // (sorted: up implies here)
            d[s] = up ? d[s - 1] : here ? cd : d[s];
            i[s] = up ? i[s - 1] : here ? ci : i[s];
            here = up;
        }
        d[0] = here ? cd : d[0];
        i[0] = here ? ci : i[0];
    }
};

template <int KCAP>
__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(KNNArgs A, int b0, long blk0) {
    __shared__ __attribute__((aligned(16))) float tx[KNN_TILE], ty[KNN_TILE], tz[KNN_TILE];
    __shared__ uint2 queue[KNN_QUEUE * KNN_THREADS];                            // (distance bits, index)

    const int tid = threadIdx.x, n = A.n, m = A.m, k = A.k;
    const size_t b = (size_t)b0 + blockIdx.y;
    const long blk = blk0 + blockIdx.x, i = blk * KNN_THREADS + tid;
    const float *Q = A.query + (long)b * A.qsc, *C = A.cloud + (long)b * A.csc;
    const float inf = __builtin_inff();

    unsigned bad = 0;
    for (long t = tid; t < n; t += KNN_THREADS) {                               // every query of the slot: refusal is by slot
        const float *p = Q + t * A.qsp;
        bad |= knn_out_of_range(p[0], p[A.qsa], p[2 * A.qsa]);
    }
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (i < n) {
        const float *p = Q + i * A.qsp;
        qx = p[0]; qy = p[A.qsa]; qz = p[2 * A.qsa];
    }
    const int self = A.exclude && i < n ? (int)i : -1;

    KNNList<KCAP> L;
#pragma unroll
    for (int s = 0; s < KCAP; ++s) { L.d[s] = inf; L.i[s] = -1; }
    float thr = inf;
    int queued = 0;

    auto drain = [&]() {
        for (int r = 0; r < KNN_QUEUE; ++r) {
            if (!__any(r < queued)) break;
            const uint2 e = queue[r * KNN_THREADS + tid];
            L.insert(r < queued ? __uint_as_float(e.x) : inf, (int)e.y);
        }
        queued = 0;
        thr = L.d[KCAP - 1];
    };

    // candidate base + tid of a tile, +inf where the cloud has ended
    float nx = inf, ny = inf, nz = inf;
    auto fetch = [&](long base) {
        nx = ny = nz = inf;
        if (base + tid < m) {
            const float *p = C + (base + tid) * A.csp;
            nx = p[0]; ny = p[A.csa]; nz = p[2 * A.csa];
        }
    };
    fetch(0);
    for (long base = 0; base < m; base += KNN_TILE) {
        const int cnt = m - base < KNN_TILE ? (int)(m - base) : KNN_TILE;
        __syncthreads();                                                        // the tile before has been read by every wave
        tx[tid] = nx; ty[tid] = ny; tz[tid] = nz;
        if (tid < cnt) bad |= knn_out_of_range(nx, ny, nz);                     // (looked at here, not at the load: nothing waits for it early)
        __syncthreads();
        if (base + KNN_TILE < m) fetch(base + KNN_TILE);                        // in flight while this tile is searched
        for (int g = 0; g < cnt; g += KNN_GROUP) {
            if (__any(queued > KNN_QUEUE - KNN_GROUP)) drain();
            const float4 X = *(const float4 *)&tx[g], Y = *(const float4 *)&ty[g], Z = *(const float4 *)&tz[g];
            const float cx[KNN_GROUP] = {X.x, X.y, X.z, X.w}, cy[KNN_GROUP] = {Y.x, Y.y, Y.z, Y.w}, cz[KNN_GROUP] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
            for (int u = 0; u < KNN_GROUP; ++u) {
                const int j = (int)((unsigned)base + (unsigned)(g + u));        // (< m wherever d is finite)
                const float dx = cx[u] - qx, dy = cy[u] - qy, dz = cz[u] - qz;
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < thr && j != self) {                                     // (the tile's padding: d = +inf, never below thr)
                    queue[queued * KNN_THREADS + tid] = make_uint2(__float_as_uint(d), (unsigned)j);
                    ++queued;
                }
            }
        }
    }
    drain();

    const int refused = __syncthreads_or((int)bad);                             // the same for every workgroup of the slot
    if (blk == 0 && tid == 0 && A.status) A.status[b] = refused ? DPF_KNN_REFUSED : 0;
    if (i >= n) return;
    const size_t at = (b * (size_t)n + (size_t)i) * (size_t)k;
    float *dist = A.dist + at;
    int *index = A.index + at;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int s = 0; s < KCAP; ++s)
        if (s < k) {
            dist[s] = refused ? nan : L.d[s];
            index[s] = refused ? -1 : L.i[s];
        }
}

template <int KCAP>
int knn_launch(int B, const KNNArgs &A, hipStream_t s) {
    return dispatch::chunk_grid(B, dispatch::ceil_div(A.n, KNN_THREADS), [&](int b0, unsigned nb, long k0, unsigned nk) {
        hipLaunchKernelGGL((knn_kernel<KCAP>), dim3(nk, nb), dim3(KNN_THREADS), 0, s, A, b0, k0);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" int dpf_knn_max_k(void) { return dispatch::KNN_MAX_K; }

extern "C" int dpf_knn(int B, int n, const float *query, long q_cloud_stride, long q_point_stride, long q_axis_stride, int m,
                       const float *cloud, long c_cloud_stride, long c_point_stride, long c_axis_stride, int k, int exclude_same_index,
                       int form, float *dist, int *index, int *status, dpf_stream_t stream) {
    if (B < 0 || n < 1 || m < 1 || k < 1 || form < 0 || form > 4) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!query || !cloud || !dist || !index) return DPF_EINVAL;
    if (k > dispatch::KNN_MAX_K) return DPF_ENOSUP;
    if (k > (exclude_same_index ? m - 1 : m)) return DPF_EINVAL;
    const dispatch::KNNForm f = dispatch::knn_form(k, form);
    if (f.kcap == 0) return DPF_ENOSUP;
    const KNNArgs A{query, q_cloud_stride, q_point_stride, q_axis_stride, cloud, c_cloud_stride, c_point_stride, c_axis_stride,
                    n, m, k, exclude_same_index ? 1 : 0, dist, index, status};
    hipStream_t s = (hipStream_t)stream;
    switch (f.kcap) {
        case 4: return knn_launch<4>(B, A, s);
        case 8: return knn_launch<8>(B, A, s);
        case 16: return knn_launch<16>(B, A, s);
        default: return knn_launch<32>(B, A, s);
    }
}
