// Surface sampling of triangle meshes into the collated training batch, on the device: what the reference's data loader does
// on the host per item (lib/datasets/cloud_sampling.py:4-32 and the elementwise part of lib/datasets/cloud_transformations.py).
//
// The mesh store's view, the slot rule, a face's corners and its area (numpy's fp32 sequence) are mesh_store.h's, shared with
// point_mesh.hip and mesh_point.hip; the launches are cut to the grid's limits by dispatch.h's chunkers.
//
//   dpf_mesh_cdf_build -- once per store.  Per face the area (mesh_face_area).
//     Per mesh the cumulative distribution over its faces in double.  The mesh is cut into tiles of MS_TILE faces counted from
//     ITS OWN first face; a tile's areas are summed one after the other in face order (one thread: the order is the contract, and
//     a running sum of non-negative terms is monotone, which a tree scan is not); the tile totals are summed one after the other
//     per mesh; edge[f] = (offset of f's tile + running sum inside the tile) / total.  Nothing in this depends on which meshes
//     share the store, on where the mesh sits in it, or on the launch geometry.  The last edge is total / total = 1.
//     Validation comes first: a face with an index >= the mesh's vertex count is flagged (bit 0) and its vertices are NOT read;
//     a non-finite area sets bit 1; a total of zero sets bit 2.  Such faces count as area 0.
//   dpf_mesh_variates  -- counter-based uniforms keyed by (seed, step, batch slot, sample, stream): splitmix64 as in
//     dpf_nets_amd/synthetic.py.  u_face keeps 53 bits (fp32 uniforms would make small faces of large meshes unreachable); s1 and
//     s2 are the double uniform rounded to fp32 (the reference's .astype(np.float32)).  datasets/sampling.py:host_variates returns
//     the same values bit for bit.
//   dpf_mesh_sample    -- one thread per sample: the face is the first k with edge[k] > u (numpy's searchsorted side='right':
//     a zero-area face is never chosen, u = 0 skips leading zero-area faces); the reflection, the point
//     (p0 + s1 * (p1 - p0)) + s2 * (p2 - p0) and the four elementwise transforms in fp32 in the reference's order; stores are
//     coordinate-major, even samples to cloud and odd ones to eval_cloud when the batch is split.  A slot whose mesh index is
//     outside the store or whose mesh is flagged reads no face and no vertex: its outputs are NaN and its faces -1.
//
// Compiled with -ffp-contract=off: no operation of the contract is fused.  fp32 division and square root are the correctly
// rounded ones (hipcc's default, stated in the Makefile).  Integer / fp32 / fp64 VALU only; no packed fp32, no matrix cores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "mesh_store.h"
#include "zero_fill.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_TILE = 256;                       // faces per scan tile == threads of a tile's workgroup

static_assert(MS_TILE == MS_THREADS, "one thread per face of a tile");

// the m in [0, M) with bounds[m] <= x < bounds[m + 1] (bounds is increasing, bounds[0] <= x < bounds[M])
__device__ __forceinline__ int ms_find(const long *bounds, int M, long x) {
    int lo = 0, hi = M - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (bounds[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint64_t ms_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// areas of one tile, their running sums in face order, the tile's total
__global__ __launch_bounds__(MS_THREADS) void ms_tile_kernel(MeshStore a, const long *tile_bounds, long tile0, long ntiles,
                                                             double *cdf, double *tile_sum, unsigned int *flags) {
    __shared__ double run[MS_TILE];
    const long tile = tile0 + blockIdx.x;
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    const int m = ms_find(tile_bounds, a.M, tile);
    const long lt = tile - tile_bounds[m];
    const long fb = a.face_bounds[m], F = a.face_bounds[m + 1] - fb;
    const long vb = a.vertex_bounds[m], V = a.vertex_bounds[m + 1] - vb;
    const long f = lt * MS_TILE + tid;
    double area = 0.0;
    if (f < F) {
        const unsigned int *fi = a.faces + (size_t)(fb + f) * 3;
        const unsigned int i0 = fi[0], i1 = fi[1], i2 = fi[2];
        if ((long)i0 >= V || (long)i1 >= V || (long)i2 >= V) {
            atomicOr(&flags[m], 1u);                                      // (no vertex is read through such an index)
        } else {
            const float s = mesh_face_area(mesh_corners(a, fb, vb, f));
            if (s <= 3.402823466e38f) area = (double)s;                  // (false for NaN and for +inf)
            else atomicOr(&flags[m], 2u);
        }
    }
    run[tid] = area;
    __syncthreads();
    if (tid == 0) {
        double r = 0.0;
        for (int i = 0; i < MS_TILE; ++i) { r += run[i]; run[i] = r; }
    }
    __syncthreads();
    if (f < F) cdf[fb + f] = run[tid];
    if (tid == 0) {
        const long left = F - lt * MS_TILE;
        tile_sum[tile] = run[(left < MS_TILE ? (int)left : MS_TILE) - 1];
    }
}

// per mesh: the tile totals become the tiles' offsets, summed one after the other
__global__ __launch_bounds__(MS_THREADS) void ms_mesh_kernel(int M, const long *tile_bounds, double *tile_sum, double *total,
                                                             unsigned int *flags) {
    const int m = blockIdx.x * MS_THREADS + threadIdx.x;
    if (m >= M) return;
    double r = 0.0;
    for (long t = tile_bounds[m], t1 = tile_bounds[m + 1]; t < t1; ++t) {
        const double s = tile_sum[t];
        tile_sum[t] = r;
        r += s;
    }
    total[m] = r;
    if (!(r > 0.0)) atomicOr(&flags[m], 4u);
}

__global__ __launch_bounds__(MS_THREADS) void ms_edge_kernel(MeshStore a, const long *tile_bounds, long tile0, long ntiles,
                                                             double *cdf, const double *tile_off, const double *total,
                                                             const unsigned int *flags) {
    const long tile = tile0 + blockIdx.x;
    if (tile >= ntiles) return;
    const int m = ms_find(tile_bounds, a.M, tile);
    const long lt = tile - tile_bounds[m];
    const long fb = a.face_bounds[m], F = a.face_bounds[m + 1] - fb;
    const long f = lt * MS_TILE + threadIdx.x;
    if (f >= F) return;
    cdf[fb + f] = flags[m] ? 0.0 : (tile_off[tile] + cdf[fb + f]) / total[m];
}

__global__ __launch_bounds__(MS_THREADS) void ms_variates_kernel(int S, size_t i0, size_t n, uint64_t base, double *u, float *s1,
                                                                 float *s2) {
    const size_t idx = i0 + (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (idx >= n) return;
    const uint64_t b = idx / (size_t)S, i = idx - b * (size_t)S;
    const uint64_t slot = ms_splitmix64(base ^ b);
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = (double)(ms_splitmix64(slot ^ (i * 4 + k)) >> 11) * (1.0 / 9007199254740992.0);
    u[idx] = d[0];
    s1[idx] = (float)d[1];
    s2[idx] = (float)d[2];
}

struct MeshSampleArgs {
    const double *cdf;
    const float *orig_c, *orig_s;
    int S, split, xform;
    const int *mesh_idx;
    const double *u;
    const float *s1, *s2;
    float shift[3], scale;
    float *cloud, *eval_cloud;
    int *faces_out;
};

__global__ __launch_bounds__(MS_THREADS) void ms_sample_kernel(MeshStore st, MeshSampleArgs a, int b0) {
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= a.S) return;
    const size_t b = (size_t)b0 + blockIdx.y, at = b * (size_t)a.S + i;
    const int N = a.split ? a.S >> 1 : a.S, j = a.split ? i >> 1 : i;
    float *out = ((a.split && (i & 1)) ? a.eval_cloud : a.cloud) + b * 3 * (size_t)N + j;
    const MeshSlot sl = mesh_slot(st, a.mesh_idx, b);
    if (!sl.ok) {                                                         // never sampled: no face, no vertex of it is read
        const float nan = __builtin_nanf("");
        out[0] = nan; out[N] = nan; out[2 * (size_t)N] = nan;
        if (a.faces_out) a.faces_out[at] = -1;
        return;
    }
    const int m = sl.m, F = sl.F;
    const double *edge = a.cdf + sl.fb;
    const double uu = a.u[at];
    int lo = 0, hi = F;                                                   // the first k with edge[k] > u
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (edge[mid] > uu) hi = mid; else lo = mid + 1;
    }
    const int k = lo < F ? lo : F - 1;                                    // (only a u outside [0, 1) gets here past the end)
    const MeshCorners cr = mesh_corners(st, sl.fb, sl.vb, k);
    const float *p0 = cr.p0, *p1 = cr.p1, *p2 = cr.p2;
    float t1 = a.s1[at], t2 = a.s2[at];
    if (t1 + t2 > 1.0f) { t1 = 1.0f - t1; t2 = 1.0f - t2; }
    const float os = (a.xform & 1) ? a.orig_s[m] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = (p0[c] + t1 * (p1[c] - p0[c])) + t2 * (p2[c] - p0[c]);
        if (a.xform & 1) x = os * x;
        if (a.xform & 2) x = x + a.orig_c[(size_t)m * 3 + c];
        if (a.xform & 4) x = x - a.shift[c];
        if (a.xform & 8) x = x / a.scale;
        out[(size_t)c * N] = x;
    }
    if (a.faces_out) a.faces_out[at] = k;
}

inline bool ms_store_ok(int M, const void *v, const void *vb, const void *f, const void *fb) { return M >= 1 && v && vb && f && fb; }

}  // namespace

extern "C" int dpf_mesh_cdf_tile(void) { return MS_TILE; }

extern "C" size_t dpf_mesh_cdf_workspace_bytes(int M, long n_tiles) {
    if (M < 1 || n_tiles < M) return 0;
    return ((size_t)n_tiles + (size_t)M) * sizeof(double);
}

extern "C" int dpf_mesh_cdf_build(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                                  const long *face_bounds, const long *tile_bounds, long n_tiles, double *cdf, unsigned int *flags,
                                  void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (!ms_store_ok(M, vertices, vertex_bounds, faces, face_bounds) || !tile_bounds || n_tiles < M || !cdf || !flags || !workspace)
        return DPF_EINVAL;
    if (workspace_bytes < dpf_mesh_cdf_workspace_bytes(M, n_tiles) || ((uintptr_t)workspace & 7) || ((uintptr_t)cdf & 7)) return DPF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int e = (int)dpf_zero_async(flags, (size_t)M * 4, st);
    if (e) return e;
    double *tile_sum = (double *)workspace, *total = tile_sum + n_tiles;
    const MeshStore a{M, vertices, vertex_bounds, faces, face_bounds, flags};
    e = dispatch::chunk_range(n_tiles, dispatch::MAX_BLOCKS, [&](long t0, long nb) {
        return mesh_launch(ms_tile_kernel, dim3((unsigned)nb), MS_THREADS, st, a, tile_bounds, t0, n_tiles, cdf, tile_sum, flags);
    });
    if (e) return e;
    e = mesh_launch(ms_mesh_kernel, dim3((unsigned)((M + MS_THREADS - 1) / MS_THREADS)), MS_THREADS, st, M, tile_bounds, tile_sum, total, flags);
    if (e) return e;
    return dispatch::chunk_range(n_tiles, dispatch::MAX_BLOCKS, [&](long t0, long nb) {
        return mesh_launch(ms_edge_kernel, dim3((unsigned)nb), MS_THREADS, st, a, tile_bounds, t0, n_tiles, cdf, tile_sum, total, flags);
    });
}

extern "C" int dpf_mesh_variates(int B, int S, unsigned long long seed, unsigned long long step, double *u, float *s1, float *s2,
                                 dpf_stream_t stream) {
    if (B < 1 || S < 1 || !u || !s1 || !s2) return DPF_EINVAL;
    // the host mirror: datasets/sampling.py:host_variates
    uint64_t x = seed + 0x9E3779B97F4A7C15ull, z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    x = (z ^ step) + 0x9E3779B97F4A7C15ull;
    uint64_t base = x;
    base = (base ^ (base >> 30)) * 0xBF58476D1CE4E5B9ull;
    base = (base ^ (base >> 27)) * 0x94D049BB133111EBull;
    base ^= base >> 31;
    const size_t n = (size_t)B * (size_t)S;
    return dispatch::chunk_range((long)n, dispatch::MAX_BLOCKS * MS_THREADS, [&](long i0, long cnt) {
        return mesh_launch(ms_variates_kernel, dim3((unsigned)dispatch::ceil_div(cnt, MS_THREADS)), MS_THREADS, (hipStream_t)stream, S, i0, n,
                           base, u, s1, s2);
    });
}

extern "C" int dpf_mesh_sample(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                               const long *face_bounds, const double *cdf, const unsigned int *flags, const float *orig_c,
                               const float *orig_s, int B, int S, const int *mesh_idx, const double *u, const float *s1,
                               const float *s2, int split, int xform, float shift_x, float shift_y, float shift_z, float scale,
                               float *cloud, float *eval_cloud, int *faces_out, dpf_stream_t stream) {
    if (!ms_store_ok(M, vertices, vertex_bounds, faces, face_bounds) || !cdf || !flags) return DPF_EINVAL;
    if (B < 1 || S < 1 || !mesh_idx || !u || !s1 || !s2 || !cloud) return DPF_EINVAL;
    if (split != 0 && split != 1) return DPF_EINVAL;
    if (split && ((S & 1) || !eval_cloud)) return DPF_EINVAL;
    if ((xform & ~15) || ((xform & 1) && !orig_s) || ((xform & 2) && !orig_c)) return DPF_EINVAL;
    if ((long)((S + MS_THREADS - 1) / MS_THREADS) > dispatch::MAX_BLOCKS) return DPF_ENOSUP;
    const MeshStore st{M, vertices, vertex_bounds, faces, face_bounds, flags};
    const MeshSampleArgs a{cdf, orig_c, orig_s, S, split, xform, mesh_idx, u, s1, s2, {shift_x, shift_y, shift_z}, scale,
                           cloud, eval_cloud, faces_out};
    return dispatch::chunk_range(B, dispatch::MAX_SLOTS, [&](long b0, long nb) {
        return mesh_launch(ms_sample_kernel, dim3((unsigned)((S + MS_THREADS - 1) / MS_THREADS), (unsigned)nb), MS_THREADS, (hipStream_t)stream,
                           st, a, (int)b0);
    });
}
