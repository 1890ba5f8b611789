// Mesh-to-cloud distance over the device mesh store (datasets.MeshStore): for every face of a slot's mesh the minimum over the
// slot's points of the squared distance to the closed triangle, a point that attains it, the closest point on the face to that
// point, and the face's area.  The column minimum of the (point, face) matrix whose row minimum point_mesh.hip returns; brute
// force, B * N * F point-triangle tests, the points broadcast from LDS.
//
// The contract is in include/dpf_hip.h.  The arithmetic of a pair is pm_stage / pm_eval of pm_pair.h, the one point_mesh.hip
// uses: nothing here evaluates a pair in any other way; the host side of the two forms is its pm_search.  The store view, the slot
// rule, the keys and the face area come from mesh_store.h.
//   the minimum -- (distance bits << 32 | point) as an unsigned 64-bit key: non-negative fp32 bit patterns order as the floats
//               do, the lowest point index wins among equal distances, and a minimum does not depend on the order it is taken in.
//               A non-finite point is staged as the origin with a mask of all ones that is OR-ed into its distance bits: it can
//               never be lower than the initial key, so it is never a face's nearest -- one integer operation per pair, no branch.
//   the area  -- dpf_mesh_cdf_build's, by the one function both call (mesh_face_area); 0 where it is not finite.
//
// Two kernel forms (dispatch.h: mp_form, a wrapper of split_form).  Whole: a workgroup of 4 waves holds 256 faces of one slot, one staged face per lane in
// registers, and walks every 256-point tile of the slot's cloud.  Split: the tiles are dealt round-robin to `splits` workgroups
// per 256 faces, each folds its minimum into a key buffer pre-set to all-ones with a 64-bit vector atomic minimum, and a
// finishing launch unpacks the key.  Both forms write a column through mp_write, which evaluates the winning pair once more for
// the closest point.
//
// The backward is a gather: a point's lane scans its slot's `point` row in face order and adds the terms of the faces that name
// it, so the sum has one order and needs no atomics.
//
// Compiled with -ffp-contract=off, like point_mesh.hip: the fused operations are the fmaf calls of pm_pair.h and no others.
// fp32 division and square root are the correctly rounded ones.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "pm_pair.h"

namespace {

using namespace pm;

constexpr int MP_THREADS = dispatch::MP_WG_FACES;   // threads = faces of a workgroup: one face per lane, 4 waves
constexpr int MP_TILE = dispatch::MP_TILE;          // points per LDS tile: one point staged per thread

static_assert(MP_TILE == MP_THREADS, "one thread stages one point of a tile");
static_assert(MP_THREADS == PM_THREADS, "pm_search launches workgroups of PM_THREADS");

// the outputs of column f of slot b from its key; pts: the slot's points
__device__ __forceinline__ void mp_write(const MeshStore &st, const MeshSlot &s, long f, unsigned long long key, const float *pts, size_t at,
                                         float *dist, int *point, float *closest, float *area) {
    const float nan = __builtin_nanf("");
    float d = nan, qx = nan, qy = nan, qz = nan, a = 0.0f;
    int k = -1;
    // (the key is taken apart in place, not through mesh_store.h's helpers: with them mp_kernel<false> compiles to other code)
    if (s.ok && f < s.F && (unsigned int)key != 0xffffffffu) {              // (all ones: no finite point reached this face)
        k = (int)(unsigned int)key;
        const float px = pts[(size_t)k * 3], py = pts[(size_t)k * 3 + 1], pz = pts[(size_t)k * 3 + 2];
        const MeshCorners c = mesh_corners(st, s.fb, s.vb, f);
        const PMFace face = pm_stage(c.p0, c.p1, c.p2);
        pm_eval(face, px, py, pz, qx, qy, qz);
        d = __uint_as_float((unsigned int)(key >> 32));
        const float sa = mesh_face_area(c);
        a = sa <= 3.402823466e38f ? sa : 0.0f;                              // (false for NaN and for +inf)
    }
    dist[at] = d;
    point[at] = k;
    if (closest) { closest[at * 3] = qx; closest[at * 3 + 1] = qy; closest[at * 3 + 2] = qz; }
    if (area) area[at] = a;
}

// point tiles t0, t0 + stride, ... of the slot's cloud; SPLIT: the minimum goes into keys, else straight to the outputs
template <bool SPLIT>
__global__ __launch_bounds__(MP_THREADS) void mp_kernel(MeshStore st, int N, const float *__restrict__ points, const int *mesh_idx, long W,
                                                        int b0, long blk0, unsigned long long *keys, float *dist, int *point,
                                                        float *closest, float *area) {
    __shared__ float4 pt[MP_TILE];                                          // x, y, z, the mask; a lane-uniform index broadcasts
    const int tid = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    const long f0 = (blk0 + blockIdx.x) * MP_THREADS, f = f0 + tid;
    const MeshSlot s = mesh_slot(st, mesh_idx, b);
    const float *pts = points + b * (size_t)N * 3;
    const bool mine = s.ok && f < s.F && f < W;
    PMFace face{};                                                          // (a lane without a face evaluates a point-like thin face; unused)
    if (mine) face = pm_stage_face(st, s, (int)f);
    unsigned int best = 0xffffffffu, bestp = 0xffffffffu;
    if (s.ok && f0 < s.F) {                                                 // (the same for the whole workgroup)
        const int ntiles = (N + MP_TILE - 1) / MP_TILE;
        const int t0 = SPLIT ? (int)blockIdx.z : 0, stride = SPLIT ? (int)gridDim.z : 1;
        for (int t = t0; t < ntiles; t += stride) {
            const int base = t * MP_TILE, cnt = N - base < MP_TILE ? N - base : MP_TILE;
            __syncthreads();
            if (tid < cnt) {
                const float *p = pts + (size_t)(base + tid) * 3;
                const float x = p[0], y = p[1], z = p[2];
                const bool finite = pm_finite(x, y, z);
                pt[tid] = finite ? make_float4(x, y, z, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const float4 p = pt[j];
                float qx, qy, qz;
                const unsigned int d = __float_as_uint(pm_eval(face, p.x, p.y, p.z, qx, qy, qz)) | __float_as_uint(p.w);
                const bool lower = d < best;                                // points come in ascending order: strict keeps the lowest index
                best = lower ? d : best;
                bestp = lower ? (unsigned int)(base + j) : bestp;
            }
        }
    }
    if (f >= W) return;
    const size_t at = b * (size_t)W + (size_t)f;
    const unsigned long long key = mesh_key(best, bestp);
    if (SPLIT) {
        if (mine && bestp != 0xffffffffu) atomicMin(&keys[at], key);
    } else {
        mp_write(st, s, f, key, pts, at, dist, point, closest, area);
    }
}

__global__ __launch_bounds__(MP_THREADS) void mp_finish_kernel(MeshStore st, int N, const float *__restrict__ points, const int *mesh_idx,
                                                               long W, int b0, long blk0, const unsigned long long *keys, float *dist,
                                                               int *point, float *closest, float *area) {
    const size_t b = (size_t)b0 + blockIdx.y;
    const long f = (blk0 + blockIdx.x) * MP_THREADS + threadIdx.x;
    if (f >= W) return;
    const size_t at = b * (size_t)W + (size_t)f;
    const MeshSlot s = mesh_slot(st, mesh_idx, b);
    mp_write(st, s, f, keys[at], points + b * (size_t)N * 3, at, dist, point, closest, area);
}

// one thread per point: the terms of the faces that name it, in ascending face order
__global__ __launch_bounds__(MP_THREADS) void mp_grad_kernel(int N, long W, int b0, long blk0, const float *__restrict__ points,
                                                             const int *__restrict__ point, const float *__restrict__ closest,
                                                             const float *__restrict__ grad_dist, float *__restrict__ grad_points) {
    __shared__ int who[MP_TILE];
    const int tid = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    const long n = (blk0 + blockIdx.x) * MP_THREADS + tid;
    const size_t row = b * (size_t)W, at = b * (size_t)N + (size_t)n;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (n < N) { px = points[at * 3]; py = points[at * 3 + 1]; pz = points[at * 3 + 2]; }
    const int me = n < N ? (int)n : -2;                                     // (-1 marks a column without a nearest point)
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (long base = 0; base < W; base += MP_TILE) {
        const int cnt = W - base < MP_TILE ? (int)(W - base) : MP_TILE;
        __syncthreads();
        if (tid < cnt) who[tid] = point[row + base + tid];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            if (who[j] != me) continue;
            const size_t c = row + base + j;
            const float g2 = 2.0f * grad_dist[c];
            const float qx = closest[c * 3], qy = closest[c * 3 + 1], qz = closest[c * 3 + 2];
            gx += qx == qx ? g2 * (px - qx) : 0.0f;                         // no closest point (NaN): no gradient
            gy += qy == qy ? g2 * (py - qy) : 0.0f;
            gz += qz == qz ? g2 * (pz - qz) : 0.0f;
        }
    }
    if (n >= N) return;
    grad_points[at * 3] = gx; grad_points[at * 3 + 1] = gy; grad_points[at * 3 + 2] = gz;
}

}  // namespace

extern "C" int dpf_mesh_point_tile(void) { return MP_TILE; }

extern "C" size_t dpf_mesh_point_workspace_bytes(int B, long max_faces) {
    if (B < 1 || max_faces < 1) return 0;
    return (size_t)B * (size_t)max_faces * sizeof(unsigned long long);
}

extern "C" int dpf_mesh_point_distance(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                                       const long *face_bounds, const unsigned int *flags, int B, int N, const float *points,
                                       const int *mesh_idx, long max_faces, int form, float *dist, int *point, float *closest,
                                       float *area, void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || N < 0 || max_faces < 0 || max_faces > 0x7fffffffL || form < 0 || form > 2) return DPF_EINVAL;
    const long W = max_faces;
    if (B == 0 || W == 0) return 0;
    if (M < 1 || !vertices || !vertex_bounds || !faces || !face_bounds || !flags || (!points && N > 0) || !mesh_idx || !dist || !point)
        return DPF_EINVAL;
    const dispatch::PMForm mf = dispatch::mp_form(B, N, W, form);
    hipStream_t s = (hipStream_t)stream;
    const MeshStore st{M, vertices, vertex_bounds, faces, face_bounds, flags};
    unsigned long long *keys = (unsigned long long *)workspace;
    auto pass = [=](auto kernel, int z) {
        return [=](int b0, unsigned nb, long k0, unsigned nk) {
            return mesh_launch(kernel, dim3(nk, nb, (unsigned)z), MP_THREADS, s, st, N, points, mesh_idx, W, b0, k0, keys, dist, point,
                               closest, area);
        };
    };
    return pm_search(mf, B, W, workspace, workspace_bytes, s, pass(mp_kernel<false>, 1), pass(mp_kernel<true>, mf.splits),
                     pass(mp_finish_kernel, 1));
}

extern "C" int dpf_mesh_point_distance_grad(int B, int N, long max_faces, const float *points, const int *point, const float *closest,
                                            const float *grad_dist, float *grad_points, dpf_stream_t stream) {
    if (B < 0 || N < 0 || max_faces < 0 || max_faces > 0x7fffffffL) return DPF_EINVAL;
    if (B == 0 || N == 0) return 0;
    if (!points || !grad_points || (max_faces > 0 && (!point || !closest || !grad_dist))) return DPF_EINVAL;
    return dispatch::chunk_grid(B, dispatch::ceil_div(N, MP_THREADS), [&](int b0, unsigned nb, long k0, unsigned nk) {
        return mesh_launch(mp_grad_kernel, dim3(nk, nb), MP_THREADS, (hipStream_t)stream, N, max_faces, b0, k0, points, point, closest,
                           grad_dist, grad_points);
    });
}
