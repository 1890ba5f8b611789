// Exact squared distance from query points to the triangle meshes of the device mesh store (datasets.MeshStore): for every
// point the minimum over the faces of its slot's mesh of the squared distance to the closed triangle, a face that attains it
// and the closest point on that face.  Brute force, B * N * F point-triangle tests, the faces broadcast from LDS.
//
// The contract is in include/dpf_hip.h; the arithmetic of a pair and the host side of the two forms live in pm_pair.h, shared with
// mesh_point.hip; the store view, the slot rule and the keys in mesh_store.h, shared with mesh_sample.hip too.  In short
//   pm_stage -- per face, once per tile and workgroup: 16 floats every lane of a wave shares (corner a, the edge vectors
//               ab = b - a and ac = c - a, their dot products aa, g = ab.ac, cc, and the reciprocals 1/aa, 1/cc, 1/|c - b|^2,
//               1/det with det = aa * cc - g * g).  A face is THIN when !(det > 2^-14 * (aa * cc)): degenerate faces (zero area,
//               repeated vertices) and slivers whose determinant is mostly rounding; its 1/det is stored as 0.
//   pm_eval  -- per (point, face): Ericson's region classification (Real-Time Collision Detection, 5.1.5) on d1 = ab.ap,
//               d2 = ac.ap and the staged dot products -- d3 = d1 - aa, d4 = d2 - g, d5 = d1 - g, d6 = d2 - cc, vb = cc * d1 - g * d2,
//               vc = aa * d2 - g * d1 -- as a chain of selects; every quotient is a product with a staged reciprocal, so a pair
//               costs no division.  A thin face is the nearest of its three edges (segments, or points where an edge has no
//               length), ties to AB, then AC, then BC.  The closest point is q = a + v * ab + w * ac, the distance |p - q|^2.
//   the minimum -- (distance bits << 32 | face) as an unsigned 64-bit key: non-negative fp32 bit patterns order as the floats
//               do, the lowest face index wins among equal distances, and a minimum does not depend on the order it is taken in.
//
// Two kernel forms (dispatch.h: pm_form, a wrapper of split_form), driven by pm_pair.h's pm_search.  Whole: a workgroup of 4 waves holds 256 points of one slot, one per lane, and walks
// every tile of the slot's mesh.  Split: the tiles of a mesh are dealt round-robin to `splits` workgroups per 256 points, each
// folds its minimum into a key buffer pre-set to all-ones with a 64-bit vector atomic minimum, and a finishing launch unpacks
// the key and recomputes the closest point on the winning face with the same pm_stage / pm_eval.
//
// Compiled with -ffp-contract=off: the fused operations are the fmaf calls written out below and no others, so both forms and
// the finishing pass round alike.  fp32 division (staging only) is the correctly rounded one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "pm_pair.h"

namespace {

using namespace pm;                                 // PMFace, pm_stage, pm_eval, PM_THREADS (= points of a workgroup), pm_search, ...

constexpr int PM_TILE = dispatch::PM_TILE;          // faces per LDS tile: one face staged per thread

static_assert(PM_TILE == PM_THREADS, "one thread stages one face of a tile");

// the outputs of one point from its key
__device__ __forceinline__ void pm_write(const MeshStore &st, const MeshSlot &s, bool finite, unsigned long long key, float px, float py,
                                         float pz, size_t at, float *dist, int *face, float *closest) {
    const float nan = __builtin_nanf("");
    float d = nan, qx = nan, qy = nan, qz = nan;
    int k = -1;
    if (s.ok && finite) {
        k = mesh_key_index(key);
        const PMFace f = pm_stage_face(st, s, k);
        pm_eval(f, px, py, pz, qx, qy, qz);
        d = mesh_key_dist(key);
    }
    dist[at] = d;
    face[at] = k;
    if (closest) { closest[at * 3] = qx; closest[at * 3 + 1] = qy; closest[at * 3 + 2] = qz; }
}

// tiles t0, t0 + stride, ... of the slot's mesh; SPLIT: the minimum goes into keys, else straight to the outputs
template <bool SPLIT>
__global__ __launch_bounds__(PM_THREADS) void pm_kernel(MeshStore st, int N, const float *__restrict__ points, const int *mesh_idx,
                                                        int b0, long blk0, unsigned long long *keys, float *dist, int *face,
                                                        float *closest) {
    __shared__ float4 q0[PM_TILE], q1[PM_TILE], q2[PM_TILE], q3[PM_TILE];   // structure of arrays: a lane-uniform index broadcasts
    const int tid = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    const long n = (blk0 + blockIdx.x) * PM_THREADS + tid;
    const size_t at = b * (size_t)N + (size_t)n;
    const MeshSlot s = mesh_slot(st, mesh_idx, b);
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    bool finite = false;
    if (n < N) {
        px = points[at * 3]; py = points[at * 3 + 1]; pz = points[at * 3 + 2];
        finite = pm_finite(px, py, pz);
        if (!finite) px = py = pz = 0.0f;
    }
    unsigned int best = 0xffffffffu, bestf = 0xffffffffu;
    if (s.ok) {                                                             // (the same for the whole workgroup)
        const int ntiles = (s.F + PM_TILE - 1) / PM_TILE;
        const int t0 = SPLIT ? (int)blockIdx.z : 0, stride = SPLIT ? (int)gridDim.z : 1;
        for (int t = t0; t < ntiles; t += stride) {
            const int base = t * PM_TILE, cnt = s.F - base < PM_TILE ? s.F - base : PM_TILE;
            __syncthreads();
            if (tid < cnt) {
                const PMFace f = pm_stage_face(st, s, base + tid);
                q0[tid] = make_float4(f.ax, f.ay, f.az, f.aa);
                q1[tid] = make_float4(f.abx, f.aby, f.abz, f.g);
                q2[tid] = make_float4(f.acx, f.acy, f.acz, f.cc);
                q3[tid] = make_float4(f.iaa, f.icc, f.ibc, f.idet);
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const float4 a0 = q0[j], a1 = q1[j], a2 = q2[j], a3 = q3[j];
                const PMFace f{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w};
                float qx, qy, qz;
                const unsigned int d = __float_as_uint(pm_eval(f, px, py, pz, qx, qy, qz));
                const bool lower = d < best;                                // faces come in ascending order: strict keeps the lowest index
                best = lower ? d : best;
                bestf = lower ? (unsigned int)(base + j) : bestf;
            }
        }
    }
    if (n >= N) return;
    const unsigned long long key = mesh_key(best, bestf);
    if (SPLIT) {
        if (s.ok && finite && bestf != 0xffffffffu) atomicMin(&keys[at], key);
    } else {
        pm_write(st, s, finite, key, px, py, pz, at, dist, face, closest);
    }
}

__global__ __launch_bounds__(PM_THREADS) void pm_finish_kernel(MeshStore st, int N, const float *__restrict__ points, const int *mesh_idx,
                                                               int b0, long blk0, const unsigned long long *keys, float *dist, int *face,
                                                               float *closest) {
    const size_t b = (size_t)b0 + blockIdx.y;
    const long n = (blk0 + blockIdx.x) * PM_THREADS + threadIdx.x;
    if (n >= N) return;
    const size_t at = b * (size_t)N + (size_t)n;
    const MeshSlot s = mesh_slot(st, mesh_idx, b);
    const float px = points[at * 3], py = points[at * 3 + 1], pz = points[at * 3 + 2];
    pm_write(st, s, pm_finite(px, py, pz), keys[at], px, py, pz, at, dist, face, closest);
}

__global__ __launch_bounds__(PM_THREADS) void pm_grad_kernel(size_t i0, size_t n, const float *__restrict__ points,
                                                             const float *__restrict__ closest, const float *__restrict__ grad_dist,
                                                             float *__restrict__ grad_points) {
    const size_t i = i0 + (size_t)blockIdx.x * PM_THREADS + threadIdx.x;    // one thread per point
    if (i >= n) return;
    const float g2 = 2.0f * grad_dist[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q = closest[i * 3 + c];
        grad_points[i * 3 + c] = q == q ? g2 * (points[i * 3 + c] - q) : 0.0f;          // no closest point (NaN): no gradient
    }
}

}  // namespace

extern "C" int dpf_point_mesh_tile(void) { return PM_TILE; }

extern "C" size_t dpf_point_mesh_workspace_bytes(int B, int N) {
    if (B < 1 || N < 1) return 0;
    return (size_t)B * (size_t)N * sizeof(unsigned long long);
}

extern "C" int dpf_point_mesh_distance(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                                       const long *face_bounds, const unsigned int *flags, int B, int N, const float *points,
                                       const int *mesh_idx, long max_faces, int form, float *dist, int *face, float *closest,
                                       void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || N < 0 || form < 0 || form > 2) return DPF_EINVAL;
    if (B == 0 || N == 0) return 0;
    if (M < 1 || !vertices || !vertex_bounds || !faces || !face_bounds || !flags || !points || !mesh_idx || !dist || !face)
        return DPF_EINVAL;
    if (max_faces < 1) return DPF_EINVAL;
    const dispatch::PMForm pf = dispatch::pm_form(B, N, max_faces, form);
    hipStream_t s = (hipStream_t)stream;
    const MeshStore st{M, vertices, vertex_bounds, faces, face_bounds, flags};
    unsigned long long *keys = (unsigned long long *)workspace;
    auto pass = [=](auto kernel, int z) {
        return [=](int b0, unsigned nb, long k0, unsigned nk) {
            return mesh_launch(kernel, dim3(nk, nb, (unsigned)z), PM_THREADS, s, st, N, points, mesh_idx, b0, k0, keys, dist, face, closest);
        };
    };
    return pm_search(pf, B, N, workspace, workspace_bytes, s, pass(pm_kernel<false>, 1), pass(pm_kernel<true>, pf.splits),
                     pass(pm_finish_kernel, 1));
}

extern "C" int dpf_point_mesh_distance_grad(int B, int N, const float *points, const float *closest, const float *grad_dist,
                                            float *grad_points, dpf_stream_t stream) {
    if (B < 0 || N < 0) return DPF_EINVAL;
    if (B == 0 || N == 0) return 0;
    if (!points || !closest || !grad_dist || !grad_points) return DPF_EINVAL;
    const size_t n = (size_t)B * (size_t)N;
    return dispatch::chunk_range((long)n, dispatch::MAX_BLOCKS * PM_THREADS, [&](long i0, long cnt) {
        return mesh_launch(pm_grad_kernel, dim3((unsigned)dispatch::ceil_div(cnt, PM_THREADS)), PM_THREADS, (hipStream_t)stream, i0, n,
                           points, closest, grad_dist, grad_points);
    });
}
