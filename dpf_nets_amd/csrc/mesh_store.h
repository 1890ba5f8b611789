// The device mesh store (datasets.MeshStore) as the kernels see it, defined ONCE for everything that reads it: mesh_sample.hip
// (the area distribution and the sampler), point_mesh.hip and mesh_point.hip (through pm_pair.h).  The layout mirrors the
// reference's meshes.h5: packed fp32 vertices (sum V, 3), packed faces (sum F, 3) whose vertex indices are LOCAL to their mesh,
// two bounds arrays of M + 1 entries, and the validation flags dpf_mesh_cdf_build leaves per mesh.
//   mesh_slot      -- the mesh of a batch slot.  An index outside the store, a flagged mesh or one without a face is not ok:
//                     nothing of it is read, and the caller writes NaN / -1.
//   mesh_corners   -- the three vertices of face k of a slot's mesh (validated by dpf_mesh_cdf_build wherever flags[m] == 0).
//   mesh_face_area -- the area as numpy forms it, in fp32, every operation rounded on its own (the includers are compiled with
//                     -ffp-contract=off and the correctly rounded square root): e1 = p2 - p0, e2 = p2 - p1,
//                     c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x), sqrt((c0*c0 + c1*c1) + c2*c2) / 2.
//   mesh_key*      -- a search's minimum as an unsigned 64-bit key (distance bits << 32 | index): non-negative fp32 bit patterns
//                     order as the floats do, the lowest index wins among equal distances, and an index of all ones names nothing.
//   mesh_launch    -- a launch and its error, the value dispatch.h's chunkers take from their launch functors.
#ifndef DPF_MESH_STORE_H
#define DPF_MESH_STORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

struct MeshStore {
    int M;
    const float *vertices;
    const long *vertex_bounds;
    const unsigned int *faces;
    const long *face_bounds;
    const unsigned int *flags;
};

struct MeshSlot { bool ok; int m; long fb, vb; int F; };

__device__ __forceinline__ MeshSlot mesh_slot(const MeshStore &st, const int *mesh_idx, size_t b) {
    MeshSlot s{false, mesh_idx[b], 0, 0, 0};
    if (s.m < 0 || s.m >= st.M || st.flags[s.m] != 0u) return s;            // nothing of such a mesh is read
    s.fb = st.face_bounds[s.m]; s.vb = st.vertex_bounds[s.m];
    s.F = (int)(st.face_bounds[s.m + 1] - s.fb);
    s.ok = s.F >= 1;
    return s;
}

struct MeshCorners { const float *p0, *p1, *p2; };

// fb, vb: the mesh's first face and first vertex
__device__ __forceinline__ MeshCorners mesh_corners(const MeshStore &st, long fb, long vb, long k) {
    const unsigned int *fi = st.faces + (size_t)(fb + k) * 3;
    return {st.vertices + (size_t)(vb + fi[0]) * 3, st.vertices + (size_t)(vb + fi[1]) * 3, st.vertices + (size_t)(vb + fi[2]) * 3};
}

__device__ __forceinline__ float mesh_face_area(const MeshCorners &c) {
    const float ax = c.p2[0] - c.p0[0], ay = c.p2[1] - c.p0[1], az = c.p2[2] - c.p0[2];
    const float bx = c.p2[0] - c.p1[0], by = c.p2[1] - c.p1[1], bz = c.p2[2] - c.p1[2];
    const float c0 = ay * bz - az * by, c1 = az * bx - ax * bz, c2 = ax * by - ay * bx;
    return sqrtf((c0 * c0 + c1 * c1) + c2 * c2) / 2.0f;
}

__device__ __forceinline__ unsigned long long mesh_key(unsigned long long dist_bits, unsigned int index) {
    return (dist_bits << 32) | index;
}
__device__ __forceinline__ int mesh_key_index(unsigned long long key) { return (int)(unsigned int)key; }
__device__ __forceinline__ float mesh_key_dist(unsigned long long key) { return __uint_as_float((unsigned int)(key >> 32)); }

template <class... P, class... A>
inline int mesh_launch(void (*kernel)(P...), dim3 grid, int threads, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, stream, args...);
    return (int)hipGetLastError();
}

#endif  // DPF_MESH_STORE_H
