// The arithmetic of one (point, triangle) pair over the device mesh store, defined ONCE for both directions of the surface
// distance: point_mesh.hip (for every point the nearest face) and mesh_point.hip (for every face the nearest point) include
// this header and nothing else evaluates a pair.  The contract is in include/dpf_hip.h; in short
//   pm_stage -- per face: 16 floats (corner a, the edge vectors ab = b - a and ac = c - a, their dot products aa, g = ab.ac, cc,
//               and the reciprocals 1/aa, 1/cc, 1/|c - b|^2, 1/det with det = aa * cc - g * g).  A face is THIN when
//               !(det > 2^-14 * (aa * cc)): degenerate faces (zero area, repeated vertices) and slivers whose determinant is
//               mostly rounding; its 1/det is stored as 0.
//   pm_eval  -- per (point, face): Ericson's region classification (Real-Time Collision Detection, 5.1.5) on d1 = ab.ap,
//               d2 = ac.ap and the staged dot products -- d3 = d1 - aa, d4 = d2 - g, d5 = d1 - g, d6 = d2 - cc, vb = cc * d1 - g * d2,
//               vc = aa * d2 - g * d1 -- as a chain of selects; every quotient is a product with a staged reciprocal, so a pair
//               costs no division.  A thin face is the nearest of its three edges (segments, or points where an edge has no
//               length), ties to AB, then AC, then BC.  The closest point is q = a + v * ab + w * ac, the distance |p - q|^2.
//
// The store view, the slot rule, a face's corners and the keys of the minimum come from mesh_store.h.  Below the arithmetic, what
// the host side of both searches shares: pm_fill_kernel and pm_search, the driver of the Whole and the Split form.
//
// Both translation units are compiled with -ffp-contract=off: the fused operations are the fmaf calls written out below and no
// others.  fp32 division (staging only) is the correctly rounded one.
#ifndef DPF_PM_PAIR_H
#define DPF_PM_PAIR_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"
#include "mesh_store.h"

namespace pm {

constexpr float PM_THIN = 6.103515625e-05f;         // 2^-14

// what the lanes of a wave share about a face (point_mesh.hip), or what a lane keeps of its own face (mesh_point.hip)
struct PMFace {
    float ax, ay, az, aa;
    float abx, aby, abz, g;
    float acx, acy, acz, cc;
    float iaa, icc, ibc, idet;
};

__device__ __forceinline__ float pm_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ PMFace pm_stage(const float *v0, const float *v1, const float *v2) {
    PMFace f;
    f.ax = v0[0]; f.ay = v0[1]; f.az = v0[2];
    f.abx = v1[0] - f.ax; f.aby = v1[1] - f.ay; f.abz = v1[2] - f.az;
    f.acx = v2[0] - f.ax; f.acy = v2[1] - f.ay; f.acz = v2[2] - f.az;
    f.aa = pm_dot(f.abx, f.aby, f.abz, f.abx, f.aby, f.abz);
    f.g = pm_dot(f.abx, f.aby, f.abz, f.acx, f.acy, f.acz);
    f.cc = pm_dot(f.acx, f.acy, f.acz, f.acx, f.acy, f.acz);
    const float ex = f.acx - f.abx, ey = f.acy - f.aby, ez = f.acz - f.abz;
    const float bb = pm_dot(ex, ey, ez, ex, ey, ez);
    const float det = fmaf(f.aa, f.cc, -(f.g * f.g));
    f.iaa = f.aa > 0.0f ? 1.0f / f.aa : 0.0f;
    f.icc = f.cc > 0.0f ? 1.0f / f.cc : 0.0f;
    f.ibc = bb > 0.0f ? 1.0f / bb : 0.0f;
    f.idet = det > PM_THIN * (f.aa * f.cc) ? 1.0f / det : 0.0f;
    return f;
}

__device__ __forceinline__ float pm_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }     // (a NaN becomes 0)

// q = a + v * ab + w * ac and |p - q|^2
__device__ __forceinline__ float pm_point(const PMFace &f, float px, float py, float pz, float v, float w, float &qx, float &qy,
                                          float &qz) {
    qx = fmaf(w, f.acx, fmaf(v, f.abx, f.ax));
    qy = fmaf(w, f.acy, fmaf(v, f.aby, f.ay));
    qz = fmaf(w, f.acz, fmaf(v, f.abz, f.az));
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

__device__ __forceinline__ float pm_eval(const PMFace &f, float px, float py, float pz, float &qx, float &qy, float &qz) {
    const float apx = px - f.ax, apy = py - f.ay, apz = pz - f.az;
    const float d1 = pm_dot(f.abx, f.aby, f.abz, apx, apy, apz), d2 = pm_dot(f.acx, f.acy, f.acz, apx, apy, apz);
    const float d3 = d1 - f.aa, d4 = d2 - f.g, d5 = d1 - f.g, d6 = d2 - f.cc;
    const float tab = pm_clamp01(d1 * f.iaa), tac = pm_clamp01(d2 * f.icc), tbc = pm_clamp01((d4 - d3) * f.ibc);
    if (f.idet == 0.0f) {                                                   // a thin face: the nearest of its three edges
        float d = pm_point(f, px, py, pz, tab, 0.0f, qx, qy, qz);
        float x, y, z;
        float e = pm_point(f, px, py, pz, 0.0f, tac, x, y, z);
        if (e < d) { d = e; qx = x; qy = y; qz = z; }
        e = pm_point(f, px, py, pz, 1.0f - tbc, tbc, x, y, z);
        if (e < d) { d = e; qx = x; qy = y; qz = z; }
        return d;
    }
    const float vb = fmaf(f.cc, d1, -(f.g * d2)), vc = fmaf(f.aa, d2, -(f.g * d1));
    float v = vb * f.idet, w = vc * f.idet;                                // inside the triangle
    bool c = v + w >= 1.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f;           // edge BC (va <= 0)
    v = c ? 1.0f - tbc : v; w = c ? tbc : w;
    c = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;                             // edge AC
    v = c ? 0.0f : v; w = c ? tac : w;
    c = d6 >= 0.0f && d5 <= d6;                                             // corner C
    v = c ? 0.0f : v; w = c ? 1.0f : w;
    c = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;                             // edge AB
    v = c ? tab : v; w = c ? 0.0f : w;
    c = d3 >= 0.0f && d4 <= d3;                                             // corner B
    v = c ? 1.0f : v; w = c ? 0.0f : w;
    c = d1 <= 0.0f && d2 <= 0.0f;                                           // corner A
    v = c ? 0.0f : v; w = c ? 0.0f : w;
    v = pm_clamp01(v);                                                      // whatever rounding did to the classification,
    w = fminf(fmaxf(w, 0.0f), 1.0f - v);                                    // q lies on the closed triangle
    return pm_point(f, px, py, pz, v, w, qx, qy, qz);
}

__device__ __forceinline__ PMFace pm_stage_face(const MeshStore &st, const MeshSlot &s, int face) {
    const MeshCorners c = mesh_corners(st, s.fb, s.vb, face);
    return pm_stage(c.p0, c.p1, c.p2);
}

__device__ __forceinline__ bool pm_finite(float x, float y, float z) {
    return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;   // (false for NaN)
}

// ---- the host side of a search in either direction ------------------------------------------------------------------------------
constexpr int PM_THREADS = dispatch::PM_WG_POINTS;  // threads of every workgroup of both directions: 4 waves, one row item per lane
static_assert(PM_THREADS == dispatch::MP_WG_FACES, "both directions launch the same workgroups");

static __global__ __launch_bounds__(PM_THREADS) void pm_fill_kernel(unsigned long long *keys, size_t i0, size_t n) {
    const size_t i = i0 + (size_t)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i < n) keys[i] = ~0ull;
}

// B slots of `row` items (points, or columns of faces), PM_THREADS items per workgroup.  whole / split / finish launch one chunk
// (b0, nb, k0, nk) of the grid and return the launch's error.  Whole: one pass.  Split: the keys (the workspace, B * row of them)
// are set to all ones, `split` folds its minima into them, `finish` unpacks them.
template <class Whole, class Split, class Finish>
inline int pm_search(dispatch::PMForm form, int B, long row, void *workspace, size_t workspace_bytes, hipStream_t stream, Whole whole,
                     Split split, Finish finish) {
    const long blocks = dispatch::ceil_div(row, PM_THREADS);
    if (form.kernel == dispatch::PMKernel::Whole) return dispatch::chunk_grid(B, blocks, whole);
    unsigned long long *keys = (unsigned long long *)workspace;
    const size_t n = (size_t)B * (size_t)row;
    if (!keys || ((uintptr_t)keys & 7) || workspace_bytes < n * sizeof(*keys)) return DPF_EINVAL;
    int e = dispatch::chunk_range((long)n, dispatch::MAX_BLOCKS * PM_THREADS, [&](long i0, long cnt) {
        return mesh_launch(pm_fill_kernel, dim3((unsigned)dispatch::ceil_div(cnt, PM_THREADS)), PM_THREADS, stream, keys, i0, n);
    });
    if (!e) e = dispatch::chunk_grid(B, blocks, split);
    if (!e) e = dispatch::chunk_grid(B, blocks, finish);
    return e;
}

}  // namespace pm
#endif  // DPF_PM_PAIR_H
