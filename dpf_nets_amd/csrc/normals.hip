// Point-cloud normals by local PCA: per query point the covariance of its k listed neighbours, the eigen-decomposition of that 3 x 3
// matrix by cyclic Jacobi, and the unit eigenvector of the smallest eigenvalue with a defined sign.  The contract (validity, the
// bit-defined covariance, the rotation, the order, the sign) is in include/dpf_hip.h; tests/normals_ref.py restates it in numpy.
//
// One lane per point, one wave per workgroup: no LDS, no barrier, no workspace, no atomics, and no lane looks at another's data, so
// a point's outputs cannot depend on the batch or the launch shape.  A lane reads its k indices (dpf_knn's row), range-checks each
// BEFORE it becomes an address (a refused index reads point 0 and its value is dropped), gathers the k points once and keeps them in
// registers as fp32 -- 3 * KCAP VGPRs -- for the two passes of the covariance: the centroid, then the centred products.  The gather is
// unrolled over the capacity KCAP (4 | 8 | 16 | 32, the smallest >= k; dispatch.h: normals_form) and free of branches -- a branch per
// list slot made every load wait for the one before it -- so every load of a lane is in flight before the first is used, and the
// points are subscripted with compile-time indices only: the Makefile refuses a build of these kernels that uses scratch.  The
// arithmetic skips the slots past k under the wave-uniform test s < k.
//
// The matrix, the rotations' accumulated columns and the compare network are named scalars: nothing is subscripted at all.  The sweep
// loop is left rolled (a fixed trip count, dispatch::NORMALS_SWEEPS) -- unrolled it would only repeat three rotations' division and
// square-root expansions six times in the instruction cache.  A rotation whose off-diagonal entry is exactly 0 is skipped by a
// branch; lanes of a wave may disagree there, and the ones that skip wait for the others.
//
// Bounded: the loops run over the capacity, over the sweep count and over three pairs; there is no convergence test.
// Compiled with -ffp-contract=off: every float64 operation of the covariance rounds on its own, in the header's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"

namespace {

constexpr int NRM_THREADS = dispatch::NORMALS_WG_POINTS;
constexpr int NRM_SWEEPS = dispatch::NORMALS_SWEEPS;

struct NormalsArgs {
    const float *cloud;
    long csc, csp, csa;                             // floats between clouds, points, axes
    const int *index;                               // (B, n, k)
    int n, m, k;
    const float *view;                              // 3 floats a slot, or NULL
    long vss;                                       // floats between the slots' viewpoints
    double *normal, *lambda;                        // (B, n, 3)
    double *cov;                                    // (B, n, 6) or NULL
    int *flag;                                      // (B, n)
};

// a coordinate the contract refuses: not finite, or larger in magnitude than 2^61 (NaN fails the comparison too)
__device__ __forceinline__ unsigned nrm_out_of_range(float x, float y, float z) {
    const float lim = 0x1p61f;
    return (unsigned)!(__builtin_fabsf(x) <= lim) | (unsigned)!(__builtin_fabsf(y) <= lim) | (unsigned)!(__builtin_fabsf(z) <= lim);
}

// One Jacobi rotation in the (p, q) plane of the symmetric matrix; r is the third index.  (v0p, v0q), (v1p, v1q), (v2p, v2q): rows 0-2
// of the columns p and q of the accumulated eigenvectors.
__device__ __forceinline__ void nrm_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                           double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);                              // (theta^2 = +inf: t = 0, the identity)
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + root);
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y; arq = s * x + c * y;
    x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
    x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
    x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
}

// one compare-and-swap of the stable network: the (eigenvalue, column) pairs trade places only where the left value is strictly greater
__device__ __forceinline__ void nrm_order(double &la, double &lb, double &xa, double &ya, double &za, double &xb, double &yb, double &zb) {
    const bool swap = la > lb;
    const double l = la, x = xa, y = ya, z = za;
    la = swap ? lb : l; lb = swap ? l : lb;
    xa = swap ? xb : x; xb = swap ? x : xb;
    ya = swap ? yb : y; yb = swap ? y : yb;
    za = swap ? zb : z; zb = swap ? z : zb;
}

template <int KCAP>
__global__ __launch_bounds__(NRM_THREADS) void normals_kernel(NormalsArgs A, int b0, long blk0) {
    const size_t b = (size_t)b0 + blockIdx.y;
    const long i = (blk0 + blockIdx.x) * NRM_THREADS + threadIdx.x;
    if (i >= A.n) return;
    const int k = A.k, m = A.m;
    const size_t row = b * (size_t)A.n + (size_t)i;
    const int *idx = A.index + row * (size_t)k;
    const float *C = A.cloud + (long)b * A.csc;

    // Branch-free, so that nothing waits between the loads: a list slot at or past k re-reads slot 0 (an address inside the row; its
    // point is gathered and never used), and an index outside [0, m) -- checked before it is an address -- reads point 0
    int jj[KCAP];
#pragma unroll
    for (int s = 0; s < KCAP; ++s) jj[s] = idx[s < k ? s : 0];
    float px[KCAP], py[KCAP], pz[KCAP];
    unsigned bad = 0;
#pragma unroll
    for (int s = 0; s < KCAP; ++s) {
        const bool inside = (unsigned)jj[s] < (unsigned)m;
        const float *p = C + (long)(inside ? jj[s] : 0) * A.csp;
        px[s] = p[0]; py[s] = p[A.csa]; pz[s] = p[2 * A.csa];
        bad |= (unsigned)!inside;                                               // (slots past k repeat slot 0's verdict)
    }
#pragma unroll
    for (int s = 0; s < KCAP; ++s) bad |= nrm_out_of_range(px[s], py[s], pz[s]);

    double *normal = A.normal + row * 3, *lambda = A.lambda + row * 3, *cov = A.cov ? A.cov + row * 6 : nullptr;
    A.flag[row] = bad ? 1 : 0;
    if (bad) {
        const double nan = __builtin_nan("");
        normal[0] = normal[1] = normal[2] = nan;
        lambda[0] = lambda[1] = lambda[2] = nan;
        if (cov) cov[0] = cov[1] = cov[2] = cov[3] = cov[4] = cov[5] = nan;
        return;
    }

    // the centroid: ascending s from p_0, one division by (double) k
    double sx = (double)px[0], sy = (double)py[0], sz = (double)pz[0];
#pragma unroll
    for (int s = 1; s < KCAP; ++s)
        if (s < k) { sx = sx + (double)px[s]; sy = sy + (double)py[s]; sz = sz + (double)pz[s]; }
    const double kd = (double)k;
    const double cx = sx / kd, cy = sy / kd, cz = sz / kd;

    // the centred products: each rounded on its own, added in ascending s from the s = 0 term
    double a00, a01, a02, a11, a12, a22;
    {
        const double dx = (double)px[0] - cx, dy = (double)py[0] - cy, dz = (double)pz[0] - cz;
        a00 = dx * dx; a01 = dx * dy; a02 = dx * dz; a11 = dy * dy; a12 = dy * dz; a22 = dz * dz;
    }
#pragma unroll
    for (int s = 1; s < KCAP; ++s)
        if (s < k) {
            const double dx = (double)px[s] - cx, dy = (double)py[s] - cy, dz = (double)pz[s] - cz;
            a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
            a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
        }
    if (cov) { cov[0] = a00; cov[1] = a01; cov[2] = a02; cov[3] = a11; cov[4] = a12; cov[5] = a22; }

    // cyclic Jacobi, a fixed number of sweeps over (0, 1), (0, 2), (1, 2); vRC: row R of column C of the accumulated rotations
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < NRM_SWEEPS; ++sweep) {
        nrm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        nrm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        nrm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }

    // ascending, the lower column first among equals
    nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
    nrm_order(a11, a22, v01, v11, v21, v02, v12, v22);
    nrm_order(a00, a11, v00, v10, v20, v01, v11, v21);
    lambda[0] = a00; lambda[1] = a11; lambda[2] = a22;

    const double norm = sqrt((v00 * v00 + v10 * v10) + v20 * v20);
    double nx = v00 / norm, ny = v10 / norm, nz = v20 / norm;

    // canonical sign: the component of largest magnitude is positive, the lowest axis among equal magnitudes
    double pick = nx, mag = __builtin_fabs(nx);
    if (__builtin_fabs(ny) > mag) { pick = ny; mag = __builtin_fabs(ny); }
    if (__builtin_fabs(nz) > mag) pick = nz;
    bool flip = pick < 0.0;
    if (A.view) {
        const float *w = A.view + (long)b * A.vss;
        const float wx = w[0], wy = w[1], wz = w[2];
        const float inf = __builtin_inff();
        if (__builtin_fabsf(wx) < inf && __builtin_fabsf(wy) < inf && __builtin_fabsf(wz) < inf) {     // (NaN fails the comparison)
            const double ux = flip ? -nx : nx, uy = flip ? -ny : ny, uz = flip ? -nz : nz;
            const double t = (ux * ((double)wx - cx) + uy * ((double)wy - cy)) + uz * ((double)wz - cz);
            flip = flip != (t < 0.0);
        }
    }
    normal[0] = flip ? -nx : nx; normal[1] = flip ? -ny : ny; normal[2] = flip ? -nz : nz;
}

template <int KCAP>
int normals_launch(int B, const NormalsArgs &A, hipStream_t s) {
    return dispatch::chunk_grid(B, dispatch::ceil_div(A.n, NRM_THREADS), [&](int b0, unsigned nb, long k0, unsigned nk) {
        hipLaunchKernelGGL((normals_kernel<KCAP>), dim3(nk, nb), dim3(NRM_THREADS), 0, s, A, b0, k0);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" int dpf_normals(int B, int n, int m, const float *cloud, long cloud_stride, long point_stride, long axis_stride,
                           const int *index, int k, const float *viewpoint, long viewpoint_stride, double *normal, double *eigenvalues,
                           double *cov, int *flag, dpf_stream_t stream) {
    if (B < 0 || n < 1 || m < 1 || k < dispatch::NORMALS_MIN_K) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!cloud || !index || !normal || !eigenvalues || !flag) return DPF_EINVAL;
    const dispatch::NormalsForm f = dispatch::normals_form(k);
    if (f.kcap == 0) return DPF_ENOSUP;
    const NormalsArgs A{cloud, cloud_stride, point_stride, axis_stride, index, n, m, k, viewpoint, viewpoint_stride,
                        normal, eigenvalues, cov, flag};
    hipStream_t s = (hipStream_t)stream;
    switch (f.kcap) {
        case 4: return normals_launch<4>(B, A, s);
        case 8: return normals_launch<8>(B, A, s);
        case 16: return normals_launch<16>(B, A, s);
        default: return normals_launch<32>(B, A, s);
    }
}
