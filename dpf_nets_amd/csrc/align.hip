// Rigid alignment: the weighted Procrustes fit of given correspondences (dpf_rigid_fit) and trimmed point-to-point ICP (dpf_icp).
// The contract (the transform's rounding, the match, the trim, the eighteen sums and their order, Horn's closed form, the fixed sweeps,
// the statuses) is in include/dpf_hip.h; tests/align_ref.py restates it in numpy.
//
// Two kernels, launched in turn on the caller's stream, iters + 1 times each (once each for dpf_rigid_fit):
//   * align_match_kernel -- knn.hip's scan at k = 1 with the transform in front.  A workgroup of 4 waves holds 256 source points of
//     one slot, one per lane: the lane turns its point by the slot's current transform in float64, rounds once to fp32, and walks the
//     slot's target in tiles of 256 points, structure of arrays in LDS, four candidates per ds_read_b128, the next tile's global loads
//     in flight.  One running minimum under a strict d < best: candidates come in ascending index, so the lowest index wins among
//     equal distances.  It then reads the index it wrote an iteration ago, counts the changes, gathers its match and adds its eighteen
//     float64 terms into the workgroup's pairwise tree in LDS (stride 128, 64, ... 1 over the 256 lanes; lanes past n hold +0.0).
//     The 18 block sums and the two counts go to the workspace: no atomics, no workgroup waits on another.
//     With GIVEN the correspondences are the caller's (point i with point i, an optional weight): the same terms, the same tree.
//   * align_solve_kernel -- one wave per slot.  Lanes 0-17 each add one quantity's block partials in ascending block order, lanes 18
//     and 19 the inlier and changed counts; lane 0 gathers them by shuffles under compile-time indices and solves: Horn's 4 x 4
//     matrix, a fixed number of cyclic Jacobi sweeps with normals.hip's rotation, the column of the largest diagonal entry as a unit
//     quaternion.  The matrices are subscripted with compile-time indices only (unrolled pairs under a rolled sweep loop): they live
//     in registers, and the Makefile refuses a build of these kernels that uses scratch.
//
// Point-to-plane ICP (dpf_icp_plane; tests/align_plane_ref.py restates it) is the same pair under the same launch pattern:
//   * align_plane_match_kernel -- the body of align_match_kernel under another FORM: the scan, the tie rule, the trim, the changed
//     count and the refusal are one text.  The lane then gathers its match's normal and adds thirty-one float64 terms (W, the upper
//     triangle of sum a a^T for a = (y' x n ; n), sum a r, S_d, S_r, S_yy); the trees run in two batches of 16 over 32 KB of LDS.
//   * align_plane_solve_kernel -- one wave per slot, lanes 0-30 the sums, lanes 31 and 32 the counts; lane 0 solves the damped 6 x 6
//     normal equations by LDL^T without pivoting (a pivot that is not > 0 drops its unknown) and composes the increment, a unit
//     quaternion, onto the transform.  Only + - * / sqrt; compile-time indices only.
//
// The current transform lives in the outputs R, t, s (iteration 0 reads the caller's init, or the identity); a slot's two flags --
// done, refused -- in the workspace.  A done slot's later launches return on a block-uniform branch.  Iteration 0 takes "everything
// changed" and "not done" from the argument k == 0, never from memory: nothing is cleared before the first launch.
//
// Refusal is by slot, so every workgroup of a slot looks at all of the slot's coordinates (as knn.hip does).
// Bounded: the loops run over n / 256, m, the block count, the sweep count and the six pairs.
// Compiled with -ffp-contract=off: every float64 and fp32 operation rounds on its own, in the header's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_hip.h"
#include "dispatch.h"

namespace {

constexpr int AL_THREADS = dispatch::ALIGN_WG_POINTS;
constexpr int AL_TILE = dispatch::ALIGN_TILE;
constexpr int AL_Q = dispatch::ALIGN_SUMS;
constexpr int AL_SWEEPS = dispatch::ALIGN_SWEEPS;
constexpr int AL_GROUP = 4;                         // candidates per LDS read
constexpr int AL_T = 13;                            // doubles of a packed transform: R row-major, t, s
constexpr int AP_Q = dispatch::ALIGN_PLANE_SUMS;    // dpf_icp_plane: float64 quantities per slot
constexpr int AP_BATCH = 16;                        // of them a pass of the tree takes: two passes, 32 KB of LDS
constexpr int AP_MIN_INLIERS = dispatch::ALIGN_PLANE_MIN_INLIERS;
enum { AL_ICP = 0, AL_GIVEN = 1, AL_PLANE = 2 };    // what a match launch reduces: dpf_icp, dpf_rigid_fit, dpf_icp_plane

static_assert(AL_TILE == AL_THREADS && AL_TILE % AL_GROUP == 0, "one thread stages one candidate of a tile");
static_assert((AL_THREADS & (AL_THREADS - 1)) == 0 && AL_Q <= 18, "the tree halves the block; lanes 0-17 own the sums");
static_assert(AP_Q == 31 && AP_Q + 2 <= 64 && AP_BATCH <= AL_THREADS, "lanes 0-30 own the plane sums, lanes 31 and 32 the counts");

struct AlignArgs {
    const float *src;
    long ssc, ssp, ssa;                             // floats between clouds, points, axes
    const float *dst;
    long dsc, dsp, dsa;
    const float *weights;                           // GIVEN: (B, n) or NULL
    const double *init;                             // (B, 13) or NULL
    int n, m, iters, with_scale;
    float max_dist2;                                // the trim; <= 0, +inf or NaN: none
    double *R, *t, *s;                              // (B, 9), (B, 3), (B)
    int *index;                                     // (B, n)
    float *dist;                                    // (B, n)
    double *rmse;                                   // (B, iters + 1)
    int *inliers;                                   // (B, iters + 1) or NULL
    int *iterations;                                // (B) or NULL
    double *sums;                                   // (B, 18) or NULL
    int *status;                                    // (B)
    double *partial;                                // workspace: (B, nblk, 18)
    int *count;                                     //            (B, nblk, 2): inliers, changed
    int *state;                                     //            (B, 2): done, refused
    long nblk;
};

// dpf_icp_plane: the same, and (with_scale 0, weights NULL, s written as 1; partial is (B, nblk, 31))
struct PlaneArgs : AlignArgs {
    const double *normals;                          // (B, m, 3) dense
    double tol2;                                    // tol * tol
    double *rmse_plane, *step;                      // (B, iters + 1) each
    double *step2;                                  // workspace: (B): the squared step of the slot's last solve
};

// a coordinate, a transform entry or a weight the contract refuses: not finite, or larger in magnitude than 2^30 (NaN fails the comparison)
__device__ __forceinline__ unsigned al_out_of_range(float x) { return (unsigned)!(__builtin_fabsf(x) <= 0x1p30f); }
__device__ __forceinline__ unsigned al_out_of_range(double x) { return (unsigned)!(__builtin_fabs(x) <= 0x1p30); }

// the slot's current transform: the caller's init (the identity without one) in front of iteration 0, the outputs afterwards
__device__ __forceinline__ void al_transform(const AlignArgs &A, size_t b, int k, double (&T)[AL_T]) {
    if (k == 0) {
        const double *I = A.init ? A.init + b * AL_T : nullptr;
#pragma unroll
        for (int e = 0; e < AL_T; ++e) T[e] = I ? I[e] : (e == 0 || e == 4 || e == 8 || e == 12 ? 1.0 : 0.0);
    } else {
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = A.R[b * 9 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) T[9 + e] = A.t[b * 3 + e];
        T[12] = A.s[b];
    }
}

// upper triangle of a symmetric 6 x 6 matrix, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
__host__ __device__ constexpr int ap_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// The body of a match launch.  FORM picks what follows the scan; the scan itself -- the transform, the distance, the tie rule, the
// trim, the changed count, the refusal -- is one text for dpf_icp and dpf_icp_plane.
template <int FORM, class Args>
__device__ __forceinline__ void al_match_body(const Args &A, int k, int b0, long blk0) {
    constexpr bool GIVEN = FORM == AL_GIVEN, PLANE = FORM == AL_PLANE;
    __shared__ __attribute__((aligned(16))) float tx[AL_TILE], ty[AL_TILE], tz[AL_TILE];
    __shared__ double red[PLANE ? AP_BATCH : AL_Q][AL_THREADS];

    const int tid = threadIdx.x, n = A.n, m = A.m;
    const size_t b = (size_t)b0 + blockIdx.y;
    int *state = A.state + b * 2;
    if (k > 0 && state[0]) return;                                              // done: the same for every workgroup of the slot
    const long blk = blk0 + blockIdx.x, i = blk * AL_THREADS + tid;
    const float *P = A.src + (long)b * A.ssc, *C = A.dst + (long)b * A.dsc;
    const float inf = __builtin_inff();

    unsigned bad = 0;
    for (long u = tid; u < n; u += AL_THREADS) {                                // every source point of the slot: refusal is by slot
        const float *p = P + u * A.ssp;
        bad |= al_out_of_range(p[0]) | al_out_of_range(p[A.ssa]) | al_out_of_range(p[2 * A.ssa]);
        if (GIVEN) {
            const float *q = C + u * A.dsp;
            bad |= al_out_of_range(q[0]) | al_out_of_range(q[A.dsa]) | al_out_of_range(q[2 * A.dsa]);
            if (A.weights) {
                const float w = A.weights[b * (size_t)n + (size_t)u];
                bad |= al_out_of_range(w) | (unsigned)(w < 0.0f);
            }
        }
    }
    if constexpr (PLANE) {                                                      // every normal of the slot: finite and above 2^30 refuses,
        const double *N = A.normals + b * (size_t)m * 3;                        // not finite only takes its own match out
        for (long u = tid; u < 3L * m; u += AL_THREADS) {
            const double v = __builtin_fabs(N[u]);
            bad |= (unsigned)(v > 0x1p30 && v < __builtin_inf());
        }
    }
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (i < n) {
        const float *p = P + i * A.ssp;
        px = p[0]; py = p[A.ssa]; pz = p[2 * A.ssa];
    }

    int idx = -1;
    float d = inf;
    float yx = 0.0f, yy = 0.0f, yz = 0.0f;                                      // PLANE: the transformed point, kept for the terms
    if (!GIVEN) {
        double T[AL_T];
        al_transform(A, b, k, T);
        if (k == 0 && tid < AL_T) {                                             // (the solve's own results are finite by its status rules)
            double mine = T[0];
#pragma unroll
            for (int e = 1; e < AL_T; ++e) mine = tid == e ? T[e] : mine;
            bad |= al_out_of_range(mine);
        }
        if (PLANE && k == 0) bad |= (unsigned)!(T[12] == 1.0);                  // no scale is fitted: an init carries s = 1
        // y = fp32(s (R p) + t): float64, every operation rounded on its own, one rounding to fp32
        const double x = (double)px, y = (double)py, z = (double)pz;
        const float qx = (float)(((T[0] * x + T[1] * y) + T[2] * z) * T[12] + T[9]);
        const float qy = (float)(((T[3] * x + T[4] * y) + T[5] * z) * T[12] + T[10]);
        const float qz = (float)(((T[6] * x + T[7] * y) + T[8] * z) * T[12] + T[11]);
        const float lim = 0x1p61f;
        const bool usable = __builtin_fabsf(qx) <= lim && __builtin_fabsf(qy) <= lim && __builtin_fabsf(qz) <= lim;

        float best = inf;
        int bj = -1;
        float nx = inf, ny = inf, nz = inf;                                     // candidate base + tid of a tile, +inf where the target has ended
        auto fetch = [&](long base) {
            nx = ny = nz = inf;
            if (base + tid < m) {
                const float *p = C + (base + tid) * A.dsp;
                nx = p[0]; ny = p[A.dsa]; nz = p[2 * A.dsa];
            }
        };
        fetch(0);
        for (long base = 0; base < m; base += AL_TILE) {
            const int cnt = m - base < AL_TILE ? (int)(m - base) : AL_TILE;
            __syncthreads();                                                    // the tile before has been read by every wave
            tx[tid] = nx; ty[tid] = ny; tz[tid] = nz;
            if (tid < cnt) bad |= al_out_of_range(nx) | al_out_of_range(ny) | al_out_of_range(nz);
            __syncthreads();
            if (base + AL_TILE < m) fetch(base + AL_TILE);                      // in flight while this tile is searched
            for (int g = 0; g < cnt; g += AL_GROUP) {
                const float4 X = *(const float4 *)&tx[g], Y = *(const float4 *)&ty[g], Z = *(const float4 *)&tz[g];
                const float cx[AL_GROUP] = {X.x, X.y, X.z, X.w}, cy[AL_GROUP] = {Y.x, Y.y, Y.z, Y.w}, cz[AL_GROUP] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
                for (int u = 0; u < AL_GROUP; ++u) {
                    const float dx = cx[u] - qx, dy = cy[u] - qy, dz = cz[u] - qz;
                    const float du = (dx * dx + dy * dy) + dz * dz;
                    const bool take = du < best;                                // (the tile's padding: +inf, never below; a NaN neither)
                    best = take ? du : best;
                    bj = take ? (int)((unsigned)base + (unsigned)(g + u)) : bj;
                }
            }
        }
        if (usable && i < n) { idx = bj; d = best; }                            // (m >= 1 and every real distance is finite: bj >= 0)
        if (PLANE) { yx = qx; yy = qy; yz = qz; }
        const bool trim = A.max_dist2 > 0.0f && A.max_dist2 < inf;
        if (trim && d > A.max_dist2) idx = -1;
    }

    const int refused = __syncthreads_or((int)bad);                             // the same for every workgroup of the slot
    if (blk == 0 && tid == 0) state[1] = refused;
    if (refused) {
        if (!GIVEN && i < n) {
            A.index[b * (size_t)n + (size_t)i] = -1;
            A.dist[b * (size_t)n + (size_t)i] = __builtin_nanf("");
        }
        return;
    }

    // the pair of this lane: its weight, its match, and whether the match is another one than an iteration ago
    double w = 0.0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int changed = 0;
    if (GIVEN) {
        if (i < n) {
            const float *q = C + i * A.dsp;
            qx = q[0]; qy = q[A.dsa]; qz = q[2 * A.dsa];
            w = A.weights ? (double)A.weights[b * (size_t)n + (size_t)i] : 1.0;
        }
    } else if (i < n) {
        int *at = A.index + b * (size_t)n + (size_t)i;
        changed = k == 0 ? 1 : (int)(*at != idx);
        *at = idx;
        A.dist[b * (size_t)n + (size_t)i] = d;
        if (idx >= 0) {
            const float *q = C + (long)idx * A.dsp;
            qx = q[0]; qy = q[A.dsa]; qz = q[2 * A.dsa];
            w = 1.0;
        }
    }
    if constexpr (PLANE) {
        // the target normal of the match; one that is not finite takes the pair out (weight 0) and leaves the index in place
        double nv[3] = {0.0, 0.0, 0.0};
        if (w > 0.0) {
            const double *N = A.normals + (b * (size_t)m + (size_t)idx) * 3;
            nv[0] = N[0]; nv[1] = N[1]; nv[2] = N[2];
            const double inf64 = __builtin_inf();
            if (!(__builtin_fabs(nv[0]) < inf64 && __builtin_fabs(nv[1]) < inf64 && __builtin_fabs(nv[2]) < inf64)) w = 0.0;
        }
        const bool inlier = w > 0.0;
        // the thirty-one terms; +0.0 where there is no pair (and past n), and a zero term is +0.0 whatever the normal's sign
        double term[AP_Q];
#pragma unroll
        for (int q = 0; q < AP_Q; ++q) term[q] = 0.0;
        if (inlier) {
            const double y[3] = {(double)yx, (double)yy, (double)yz};
            const double yp[3] = {y[0] - (double)C[0], y[1] - (double)C[A.dsa], y[2] - (double)C[2 * A.dsa]};
            const double r = (nv[0] * (y[0] - (double)qx) + nv[1] * (y[1] - (double)qy)) + nv[2] * (y[2] - (double)qz);
            const double a[6] = {yp[1] * nv[2] - yp[2] * nv[1], yp[2] * nv[0] - yp[0] * nv[2], yp[0] * nv[1] - yp[1] * nv[0],
                                 nv[0], nv[1], nv[2]};
            term[0] = 1.0;
#pragma unroll
            for (int r0 = 0; r0 < 6; ++r0) {
#pragma unroll
                for (int c0 = r0; c0 < 6; ++c0) term[1 + ap_tri(r0, c0)] = a[r0] * a[c0] + 0.0;
                term[22 + r0] = a[r0] * r + 0.0;
            }
            term[28] = (double)d;
            term[29] = r * r;
            term[30] = (yp[0] * yp[0] + yp[1] * yp[1]) + yp[2] * yp[2];
        }
        const int n_in = __syncthreads_count((int)inlier);
        const int n_ch = __syncthreads_count(changed);
        const size_t slot_blk = b * (size_t)A.nblk + (size_t)blk;
#pragma unroll
        for (int h = 0; h < AP_Q; h += AP_BATCH) {                              // the pairwise tree, AP_BATCH quantities a pass
            if (h) __syncthreads();                                             // the pass before has been stored
#pragma unroll
            for (int q = 0; q < AP_BATCH; ++q)
                if (h + q < AP_Q) red[q][tid] = term[h + q];
            __syncthreads();
            for (int stride = AL_THREADS / 2; stride >= 1; stride >>= 1) {
                if (tid < stride) {
#pragma unroll
                    for (int q = 0; q < AP_BATCH; ++q)
                        if (h + q < AP_Q) red[q][tid] = red[q][tid] + red[q][tid + stride];
                }
                __syncthreads();
            }
            if (tid < AP_BATCH && h + tid < AP_Q) A.partial[slot_blk * AP_Q + h + tid] = red[tid][0];
        }
        if (tid == 0) { A.count[slot_blk * 2] = n_in; A.count[slot_blk * 2 + 1] = n_ch; }
        return;
    }
    const bool inlier = w > 0.0;

    // the eighteen terms over the pivoted points p' = p - a, q' = q - c; +0.0 where there is no pair (and past n)
    const double ax = (double)P[0], ay = (double)P[A.ssa], az = (double)P[2 * A.ssa];
    const double cx = (double)C[0], cy = (double)C[A.dsa], cz = (double)C[2 * A.dsa];
    double term[AL_Q];
#pragma unroll
    for (int q = 0; q < AL_Q; ++q) term[q] = 0.0;
    if (GIVEN ? i < n : inlier) {
        const double pp[3] = {(double)px - ax, (double)py - ay, (double)pz - az};
        const double qq[3] = {(double)qx - cx, (double)qy - cy, (double)qz - cz};
        term[0] = w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wp = w * pp[a];
            term[1 + a] = wp;
            term[4 + a] = w * qq[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) term[7 + 3 * a + c] = wp * qq[c];
        }
        term[16] = w * ((pp[0] * pp[0] + pp[1] * pp[1]) + pp[2] * pp[2]);
        term[17] = GIVEN ? w * ((qq[0] * qq[0] + qq[1] * qq[1]) + qq[2] * qq[2]) : w * (double)d;
    }
#pragma unroll
    for (int q = 0; q < AL_Q; ++q) red[q][tid] = term[q];
    const int n_in = __syncthreads_count((int)inlier);
    const int n_ch = __syncthreads_count(changed);
    for (int stride = AL_THREADS / 2; stride >= 1; stride >>= 1) {              // the pairwise tree, every quantity at once
        if (tid < stride) {
#pragma unroll
            for (int q = 0; q < AL_Q; ++q) red[q][tid] = red[q][tid] + red[q][tid + stride];
        }
        __syncthreads();
    }
    const size_t slot_blk = b * (size_t)A.nblk + (size_t)blk;
    if (tid < AL_Q) A.partial[slot_blk * AL_Q + tid] = red[tid][0];
    if (tid == 0) { A.count[slot_blk * 2] = n_in; A.count[slot_blk * 2 + 1] = n_ch; }
}

template <bool GIVEN>
__global__ __launch_bounds__(AL_THREADS) void align_match_kernel(AlignArgs A, int k, int b0, long blk0) {
    al_match_body<GIVEN ? AL_GIVEN : AL_ICP>(A, k, b0, blk0);
}

__global__ __launch_bounds__(AL_THREADS) void align_plane_match_kernel(PlaneArgs A, int k, int b0, long blk0) {
    al_match_body<AL_PLANE>(A, k, b0, blk0);
}

// One Jacobi rotation in the (P, Q) plane of the symmetric 4 x 4 matrix (both halves kept), normals.hip's formula; the columns P and Q
// of the accumulated rotations turn the same way
template <int P, int Q>
__device__ __forceinline__ void al_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);                              // (theta^2 = +inf: t = 0, the identity)
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + root);
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    a[P][P] = a[P][P] - h;
    a[Q][Q] = a[Q][Q] + h;
    a[P][Q] = a[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r != P && r != Q) {
            const double x = a[r][P], y = a[r][Q];
            a[r][P] = a[P][r] = c * x - s * y;
            a[r][Q] = a[Q][r] = s * x + c * y;
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double x = v[r][P], y = v[r][Q];
        v[r][P] = c * x - s * y;
        v[r][Q] = s * x + c * y;
    }
}

// the rotation of the unit quaternion (q0; q1, q2, q3) = (w; x, y, z), the header's formula
__device__ __forceinline__ void al_rotation(double q0, double q1, double q2, double q3, double (&R)[3][3]) {
    const double ww = q0 * q0, xx = q1 * q1, yy = q2 * q2, zz = q3 * q3;
    const double xy = q1 * q2, xz = q1 * q3, yz = q2 * q3, wx = q0 * q1, wy = q0 * q2, wz = q0 * q3;
    R[0][0] = ((ww + xx) - yy) - zz; R[0][1] = 2.0 * (xy - wz);         R[0][2] = 2.0 * (xz + wy);
    R[1][0] = 2.0 * (xy + wz);         R[1][1] = ((ww - xx) + yy) - zz; R[1][2] = 2.0 * (yz - wx);
    R[2][0] = 2.0 * (xz - wy);         R[2][1] = 2.0 * (yz + wx);         R[2][2] = ((ww - xx) - yy) + zz;
}

// The closed form on a slot's sums: false where the slot is degenerate (T is then left as it was).  a, c: the pivots.
// res: the weighted residual sum of the fit by its closed form, from S[17] = sum w |q'|^2 (dpf_rigid_fit's eighteenth quantity).
__device__ __forceinline__ bool al_solve(const double (&S)[AL_Q], int inliers, const double (&pa)[3], const double (&pc)[3], int with_scale,
                                         double (&T)[AL_T], double &res) {
    const double W = S[0];
    if (inliers < dispatch::ALIGN_MIN_INLIERS || !(W > 0.0)) return false;
    double M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[a][c] = S[7 + 3 * a + c] - (S[1 + a] * S[4 + c]) / W;
    const double v = S[16] - ((S[1] * S[1] + S[2] * S[2]) + S[3] * S[3]) / W;
    const double vq = S[17] - ((S[4] * S[4] + S[5] * S[5]) + S[6] * S[6]) / W;
    if (with_scale && !(v > 0.0)) return false;

    double N[4][4], V[4][4];
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    N[0][1] = N[1][0] = M[1][2] - M[2][1];
    N[0][2] = N[2][0] = M[2][0] - M[0][2];
    N[0][3] = N[3][0] = M[0][1] - M[1][0];
    N[1][2] = N[2][1] = M[0][1] + M[1][0];
    N[1][3] = N[3][1] = M[2][0] + M[0][2];
    N[2][3] = N[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < AL_SWEEPS; ++sweep) {
        al_rotate<0, 1>(N, V); al_rotate<0, 2>(N, V); al_rotate<0, 3>(N, V);
        al_rotate<1, 2>(N, V); al_rotate<1, 3>(N, V); al_rotate<2, 3>(N, V);
    }
    // the column of the largest diagonal entry, the lowest among equals
    double lam = N[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool take = N[c][c] > lam;
        lam = take ? N[c][c] : lam;
        q0 = take ? V[0][c] : q0; q1 = take ? V[1][c] : q1; q2 = take ? V[2][c] : q2; q3 = take ? V[3][c] : q3;
    }
    const double norm = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    q0 = q0 / norm; q1 = q1 / norm; q2 = q2 / norm; q3 = q3 / norm;
    // canonical sign: the component of largest magnitude is positive, the lowest among equal magnitudes
    double pick = q0, mag = __builtin_fabs(q0);
    if (__builtin_fabs(q1) > mag) { pick = q1; mag = __builtin_fabs(q1); }
    if (__builtin_fabs(q2) > mag) { pick = q2; mag = __builtin_fabs(q2); }
    if (__builtin_fabs(q3) > mag) pick = q3;
    if (pick < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }

    double R[3][3];
    al_rotation(q0, q1, q2, q3, R);

    // tr = sum_ab R_ab M_ba, row by row
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double row = (R[a][0] * M[0][a] + R[a][1] * M[1][a]) + R[a][2] * M[2][a];
        tr = a == 0 ? row : tr + row;
    }
    const double s = with_scale ? tr / v : 1.0;
    double tt[3];
    const double gp[3] = {pa[0] + S[1] / W, pa[1] + S[2] / W, pa[2] + S[3] / W};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double rp = (R[a][0] * gp[0] + R[a][1] * gp[1]) + R[a][2] * gp[2];
        tt[a] = (pc[a] + S[4 + a] / W) - s * rp;
    }
    bool finite = __builtin_fabs(s) < __builtin_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        finite = finite && __builtin_fabs(tt[a]) < __builtin_inf();
#pragma unroll
        for (int c = 0; c < 3; ++c) finite = finite && __builtin_fabs(R[a][c]) < __builtin_inf();
    }
    if (!finite) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * a + c] = R[a][c];
        T[9 + a] = tt[a];
    }
    T[12] = s;
    const double e = ((s * s) * v + vq) - (2.0 * s) * tr;
    res = e > 0.0 ? e : 0.0;
    return true;
}

// k: the iteration whose match is reduced; LAST: no solve follows (the match under the returned transform); FIT: dpf_rigid_fit
template <bool FIT>
__global__ __launch_bounds__(64) void align_solve_kernel(AlignArgs A, int k, int last, int b0) {
    const int lane = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    int *state = A.state + b * 2;
    const size_t K1 = (size_t)A.iters + 1;
    if (k > 0 && state[0]) {                                                    // done: the entries of this match repeat the last ones
        if (lane == 0) {
            A.rmse[b * K1 + k] = A.rmse[b * K1 + k - 1];
            if (A.inliers) A.inliers[b * K1 + k] = A.inliers[b * K1 + k - 1];
        }
        return;
    }
    const int refused = state[1];
    double acc = 0.0;
    int cnt = 0;
    if (!refused) {
        const double *part = A.partial + b * (size_t)A.nblk * AL_Q;
        const int *count = A.count + b * (size_t)A.nblk * 2;
        if (lane < AL_Q) {
            acc = part[lane];
            for (long blk = 1; blk < A.nblk; ++blk) acc = acc + part[blk * AL_Q + lane];     // ascending block order
        } else if (lane < AL_Q + 2) {
            for (long blk = 0; blk < A.nblk; ++blk) cnt += count[blk * 2 + (lane - AL_Q)];
        }
    }
    const double nan = __builtin_nan("");
    if (A.sums && lane < AL_Q) A.sums[b * AL_Q + lane] = refused ? nan : acc;
    double S[AL_Q];
#pragma unroll
    for (int q = 0; q < AL_Q; ++q) S[q] = __shfl(acc, q);
    const int n_in = __shfl(cnt, AL_Q), n_ch = __shfl(cnt, AL_Q + 1);
    if (lane != 0) return;

    double *R = A.R + b * 9, *t = A.t + b * 3;
    if (refused) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = nan;
        t[0] = t[1] = t[2] = nan;
        A.s[b] = nan;
        A.rmse[b * K1 + k] = nan;
        if (A.inliers) A.inliers[b * K1 + k] = 0;
        if (A.iterations) A.iterations[b] = 0;
        A.status[b] = DPF_ALIGN_REFUSED;
        state[0] = 1;
        return;
    }
    double T[AL_T];
    al_transform(A, b, FIT ? 0 : k, T);
    if (!FIT) A.rmse[b * K1 + k] = sqrt(S[AL_Q - 1] / S[0]);
    if (A.inliers) A.inliers[b * K1 + k] = n_in;

    int done = 0, status = 0;
    bool solved = false;
    if (!FIT && k > 0 && n_ch == 0) done = 1;                                   // a fixed point: the next solve would return these bits
    else if (last) done = 1;
    else {
        const float *P = A.src + (long)b * A.ssc, *C = A.dst + (long)b * A.dsc;
        const double pa[3] = {(double)P[0], (double)P[A.ssa], (double)P[2 * A.ssa]};
        const double pc[3] = {(double)C[0], (double)C[A.dsa], (double)C[2 * A.dsa]};
        double res = 0.0;
        solved = al_solve(S, n_in, pa, pc, A.with_scale, T, res);
        if (!solved) { done = 1; status = DPF_ALIGN_DEGENERATE; }
        if (FIT) A.rmse[b] = solved ? sqrt(res / S[0]) : nan;
    }
    if (k == 0 || solved) {                                                     // (a slot that keeps its transform past iteration 0 has it in place)
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = T[e];
        t[0] = T[9]; t[1] = T[10]; t[2] = T[11];
        A.s[b] = T[12];
    }
    if (k == 0 || status) A.status[b] = status;
    if (A.iterations && done) A.iterations[b] = k;                              // solves that gave the transform
    state[0] = done;
}

// One Gauss-Newton step of point-to-plane on a slot's thirty-one sums: false where the slot is degenerate (T is then left as it was).
// The damped normal equations A x = -b by LDL^T without pivoting, a pivot that is not > 0 dropping its unknown; the increment as a
// unit quaternion, composed onto T about the pivot pc.  Every operation is one of + - * / sqrt, in the header's order; the matrices
// are subscripted with compile-time indices only.
__device__ __forceinline__ bool ap_solve(const double (&S)[AP_Q], int inliers, const double (&pc)[3], double (&T)[AL_T], double &step2) {
    const double W = S[0];
    if (inliers < AP_MIN_INLIERS || !(W > 0.0)) return false;
    const double damp = 1.0 + 0x1p-40;
    double D[6], L[6][6], x[6];
    bool ok[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = S[1 + ap_tri(j, j)] * damp;
#pragma unroll
        for (int c = 0; c < j; ++c) d = d - (L[j][c] * L[j][c]) * D[c];
        ok[j] = d > 0.0;
        D[j] = ok[j] ? d : 0.0;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = S[1 + ap_tri(j, i)];
#pragma unroll
            for (int c = 0; c < j; ++c) e = e - (L[i][c] * L[j][c]) * D[c];
            L[i][j] = ok[j] ? e / d : 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                               // L y = -b
        double y = -S[22 + i];
#pragma unroll
        for (int c = 0; c < i; ++c) y = y - L[i][c] * x[c];
        x[i] = ok[i] ? y : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = ok[i] ? x[i] / D[i] : 0.0;               // D z = y
#pragma unroll
    for (int i = 5; i >= 0; --i) {                                              // L^T x = z
        double v = x[i];
#pragma unroll
        for (int c = i + 1; c < 6; ++c) v = v - L[c][i] * x[c];
        x[i] = ok[i] ? v : 0.0;
    }
    // the increment: the unit quaternion (1; omega / 2) / norm
    const double h0 = 0.5 * x[0], h1 = 0.5 * x[1], h2 = 0.5 * x[2];
    const double norm = sqrt(((1.0 + h0 * h0) + h1 * h1) + h2 * h2);
    double dR[3][3], R[3][3], tt[3];
    al_rotation(1.0 / norm, h0 / norm, h1 / norm, h2 / norm, dR);
    const double u[3] = {T[9] - pc[0], T[10] - pc[1], T[11] - pc[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[a][c] = (dR[a][0] * T[c] + dR[a][1] * T[3 + c]) + dR[a][2] * T[6 + c];
        tt[a] = (((dR[a][0] * u[0] + dR[a][1] * u[1]) + dR[a][2] * u[2]) + pc[a]) + x[3 + a];
    }
    const double s2 = ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + ((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) / (S[30] / W);
    bool finite = __builtin_fabs(s2) < __builtin_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        finite = finite && __builtin_fabs(tt[a]) < __builtin_inf();
#pragma unroll
        for (int c = 0; c < 3; ++c) finite = finite && __builtin_fabs(R[a][c]) < __builtin_inf();
    }
    if (!finite) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * a + c] = R[a][c];
        T[9 + a] = tt[a];
    }
    step2 = s2;
    return true;
}

// k: the iteration whose match is reduced; last: no solve follows (the match under the returned transform)
__global__ __launch_bounds__(64) void align_plane_solve_kernel(PlaneArgs A, int k, int last, int b0) {
    const int lane = threadIdx.x;
    const size_t b = (size_t)b0 + blockIdx.y;
    int *state = A.state + b * 2;
    const size_t K1 = (size_t)A.iters + 1, at = b * K1 + k;
    if (k > 0 && state[0]) {                                                    // done: the entries of this match repeat the last ones
        if (lane == 0) {
            A.rmse[at] = A.rmse[at - 1];
            A.rmse_plane[at] = A.rmse_plane[at - 1];
            A.step[at] = A.step[at - 1];
            A.inliers[at] = A.inliers[at - 1];
        }
        return;
    }
    const int refused = state[1];
    double acc = 0.0;
    int cnt = 0;
    if (!refused) {
        const double *part = A.partial + b * (size_t)A.nblk * AP_Q;
        const int *count = A.count + b * (size_t)A.nblk * 2;
        if (lane < AP_Q) {
            acc = part[lane];
            for (long blk = 1; blk < A.nblk; ++blk) acc = acc + part[blk * AP_Q + lane];     // ascending block order
        } else if (lane < AP_Q + 2) {
            for (long blk = 0; blk < A.nblk; ++blk) cnt += count[blk * 2 + (lane - AP_Q)];
        }
    }
    const double nan = __builtin_nan("");
    if (A.sums && lane < AP_Q) A.sums[b * AP_Q + lane] = refused ? nan : acc;
    double S[AP_Q];
#pragma unroll
    for (int q = 0; q < AP_Q; ++q) S[q] = __shfl(acc, q);
    const int n_in = __shfl(cnt, AP_Q), n_ch = __shfl(cnt, AP_Q + 1);
    if (lane != 0) return;

    double *R = A.R + b * 9, *t = A.t + b * 3;
    if (refused) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = nan;
        t[0] = t[1] = t[2] = nan;
        A.s[b] = nan;
        A.rmse[at] = nan;
        A.rmse_plane[at] = nan;
        A.step[at] = nan;
        A.inliers[at] = 0;
        A.iterations[b] = 0;
        A.status[b] = DPF_ALIGN_REFUSED;
        state[0] = 1;
        return;
    }
    double T[AL_T];
    al_transform(A, b, k, T);
    A.rmse[at] = sqrt(S[28] / S[0]);
    A.rmse_plane[at] = sqrt(S[29] / S[0]);
    A.inliers[at] = n_in;

    int done = 0, status = 0;
    bool solved = false;
    double step2 = 0.0;
    if (k > 0 && n_ch == 0 && A.step2[b] <= A.tol2) done = 1;                   // the matches stand and the step that led here was small
    else if (last) done = 1;
    else {
        const float *C = A.dst + (long)b * A.dsc;
        const double pc[3] = {(double)C[0], (double)C[A.dsa], (double)C[2 * A.dsa]};
        solved = ap_solve(S, n_in, pc, T, step2);
        if (!solved) { done = 1; status = DPF_ALIGN_DEGENERATE; }
    }
    A.step[at] = solved ? sqrt(step2) : 0.0;                                    // the step taken from this match: none where no solve follows
    if (solved) A.step2[b] = step2;
    if (k == 0 || solved) {                                                     // (a slot that keeps its transform past iteration 0 has it in place)
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = T[e];
        t[0] = T[9]; t[1] = T[10]; t[2] = T[11];
        A.s[b] = 1.0;
    }
    if (k == 0 || status) A.status[b] = status;
    if (done) A.iterations[b] = k;                                              // solves that gave the transform
    state[0] = done;
}

size_t al_partial_bytes(int B, long nblk) { return (size_t)B * (size_t)nblk * AL_Q * sizeof(double); }
size_t al_count_bytes(int B, long nblk) { return (size_t)B * (size_t)nblk * 2 * sizeof(int); }

void al_carve(AlignArgs &A, int B, void *workspace) {
    char *w = (char *)workspace;
    A.partial = (double *)w;
    A.count = (int *)(w + al_partial_bytes(B, A.nblk));
    A.state = (int *)(w + al_partial_bytes(B, A.nblk) + al_count_bytes(B, A.nblk));
}

template <bool GIVEN>
int al_round(int B, const AlignArgs &A, int k, int last, hipStream_t s) {
    if (const int e = dispatch::chunk_grid(B, A.nblk, [&](int b0, unsigned nb, long k0, unsigned nk) {
            hipLaunchKernelGGL((align_match_kernel<GIVEN>), dim3(nk, nb), dim3(AL_THREADS), 0, s, A, k, b0, k0);
            return (int)hipGetLastError();
        }))
        return e;
    return dispatch::chunk_grid(B, 1, [&](int b0, unsigned nb, long, unsigned) {
        hipLaunchKernelGGL((align_solve_kernel<GIVEN>), dim3(1, nb), dim3(64), 0, s, A, k, last, b0);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" size_t dpf_align_workspace_bytes(int B, int n) {
    if (B < 1 || n < 1) return 0;
    const long nblk = dispatch::align_form(n, 0).blocks;
    return al_partial_bytes(B, nblk) + al_count_bytes(B, nblk) + (size_t)B * 2 * sizeof(int);
}

extern "C" int dpf_rigid_fit(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride,
                             const float *dst, long d_cloud_stride, long d_point_stride, long d_axis_stride, const float *weights,
                             int with_scale, double *R, double *t, double *s, double *rmse, double *sums, int *status,
                             void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || n < 1) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!src || !dst || !R || !t || !s || !rmse || !status || !workspace || ((uintptr_t)workspace & 7)) return DPF_EINVAL;
    if (workspace_bytes < dpf_align_workspace_bytes(B, n)) return DPF_EINVAL;
    AlignArgs A{src, s_cloud_stride, s_point_stride, s_axis_stride, dst, d_cloud_stride, d_point_stride, d_axis_stride, weights, nullptr,
                n, n, 0, with_scale ? 1 : 0, 0.0f, R, t, s, nullptr, nullptr, rmse, nullptr, nullptr, sums, status,
                nullptr, nullptr, nullptr, dispatch::align_form(n, 0).blocks};
    al_carve(A, B, workspace);
    return al_round<true>(B, A, 0, 0, (hipStream_t)stream);
}

extern "C" int dpf_icp(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride, int m,
                       const float *dst, long d_cloud_stride, long d_point_stride, long d_axis_stride, int iters, float max_dist2,
                       int with_scale, const double *init, double *R, double *t, double *s, int *index, float *dist, double *rmse,
                       int *inliers, int *iterations, double *sums, int *status, void *workspace, size_t workspace_bytes,
                       dpf_stream_t stream) {
    if (B < 0 || n < 1 || m < 1 || iters < 0) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!src || !dst || !R || !t || !s || !index || !dist || !rmse || !inliers || !iterations || !status || !workspace ||
        ((uintptr_t)workspace & 7))
        return DPF_EINVAL;
    if (workspace_bytes < dpf_align_workspace_bytes(B, n)) return DPF_EINVAL;
    AlignArgs A{src, s_cloud_stride, s_point_stride, s_axis_stride, dst, d_cloud_stride, d_point_stride, d_axis_stride, nullptr, init,
                n, m, iters, with_scale ? 1 : 0, max_dist2, R, t, s, index, dist, rmse, inliers, iterations, sums, status,
                nullptr, nullptr, nullptr, dispatch::align_form(n, iters).blocks};
    al_carve(A, B, workspace);
    for (int k = 0; k <= iters; ++k)
        if (const int e = al_round<false>(B, A, k, k == iters, (hipStream_t)stream)) return e;
    return 0;
}

extern "C" size_t dpf_icp_plane_workspace_bytes(int B, int n) {
    if (B < 1 || n < 1) return 0;
    const long nblk = dispatch::align_plane_form(n, 0).blocks;
    return (size_t)B * (size_t)nblk * AP_Q * sizeof(double) + (size_t)B * sizeof(double) + al_count_bytes(B, nblk) +
           (size_t)B * 2 * sizeof(int);
}

extern "C" int dpf_icp_plane(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride, int m,
                             const float *dst, long d_cloud_stride, long d_point_stride, long d_axis_stride, const double *normals,
                             int iters, float max_dist2, double tol, const double *init, double *R, double *t, double *s, int *index,
                             float *dist, double *rmse, double *rmse_plane, double *step, int *inliers, int *iterations, double *sums,
                             int *status, void *workspace, size_t workspace_bytes, dpf_stream_t stream) {
    if (B < 0 || n < 1 || m < 1 || iters < 0 || !(tol >= 0.0)) return DPF_EINVAL;
    if (B == 0) return 0;
    if (!src || !dst || !normals || !R || !t || !s || !index || !dist || !rmse || !rmse_plane || !step || !inliers || !iterations ||
        !status || !workspace || ((uintptr_t)workspace & 7))
        return DPF_EINVAL;
    if (workspace_bytes < dpf_icp_plane_workspace_bytes(B, n)) return DPF_EINVAL;
    PlaneArgs A{};
    static_cast<AlignArgs &>(A) = AlignArgs{src, s_cloud_stride, s_point_stride, s_axis_stride, dst, d_cloud_stride, d_point_stride,
                                            d_axis_stride, nullptr, init, n, m, iters, 0, max_dist2, R, t, s, index, dist, rmse, inliers,
                                            iterations, sums, status, nullptr, nullptr, nullptr,
                                            dispatch::align_plane_form(n, iters).blocks};
    A.normals = normals;
    A.tol2 = tol * tol;
    A.rmse_plane = rmse_plane;
    A.step = step;
    char *w = (char *)workspace;
    const size_t pbytes = (size_t)B * (size_t)A.nblk * AP_Q * sizeof(double);
    A.partial = (double *)w;
    A.step2 = (double *)(w + pbytes);
    A.count = (int *)(w + pbytes + (size_t)B * sizeof(double));
    A.state = (int *)(w + pbytes + (size_t)B * sizeof(double) + al_count_bytes(B, A.nblk));
    const hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k <= iters; ++k) {
        if (const int e = dispatch::chunk_grid(B, A.nblk, [&](int b0, unsigned nb, long k0, unsigned nk) {
                hipLaunchKernelGGL(align_plane_match_kernel, dim3(nk, nb), dim3(AL_THREADS), 0, st, A, k, b0, k0);
                return (int)hipGetLastError();
            }))
            return e;
        if (const int e = dispatch::chunk_grid(B, 1, [&](int b0, unsigned nb, long, unsigned) {
                hipLaunchKernelGGL(align_plane_solve_kernel, dim3(1, nb), dim3(64), 0, st, A, k, k == iters ? 1 : 0, b0);
                return (int)hipGetLastError();
            }))
            return e;
    }
    return 0;
}
