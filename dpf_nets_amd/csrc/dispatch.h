// dispatch.h -- which kernel form serves a call, decided in ONE place: pure functions of (shape, switches) beside the
// measurements their thresholds come from.  Host-only, plain C++17, no HIP header: tests/test_dispatch_cpu.py compiles it with
// the host compiler alone and asserts the form of every threshold.  The launchers are a `switch` over what these return.
#ifndef DPF_DISPATCH_H
#define DPF_DISPATCH_H

#include <atomic>
#include <cstdlib>

#include "dpf_hip.h"

namespace dispatch {

// ---- the switches -------------------------------------------------------------------------------------------------------
// Every environment switch a launch path reads (the table of names, values and defaults), as the value "not set" has.
// The four with a setter (flow_tile16, nn_small, cg_lds, emd_matrix_set) hold the process default of the moment in a snapshot().
struct Switches {
    int flow_tile16 = -1;         // DPF_FLOW_TILE16   -1: by size; 0: never the 16-point kernel; 1: whenever the precision allows
    int flow16_cw = 0;            // DPF_FLOW16_CW     0: by size; compute waves per 16-point workgroup (>= 4: 4, else 2)
    int flow16_split = -1;        // DPF_FLOW16_SPLIT  -1: by size; 0 / 1 forces the two-waves-per-tile kernel off / on
    int flow_waves = 0;           // DPF_FLOW_WAVES    0: by size; waves per 32-point workgroup (8 | 4 | 2 | 1)
    int flow_lpb = 0;             // DPF_FLOW_LPB      0: by size; 1 / 2 forces one / two layers per LDS buffer
    int flow_skew = 1;            // DPF_FLOW_SKEW     0: the 8-wave two-part kernel without its skewed form
    int nn_small = -1;            // DPF_NN_SMALL      -1: by size; 0: never the LDS-staged scan; 1: whenever the clouds fit
    int nn_ksw = 0;               // DPF_NN_KSW        0: by size; waves of a staged-scan workgroup (4 | 8, anything else 16)
    int nn_ks = 0;                // DPF_NN_KS         0: by size; 8 | 16: the sliced scan (and never the staged one)
    int nnm_qw = 0;               // DPF_NNM_QW        0: by size; waves of a matrix-core filter workgroup (4 | 8 | 16)
    int cg_lds = -1;              // DPF_CG_LDS        -1: by size; 0: the deterministic Chamfer backward never sorts in LDS alone
    int emd_matrix_env = 1;       // DPF_EMD_MATRIX    0 only when its first character is '0': never the matrix-core family
    int emd_matrix_set = 1;       //                   dpf_emd_set_matrix_path's value (ANDed with the environment's)
    int train_split = -1;         // DPF_TRAIN_SPLIT   -1: by size; 0 / 1 forces the two-workgroups-per-branch forms
    int train_roles = -1;         // DPF_TRAIN_ROLES   -1: by size; 0 / 1 forces pass 2's role workgroups
    int train_fuse_colsum = 1;    // DPF_TRAIN_FUSE_COLSUM  0: the column sums keep a launch of their own
};

inline const Switches &env_switches() {            // filled once per process
    static const Switches sw = [] {
        auto env = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        Switches s;
        s.flow_tile16 = env("DPF_FLOW_TILE16", -1); s.flow16_cw = env("DPF_FLOW16_CW", 0); s.flow16_split = env("DPF_FLOW16_SPLIT", -1);
        s.flow_waves = env("DPF_FLOW_WAVES", 0); s.flow_lpb = env("DPF_FLOW_LPB", 0); s.flow_skew = env("DPF_FLOW_SKEW", 1);
        s.nn_small = env("DPF_NN_SMALL", -1); s.nn_ksw = env("DPF_NN_KSW", 0); s.nn_ks = env("DPF_NN_KS", 0); s.nnm_qw = env("DPF_NNM_QW", 0);
        s.cg_lds = env("DPF_CG_LDS", -1);
        const char *e = getenv("DPF_EMD_MATRIX");
        s.emd_matrix_env = !(e && e[0] == '0');
        s.train_split = env("DPF_TRAIN_SPLIT", -1); s.train_roles = env("DPF_TRAIN_ROLES", -1);
        s.train_fuse_colsum = env("DPF_TRAIN_FUSE_COLSUM", 1);
        return s;
    }();
    return sw;
}

// The process defaults that have a setter (dpf_flow_set_tile16, dpf_nn_small_mode, dpf_chamfer_grad_lds_mode, dpf_emd_set_matrix_path), seeded from the
// environment, and the 16-point kernel's launch counter.  An entry reads them once, at its top: snapshot().
struct Settable {
    std::atomic<int> flow_tile16{env_switches().flow_tile16}, nn_small{env_switches().nn_small}, emd_matrix{1};
    std::atomic<int> cg_lds{env_switches().cg_lds};
    std::atomic<long> tile16_launches{0};
};
inline Settable &settable() { static Settable s; return s; }
inline int set_mode(std::atomic<int> &v, int mode) { return v.exchange(mode < 0 ? -1 : (mode ? 1 : 0)); }     // the old mode
inline Switches snapshot() {
    Switches sw = env_switches();
    Settable &s = settable();
    sw.flow_tile16 = s.flow_tile16.load(std::memory_order_relaxed);
    sw.nn_small = s.nn_small.load(std::memory_order_relaxed);
    sw.emd_matrix_set = s.emd_matrix.load(std::memory_order_relaxed);
    sw.cg_lds = s.cg_lds.load(std::memory_order_relaxed);
    return sw;
}

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// ---- launches cut to the grid's limits (mesh_sample.hip, point_mesh.hip, mesh_point.hip) -----------------------------------------
constexpr long MAX_BLOCKS = 1L << 22;   // workgroups of one launch along x
constexpr int MAX_SLOTS = 32768;        // batch slots of one launch (grid.y)
// [0, total) in order, in pieces of at most `per`: launch(first, count) launches one and returns its error; the first non-zero
// return ends the loop and is returned
template <class Launch>
inline int chunk_range(long total, long per, Launch &&launch) {
    for (long i0 = 0; i0 < total; i0 += per)
        if (const int e = launch(i0, total - i0 < per ? total - i0 : per)) return e;
    return 0;
}
// the same over slots x blocks, the blocks of a piece of slots before the next slots: launch(b0, nb, k0, nk)
template <class Launch>
inline int chunk_grid(int slots, long blocks, Launch &&launch, int max_slots = MAX_SLOTS, long max_blocks = MAX_BLOCKS) {
    return chunk_range(slots, max_slots, [&](long b0, long nb) {
        return chunk_range(blocks, max_blocks, [&](long k0, long nk) { return launch((int)b0, (unsigned)nb, k0, (unsigned)nk); });
    });
}

// ---- the eval flow stack (flow.hip, flow16.hip) ---------------------------------------------------------------------------
enum class FlowKernel { Tile16Split, Tile16, Tile32 };
// cw: compute waves of a 16-point workgroup (4 | 2); fw: waves of a 32-point workgroup (8 | 4 | 2 | 1); lpb: layers per LDS
// buffer (0: the skewed form, 1, 2); xs_rows: the moment epilogue's partial rows per cloud, one per workgroup
struct FlowForm { FlowKernel kernel; int cw, fw, lpb, xs_rows; };
inline FlowForm flow_form(int L, int B, int N, int precision, bool has_xs, bool packed16_ok, const Switches &sw) {
    FlowForm f{FlowKernel::Tile32, 0, 0, 1, 0};
    // 16-point tiles pay while they leave SIMDs a single wave: up to 1024 tiles (one per SIMD of the 256 CUs); f16x3 only; the
    // training forward's moment epilogue lives in the 32-point kernel
    const long tiles16 = B * ceil_div(N, 16);
    if (packed16_ok && precision == DPF_PREC_F16X3 && !has_xs && sw.flow_tile16 != 0 && L <= 128 && B <= 65535 &&
        (sw.flow_tile16 == 1 || tiles16 <= 1024)) {
        // at most half a tile per SIMD: split every tile's two branches over two waves
        const bool split = sw.flow16_split >= 0 ? sw.flow16_split != 0 : tiles16 <= 512;
        f.kernel = split ? FlowKernel::Tile16Split : FlowKernel::Tile16;
        // compute waves per workgroup (the loaders share their SIMDs): 4 = one per SIMD; 2 when that is what gives every CU a
        // workgroup (8 + 4 waves would have to live in 168 registers each: the kernel spills there, so it is not built)
        const int cw = sw.flow16_cw ? sw.flow16_cw : (B * ceil_div(N, 64) < 160 ? 2 : 4);
        f.cw = split || cw >= 4 ? 4 : 2;
        return f;
    }
    // waves (32-point tiles) per workgroup: as many as possible (each workgroup streams the layer
    // weights through its own LDS) while the launch still has a workgroup for every CU
    // (measured r01: below 4 waves the LDS-DMA fill of a layer, ~1.5 us for 38 KB on one CU, is no
    // longer hidden, so 2- and 1-wave workgroups are only for clouds of <= 64 / <= 32 points)
    int fw = sw.flow_waves;
    if (!fw) {
        fw = 8;                                       // 8-wave workgroups (256 points of one cloud) unless that leaves CUs without one
        if (B * ceil_div(N, 256) < 224) fw = 4;
        if (N <= 64) fw = 2;
        if (N <= 32) fw = 1;
    }
    f.fw = fw >= 8 ? 8 : fw >= 4 ? 4 : fw >= 2 ? 2 : 1;
    f.xs_rows = (int)ceil_div(N, 32 * f.fw);
    // two layers per LDS buffer where a CU gets one workgroup anyway and the 2 x 2 layers fit its LDS (two-part precisions)
    const bool two_part = precision != DPF_PREC_BF16X6;
    const bool pair_ok = two_part && L >= 2 && sw.flow_lpb != 1 && (sw.flow_lpb == 2 || B * ceil_div(N, 256) <= 256);
    if (f.fw == 8) f.lpb = sw.flow_skew && two_part ? 0 : pair_ok ? 2 : 1;
    return f;
}

// ---- Chamfer (chamfer.hip, chamfer_mfma.hip) --------------------------------------------------------------------------------
constexpr int NN_QPW = 128;      // the scan's query points per wave
constexpr int NNM_CT = 64;       // the matrix-core filter's candidate tiles resident in LDS at a time

// rank-sized batches of mid-sized clouds: the LDS-staged kernel.  One workgroup per CU or fewer (B = 4 clouds of 2048 points:
// 10.4 us against the scalar-load scan's 14.9); with more the CUs that hold two workgroups set the pace and the scan that
// streams its candidates through SGPRs is as fast (B = 8: 16.0 vs 15.9 us; r04_small/sweep.txt).
inline bool nn_small_serves(int b, int n, int m, const Switches &sw) {
    const int nmax = n > m ? n : m, minc = n < m ? n : m;
    if (sw.nn_small == 0 || nmax > 8192 || b > 65535) return false;
    if (sw.nn_small == 1) return true;
    return minc >= 1024 && ceil_div(nmax, 64) * b * 2 <= 256;
}
// its candidate slices per workgroup: enough waves for two per SIMD (a lone wave is bound by its own issue rate)
inline int nn_small_ksw(int b, int nmax, const Switches &sw) {
    const int ksw = sw.nn_ksw ? sw.nn_ksw : (ceil_div(nmax, 64) * b * 2 * 4 >= 2048 ? 4 : 8);
    return ksw == 4 || ksw == 8 ? ksw : 16;
}
// Staged: nn_small_kernel<width>; Sliced: nn_kernel<width, width>, width = 8 | 16 candidate slices; Scan: nn_kernel<width>,
// width = 1 | 2 | 4 candidate slices over the 4 waves
enum class NNKernel { Staged, Sliced, Scan };
struct NNForm { NNKernel kernel; int width; };
inline NNForm nn_form(int b, int n, int m, const Switches &sw) {
    const int nmax = n > m ? n : m, minc = n < m ? n : m;
    if (nn_small_serves(b, n, m, sw) && !sw.nn_ks) return {NNKernel::Staged, nn_small_ksw(b, nmax, sw)};
    // pick the candidate split so that the launch has >= ~2 waves per SIMD on 256 CUs
    const long waves1 = b * (ceil_div(n, NN_QPW) + ceil_div(m, NN_QPW));
    // Small problems (a rank's 4-8 clouds of 2048 points): with one wave per SIMD the scan is bound by the LATENCY of its
    // scalar loads (one chunk of prefetch covers ~300 cycles of VALU work, an L2-served s_load takes longer), so the
    // candidates are split over MORE waves -- 8 or 16 slices merged in LDS in ascending order -- until every SIMD has two
    int ks = sw.nn_ks;
    if (!ks && waves1 < 512 && minc >= 1024) ks = 8;    // r04, B=4 N=2048: 4 slices 18.4 us, 8: 15.3, 16: 16.8
    if (ks == 16 || ks == 8) return {NNKernel::Sliced, ks};
    return {NNKernel::Scan, waves1 >= 2048 || (n < 64 && m < 64) ? 1 : waves1 >= 1024 ? 2 : 4};
}

inline long nnm_workgroups(int b, int n, int m, int qw) { return b * (ceil_div(n, qw * 32) + ceil_div(m, qw * 32)); }
// The matrix-core filter pays with
// enough pairs to amortise building the fragments and enough workgroups to fill the chip (r01, tools/nn_impl_sweep.py:
// 25 vs 52 us at B=32, n=m=2048; 76 vs 190 us at B=8, n=m=8192; 50 vs 64 us at B=2, n=m=8192); small clouds and small
// batches are launch-bound either way and few workgroups leave the matrix cores idle
// r04, after the filter's bookkeeping was rebuilt (see nnm_kernel): it also wins for mid-sized batches of clouds whose
// fragments fit one pass -- B = 6 / 8 / 10 clouds of 2048: 13.4 / 12.0 / 12.1 us against the scans' 15.2 / 15.3 / 24.4; 16 clouds
// of 1024: 8.2 vs 10.0 -- but not where the LDS-staged scan serves (one workgroup per CU or fewer: B = 4: 10.4 vs 13.3) and not
// for clouds a little over one pass (B = 4, N = 2500: 22.8 vs 17.3).
inline bool nnm_pays(int b, int n, int m, const Switches &sw) {
    if (b <= 0 || n <= 0 || m <= 0 || b > 65535 || n > 65535 * 32 || m > 65535 * 32) return false;
    if (nnm_workgroups(b, n, m, 8) < 64) return false;                // B=1, n=m=8192: 48 vs 57 us
    const double pairs = 2.0 * (double)b * (double)n * (double)m;
    if (pairs >= 1.0e8) return true;
    return pairs >= 3.0e7 && (n > m ? n : m) <= NNM_CT * 32 && !nn_small_serves(b, n, m, sw);
}
// its waves per workgroup: 16 waves (512 queries) share one build of the candidates' fragments; when that leaves fewer than 128
// workgroups (small batches of big clouds, e.g. B = 2, N = 8192 per GPU in cfg-5) 8-wave workgroups fill twice the CUs
inline int nnm_qw(int b, int n, int m, bool force16, const Switches &sw) {
    if (force16 || sw.nnm_qw == 16) return 16;
    if (sw.nnm_qw == 8 || sw.nnm_qw == 4) return sw.nnm_qw;
    return nnm_workgroups(b, n, m, 16) >= 128 ? 16 : nnm_workgroups(b, n, m, 8) >= 128 ? 8 : 4;
}
// dpf_pairwise_cd: 512-query workgroups; 256-query ones for clouds of <= 256 points (half of a 16-wave workgroup would idle)
inline int pairwise_qw(int nmax) { return nmax <= 256 ? 8 : 16; }

// ---- the deterministic Chamfer backward (chamfer_grad.hip) ------------------------------------------------------------------
// One form per output ("targets": the points of the cloud whose gradient it is; "queries": the other cloud's, whose indices are
// sorted).  Lds: one workgroup sorts a cloud's 32-bit keys (index << 13 | query) in LDS -- 4 bytes per key slot and 12 per
// contribution, 128 KB of the CU's 160 at 8192 queries -- and serves all its targets alone, so their number is capped too.
// Workspace: 64-bit keys and the contributions in the caller's scratch, any size dpf_nndistance serves.
constexpr int CG_LDS_QUERIES = 8192;
constexpr int CG_LDS_TARGETS = 65536;
// a target's list of queries is added up by the thread that finds its head while it has at most this many entries (ordinary clouds:
// one on average); a longer one (collapsed or duplicated clouds) by a wave that fetches 64 contributions at a time
constexpr int CG_LONG_LIST = 64;
enum class CGKernel { Lds, Workspace };
struct CGForm { CGKernel kernel; int long_list; };
inline CGForm cg_form(int targets, int queries, const Switches &sw) {
    const bool lds = sw.cg_lds != 0 && queries <= CG_LDS_QUERIES && targets <= CG_LDS_TARGETS;
    return {lds ? CGKernel::Lds : CGKernel::Workspace, CG_LONG_LIST};
}

// ---- approx-EMD (emd.hip) ---------------------------------------------------------------------------------------------------
constexpr int EMD_MAXS = 16;     // max inner-loop slices (waves) per workgroup
constexpr int EMD_PPW = 128;     // points per wave in the deferred kernels
constexpr int EMD_MPW = 128;     // points per wave / workgroup of the matrix-core passes
constexpr int EMD_MSL = 8;       // their max candidate slices (waves) per workgroup
constexpr int EMD_GROWS = 21;
constexpr int EMD_GSL = 8;       // max row slices (waves) per workgroup: two waves per SIMD keep the 64 butterfly values in registers

// the numerical realisation of a call: the matrix-core family exactly when the call is deferred (has its workspace), the
// setting is on and the environment allows it; else the packed-VALU kernels
inline bool emd_matrix_family(bool deferred, const Switches &sw) { return deferred && sw.emd_matrix_set && sw.emd_matrix_env; }

// inner-loop slices per workgroup so that the launch has >= ~2048 waves
// slices for the approxmatch passes (both paths use the same ones, so their sums associate identically): enough
// that the deferred kernels (128 points per wave) put ~4 waves on every SIMD
inline int pick_match_slices(int b, int npoints, int ninner) {
    const long groups = b * ceil_div(npoints, EMD_PPW);
    int s = 1;
    while (s < EMD_MAXS && groups * s < 4096 && ninner / (2 * s) >= 64) s *= 2;
    return s;
}
inline int pick_mfma_slices(int b, int npoints, int ninner) {
    const long groups = b * ceil_div(npoints, EMD_MPW);
    const int tiles = (ninner + 31) / 32;
    int s = 1;
    while (s < EMD_MSL && groups * s < 4096 && tiles / (2 * s) >= 4) s *= 2;
    return s;
}
inline int pick_slices(int b, int npoints, int ninner) {
    const long groups = b * ceil_div(npoints, 64);
    int s = 1;
    while (s < EMD_MAXS && groups * s < 2048 && ninner / (2 * s) >= 64) s *= 2;
    return s;
}
// row slices of the packed-VALU family's recomputing gradient (dpf_matchcostgrad_recompute_ws)
inline int pick_grad_slices(int b, int n, int m) {
    const long nkb = ceil_div(n, EMD_PPW);
    int gs = 1;
    while (gs < EMD_GSL && b * nkb * gs < 2048 && m / (2 * gs) >= 2 * EMD_GROWS) gs *= 2;
    return gs;
}
// dpf_matchcostgrad_ws: one workgroup per 256 columns and cloud: with fewer than one per CU the row-parallel two-pass kernels win
// (measured r01, one pass vs two kernels: B=2, N=8192: 0.58 vs 0.29 ms; B=32, N=2048: 0.37 vs 0.30 ms;
// B=16, N=8192: 1.52 vs 2.26 ms); fewer than four column-waves per SIMD: two row slices per workgroup
enum class GradForm { TwoPass, Fused2, Fused1 };
inline GradForm grad_form(int b, int n, int m, bool has_workspace) {
    const long wgs = b * ceil_div(n, 256);
    if (!has_workspace || wgs < 512) return GradForm::TwoPass;
    return wgs < 1024 && m >= 4 * EMD_GROWS ? GradForm::Fused2 : GradForm::Fused1;
}

// ---- the training stack (flow_train.hip) ------------------------------------------------------------------------------------
constexpr int TRAIN_MJ_ROLES = (516 + 31) / 32;     // pass 2's role workgroups
// the forms of a layer's kernels at nblk ordinary workgroups per launch, on a chip of n_cu compute units (the caller looks
// the count up once, at the first training call)
struct TrainForm { bool split_h1, split1, split2, roles, fuse_colsum; };
inline TrainForm train_form(int ns, int nblk, int n_cu, const Switches &sw) {
    const bool forced = sw.train_split >= 0, on = sw.train_split != 0;
    TrainForm f;
    // small batches: the two conditioner branches in two workgroups each (at most half a workgroup per CU otherwise).  r04,
    // B = 8: tstats_h1 9.5 -> 8.7 us; at 128 workgroups -- B = 16 -- the statistics and pass 1 are better off unsplit (tbwd1
    // 15.7 us unsplit, 18.1 split), only pass 2 gains
    f.split_h1 = f.split1 = forced ? on : nblk <= 64;
    // (bf16x6's three forward parts do not leave the one-branch-per-wave form its registers: that precision keeps one branch per workgroup)
    f.split2 = ns == 3 || (forced ? on : nblk <= 128);
    // Who finishes pass 1 -- per-cloud totals, FiLM gradients, dW2 / db2, the BN1-backward means?  Pass 2 needs a CU per workgroup
    // (158 KB of LDS): role workgroups at the front of its grid (MeansJob) cost nothing where CUs are idle and a whole round of
    // late workgroups where they are not.  So: roles while the ordinary workgroups + MJ_ROLES fit the chip's CUs, else pass 1's
    // per-cloud ticket and a recomputation of the means by every workgroup of pass 2 (r02-r04).  DPF_TRAIN_ROLES=0/1 forces either.
    // (the role form is built for the one-branch-per-workgroup kernel only: that is the form small batches run)
    f.roles = f.split2 && (sw.train_roles >= 0 ? sw.train_roles != 0 : 2 * nblk + TRAIN_MJ_ROLES <= n_cu);
    // r04: the column sums of the layer above's pass-2 partials ride in pass 1's launch (ColsumJob) instead of a tcolsum launch
    // of their own between the two layers; DPF_TRAIN_FUSE_COLSUM=0 keeps the separate launch
    f.fuse_colsum = sw.train_fuse_colsum != 0;
    return f;
}

// ---- point-to-mesh and mesh-to-cloud distance (point_mesh.hip, mesh_point.hip) --------------------------------------------------
constexpr int PM_WG_POINTS = 256;   // query points of a workgroup: 4 waves, one point per lane
constexpr int PM_TILE = 256;        // faces per LDS tile (16 KB of staged faces)
constexpr int MP_WG_FACES = 256;    // mesh_point.hip: faces of a workgroup, 4 waves, one staged face per lane
constexpr int MP_TILE = 256;        // points per LDS tile (4 KB)
constexpr int PM_FILL_WGS = 512;    // workgroups that fill the chip: two per CU (profiles/point_mesh_forms.txt, mesh_point_forms.txt)
constexpr int MAX_SPLITS = 1024, PM_MAX_SPLITS = MAX_SPLITS, MP_MAX_SPLITS = MAX_SPLITS;
// A search keeps a workgroup's 256 row items (points; faces in mesh_point.hip) in registers and walks LDS tiles of the other side.
// Whole: every workgroup walks all tiles of its slot.  Split: the tiles are dealt round-robin to `splits` workgroups per 256 row
// items (64-bit atomic minimum, then a finishing launch) -- where the row items alone leave CUs idle, as many splits as bring the
// launch to PM_FILL_WGS workgroups, never more than there are tiles.  force: 0 by size, 1 Whole, 2 Split (with the splits the
// sizes ask for, at least one).  Total: any arguments >= 1 give a form with 1 <= splits <= MAX_SPLITS.
enum class PMKernel { Whole, Split };
struct PMForm { PMKernel kernel; int splits; };
inline PMForm split_form(long workgroups, long tiles, int force) {
    long splits = workgroups >= PM_FILL_WGS ? 1 : ceil_div(PM_FILL_WGS, workgroups);
    if (splits > tiles) splits = tiles;
    if (splits > MAX_SPLITS) splits = MAX_SPLITS;
    if (force == 1 || (force != 2 && splits < 2)) return {PMKernel::Whole, 1};
    return {PMKernel::Split, (int)splits};
}
inline long at_least_one(long items, long per) { return items > 0 ? ceil_div(items, per) : 1; }
// points in rows, tiles of the largest mesh's faces
inline PMForm pm_form(int b, int n, long max_faces, int force) {
    return split_form(at_least_one(b, 1) * at_least_one(n, PM_WG_POINTS), at_least_one(max_faces, PM_TILE), force);
}
// the roles swapped: the widest mesh's faces in rows, tiles of the cloud's points
inline PMForm mp_form(int b, int n, long max_faces, int force) {
    return split_form(at_least_one(b, 1) * at_least_one(max_faces, MP_WG_FACES), at_least_one(n, MP_TILE), force);
}

// ---- exact EMD (emd_exact.hip) ------------------------------------------------------------------------------------------------
constexpr int EE_MAX_POINTS = 8192;     // points per cloud: the bidder tag of a bid key has 13 bits, the streamed form's LDS 128 KB
constexpr int EE_LDS_POINTS = 4096;     // the resident form's: 36 bytes a point, 144 KB of the CU's 160
constexpr int EE_MIN_BITS = 1, EE_MAX_BITS = 24;   // the cost grid's bits: rint(d * s) < 2^bits is an exact fp32 integer up to 24
constexpr int EE_EPS0_SHIFT = 4;        // the first epsilon: ((n + 1) << bits) >> 4
constexpr int EE_EPS_SHIFT = 3;         // epsilon falls by 3 bits a phase (oracle, Gaussian clouds of 2 048 points: 10 780 rounds against
                                        // 27 114 at 2 bits and 25 865 at 1)
// Resident: the second cloud and the bids in LDS; Streamed: the cloud read from global memory, the bids in the caller's workspace.
// The resident form wherever it fits (it never waits on L2).  force: 0 by size, 1 Resident, 2 Streamed; Unserved: n outside
// 1..EE_MAX_POINTS, or the resident form forced past EE_LDS_POINTS.  threads: a wave for clouds of up to 64 points (its barriers are
// free), 4 waves up to 512, else 16 -- late rounds cut a lone bidder's candidates into slices of >= 64 for the idle waves.
enum class EEKernel { Resident, Streamed, Unserved };
struct EEForm { EEKernel kernel; int threads, lds_per_point; };
inline EEForm ee_form(int n, int force) {
    if (n < 1 || n > EE_MAX_POINTS || (force == 1 && n > EE_LDS_POINTS)) return {EEKernel::Unserved, 0, 0};
    const int threads = n <= 64 ? 64 : n <= 512 ? 256 : 1024;
    if (force == 2 || (force != 1 && n > EE_LDS_POINTS)) return {EEKernel::Streamed, threads, 16};
    return {EEKernel::Resident, threads, 36};
}

// ---- farthest-point sampling (fps.hip) ------------------------------------------------------------------------------------------
constexpr int FPS_MAX_POINTS = 8192;    // points per cloud: 12 bytes a point in LDS, 96 KB of the CU's 160
constexpr int FPS_WAVE_MAX = 512;       // the one-wave form's: 8 points a lane
constexpr int FPS_QUAD_MAX = 8192;      // the four-wave form's: 32 points a thread (198 registers, one wave per SIMD)
constexpr int FPS_QUAD_UPTO = 4096;     // by size: four waves up to here, sixteen above
// Wave: 64 threads, no barrier in a round; Quad: 256 threads, one wave per SIMD; Full: 1024 threads, four waves per SIMD.  ppt: the
// points a thread keeps in registers, the lowest power of two with threads * ppt >= n.  force: 0 by size, 1 Wave, 2 Quad, 3 Full;
// Unserved: n outside 1..FPS_MAX_POINTS, a form forced past its limit, an unknown form.
// By size (profiles/fps_forms.txt; us per round at B = 1 | ms per call at B = 1024 clouds, k = n):
//   n =  256: Wave 0.341 | 0.101, Quad 0.451 | 0.158, Full 0.736 | 0.543    n =  512: Wave 0.395 | 0.232, Quad 0.443 | 0.342, Full 0.711 | 1.059
//   n = 1024:                     Quad 0.473 | 0.790, Full 0.698 | 2.110    n = 4096:                     Quad 0.727 | 6.51,  Full 0.848 | 10.97
//   n = 8192:                     Quad 1.175 | 38.8,  Full 1.133 | 37.4
// One wave wins wherever it serves: a round without a barrier, and four times the clouds on a CU.  Sixteen waves pay a dearer
// meeting (0.70 us a round with one point a thread) and win only where four waves would hold 32 points a thread.
enum class FPSKernel { Wave, Quad, Full, Unserved };
struct FPSForm { FPSKernel kernel; int threads, ppt; };
inline FPSForm fps_form(int n, int force) {
    if (n < 1 || n > FPS_MAX_POINTS || force < 0 || force > 3) return {FPSKernel::Unserved, 0, 0};
    if ((force == 1 && n > FPS_WAVE_MAX) || (force == 2 && n > FPS_QUAD_MAX)) return {FPSKernel::Unserved, 0, 0};
    const FPSKernel kernel = force == 1 ? FPSKernel::Wave : force == 2 ? FPSKernel::Quad : force == 3 ? FPSKernel::Full
                             : n <= FPS_WAVE_MAX ? FPSKernel::Wave : n <= FPS_QUAD_UPTO ? FPSKernel::Quad : FPSKernel::Full;
    const int threads = kernel == FPSKernel::Wave ? 64 : kernel == FPSKernel::Quad ? 256 : 1024;
    int ppt = 1;
    while (threads * ppt < n) ppt *= 2;
    return {kernel, threads, ppt};
}

// ---- sliced Wasserstein: the per-(cloud, direction) sort (swd.hip) ---------------------------------------------------------------
constexpr int SWD_MAX_POINTS = 8192;    // keys per sort: 8 bytes a key in LDS, 64 KB of the CU's 160
constexpr int SWD_WAVE_MAX = 512;       // the one-wave form's: 8 keys a lane, no LDS and no barrier in the sort
constexpr int SWD_QUAD_MAX = 8192;      // the four-wave form's: 32 keys a thread
constexpr int SWD_QUAD_UPTO = 2048;     // by size: four waves up to here, sixteen above
// Wave: 64 threads; Quad: 256; Full: 1024.  kpt: the keys a thread keeps in registers, the lowest power of two with
// threads * kpt >= n -- the bitonic network sorts threads * kpt keys, so one instantiation serves one power-of-two class of n.
// force: 0 by size, 1 Wave, 2 Quad, 3 Full; Unserved: n outside 1..SWD_MAX_POINTS, a form forced past its limit, an unknown form.
// By size (profiles/swd_forms.txt, the rows "the sort by form": us per sort with 8192 sorts in flight | us for one sort alone):
//   n =  512: Wave 0.013 | 49.4, Quad 0.016 | 28.8, Full 0.047 | 32.1     n = 1024: Quad 0.026 | 40.1, Full 0.048 | 32.6
//   n = 2048: Quad 0.050 | 62.4, Full 0.072 | 42.5                        n = 4096: Quad 0.124 | 110.0, Full 0.123 | 60.1
//   n = 8192: Quad 0.438 | 213.0, Full 0.238 | 100.6
// The thresholds follow the throughput column, the one a table build of many sorts pays: one wave wins wherever it serves (no
// LDS pass, no barrier, four times the sorts on a CU); four waves win up to 2048; at 4096 the two tie in throughput and sixteen
// waves halve the latency; at 8192 sixteen waves win by 1.8 (four waves hold 32 keys a thread there).
enum class SWDKernel { Wave, Quad, Full, Unserved };
struct SWDForm { SWDKernel kernel; int threads, kpt; };
inline SWDForm swd_form(int n, int force) {
    if (n < 1 || n > SWD_MAX_POINTS || force < 0 || force > 3) return {SWDKernel::Unserved, 0, 0};
    if ((force == 1 && n > SWD_WAVE_MAX) || (force == 2 && n > SWD_QUAD_MAX)) return {SWDKernel::Unserved, 0, 0};
    const SWDKernel kernel = force == 1 ? SWDKernel::Wave : force == 2 ? SWDKernel::Quad : force == 3 ? SWDKernel::Full
                             : n <= SWD_WAVE_MAX ? SWDKernel::Wave : n <= SWD_QUAD_UPTO ? SWDKernel::Quad : SWDKernel::Full;
    const int threads = kernel == SWDKernel::Wave ? 64 : kernel == SWDKernel::Quad ? 256 : 1024;
    int kpt = 1;
    while (threads * kpt < n) kpt *= 2;
    return {kernel, threads, kpt};
}

// ---- k nearest neighbours (knn.hip) ------------------------------------------------------------------------------------------------
constexpr int KNN_MAX_K = 32;           // the largest list a lane keeps in registers: 64 VGPRs of (distance, index)
constexpr int KNN_WG_QUERIES = 256;     // queries of a workgroup: 4 waves, one query per lane
constexpr int KNN_TILE = 256;           // candidates per LDS tile (3 KB, structure of arrays)
constexpr int KNN_QUEUE = 16;           // deferred candidates per lane (8 bytes each: 32 KB of LDS a workgroup)
// kcap: the list capacity the kernel is instantiated for, 4 | 8 | 16 | 32; it serves k <= kcap and its outputs do not depend on it.
// force: 0 = the smallest capacity >= k (the insertion chain costs 5 instructions per slot, so a larger one only costs); 1..4 force
// capacity 4, 8, 16, 32.  Unserved (kcap 0): k outside 1..KNN_MAX_K, a forced capacity below k, an unknown form.
struct KNNForm { int kcap; };
inline KNNForm knn_form(int k, int force) {
    if (k < 1 || k > KNN_MAX_K || force < 0 || force > 4) return {0};
    if (force) return {(4 << (force - 1)) >= k ? 4 << (force - 1) : 0};
    return {k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32};
}

// ---- point-cloud normals (normals.hip) ---------------------------------------------------------------------------------------------
constexpr int NORMALS_MIN_K = 3;        // fewer points span no plane
constexpr int NORMALS_MAX_K = KNN_MAX_K;    // dpf_knn's largest list: a lane keeps its k gathered points in registers (3 VGPRs each)
constexpr int NORMALS_WG_POINTS = 64;   // one wave a workgroup, one point a lane: no LDS, no barrier, so the smallest workgroup spreads best
constexpr int NORMALS_SWEEPS = 6;       // cyclic Jacobi sweeps of the 3 x 3 covariance: 4 reach the rounding floor, 6 are run
// kcap: the neighbourhood capacity the kernel is instantiated for, 4 | 8 | 16 | 32 -- the smallest >= k (its gather is unrolled over
// kcap; the outputs do not depend on it).  Unserved (kcap 0): k outside NORMALS_MIN_K..NORMALS_MAX_K.
struct NormalsForm { int kcap; };
inline NormalsForm normals_form(int k) {
    if (k < NORMALS_MIN_K || k > NORMALS_MAX_K) return {0};
    return {k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32};
}

// ---- rigid alignment (align.hip) ---------------------------------------------------------------------------------------------------
constexpr int ALIGN_WG_POINTS = 256;    // source points of a workgroup: 4 waves, one point per lane -- and the block of the sums' tree
constexpr int ALIGN_TILE = 256;         // target points per LDS tile (3 KB, structure of arrays), as KNN_TILE
constexpr int ALIGN_SUMS = 18;          // float64 quantities per slot: W, S_p (3), S_q (3), S_pq (9), S_pp, S_d
constexpr int ALIGN_SWEEPS = 7;         // cyclic Jacobi sweeps of Horn's 4 x 4 matrix: 5 reach the rounding floor, 7 are run
constexpr int ALIGN_MIN_INLIERS = 3;    // fewer matched points fix no rotation
// blocks: workgroups of a slot's match (or accumulate) launch = block partials a slot's solve wave adds up, in ascending order;
// launches: kernels a call puts on the stream -- a match and a solve per iteration and one more pair for the returned transform
// (dpf_rigid_fit: iters = 0).  Unserved (blocks 0): n < 1 or iters < 0.
struct AlignForm { long blocks; long launches; };
inline AlignForm align_form(int n, int iters) {
    if (n < 1 || iters < 0) return {0, 0};
    return {ceil_div(n, ALIGN_WG_POINTS), 2 * ((long)iters + 1)};
}
// point-to-plane ICP (dpf_icp_plane): the same workgroups and the same launch pattern, thirty-one sums a block
constexpr int ALIGN_PLANE_SUMS = 31;        // W, the upper triangle of sum a a^T (21), sum a r (6), S_d, S_r, S_yy
constexpr int ALIGN_PLANE_MIN_INLIERS = 6;  // fewer planes than unknowns fix no step
// blocks, launches: as AlignForm's; partial_doubles: the float64 block partials a slot keeps in the workspace.
// Unserved (blocks 0): n < 1 or iters < 0.
struct AlignPlaneForm { long blocks; long launches; long partial_doubles; };
inline AlignPlaneForm align_plane_form(int n, int iters) {
    if (n < 1 || iters < 0) return {0, 0, 0};
    const long blocks = ceil_div(n, ALIGN_WG_POINTS);
    return {blocks, 2 * ((long)iters + 1), blocks * ALIGN_PLANE_SUMS};
}

// ---- density-aware Chamfer distance (dcd.hip) ----------------------------------------------------------------------------------------
constexpr int DCD_BLOCK = 256;            // queries of a block of the sums' tree (ALIGN_WG_POINTS: the same tree)
constexpr int DCD_LDS_THREADS = 1024;     // the one-workgroup form: four blocks of the tree a step
constexpr int DCD_LDS_TARGETS = 32768;    // its histogram: 4 bytes a target, 128 KB of the workgroup's 160, 8 KB beside it for the tree
// Lds: one workgroup a cloud, the counts an int32 histogram in LDS, ONE launch; Workspace: the counts in the workspace, four launches
// (zero, count, terms over (cloud, block), one finishing wave a cloud).  Both return the same bits.  blocks1 / blocks2: the blocks of
// side 1's n and side 2's m queries = the float64 partials a cloud's finishing wave adds up, in ascending order.
// force: 0 by size, 1 Lds, 2 Workspace; Unserved: B < 0, n < 1, m < 1, an unknown form, Lds forced past DCD_LDS_TARGETS.
// By size: Lds wherever both target sets fit its histogram (profiles/dcd_forms.txt, us per call, Lds | Workspace):
//   32 x 2048 x 2048: 28.5 | 35.0     50 x 2500 x 2500: 29.4 | 36.8     1 x 32768 x 32768: 114.0 | 82.6
// One launch wins at the evaluation shapes.  One cloud at the cap is the other way round (one workgroup walks 65536 queries while
// the chip idles); that is one measured point, not a threshold, so by size stays Lds there and a caller with such a shape asks for 2.
enum class DCDKernel { Lds, Workspace, Unserved };
struct DCDForm { DCDKernel kernel; long blocks1, blocks2; int launches; };
inline DCDForm dcd_form(int B, int n, int m, int force) {
    if (B < 0 || n < 1 || m < 1 || force < 0 || force > 2) return {DCDKernel::Unserved, 0, 0, 0};
    const bool fits = n <= DCD_LDS_TARGETS && m <= DCD_LDS_TARGETS;
    if (force == 1 && !fits) return {DCDKernel::Unserved, 0, 0, 0};
    const bool lds = force == 1 || (force == 0 && fits);
    return {lds ? DCDKernel::Lds : DCDKernel::Workspace, ceil_div(n, DCD_BLOCK), ceil_div(m, DCD_BLOCK), lds ? 1 : 4};
}

}  // namespace dispatch
#endif  // DPF_DISPATCH_H
