/*
 * dpf_hip.h -- C ABI of libdpf_hip.so: the MI355X (gfx950) implementation of
 * dpf-nets' per-point flow decoder and structural losses.
 *
 * Drop-in boundary.  Every entry point takes raw DEVICE pointers, plain ints
 * and a HIP stream (hipStream_t passed as void*); no torch / ATen types.  The
 * caller owns every buffer (inputs, outputs and scratch); nothing here
 * allocates, frees or synchronises.  All launches are asynchronous on
 * `stream`.  Return value: 0 on success, otherwise the hipError_t of the failed
 * launch, or a negative DPF_E* code for an argument the kernels do not support
 * (the reference returned void and, for Chamfer, checked nothing:
 * nndistance.cu:125-128).
 *
 * File:line citations are into the reference tree (Regenerator/dpf-nets).
 */
#ifndef DPF_HIP_H
#define DPF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *dpf_stream_t; /* hipStream_t */

#define DPF_EINVAL (-1)  /* bad size / null pointer */
#define DPF_ENOSUP (-2)  /* shape the kernels are not built for (e.g. F != 64) */

/* ------------------------------------------------------------------------ *
 * Structural losses.  Same argument order and meaning as the reference's C
 * launchers, which lib/metrics/pytorch_structural_losses/src/structural_loss.cpp
 * binds (:35, :50, :67, :97, :118).  Point clouds are point-major fp32
 * (B, n, 3) contiguous; indices int32.
 * ------------------------------------------------------------------------ */

/* replaces nndistance(...)      src/nndistance.cuh:1, nndistance.cu:125-128.
 * result[b,j]  = min_k |xyz[b,j]-xyz2[b,k]|^2, result_i = its FIRST argmin;
 * result2/_i the same with the clouds swapped.  Bit-exact contract:
 * d = (dx*dx + dy*dy) + dz*dz, dx = xyz2 - xyz, no FMA contraction.
 * Non-finite input (NaN / Inf coordinates, or coordinates whose squared
 * distances overflow): the result of the reference's own loop,
 * nndistance.cu:5-122 -- candidates in batches of 512, the first of a batch
 * taken unconditionally, strict '<' inside a batch (:26, 116), strict '>'
 * across batches (:120) -- so a NaN distance at candidate 0 gives (NaN, 0), at
 * candidate 512k it makes batch k lose, elsewhere it is skipped.  Every
 * implementation below (scan, matrix-core filter, strided, _cd, pairwise)
 * detects such input and runs that loop for the affected queries
 * (csrc/nn_refscan.h); NaN payloads are not specified. */
int dpf_nndistance(int b, int n, const float *xyz, int m, const float *xyz2,
                   float *result, int *result_i, float *result2, int *result2_i,
                   dpf_stream_t stream);

/* Which kernel serves dpf_nndistance(_strided) for rank-sized batches of 1024..8192-point clouds (< 512 waves of the scan):
 * the LDS-staged one-query-per-lane kernel (csrc/chamfer.hip nn_small_kernel, r04) or the scalar-load scan.  Same bits.
 * mode: -1 = by size (default; env DPF_NN_SMALL), 0 = never, 1 = whenever the clouds fit.  Returns the previous mode.
 * Sets an atomic process default; meant for tests and tools.  A call in flight keeps the value it read at entry. */
int dpf_nn_small_mode(int mode);

/* dpf_nndistance with explicit strides (in floats) between consecutive clouds of
 * each set; stride 0 broadcasts one cloud over the batch -- the "expand +
 * contiguous" copy of pairwise_CD (lib/networks/utils.py:104-107) disappears. */
int dpf_nndistance_strided(int b, int n, const float *xyz, long xyz_stride, int m,
                           const float *xyz2, long xyz2_stride, float *result, int *result_i,
                           float *result2, int *result2_i, dpf_stream_t stream);

/* Same results as dpf_nndistance, bit for bit, matrix-core filtered: one bf16
 * MFMA per 32x32 pairs bounds every distance to within 2^-14*R2, and only the
 * candidates that can still be the fp32-exact minimiser (or tie with it) are
 * evaluated with the exact formula.  The fragments are built inside the kernel:
 * `workspace` is unused (kept for the ABI; _workspace_bytes returns 0).  Both
 * clouds under 32 points -> the brute-force kernel. */
size_t dpf_nndistance_mfma_workspace_bytes(int b, int n, int m);
int dpf_nndistance_mfma(int b, int n, const float *xyz, int m, const float *xyz2,
                        float *result, int *result_i, float *result2, int *result2_i,
                        void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* dpf_nndistance's contract and bits; the matrix-core filtered kernel where it is the faster
 * one (>= 1e8 pair evaluations and >= 64 workgroups of 256 queries), the VALU scan otherwise.
 * This is what the Python mirror calls by default. */
int dpf_nndistance_auto(int b, int n, const float *xyz, int m, const float *xyz2,
                        float *result, int *result_i, float *result2, int *result2_i,
                        dpf_stream_t stream);
int dpf_nndistance_strided_auto(int b, int n, const float *xyz, long xyz_stride, int m,
                                const float *xyz2, long xyz2_stride, float *result,
                                int *result_i, float *result2, int *result2_i,
                                dpf_stream_t stream);   /* dpf_nndistance_strided, same choice */

/* replaces nndistancegrad(...)  src/nndistance.cuh:2, nndistance.cu:149-154.
 * grad_xyz1 / grad_xyz2 are fully overwritten (the zero-fill happens on
 * `stream`, not on the null stream as at nndistance.cu:150-151). */
int dpf_nndistancegrad(int b, int n, const float *xyz1, int m, const float *xyz2,
                       const float *grad_dist1, const int *idx1,
                       const float *grad_dist2, const int *idx2,
                       float *grad_xyz1, float *grad_xyz2, dpf_stream_t stream);

/* dpf_nndistancegrad with a DEFINED order of additions: the same bits on every run (csrc/chamfer_grad.hip; no float atomics).
 * Per cloud, every operation a separately rounded fp32 one (no FMA contraction):
 *   grad_xyz1[j] = (2*grad_dist1[j]) * (xyz1[j] - xyz2[idx1[j]])                                     (the direct term), then
 *   grad_xyz1[idx2[l]] = grad_xyz1[idx2[l]] + (-((2*grad_dist2[l]) * (xyz2[l] - xyz1[idx2[l]])))     for l = 0 .. m-1 ASCENDING;
 * grad_xyz2 the same with the clouds swapped (direct term from grad_dist2 / idx2, then j = 0 .. n-1 ascending).  This is one of
 * the orders dpf_nndistancegrad may produce, so its tolerances hold.  grad_xyz1 or grad_xyz2 may be NULL: that gradient is
 * neither computed nor written.  Serves every size dpf_nndistance serves (3n, 3m < 2^31, b <= 65535; n != m included); an index
 * outside its cloud is read as the nearest valid one.
 * workspace: dpf_nndistancegrad_det_workspace_bytes(b, n, m) bytes, 8-byte aligned, caller-owned; 0 bytes (NULL allowed) while the
 * clouds are sorted in LDS (<= 8192 queries and <= 65536 targets per output).  It may come in dirty and is left dirty: nothing
 * in it has to be zero, the call writes every word it reads.  No allocation, no host synchronisation: capture-safe. */
size_t dpf_nndistancegrad_det_workspace_bytes(int b, int n, int m);
int dpf_nndistancegrad_det(int b, int n, const float *xyz1, int m, const float *xyz2,
                           const float *grad_dist1, const int *idx1,
                           const float *grad_dist2, const int *idx2,
                           float *grad_xyz1, float *grad_xyz2,
                           void *workspace, size_t workspace_bytes, dpf_stream_t stream);
/* The same for the per-cloud Chamfer distance cd[i] = mean(dist1[i]) + mean(dist2[i]): grad_dist1[i][j] = grad_cd[i] / (float)n and
 * grad_dist2[i][l] = grad_cd[i] / (float)m (correctly rounded fp32 divisions, what autograd's mean hands back); no (B, n) row is
 * read.  Same workspace, same NULL rule: one output is the common case (the target cloud does not require a gradient). */
int dpf_chamfer_cd_backward(int b, int n, const float *xyz1, int m, const float *xyz2,
                            const int *idx1, const int *idx2, const float *grad_cd,
                            float *grad_xyz1, float *grad_xyz2,
                            void *workspace, size_t workspace_bytes, dpf_stream_t stream);
/* Which form serves them: -1 = by size (default; env DPF_CG_LDS), 0 = never the LDS-only form (every output sorts in the
 * workspace), 1 = as -1.  Same bits.  Returns the previous mode; an atomic process default for tests and tools, like
 * dpf_nn_small_mode (ask dpf_nndistancegrad_det_workspace_bytes after setting it). */
int dpf_chamfer_grad_lds_mode(int mode);

/* replaces approxmatch(...)     src/approxmatch.cuh:6, approxmatch.cu:299-307.
 * match: (b, m, n) fp32, fully overwritten.  temp: (b, 2*(n+m)) fp32 scratch
 * (remainL | remainR | ratioL | ratioR per cloud, approxmatch.cu:4). */
int dpf_approxmatch(int b, int n, int m, const float *xyz1, const float *xyz2,
                    float *match, float *temp, dpf_stream_t stream);

/* dpf_approxmatch with `match` written ONCE: the nine levels' ratio vectors and the passes' operand records are kept in
 * `workspace` and the matching is materialised by a final pass (4*n*m instead of 68*n*m bytes of HBM traffic per
 * cloud).  dpf_approxmatch_workspace_bytes covers both kernel families below: ~ 36*(n+m) + 16*(n+2m) + 48*m + n/2 bytes
 * per cloud for the packed-VALU one (bit-identical to dpf_approxmatch) + ~ 64*n + 350*m for the matrix-core one.
 * NULL / short workspace -> the read-modify-write path. */
size_t dpf_approxmatch_workspace_bytes(int b, int n, int m);
/* r05 / r06: with a workspace the 27 level passes run on the matrix cores (expanded-form squared distance, two chained MFMAs
 * per 32 x 32 pairs whose large terms are exact integer arithmetic on a per-call grid; csrc/emd.hip) when every point of
 * both clouds, centred on cloud 1's centroid c, has log2(e) |x - c|^2 <= 16 and is finite -- decided per call on the device;
 * otherwise, and after dpf_emd_set_matrix_path(0), the packed-VALU kernels run, whose results are bit-identical to
 * dpf_approxmatch.  The matrix-core results are within the tolerance contract (cost 1e-4; the exp2 arguments within 2e-5 of
 * float64 at the steepest level on unit-size clouds, measured by dpf_debug_emd_exponents), not bit-identical -- with one measured
 * exception: on clouds of a few dozen points a rare pair leaves 1e-4 (32-point Gaussian clouds: 27 of 65 535 pairs, worst 6.5e-4,
 * on inputs the fp32 oracle resolves to 1e-8; tests/test_gpu_pairwise_emd.py, the launch-limit test), where the packed-VALU
 * kernels stay within 1e-4 (worst 8.8e-5 on the same pairs).  DETERMINISM of
 * the matrix-core kernels is a property of the compiled code, not of the source: two builds of r05 returned run-to-run
 * differing bits (csrc/emd.hip, opaque_zero).  r06 found why: the compiler's vectoriser had written a packed fp32 instruction form
 * (low half reading the high word of a VGPR pair) that gfx950 executes wrongly in lanes 48-63 while another wave of the SIMD issues
 * MFMAs (tools/ubench/pk_vs_mfma_forms.hip).  The Makefile refuses to link ANY object that holds that form, or packed
 * fp32 beside MFMAs, or an emd.o whose MFMAs do not have the properties of the build that repeats (tools/mfma_overlap_check.py);
 * tests/test_gpu_emd.py holds the repeat tests, tests/test_gpu_interference.py runs the kernels beside an MFMA-issuing kernel of
 * another stream.  Returns the previous setting.  Sets an atomic process default (ANDed with env DPF_EMD_MATRIX, which the
 * setter cannot override); meant for tests and tools.  A call in flight keeps the value it read at entry. */
int dpf_emd_set_matrix_path(int on);
int dpf_approxmatch_ws(int b, int n, int m, const float *xyz1, const float *xyz2,
                       float *match, float *temp, void *workspace, size_t workspace_bytes,
                       dpf_stream_t stream);

/* dpf_approxmatch_ws followed by dpf_matchcost in one call (what MatchCostFunction.forward does,
 * match_cost.py:20-22): the pass that materialises `match` also accumulates
 * cost[b] = sum match * |xyz1 - xyz2| (the distance is at hand), saving matchcost's pass over
 * the (b, m, n) matching.  Fixed-order partial sums (deterministic); agrees with dpf_matchcost
 * to fp32 summation order.  The workspace (dpf_approxmatch_workspace_bytes) is required. */
int dpf_approxmatch_cost_ws(int b, int n, int m, const float *xyz1, const float *xyz2,
                            float *match, float *temp, float *cost, void *workspace,
                            size_t workspace_bytes, dpf_stream_t stream);

/* dpf_approxmatch_cost_ws without the matching: no `match` argument, nothing of size n*m written or allocated.  The launches,
 * the slices and every operation of the sums are those of dpf_approxmatch_cost_ws (its last pass runs without its stores), so
 * `cost` and temp[:, :n+m] carry the same bits on the same input -- both kernel families, and clouds the device hands to the
 * packed-VALU family (out of range, not finite).  workspace: dpf_approxmatch_workspace_bytes, required.
 * On return the workspace is the SAVED STATE of dpf_matchcostgrad_recompute_ws, which reads
 *   - the nine per-level ratio slots [ratioL (n) | ratioR (m)] per cloud (the front of the workspace);
 *   - the packed-VALU family's materialisation records (xyz2, ratioR of the nine levels: 12 floats per point of cloud 2), behind
 *     the passes' packed (x, y, z, w) records;
 *   - of the matrix-core regions: recB1 (cloud 1's operand records), recAs / rrs / c2s / ls (cloud 2's operand records, per-level
 *     ratioR, coordinates and row numbers in the order the points left the auction) and counts (the levels' list lengths);
 *   - the flag region: word 0 the device's per-call verdict (1: packed-VALU), word 1 the matrix-path setting of THIS call
 *     (written by this entry only).
 * The caller keeps the workspace unchanged, and xyz1 / xyz2 as they were, until the backward has run. */
int dpf_approxmatch_costonly_ws(int b, int n, int m, const float *xyz1, const float *xyz2,
                                float *temp, float *cost, void *workspace, size_t workspace_bytes,
                                dpf_stream_t stream);

/* The gradients of dpf_matchcostgrad with the matching REBUILT, tile by tile in registers, from the state
 * dpf_approxmatch_costonly_ws left in `saved_workspace`: no (b, m, n) tensor exists at any time.  The rebuilt weights are the
 * bits the materialising pass would have stored (the same level loop on the same operands: the same MFMAs for the matrix-core
 * family, the same packed-VALU level sum for the other); only the order of the gradients' sums differs from
 * dpf_matchcostgrad_ws.  The family is the one the forward ran: read from the saved verdict and setting, not from
 * dpf_emd_set_matrix_path at the time of this call.  saved_workspace is only read (a second call returns the same bits);
 * scratch (dpf_matchcostgrad_recompute_workspace_bytes: 12 bytes per 64-column block and row, 3 / (16 n) of the matching)
 * takes grad2's per-column-block partial sums, added in a fixed order: deterministic, no atomics.  Allocates nothing, does not
 * synchronise, safe under stream capture. */
size_t dpf_matchcostgrad_recompute_workspace_bytes(int b, int n, int m);
int dpf_matchcostgrad_recompute_ws(int b, int n, int m, const float *xyz1, const float *xyz2,
                                   const void *saved_workspace, size_t saved_bytes,
                                   float *grad1, float *grad2, void *scratch, size_t scratch_bytes,
                                   dpf_stream_t stream);

/* replaces matchcost(...)       src/approxmatch.cuh:7, approxmatch.cu:309-316.
 * out: (b,) = sum_{l,k} match[b,l,k] * |xyz1[b,k]-xyz2[b,l]|_2. */
int dpf_matchcost(int b, int n, int m, const float *xyz1, const float *xyz2,
                  const float *match, float *out, dpf_stream_t stream);

/* replaces matchcostgrad(...)   src/approxmatch.cuh:8, approxmatch.cu:318-326. */
int dpf_matchcostgrad(int b, int n, int m, const float *xyz1, const float *xyz2,
                      const float *match, float *grad1, float *grad2,
                      dpf_stream_t stream);

/* The same two gradients with `match` read ONCE instead of twice (one workgroup per
 * 256 columns walks all rows; per-row lane sums by a halving butterfly; partials in
 * `workspace`, added in a fixed order).  Deterministic; agrees with
 * dpf_matchcostgrad to fp32 summation order.  NULL / short workspace -> that. */
size_t dpf_matchcostgrad_workspace_bytes(int b, int n, int m);
int dpf_matchcostgrad_ws(int b, int n, int m, const float *xyz1, const float *xyz2,
                         const float *match, float *grad1, float *grad2,
                         void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* Chamfer caller reductions, lib/networks/evaluating.py:112:
 * cd[b] = mean_j dist1[b,j] + mean_k dist2[b,k]  (the reference then takes
 * .mean() over the batch).  Deterministic: one workgroup per cloud, fixed tree. */
int dpf_chamfer_reduce(int b, int n, int m, const float *dist1, const float *dist2,
                       float *cd, dpf_stream_t stream);

/* f_score's reductions, lib/networks/utils.py:38-42, from the two distance rows of one nn_distance call:
 * out[b] = 2 P R / (P + R + 1e-7), P = 100 * mean(dist2[b] < threshold), R = 100 * mean(dist1[b] < threshold).
 * One launch instead of ~10 elementwise / reduction launches; counts are integers (exact). */
int dpf_fscore_reduce(int b, int n, int m, const float *dist1, const float *dist2, float threshold,
                      float *out, dpf_stream_t stream);

/* nn_distance and its callers' reduction in one call (lib/networks/evaluating.py:110-113): the four outputs of
 * dpf_nndistance (same bits) plus cd[b] = mean(result[b]) + mean(result2[b]).  With the matrix-core kernel the
 * workgroups publish fixed-order sums of their distances and the LAST workgroup of every cloud (a ticket per cloud,
 * device-coherent stores / loads on both sides) adds them in tile order: no second launch.  workspace:
 * dpf_nndistance_cd_workspace_bytes bytes, caller-owned; its first b words are the tickets -- they must be zero on
 * entry and are zero again on exit: pass tickets_are_zero = 1 for a workspace that was cleared once and is kept,
 * 0 to have this call clear them.  Small problems: dpf_nndistance_auto + dpf_chamfer_reduce. */
size_t dpf_nndistance_cd_workspace_bytes(int b, int n, int m);
int dpf_nndistance_cd(int b, int n, const float *xyz, int m, const float *xyz2,
                      float *result, int *result_i, float *result2, int *result2_i, float *cd,
                      void *workspace, size_t workspace_bytes, int tickets_are_zero, dpf_stream_t stream);

/* pairwise_CD, lib/networks/utils.py:90-117 (called three times per generative evaluation, evaluating.py:245-247):
 * cds[i, j] = mean(dist1) + mean(dist2) of nn_distance(clouds1[i], clouds2[j]) for ALL pairs in ONE launch (the last
 * workgroup of every pair adds the workgroups' fixed-order partial sums; + a memset of the pairs' tickets).  clouds1 (n1, n, 3), clouds2 (n2, m, 3), cds (n1, n2),
 * all point-major fp32; the reference's per-i `expand + contiguous + nn_distance` loop (utils.py:104-107) and its
 * (N2, n) intermediates disappear.  Distances are those of dpf_nndistance (bit-exact minima); the means are summed
 * per 512-query workgroup, then in ascending tile order.  n, m >= 32; n1 <= 32767, n2 <= 65535.
 * A row-sharded evaluation passes its own rows of clouds1 and gathers the (rows, n2) blocks. */
size_t dpf_pairwise_cd_workspace_bytes(int n1, int n2, int n, int m);
int dpf_pairwise_cd(int n1, int n2, int n, int m, const float *clouds1, const float *clouds2, float *cds,
                    void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* The EMD half of _pairwise_EMD_CD_, lib/metrics/evaluation_metrics.py:85-121 (compute_all_metrics' three matrices,
 * :172-200): cost[i * n2 + j] = sum match * |x1 - x2| of the approximate matching of seta = clouds1[i], setb = clouds2[j] --
 * what dpf_approxmatch_cost_ws returns for that pair, NOT divided by n -- for all rows x n2 pairs in one call.  The reference's
 * per-i `expand + contiguous + match_cost` loop and its (b, m, n) matchings disappear: clouds1 (rows, n, 3) and clouds2
 * (n2, m, 3), point-major fp32, are read in place, and no matching is written anywhere (the last pass of either kernel family
 * only sums match * distance).  The pairs are the batch of dpf_approxmatch_ws's deferred path; each pair picks its kernel family
 * itself (matrix-core when its own two clouds are in range and finite, else packed-VALU), so an out-of-range or NaN cloud changes
 * only its own entries.  The slice counts depend on (n, m) alone: an entry has the same bits whichever rows / columns the call
 * covers (a row-sharded or chunked evaluation computes the same matrix).  dpf_emd_set_matrix_path(0) / DPF_EMD_MATRIX=0 apply
 * as to dpf_approxmatch_ws.  Tolerance class of dpf_approxmatch_cost_ws (cost 1e-4 against the reference's kernels).
 * rows * n2 <= 65535 (DPF_ENOSUP above: the caller chunks).  workspace: dpf_pairwise_emd_workspace_bytes bytes, caller-owned,
 * no state across calls -- dpf_approxmatch_workspace_bytes(rows * n2, n, m) + 8 (n + m) + 4 bytes per pair. */
size_t dpf_pairwise_emd_workspace_bytes(int rows, int n2, int n, int m);
int dpf_pairwise_emd(int rows, int n2, int n, int m, const float *clouds1, const float *clouds2, float *cost,
                     void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Per-point conditional affine-coupling flow (eval-mode BatchNorm), i.e.
 * LocalCondRNVPDecoder.forward (lib/networks/decoders.py:54-72) over
 * CondRealNVPFlow3D.forward (lib/networks/flows.py:95-117), F = 64.
 *
 * Weights arrive as one "canonical" fp32 block per coupling layer, layers in
 * DIRECT order (decoders.py:58-64).  dpf_flow_canon_floats(G) floats per layer:
 *
 *   for br in (logvar, mu):                               offsets in floats
 *     W0   [64][2]   sd0.weight, columns = the (up to) two keep channels,
 *                    zero column if the layer keeps one            flows.py:26/61
 *     BN0  gamma[64] beta[64] running_mean[64] running_var[64]     flows.py:27/62
 *     W1   [64][64]  sd1.weight                                    flows.py:29/64
 *     BN1  running_mean[64] running_var[64]  (affine=False)        flows.py:30/65
 *     W2   [2][64]   sd2.weight, rows = the (up to) two warp channels,
 *                    zero row if the layer warps one               flows.py:49/84
 *     b2   [4]       sd2.bias in [0..1], [2..3] unused
 *     for s in (w, b):                                             flows.py:33-45/68-80
 *       Wf0 [64][G]  film_{s}0.weight
 *       BNf gamma[64] beta[64] running_mean[64] running_var[64]
 *       Wf1 [64][64] film_{s}1.weight
 *       bf1 [64]     film_{s}1.bias
 *
 * meta: int32 [n_layers][4] = {keep_a, keep_b, warp_a, warp_b}, -1 = absent
 * (keep_inds / warp_inds of flows.py:17-23), device memory.
 * ------------------------------------------------------------------------ */

#define DPF_FLOW_F 64

/* precision of the 64x64 conditioner contraction on the matrix cores */
#define DPF_PREC_BF16   1  /* one bf16 MFMA product                      ~3e-3 rel */
#define DPF_PREC_BF16X3 2  /* hi/lo split, 3 bf16 MFMA products          ~1e-5 rel */
#define DPF_PREC_BF16X6 3  /* hi/mid/lo split, 6 bf16 MFMA products      fp32-class */
#define DPF_PREC_F16X3  4  /* hi/lo split in fp16 (11 + 11 bits), 3 MFMA products ~1e-6 rel; the activations'
                            * split costs 5 instead of 8 VALU per pair (v_cvt_pkrtz_f16_f32 + v_fma_mixlo/hi_f16).
                            * Hidden activations and W1 must stay below 65504 in magnitude (fp16 range). */

#define DPF_MODE_DIRECT  0 /* p_out = sqrt(eps+exp(logvar))*p + mu     flows.py:113 */
#define DPF_MODE_INVERSE 1 /* p_out = (p-mu)/sqrt(eps+exp(logvar))     flows.py:115 */

size_t dpf_flow_canon_floats(int G);
size_t dpf_flow_packed_bytes(int n_layers, int G, int precision);
size_t dpf_flow_film_floats(int n_layers, int B);

/* canonical fp32 weights -> `packed`: MFMA-fragment-ordered bf16 parts with
 * BatchNorm folded (dpf_flow_forward), followed by the transposed fp32
 * conditioner weights (dpf_flow_film).  Run once per weight version (not per
 * batch).  The film weights of the n_layers-layer prefix of a longer packed
 * buffer are NOT at the prefix's offset: pack a stack with the n_layers it
 * will be run with. */
int dpf_flow_pack(int n_layers, int G, int precision, const float *canon,
                  const int *meta, void *packed, dpf_stream_t stream);

/* per-cloud FiLM conditioner (flows.py:33-45,68-80,100-101,105-106) for every
 * layer at once: g (B, G) -> film (dpf_flow_film_floats floats). */
int dpf_flow_film(int n_layers, int B, int G, int precision, const void *packed,
                  const float *g, float *film, float flow_eps, dpf_stream_t stream);

/* The fused L-layer stack.  p_in / p_out / sum_logvar: (B, 3, N) fp32
 * channel-major as the networks use (flows.py:95).  Optional per-layer lists
 * ps / mus / logvars: (n_layers, B, 3, N) fp32 in DIRECT layer order for both
 * modes (decoders.py:61-70), or NULL to skip materialising them.
 * sum_logvar = sum over layers of logvar (what sum(logvars) gives
 * losses.py:13); may be NULL.  p_out_pointmajor: optional (B, N, 3) copy of
 * p_out in the layout the structural losses take (the
 * `.transpose(1, 2).contiguous()` of lib/networks/evaluating.py:110), or NULL. */
int dpf_flow_forward(int n_layers, int B, int N, int mode, int precision,
                     const void *packed, const int *meta, const float *film, const float *p_in,
                     float *p_out, float *p_out_pointmajor, float *sum_logvar,
                     float *ps, float *mus, float *logvars,
                     float flow_eps, dpf_stream_t stream);
/* dpf_flow_forward in direct mode with `reparameterize` (lib/networks/models.py:76-79, called at :212 / :118) fused into
 * the prologue: `noise` (B,3,N) is what torch.randn_like drew (the generator stream stays the caller's), the stack starts
 * from z = noise * exp(0.5 * lv0) + mu0 with mu0 / lv0 read through (batch, channel, point) element strides (the models'
 * stride-0 expansions, models.py:153-158 / 203-209); z_out (B,3,N, may be NULL) receives z = p_prior_samples[0]. */
int dpf_flow_forward_base(int n_layers, int B, int N, int precision, const void *packed, const int *meta,
                          const float *film, const float *noise, const float *mu0, long mu_sb, long mu_sc, long mu_sn,
                          const float *lv0, long lv_sb, long lv_sc, long lv_sn, float *z_out, float *p_out,
                          float *p_out_pointmajor, float *sum_logvar, float *ps, float *mus, float *logvars,
                          float flow_eps, dpf_stream_t stream);

/* Tiling of dpf_flow_forward / _base (results agree to rounding; both are held to the same goldens):
 * a wave owns 32 points (v_mfma_f32_32x32x16, csrc/flow.hip) or, for small per-GPU batches at f16x3 -- at most one tile per
 * SIMD of the chip, B * ceil(N / 16) <= 1024, e.g. the 4 clouds a rank of an 8-GPU job holds of BASELINE's 32 -- 16 points
 * (v_mfma_f32_16x16x32, csrc/flow16.hip).  mode: -1 = by size (default; env DPF_FLOW_TILE16), 0 = never, 1 = whenever
 * the precision allows.  Returns the previous mode.  Sets an atomic process default; meant for tests and tools.  A call in
 * flight keeps the value it read at entry. */
int dpf_flow_set_tile16(int mode);
long dpf_flow_tile16_launches(void);   /* calls of dpf_flow_forward / _base served by the 16-point kernel so far */

/* ---------------------------------------------------------------------------
 * Training mode (model.train()) of one coupling layer: batch-statistics
 * BatchNorm in both conditioner SharedDot stacks (flows.py:27,30,62,65), and the
 * backward pass autograd derives from CondRealNVPFlow3D.forward (flows.py:95-117;
 * lib/networks/training.py:55 calls loss.backward()).  precision: DPF_PREC_BF16X3 or
 * DPF_PREC_BF16X6 (of the forward contraction and its recomputation; see
 * csrc/flow_train.hip).
 *
 * tcanon, per layer dpf_flow_train_canon_floats() floats, per branch
 * (logvar, mu) 4484 floats:
 *     W0 [64][nk] @0 (sd0.weight as stored, nk = 1 or 2 keep channels, zeros up to 128)
 *     gamma0[64] @128   beta0[64] @192   W1[64][64] @256
 *     W2 [nw][64] @4352 (zeros up to 128)                b2[nw] @4480 (zeros up to 4)
 * -- every parameter tensor appears flattened exactly as PyTorch stores it, so the
 * block is one concatenation and its gradient splits into per-parameter slices
 * (BN1 is affine=False and the running statistics are not inputs in training mode).
 * dcanon has the same layout.
 *
 * fm / dfm: the FiLM vectors (cw, cb) of flows.py:100-101 / 105-106 that the
 * per-cloud conditioner nets produced for this batch, [branch][w|b][B][64];
 * those nets (B x 64 tensors) stay with the caller.
 *
 * film_l: dpf_flow_train_film_floats(B) floats; its first B*512 floats are the
 * block dpf_flow_forward(n_layers = 1, precision, packed = packed_l, film = film_l)
 * takes.
 * stats_l: dpf_flow_train_stats_floats() floats, [branch][6][64] =
 * mean0, rstd0, mean1, rstd1, unbiased batch var0, unbiased batch var1 (what
 * BatchNorm1d feeds its running statistics with), then 8 floats of input moments.
 * ------------------------------------------------------------------------ */
size_t dpf_flow_train_canon_floats(void);
size_t dpf_flow_train_packed_bytes(int n_layers, int precision);
size_t dpf_flow_train_stats_floats(void);
size_t dpf_flow_train_film_floats(int B);
size_t dpf_flow_train_workspace_bytes(int B, int N);

/* W1 / W1^T MFMA fragments of every layer (once per optimizer step) */
int dpf_flow_train_pack(int n_layers, int precision, const float *tcanon, void *packed,
                        dpf_stream_t stream);

/* Training-mode forward of an n_layers stack (layers in DIRECT order in every array; the mode
 * decides the order they run in).  meta_host / meta_dev: the int32 [n_layers][4] keep/warp table
 * in host and in device memory.  tcanon (L, canon_floats), packed (from dpf_flow_train_pack; the
 * input-layer fragments are completed here), fm (L,[branch][w|b][B][64]).  Outputs: ps / mus /
 * logvars (L,B,3,N) in DIRECT order, stats (L, stats_floats), film (L, film_floats(B)) -- stats,
 * film and packed are what the backward call needs back. */
int dpf_flow_train_forward(int n_layers, int B, int N, int mode, int precision,
                           const int *meta_host, const int *meta_dev, const float *tcanon,
                           void *packed, const float *fm, const float *p_in, float *ps, float *mus,
                           float *logvars, float *stats, float *film, float flow_eps,
                           void *workspace, dpf_stream_t stream);

/* Backward of the stack.  ps / mus / logvars: the forward call's three (L,B,3,N) outputs, unmodified (the
 * per-point mu and logvar of a layer are read back rather than recomputed).  g_ps / g_mus / g_lvs: (L,B,3,N)
 * gradients w.r.t. the three output lists (g_mus, g_lvs may be NULL = zero).  Overwrites dp_in (B,3,N),
 * dcanon (L, canon_floats) and dfm (L,[branch][w|b][B][64]); dp_tmp: (B,3,N) scratch. */
int dpf_flow_train_backward(int n_layers, int B, int N, int mode, int precision,
                            const int *meta_host, const float *tcanon, const void *packed,
                            const float *film, const float *stats, const float *p_in,
                            const float *ps, const float *mus, const float *logvars,
                            const float *g_ps, const float *g_mus,
                            const float *g_lvs, float *dp_in, float *dp_tmp, float *dcanon,
                            float *dfm, float flow_eps, void *workspace, dpf_stream_t stream);

/* The same with ONE (B,3,N) gradient pointer per layer and output list (host arrays of n_layers
 * device pointers): autograd produces a gradient per output tensor, and training.py's loss only
 * touches ps[0], mus[0] and the logvars, so nothing is stacked into (L,B,3,N) blocks and unused
 * outputs cost no memory traffic.  Any table, and any entry, may be NULL (zero gradient). */
int dpf_flow_train_backward_lists(int n_layers, int B, int N, int mode, int precision,
                                  const int *meta_host, const float *tcanon, const void *packed,
                                  const float *film, const float *stats, const float *p_in,
                                  const float *ps, const float *mus, const float *logvars,
                                  const float *const *g_ps,
                                  const float *const *g_mus, const float *const *g_lvs,
                                  float *dp_in, float *dp_tmp, float *dcanon, float *dfm,
                                  float flow_eps, void *workspace, dpf_stream_t stream);

/* ---------------------------------------------------------------------------
 * Eval mode (model.eval(), frozen BatchNorm) under autograd: the backward pass autograd derives from
 * CondRealNVPFlow3D.forward (flows.py:95-117) when the running statistics normalise (csrc/flow_frozen.hip).  The forward is
 * dpf_flow_film + dpf_flow_forward with the three per-layer lists, precision DPF_PREC_F16X3 (anything else: DPF_ENOSUP);
 * `packed` and `film` are the buffers those two calls used -- the backward recomputes each layer from its input with the
 * forward's own fragments, FiLM blocks and operand split, so the ReLU masks are the forward's.
 *
 * tcanon / dcanon: the training-mode block above (L, dpf_flow_train_canon_floats()); dcanon is fully overwritten (zeros in
 * the padding).  fstats: per layer dpf_flow_frozen_stats_floats() = 512 floats, per branch (logvar, mu)
 *     running_mean0[64] | running_var0[64] | running_mean1[64] | running_var1[64]
 * -- inputs, no gradient.  fm / dfm: the FiLM vectors (cw, cb) of this batch and their gradients, per layer
 * [branch][w|b][B][64]; the per-cloud conditioner nets stay with the caller (frozen BatchNorm there too).
 * p_in, ps, mus, logvars, the three gradient pointer tables (any table, any entry may be NULL), dp_in, dp_tmp: as
 * dpf_flow_train_backward_lists.  B >= 1.  Two launches per layer (the layer over its points; its partial rows -> dcanon, dfm),
 * none per stack, no statistic pass; every sum in a fixed order (no floating-point atomics): repeated calls agree bit for bit.
 * workspace: dpf_flow_frozen_workspace_bytes(B, N) bytes.  Joins the call-replay cache of the training entries.
 * ------------------------------------------------------------------------ */
size_t dpf_flow_frozen_stats_floats(void);
size_t dpf_flow_frozen_workspace_bytes(int B, int N);
int dpf_flow_frozen_backward_lists(int n_layers, int B, int N, int mode, int precision, const int *meta_host,
                                   const float *tcanon, const float *fstats, const void *packed, const float *film,
                                   const float *fm, const float *p_in, const float *ps, const float *mus,
                                   const float *logvars, const float *const *g_ps, const float *const *g_mus,
                                   const float *const *g_lvs, float *dp_in, float *dp_tmp, float *dcanon, float *dfm,
                                   float flow_eps, void *workspace, dpf_stream_t stream);

/* library identification: returns e.g. "dpf_hip gfx950 r1" */
const char *dpf_version(void);

/* ---- PointNet cloud encoder + max over the points (eval-mode BatchNorm) ---------------------
 * replaces PointNetCloudEncoder.forward (lib/networks/encoders.py:27-28) for the architecture
 * every config uses, SharedDot(no bias).BatchNorm1d.ReLU x 4 over 3 -> 64 -> 128 -> 256 -> 512
 * (encoders.py:15-25, configs pc_enc_*), together with the torch.max(features, dim=2)[0] the
 * models apply to it (lib/networks/models.py:85,131,175).
 *
 * canon: dpf_encoder_canon_floats() = 176 064 fp32, per layer l = 0..3
 *   W[cout][cin] (SharedDot.weight[0]) | bn.weight | bn.bias | bn.running_mean | bn.running_var.
 * dpf_encoder_pack folds BatchNorm and lays the weights out as bf16 MFMA fragments (once per weight
 * version and precision) into `packed` (dpf_encoder_packed_bytes(precision)).
 * dpf_encoder_forward: x (B,3,N) channel-major -> gmax (B,512) fully overwritten; feat, when not
 * NULL, also receives the per-point features (B,512,N) (what the module's forward returns). */
size_t dpf_encoder_canon_floats(void);
size_t dpf_encoder_packed_bytes(int precision);
int dpf_encoder_pack(int precision, const float *canon, void *packed, dpf_stream_t stream);
int dpf_encoder_forward(int B, int N, int precision, const void *packed, const float *x,
                        float *gmax, float *feat, dpf_stream_t stream);

/* ---- PointNet cloud encoder, EVAL mode under autograd (frozen BatchNorm): forward with the argmax, and the backward ----
 * dpf_encoder_forward_arg: dpf_encoder_forward (no feature output) that also yields arg (B,512) int32, the point that attains
 *   each pooled value.  gmax is bit-identical to dpf_encoder_forward on the same inputs; arg[b,f] is the LOWEST point whose
 *   layer-3 value equals the maximum; for a dead feature (gmax == 0) it is some point of the cloud.  One launch after the
 *   zero fill of `scratch` (dpf_encoder_arg_scratch_bytes(B) bytes, 8-byte aligned, caller-owned): a 64-bit integer atomic
 *   max per (cloud, feature) on (value bits << 32) | (0xFFFFFFFF - point), unpacked by the workgroup that arrives last at the
 *   cloud's ticket -- order-independent, no floating-point atomics.  DPF_PREC_BF16X3 and DPF_PREC_BF16X6 (DPF_PREC_BF16:
 *   DPF_ENOSUP); B <= 65535.
 * dpf_encoder_frozen_backward: the backward of  pooled = max over the points of the eval-mode encoder  (running statistics;
 *   what autograd derives from lib/networks/encoders.py:15-28 + models.py:106,124 under model.eval()).  canon: the block
 *   `packed` was made from (dpf_encoder_pack, same precision); x, pooled, arg: the input and outputs of
 *   dpf_encoder_forward_arg; g_pooled (B,512) = d loss / d pooled.  -> dcanon (optional; canon layout: dW, d gamma, d beta per
 *   layer, the running-statistics slots are left untouched) and dx (optional; (B,3,N), fully written: zero away from the
 *   argmax points); at least one of the two.  workspace: dpf_encoder_frozen_workspace_bytes(B) bytes, 16-byte aligned:
 *   1.84 MB per cloud (59 MB at B = 32).  B <= 65535 is accepted as in the forward; in practice the workspace bounds B
 *   (7.5 GB at B = 4096).
 *   The work is B * 512 points whatever N is; 4 launches for dcanon, 6 with dx, whatever B and N are; no atomics, every sum in
 *   an order fixed by the shapes (bit-reproducible).  The BatchNorm statistics are only read.  B = 1 and N = 1 are legal. */
size_t dpf_encoder_arg_scratch_bytes(int B);
int dpf_encoder_forward_arg(int B, int N, int precision, const void *packed, const float *x, float *gmax, int *arg,
                            void *scratch, dpf_stream_t stream);
size_t dpf_encoder_frozen_workspace_bytes(int B);
int dpf_encoder_frozen_backward(int B, int N, int precision, const float *canon, const void *packed, const float *x,
                                const float *pooled, const int *arg, const float *g_pooled, float *dcanon, float *dx,
                                void *workspace, dpf_stream_t stream);

/* ---- PointNet cloud encoder, TRAINING mode (batch-statistics BatchNorm) + max over the points, and backward ----
 * replaces, under model.train(), PointNetCloudEncoder.forward (lib/networks/encoders.py:27-28) followed by
 * torch.max(features, dim=2)[0] (lib/networks/models.py:131), and the gradients autograd derives for the
 * encoder's parameters (lib/networks/training.py:55).  precision: DPF_PREC_BF16X6 or DPF_PREC_BF16X3 for the
 * forward contractions (they decide the ReLU masks and the argmax); gradient contractions are bf16x3; fp32
 * accumulation; every reduction in a fixed order (deterministic).
 *
 * canon: the block of dpf_encoder_forward (running_mean / running_var slots are not read).
 * ws: dpf_encoder_train_workspace_bytes(B, N) bytes; the forward pass leaves the pre-BatchNorm activations,
 *   the batch statistics and the argmax there, the backward pass of the SAME step reads them.
 * forward: x (B,3,N) -> pooled (B,512).  batch_stats (optional, 2 * 960 floats): per layer mean[C] | biased
 *   var[C], layers in order.  running (optional): HOST array of 8 DEVICE pointers running_mean_0,
 *   running_var_0, ... updated in place as torch.nn.BatchNorm1d does with `momentum` (unbiased variance).
 *   B * N must be >= 2.
 * backward: g_pooled (B,512) = d loss / d pooled, pooled = the forward's output -> dcanon (canon layout: dW,
 *   d gamma, d beta per layer; the running-statistics slots are left untouched); dx (optional, (B,3,N)) = d loss / d x. */
size_t dpf_encoder_train_workspace_bytes(int B, int N);
int dpf_encoder_train_forward(int B, int N, int precision, const float *canon, const float *x, void *ws, float *pooled,
                              float *batch_stats, float *const *running, float momentum, dpf_stream_t stream);
int dpf_encoder_train_backward(int B, int N, const float *canon, const float *x, void *ws, const float *pooled,
                               const float *g_pooled, float *dcanon, float *dx, dpf_stream_t stream);

/* The training-mode entry points (dpf_flow_train_forward / _backward[_lists], dpf_encoder_train_forward / _backward) issue
 * hundreds of small dependent launches per call; a call whose scalars AND pointers have been seen twice is recorded once
 * (stream capture) and from then on replayed as one hipGraph -- a training loop presents the same addresses every step.
 * A replay needs the stored key bytes to match, not only their hash.  Only kernel nodes are recorded (no memset nodes).
 * DPF_TRAIN_GRAPH=0 in the environment switches that off; dpf_train_graph_set_enabled(on) does so at run time and returns
 * the previous state.  dpf_train_graph_replays(): calls served by a replay so far.  dpf_train_graph_stats(out[5]):
 * {replays, eager calls, recordings, evictions, keys that could not be captured} -- evictions growing while replays stand
 * still means the loop presents more than 8 live pointer sets per entry point, or its allocator does not settle. */
/* Test hook of the matrix-core Chamfer filter (csrc/chamfer_mfma.hip): the surrogate s(q, c) = |c - mu|^2 - 2 (q - mu).(c - mu)
 * of every pair of ONE pair of clouds ((nq, 3) queries, (nc, 3) candidates), formed exactly as the filter forms it; s is
 * (nq, nc) floats, out4 = {mu_x, mu_y, mu_z, R2}.  The filter's exactness rests on |s - exact| <= 2^-14 R2. */
int dpf_debug_nn_surrogate(int nq, const float *q, int nc, const float *c, float *s, float *out4, dpf_stream_t stream);
/* Test hook of the matrix-core approx-EMD passes (csrc/emd.hip): out (m, n) = the exp2 arguments -4^j log2(e) |xyz2_l - xyz1_k|^2
 * of ONE cloud pair at annealing level j (7 .. -1), formed exactly as the passes form them (same records, level vectors and
 * MFMAs); meta8 (8 device floats or NULL) = {centroid xyz, out-of-range flag (then `out` is untouched), 2^g, T, 0, 0}.
 * Workspace as for dpf_approxmatch_ws(1, n, m). */
int dpf_debug_emd_exponents(int n, int m, const float *xyz1, const float *xyz2, int level_j, float *out, float *meta8,
                            void *workspace, size_t workspace_bytes, dpf_stream_t stream);
long dpf_train_graph_replays(void);
/* Workgroups of the training backward pass that gave up waiting for role workgroups of their own launch (pass 1: the column sums
 * of the layer above; pass 2, small batches: the per-cloud totals and BatchNorm-backward means of pass 1) and did the sums
 * themselves -- process-wide.  0 as long as the role workgroups, placed first in the grid, are dispatched first. */
long dpf_train_colsum_fallbacks(void);
void dpf_train_graph_stats(long *out);
int dpf_train_graph_set_enabled(int on);
/* Diagnostics: per-kernel time of the training stack's launches.  (1, NULL, NULL) starts collecting -- every launch of the
 * per-layer kernels is bracketed by HIP events on its stream; graph recording / replay is off while it collects --,
 * (0, us[8], calls[8]) synchronises the device, returns the summed time in microseconds and the number of launches per kernel
 * id and stops.  ids: 0 tstats_x, 1 tstats_h1, 2 tfold, 3 flow_kernel (L = 1), 4 tbwd1, 5 tbwd2, 6 tcolsum, 7 tbwd3f. */
int dpf_train_kernel_times(int enable, double *us_out, long *calls_out);

/* ---- fused AMSGrad-Adam step over one flat fp32 buffer -----------------------------------------
 * replaces the per-parameter update of the reference's optimizer, lib/networks/optimizers.py:52-74 (state['step'] and the
 * bias corrections :48, :63-64 stay with the caller): exp_avg / exp_avg_sq / max_exp_avg_sq / p updated in place in ONE pass,
 * with the roundings of the reference's op sequence as PyTorch-ROCm executes it (bit-identical, csrc/adam.hip).
 * max_exp_avg_sq = NULL: plain Adam (:59).  The hyper-parameters are the Python doubles of the parameter group;
 * bias_correction1 = 1 - beta1^step, bias_correction2 = sqrt(1 - beta2^step) (both non-zero).  Buffers 16-byte aligned. */
int dpf_adam_step(size_t n, float *p, const float *g, float *exp_avg, float *exp_avg_sq, float *max_exp_avg_sq, double lr,
                  double beta1, double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2,
                  dpf_stream_t stream);

/* ---- latent prior flow: GlobalRNVPDecoder on (B, G) codes, eval-mode BatchNorm ---------------
 * replaces GlobalRNVPDecoder.forward (lib/networks/decoders.py:21-38): n_steps = 2 * n_flows
 * RealNVPFlow steps (lib/networks/flows.py:198-213) in ONE launch, both modes.
 *
 * codes (HOST array, n_steps ints): which coordinates a step warps -- RealNVPFlowCouple's
 * patterns (flows.py:224-233): 0 even, 1 odd, 2 first half, 3 second half; G must be even.
 * canon: per step dpf_gprior_canon_floats(G, n_features) fp32, for T in (mu, logvar), K = G/2:
 *   mlp0.weight [n_features][K] | bn.weight | bn.bias | bn.running_mean | bn.running_var |
 *   mlp1.weight [K][n_features] | mlp1.bias [K]                      (flows.py:176-196).
 * dpf_gprior_pack folds BatchNorm and transposes the weights (once per weight version).
 * dpf_gprior_forward: g (B,G) -> gs, mus, lvs (n_steps,B,G) in DIRECT order whatever the mode
 * (mu / logvar zero on a step's kept coordinates, as the reference's lists), sum_lv (B,G) the sum of
 * the logvars over the steps, g_out (B,G) the end of the chain (gs[n_steps-1] direct, gs[0]
 * inverse); every output may be NULL.  eps: RealNVPFlow's logvar floor (flows.py:164,201). */
size_t dpf_gprior_canon_floats(int G, int n_features);
size_t dpf_gprior_packed_floats(int n_steps, int G, int n_features);
int dpf_gprior_pack(int n_steps, int G, int n_features, float bn_eps, const float *canon,
                    float *packed, dpf_stream_t stream);
int dpf_gprior_forward(int n_steps, int B, int G, int n_features, int mode, const int *codes,
                       const float *packed, const float *g, float *gs, float *mus, float *lvs,
                       float *sum_lv, float *g_out, float eps, dpf_stream_t stream);

/* ---- PointFlowNLL (lib/networks/losses.py:11-15) in one pass ---------------------------------
 * out[0] = 0.5 * ( sum_{b,c,n} [ sum_lv + lv0 + (s0 - mu0)^2 / exp(lv0) ] / B + log(2 pi) * C * N ).
 * s0 (B,C,N) contiguous: the cloud at the base of the flow (samples[0]); sum_lv (B,C,N) contiguous or
 * NULL: the flow's summed log-variances (dpf_flow_forward's sum_logvar); mu0 / lv0: the base
 * distribution (mus[0], logvars[0]) read through element strides (batch, channel, point) -- the
 * reference's stride-0 expansions (models.py:108-117) are never materialised.  Deterministic.
 * workspace: dpf_pointflow_nll_workspace_floats() fp32. */
size_t dpf_pointflow_nll_workspace_floats(void);
int dpf_pointflow_nll(int B, int C, int N, const float *s0, const float *mu0, long mu_sb, long mu_sc,
                      long mu_sn, const float *lv0, long lv_sb, long lv_sc, long lv_sn,
                      const float *sum_lv, float *workspace, float *out, dpf_stream_t stream);
/* Backward of dpf_pointflow_nll for a scalar upstream gradient grad_out[0] (device): d_s0 and d_sum_lv (B,C,N)
 * contiguous, and -- when non-NULL -- d_mu0 / d_lv0 as full (B,C,N) tensors (the caller's expand-backward reduces
 * them); any output pointer may be NULL.  One launch; with it the flow NLL of a training step (losses.py:48) is a single
 * autograd node over HIP kernels. */
int dpf_pointflow_nll_backward(int B, int C, int N, const float *s0, const float *mu0, long mu_sb, long mu_sc,
                               long mu_sn, const float *lv0, long lv_sb, long lv_sc, long lv_sn,
                               const float *grad_out, float *d_s0, float *d_sum_lv, float *d_mu0, float *d_lv0,
                               dpf_stream_t stream);

/* ---- latent prior flow, TRAINING mode (BatchNorm1d on the statistics of the B rows) -----------
 * replaces GlobalRNVPDecoder.forward under model.train() (decoders.py:21-38, flows.py:198-213)
 * and the backward autograd derives from it; 4 launches per step forward, 5 backward, all issued
 * by the one call.  canon: the UNPACKED canonical block of dpf_gprior_pack (the running statistics
 * in it are not read) when params_only == 0; with params_only != 0 the same without the two
 * running-statistics vectors of each net (W0 | bn.weight | bn.bias | W1 | b1: what an optimizer
 * updates, so a caller can keep all parameters in one buffer of exactly this layout and all
 * gradients in its twin).  codes, mode, eps as dpf_gprior_forward; B >= 2.
 * forward: g (B,G) -> gs, mus, lvs (S,B,G) DIRECT order, all required; save_h (S,B,2*n_features)
 *   the pre-BatchNorm activations and save_stats (S,2,2*n_features) = batch mean | biased variance per
 *   hidden unit (mu net, then logvar net) -- for the backward and for the caller's running-statistics
 *   update (nn.BatchNorm1d: momentum 0.1, unbiased variance).
 * backward: d_gs, d_mus, d_lvs (S,B,G) or NULL -> dg (B,G) and dcanon (same layout as canon: weight,
 *   BatchNorm affine and bias gradients, zeros in the running-statistics slots), both overwritten.
 * workspace: dpf_gprior_train_workspace_floats(B, G, n_features) fp32. */
size_t dpf_gprior_train_workspace_floats(int B, int G, int n_features);
int dpf_gprior_train_forward(int n_steps, int B, int G, int n_features, int mode, const int *codes,
                             int params_only, const float *canon, const float *g, float *gs, float *mus, float *lvs,
                             float *save_h, float *save_stats, float *workspace, float bn_eps,
                             float eps, dpf_stream_t stream);
int dpf_gprior_train_backward(int n_steps, int B, int G, int n_features, int mode, const int *codes,
                              int params_only, const float *canon, const float *g, const float *gs, const float *mus,
                              const float *lvs, const float *save_h, const float *save_stats,
                              const float *d_gs, const float *d_mus, const float *d_lvs, float *dg,
                              float *dcanon, float *workspace, float bn_eps, float eps,
                              dpf_stream_t stream);

/* ---- latent prior flow, EVAL mode under autograd (FROZEN BatchNorm: the running statistics) ----
 * the backward of GlobalRNVPDecoder.forward under model.eval() (decoders.py:21-38, flows.py:198-243): the forward is
 * dpf_gprior_forward itself, this call differentiates it in TWO launches whatever n_steps (a row-parallel walk of the steps
 * in reverse, then every parameter gradient as a fixed-order sum over the rows; no atomics: bit-reproducible).
 * n_steps, B, G, n_features, mode, codes, eps as dpf_gprior_forward; B >= 1 (B == 0: returns 0, nothing written).
 * canon: the parameters in either layout of dpf_gprior_train_* -- params_only == 0: the canonical block of dpf_gprior_pack,
 *   whose running statistics are read (stats is ignored, may be NULL); params_only != 0: W0 | bn.weight | bn.bias | W1 | b1
 *   per net, and stats (n_steps, 2 nets, 2, n_features) = running_mean | running_var of every net (mu net, then logvar net).
 * g (B,G) and the forward's gs, mus, lvs (n_steps,B,G); d_gs, d_mus, d_lvs (n_steps,B,G), each may be NULL (= zeros).
 * -> dg (B,G) and dcanon (the layout of canon; zeros in any running-statistics slot), both overwritten.
 * workspace: dpf_gprior_frozen_workspace_floats(n_steps, B, G, n_features) fp32, caller-owned; the call never allocates or
 * synchronises.  Bad arguments (odd G, unknown step code, B < 0, a missing required pointer) return DPF_EINVAL and launch nothing. */
size_t dpf_gprior_frozen_workspace_floats(int n_steps, int B, int G, int n_features);
int dpf_gprior_frozen_backward(int n_steps, int B, int G, int n_features, int mode, const int *codes,
                               int params_only, const float *canon, const float *stats, float bn_eps, float eps,
                               const float *g, const float *gs, const float *mus, const float *lvs,
                               const float *d_gs, const float *d_mus, const float *d_lvs, float *dg,
                               float *dcanon, float *workspace, dpf_stream_t stream);

/* BatchNorm running statistics after a training-mode forward (nn.BatchNorm1d: running = (1 - momentum) * running +
 * momentum * batch, unbiased batch variance; lib/networks/flows.py:27,30,35,42 in train()): all 8 n_layers BatchNorm1d layers
 * of the stack in one launch.  running_mean / running_var (8 n_layers, 64) and num_batches_tracked (8 n_layers, int64): rows
 * [0, 4 n_layers) the FiLM nets in (layer, branch, w|b) order with batch statistics film_mean / film_uvar (4 n_layers, 64),
 * rows [4 n_layers, 8 n_layers) BN0, BN1 of (layer, branch) from the `stats` block of dpf_flow_train_forward. */
int dpf_flow_train_update_running(int n_layers, double momentum, const float *film_mean, const float *film_uvar,
                                  const float *stats, float *running_mean, float *running_var,
                                  long long *num_batches_tracked, dpf_stream_t stream);

/* ---- FiLM conditioner nets of the coupling stack, training mode (csrc/film_train.hip) ---------------------
 * Replaces, for model.train(), the K = 4 n_layers per-cloud conditioner sub-nets of CondRealNVPFlow3D
 * (lib/networks/flows.py:33-45, 68-80: Linear(G, 64, bias=False) . BatchNorm1d over the B clouds . Swish . Linear(64, 64))
 * and what autograd derives from them (lib/networks/training.py:55) -- ~12 tensor-op launches forward and ~25 backward per
 * optimizer step in the reference's formulation, ONE launch each way here.  All arrays fp32, contiguous:
 *   g (B, G); W0 (K, 64, G); gamma, beta (K, 64); W1 (K, 64, 64) [out][in]; b1 (K, 64)
 * forward:  fm (K, B, 64) = the stack's conditioner input (dpf_flow_train_forward's `fm`); saved for the backward: xhat
 *   (K, B, 64) and rstd (K, 64); mean / uvar (K, 64) = batch mean and UNBIASED batch variance for the running-statistics
 *   update (nn.BatchNorm1d, momentum 0.1).
 * backward: dfm (K, B, 64) -> dW0 (K, 64, G), dgamma, dbeta (K, 64), dW1 (K, 64, 64), db1 (K, 64): overwritten, or added to
 *   (accumulate != 0: the flat gradient store); dg_part (K, B, G) or NULL: every sub-net's share of d loss / d g (the caller
 *   sums over K).  B <= dpf_film_train_max_batch() and G % 4 == 0, else DPF_ENOSUP (the caller keeps the tensor ops). */
int dpf_film_train_max_batch(void);
int dpf_film_train_forward(int K, int B, int G, const float *g, const float *W0, const float *gamma, const float *beta,
                           const float *W1, const float *b1, float bn_eps, float *fm, float *xhat, float *rstd,
                           float *mean, float *uvar, dpf_stream_t stream);
int dpf_film_train_backward(int K, int B, int G, const float *g, const float *W0, const float *gamma, const float *beta,
                            const float *W1, const float *xhat, const float *rstd, const float *dfm, float *dW0,
                            float *dgamma, float *dbeta, float *dW1, float *db1, float *dg_part, int accumulate,
                            dpf_stream_t stream);

/* The same K conditioner nets in eval mode under autograd (frozen BatchNorm: y = (u - running_mean) * rstd * gamma + beta with
 * rstd = 1 / sqrt(running_var + bn_eps); csrc/film_train.hip, frozen variants of the two kernels above), the companions of
 * dpf_flow_frozen_backward_lists.  One launch each way; B >= 1; B <= dpf_film_train_max_batch() and G % 4 == 0, else DPF_ENOSUP
 * (the caller keeps the tensor ops).  running_mean / running_var (K, 64) are inputs and receive no gradient.
 * forward:  fm (K, B, 64); saved for the backward: xhat (K, B, 64) and rstd (K, 64).
 * backward: as dpf_film_train_backward without the two mean-correction terms (d u = rstd * gamma * d y), and with d g FINISHED
 *   in the launch: dg (B, G) or NULL = the sum of the sub-nets' shares over k = 0 .. K - 1 in that order, formed by the workgroup
 *   that arrives last (no floating-point atomics: repeated calls agree bit for bit).  workspace: dpf_film_frozen_workspace_floats
 *   floats; ticket: one 32-bit word of device memory that is ZERO before the first call and is left zero by every call (calls
 *   that share it must be ordered on one stream).  Both may be NULL when dg is. */
int dpf_film_frozen_forward(int K, int B, int G, const float *g, const float *W0, const float *gamma, const float *beta,
                            const float *W1, const float *b1, const float *running_mean, const float *running_var,
                            float bn_eps, float *fm, float *xhat, float *rstd, dpf_stream_t stream);
size_t dpf_film_frozen_workspace_floats(int K, int B, int G);
int dpf_film_frozen_backward(int K, int B, int G, const float *g, const float *W0, const float *gamma, const float *beta,
                             const float *W1, const float *xhat, const float *rstd, const float *dfm, float *dW0,
                             float *dgamma, float *dbeta, float *dW1, float *db1, float *dg, float *workspace,
                             unsigned *ticket, int accumulate, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Occupancy grids of the two Jensen-Shannon metrics (csrc/occupancy.hip): every point of the (S, n, 3) point-major fp32
 * clouds is put into one cell of a res^3 grid; counts[cell] = points, clouds_touching[cell] = clouds with at least one
 * point there.  Integer atomics: exact and independent of order.  All three outputs are zeroed by the call.
 *   mode 0, cube bins (lib/networks/utils.py:45-80): the voxel of a coordinate x is the i with edges[i] <= x < edges[i+1],
 *     compared in double against the caller's table of res + 1 edges; cell = (ix * res + iy) * res + iz.  A point with a
 *     coordinate outside every interval, or NaN, is not counted.  centres / kept / kept_xyz are unused (kept must be NULL).
 *   mode 1, nearest centre (lib/metrics/evaluation_metrics.py:241-280): cell = the argmin over the K kept centres of
 *     (dx*dx + dy*dy) + dz*dz in double (the fp32 inputs widened), the lowest kept index on an exact tie.  centres: the res
 *     per-axis centre values, increasing; kept: (res^3) full-grid cell -> kept index or -1, increasing over the kept cells,
 *     or NULL for the full grid (then K = res^3); kept_xyz: (K, 3) the kept centres, each coordinate one of `centres`.
 *     A point with a NaN or infinite coordinate is not counted.
 * flags: 4 words -- [0] points with a non-finite coordinate, [1] NaN coordinates, [2] nonzero if some |coordinate| >
 * warn_bound, [3] unused.  res <= the value the max_res query returns (the per-cloud presence bitmap lives in LDS), else
 * DPF_ENOSUP.  workspace: the workspace_bytes query's size (nonzero only for clouds long enough to be split over several
 * workgroups); S and n are unbounded, the call chunks its launches. */
int dpf_occupancy_max_res(void);
size_t dpf_occupancy_grid_workspace_bytes(int S, int n, int res);
int dpf_occupancy_grid(int S, int n, const float *clouds, int res, int mode, const double *edges, const float *centres,
                       const int *kept, const float *kept_xyz, int K, float warn_bound, unsigned long long *counts,
                       unsigned int *clouds_touching, unsigned int *flags, void *workspace, size_t workspace_bytes,
                       dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Mesh surface sampling into the collated training batch (csrc/mesh_sample.hip; lib/datasets/cloud_sampling.py:4-32 and the
 * elementwise transforms of lib/datasets/cloud_transformations.py).  The mesh store, all device memory, mirrors meshes.h5:
 * vertices (sum V, 3) fp32, faces (sum F, 3) uint32 with indices LOCAL to their mesh, vertex_bounds / face_bounds of M + 1
 * increasing int64 entries starting at 0; every mesh has at least one face and fewer than 2^31.
 *   dpf_mesh_cdf_build: cdf (sum F) doubles, flags (M) words.  Face area in fp32 as numpy forms it (e1 = p2 - p0, e2 = p2 - p1,
 *     cross product as a product minus a product, sqrt((c0*c0 + c1*c1) + c2*c2) / 2, nothing fused).  cdf[f] of mesh m =
 *     (sum of its faces 0..f) / (sum of all its faces) in double, summed in tiles of dpf_mesh_cdf_tile() faces counted from
 *     the mesh's first face: inside a tile one after the other in face order, the tile totals one after the other, edge =
 *     (tile offset + sum inside the tile) / total.  The bits depend on the mesh alone; the edges never decrease and the last is 1.
 *     tile_bounds: (M + 1) int64, tile_bounds[m + 1] - tile_bounds[m] = ceil(F_m / tile); n_tiles = tile_bounds[M].
 *     flags[m]: bit 0 a face index >= V_m (the vertex is not read), bit 1 a non-finite area, bit 2 a total of zero; such faces
 *     count as area 0 and the cdf of a flagged mesh is zeroed.  workspace: the workspace_bytes query, 8-byte aligned; free
 *     after the call's work has run.  The caller reads flags back once -- the store's only synchronisation.
 *   dpf_mesh_variates: u (B, S) double with 53 random bits, s1 / s2 (B, S) fp32 = the double uniform rounded to fp32, from
 *     splitmix64 keyed by (seed, step, slot, sample, stream): base = mix(mix(seed) ^ step), slot key = mix(base ^ b),
 *     bits = mix(slot key ^ (4 * i + stream)), uniform = (bits >> 11) * 2^-53.  Equal meshes in two slots draw different streams.
 *   dpf_mesh_sample: B slots of S samples; mesh_idx (B) int32.  face = the first k with cdf[k] > u (searchsorted side='right');
 *     if (s1 + s2 > 1) { s1 = 1 - s1; s2 = 1 - s2; }; point = (p0 + s1 * (p1 - p0)) + s2 * (p2 - p0); then, by the bits of
 *     xform: 1 `orig_s[m] * x`, 2 `+ orig_c[m][axis]`, 4 `- shift[axis]`, 8 `/ scale` -- all fp32, each rounded on its own.
 *     split = 0: cloud (B, 3, S).  split = 1 (S even): even samples to cloud, odd ones to eval_cloud, each (B, 3, S / 2).
 *     faces_out: optional (B, S) int32.  u must lie in [0, 1).  A slot whose mesh index is outside the store or whose mesh is
 *     flagged reads nothing of the mesh: NaN points, face -1.  Launches on the caller's stream, never synchronises; B and S are
 *     chunked over launches. */
int dpf_mesh_cdf_tile(void);
size_t dpf_mesh_cdf_workspace_bytes(int M, long n_tiles);
int dpf_mesh_cdf_build(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                       const long *face_bounds, const long *tile_bounds, long n_tiles, double *cdf, unsigned int *flags,
                       void *workspace, size_t workspace_bytes, dpf_stream_t stream);
int dpf_mesh_variates(int B, int S, unsigned long long seed, unsigned long long step, double *u, float *s1, float *s2,
                      dpf_stream_t stream);
int dpf_mesh_sample(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                    const long *face_bounds, const double *cdf, const unsigned int *flags, const float *orig_c,
                    const float *orig_s, int B, int S, const int *mesh_idx, const double *u, const float *s1,
                    const float *s2, int split, int xform, float shift_x, float shift_y, float shift_z, float scale,
                    float *cloud, float *eval_cloud, int *faces_out, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Point-to-mesh distance over the same mesh store (csrc/point_mesh.hip): the exact squared distance from every query point to
 * the surface it is measured against.  points (B, N, 3) fp32, point-major; slot b queries mesh mesh_idx[b] (int32, device);
 * vertices / vertex_bounds / faces / face_bounds / flags are the arrays dpf_mesh_sample takes (flags as dpf_mesh_cdf_build
 * left them).  Outputs: dist (B, N) fp32 = min over the mesh's faces of the squared distance to the closed triangle; face
 * (B, N) int32 = the mesh-local index of a face attaining it; closest (B, N, 3) fp32, optional (NULL: not written) = the
 * closest point on that face.
 *   The arithmetic of one (point p, face (a, b, c)) pair is ONE fp32 sequence, the same in every kernel form; fma(x, y, z) is
 *   the fused operation, dot(x, y) = fma(x2, y2, fma(x1, y1, x0 * y0)), everything else rounds on its own.
 *   Per face: ab = b - a, ac = c - a, aa = dot(ab, ab), g = dot(ab, ac), cc = dot(ac, ac), bb = dot(ac - ab, ac - ab),
 *     det = fma(aa, cc, -(g * g)); iaa = aa > 0 ? 1 / aa : 0, icc and ibc likewise from cc and bb (correctly rounded divisions);
 *     the face is THIN when !(det > 2^-14 * (aa * cc)), else idet = 1 / det.
 *   Per pair: ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = d1 - aa, d4 = d2 - g, d5 = d1 - g, d6 = d2 - cc,
 *     tab = clamp01(d1 * iaa), tac = clamp01(d2 * icc), tbc = clamp01((d4 - d3) * ibc)  (clamp01(x) = min(max(x, 0), 1), NaN -> 0).
 *     Ericson's regions (Real-Time Collision Detection 5.1.5), first match: corner A (d1 <= 0 and d2 <= 0): (v, w) = (0, 0);
 *     corner B (d3 >= 0 and d4 <= d3): (1, 0); edge AB (vc <= 0, d1 >= 0, d3 <= 0): (tab, 0); corner C (d6 >= 0 and d5 <= d6):
 *     (0, 1); edge AC (vb <= 0, d2 >= 0, d6 <= 0): (0, tac); edge BC (v0 + w0 >= 1, d4 - d3 >= 0, d5 - d6 >= 0): (1 - tbc, tbc);
 *     else the interior (v0, w0) -- with vb = fma(cc, d1, -(g * d2)), vc = fma(aa, d2, -(g * d1)), v0 = vb * idet, w0 = vc * idet.
 *     Then v = clamp01(v), w = min(max(w, 0), 1 - v); q = fma(w, ac, fma(v, ab, a)) per axis; dist = dot(p - q, p - q).
 *     No division per pair.  A THIN face -- zero area, repeated vertices, or a sliver whose determinant is mostly rounding -- is
 *     the nearest of its three edges instead: (tab, 0), then (0, tac), then (1 - tbc, tbc), a later one only if strictly nearer;
 *     an edge without length is its point.  No face yields NaN for finite input.  (A sliver just above the threshold carries the
 *     interior solve's conditioning, a relative error of about 2^-23 / (det / (aa * cc)) in (v, w); DESIGN.md.)
 *   Ties: among faces of equal fp32 distance the LOWEST index is reported -- the minimum of (distance bits << 32 | face) as
 *     unsigned 64-bit keys.  dist, face and closest are bit-identical from run to run, do not depend on B, on the slot a cloud
 *     sits in or on how faces and points are spread over workgroups and launches, and are the same in both kernel forms.
 *   A slot whose mesh index is outside [0, M) or whose mesh is flagged reads nothing of the mesh: dist NaN, face -1, closest NaN.
 *     A non-finite query point gives NaN / -1 for that point alone.  (Finite coordinates whose squares overflow fp32 are outside
 *     the contract.)  A face index >= V_m flags its mesh in dpf_mesh_cdf_build, so no vertex outside the mesh is ever read.
 *   max_faces: the largest face count among the meshes queried (host knowledge, >= 1) -- it only sizes the launch; a wrong
 *     value costs time, never correctness.  form: 0 = by size (dispatch.h: pm_form), 1 = every workgroup walks all faces of its
 *     slot's mesh in tiles of dpf_point_mesh_tile() faces, 2 = the tiles are also split over workgroups, merged by a 64-bit
 *     atomic minimum into workspace (dpf_point_mesh_workspace_bytes(B, N) bytes, 8-byte aligned; only read or written when the
 *     split form runs) and unpacked by a finishing launch.
 *   Launches on the caller's stream, never synchronises, no memset nodes; B = 0 or N = 0 launches nothing; B and N are chunked
 *     over launches.
 *   dpf_point_mesh_distance_grad: grad_points (B, N, 3) = 2 * grad_dist * (points - closest), one launch; 0 where closest is NaN
 *     (the points whose dist is NaN).  The mesh is data: there is no gradient with respect to vertices. */
int dpf_point_mesh_tile(void);
size_t dpf_point_mesh_workspace_bytes(int B, int N);
int dpf_point_mesh_distance(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                            const long *face_bounds, const unsigned int *flags, int B, int N, const float *points,
                            const int *mesh_idx, long max_faces, int form, float *dist, int *face, float *closest,
                            void *workspace, size_t workspace_bytes, dpf_stream_t stream);
int dpf_point_mesh_distance_grad(int B, int N, const float *points, const float *closest, const float *grad_dist,
                                 float *grad_points, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Mesh-to-cloud distance over the same mesh store (csrc/mesh_point.hip): the other direction -- for every FACE of a slot's mesh
 * the nearest of the slot's points; the column minimum of the (point, face) matrix whose row minimum dpf_point_mesh_distance
 * returns.  Store arrays, points (B, N, 3), mesh_idx (B), max_faces, form, workspace and stream as there.  W = max_faces is the
 * width of the outputs: dist (B, W) fp32 = for face f of slot b's mesh the minimum over that slot's points of the pair's squared
 * distance; point (B, W) int32 = the index of a point attaining it; closest (B, W, 3) fp32, optional (NULL: not written) = the
 * closest point on the face to that point; area (B, W) fp32, optional = the face's area.
 *   Pair arithmetic: the sequence stated above, defined once (csrc/pm_pair.h) and included by both translation units; a pair has
 *     the same bits in both directions.
 *   Area: dpf_mesh_cdf_build's fp32 sequence, csrc/mesh_store.h's (e1 = p2 - p0, e2 = p2 - p1, cross product a product minus a product,
 *     sqrt((c0*c0 + c1*c1) + c2*c2) / 2, nothing fused), 0 where that build counts the face as 0 (a non-finite area).
 *   Ties: among points of equal fp32 distance the LOWEST point index is reported -- the minimum of (distance bits << 32 | point
 *     index) as unsigned 64-bit keys.  A non-finite point is skipped: it is never a face's nearest.
 *   Bad slots: dist NaN, point -1, closest NaN, area 0 in all W columns when the mesh index is outside [0, M), the mesh is
 *     flagged, or no point of the slot is finite (N = 0 included).  Nothing of the mesh is read in the first two cases.
 *   Padding: columns f >= F_b of any slot are NaN / -1 / NaN / 0 too, and nothing of a mesh is read for them.  (With max_faces
 *     below a mesh's face count only its first W faces are answered.)
 *   dist, point, closest and area are bit-identical from run to run and do not depend on B, on the slot, on how faces and points
 *     are spread over workgroups and launches, or on the form.
 *   form: 0 = by size (dispatch.h: mp_form), 1 = a workgroup holds dpf_mesh_point_tile() faces, one per lane, and walks all of
 *     its slot's points in tiles of as many, 2 = the point tiles are also split over workgroups, merged by a 64-bit atomic minimum
 *     into workspace (dpf_mesh_point_workspace_bytes(B, max_faces) bytes, 8-byte aligned; only read or written when the split
 *     form runs) and unpacked by a finishing launch.
 *   Launches on the caller's stream, never synchronises, no memset nodes; B = 0 or max_faces = 0 launches nothing; B and the
 *     faces are chunked over launches.  max_faces < 2^31.
 *   dpf_mesh_point_distance_grad: grad_points (B, N, 3)[i] = the sum over the faces f with point[b, f] == i, in ascending f, of
 *     2 * grad_dist[b, f] * (points[b, i] - closest[b, f]) -- each term (2 * g) * (p - q) rounded on its own and added to a sum
 *     that starts at 0; a component whose closest is NaN adds 0; a point no face names gets 0.  A gather, one launch, no
 *     floating-point atomics: bit-identical from run to run.  The mesh is data: there is no gradient with respect to vertices. */
int dpf_mesh_point_tile(void);
size_t dpf_mesh_point_workspace_bytes(int B, long max_faces);
int dpf_mesh_point_distance(int M, const float *vertices, const long *vertex_bounds, const unsigned int *faces,
                            const long *face_bounds, const unsigned int *flags, int B, int N, const float *points,
                            const int *mesh_idx, long max_faces, int form, float *dist, int *point, float *closest, float *area,
                            void *workspace, size_t workspace_bytes, dpf_stream_t stream);
int dpf_mesh_point_distance_grad(int B, int N, long max_faces, const float *points, const int *point, const float *closest,
                                 const float *grad_dist, float *grad_points, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Exact EMD (csrc/emd_exact.hip): the optimal one-to-one matching of two clouds a, b of n points each, (B, n, 3) fp32 point-major --
 * a linear assignment problem on an integer cost grid, solved exactly by an epsilon-scaling auction in 64-bit integers.  Not a port:
 * the reference has only the approximate matcher above.  tests/emd_exact_ref.py restates all of this in numpy.
 *   The grid, per pair: lo / hi = the per-axis minimum / maximum over the 2n points (exact), E = the largest of the three
 *     fl32(hi - lo).  E == 0: cost 0, qcost 0, the identity assignment, status 0.  Otherwise E = mant * 2^ex with mant in [0.5, 1)
 *     (frexp) and s = 2^(bits - 1 - ex); the integer cost of the pair of points (i, j) is
 *         c_ij = rint(sqrt((dx*dx + dy*dy) + dz*dz) * s),   d = a_i - b_j per axis,
 *     every fp32 operation rounded on its own (no contraction), the square root correctly rounded, the product with s exact, rint
 *     to nearest even; 0 <= c_ij < 2^bits (d < sqrt(3) * E and E * s < 2^(bits - 1); at bits == 1 alone a diagonal of the extent's box
 *     can round up to c_ij == 2).  bits in 1..24 (the Python default is 20).  Scaling both clouds by a power of two changes no c_ij.
 *   Refused pairs (status DPF_EMD_EXACT_REFUSED): any non-finite coordinate; E not finite; E * E not a normal fp32 number; 3 * (E * E)
 *     not finite (a diagonal's square could overflow).
 *   The auction minimises sum_i c_i,sigma(i) over permutations sigma.  Point i of a values object j (point j of b) at
 *     u_ij = (n + 1) * c_ij + price_j, integer prices from 0.  A round: every unassigned i finds its lowest u (u1, at j1: the
 *     LOWEST j among equal values) and second lowest (u2), all on the prices of the round's start, and bids price_j1 + (u2 - u1) +
 *     epsilon for j1; every object that got bids takes the HIGHEST, among equal bids the LOWEST bidder, at that price, and its
 *     previous owner is unassigned.  A phase runs rounds until every point is assigned.  epsilon is ((n + 1) << bits) >> 4 in the
 *     first phase and falls by 3 bits per phase (never below 1); the phase at epsilon 1 is the last.  Prices are kept from phase to
 *     phase, the assignment is reset.  With integer u and a final epsilon of 1 < (n + 1) / n the last assignment is an exact optimum
 *     of the integer problem.  n == 1 is answered without a round.  Scaled costs stay below 2^38 and bids below 2^50 (a pair whose
 *     bid reached 2^50 would end with DPF_EMD_EXACT_RANGE; no input is known to get there).
 *   Outputs per pair: assignment (n) int32, optional (NULL: not written): point i of a is matched to point assignment[i] of b;
 *     inverse (n) int32, optional: inverse[assignment[i]] = i; qcost int64 = sum_i c_i,assignment[i]; cost fp32 = the sum over
 *     i = 0 .. n-1 ASCENDING, from 0, of the fp32 distances sqrt((dx*dx + dy*dy) + dz*dz) of the matched points (the arithmetic above);
 *     status int32 >= 0: solved, the number of rounds used; < 0: one of the codes below, and then cost NaN, qcost -1, assignment and
 *     inverse -1.  cost is NOT divided by n.
 *   Bounded: max_rounds caps the rounds of a pair over all its phases; a pair that would need more ends with DPF_EMD_EXACT_CAP.
 *     Every loop of the kernel runs over n, over the (at most 14) phases or over counted rounds: no input makes a launch spin.
 *   Determinism: all outputs (status included) are bit-identical from run to run and depend on nothing but the pair's own 2n points,
 *     bits and max_rounds -- not on the batch, the strides, the launch shape or the form.  One pair's refusal touches no other pair.
 *   form: 0 = by size (dispatch.h: ee_form), 1 = resident: the second cloud in LDS, n <= 4096 (DPF_ENOSUP beyond), 2 = streamed: the
 *     second cloud read from global memory and n words of bids per pair in workspace (dpf_emd_exact_workspace_bytes(pairs, n) bytes,
 *     8-byte aligned; only the streamed form touches it).  n <= dpf_emd_exact_max_points() = 8192, DPF_ENOSUP beyond.
 *   One workgroup per pair, one launch, the caller's stream, no synchronisation, no memset nodes; B = 0 or n = 0 launches nothing.
 *   dpf_emd_exact: a_stride / b_stride = floats between consecutive clouds of an operand (3n for a dense batch; 0 broadcasts one cloud).
 *   dpf_pairwise_emd_exact: the (N1, N2) matrix, pair (i, j) = clouds1[i] against clouds2[j], both sets dense and read in place;
 *     qcost, cost, status are (N1, N2); no assignment is written.  N1 * N2 < 2^31.
 *   dpf_emd_exact_grad: the assignment is a constant (as the reference's match_cost backward treats its matching):
 *     grad_a[i] = grad_cost * ((a_i - b_j) / d) per axis with j = assignment[i] and d the fp32 distance above, 0 where d == 0;
 *     grad_b[j] = the negative of that term at i = inverse[j].  Either output may be NULL (not computed); an index of -1 gives 0.
 *     dense (B, n, 3) operands, grad_cost (B).  One launch, a gather, no atomics: bit-identical from run to run. */
#define DPF_EMD_EXACT_REFUSED (-1)
#define DPF_EMD_EXACT_CAP (-2)
#define DPF_EMD_EXACT_RANGE (-3)
int dpf_emd_exact_max_points(void);
size_t dpf_emd_exact_workspace_bytes(long pairs, int n);
int dpf_emd_exact(int B, int n, const float *a, long a_stride, const float *b, long b_stride, int bits, int max_rounds, int form,
                  int *assignment, int *inverse, long long *qcost, float *cost, int *status, void *workspace,
                  size_t workspace_bytes, dpf_stream_t stream);
int dpf_pairwise_emd_exact(int N1, int N2, int n, const float *clouds1, const float *clouds2, int bits, int max_rounds, int form,
                           long long *qcost, float *cost, int *status, void *workspace, size_t workspace_bytes,
                           dpf_stream_t stream);
int dpf_emd_exact_grad(int B, int n, const float *a, const float *b, const int *assignment, const int *inverse,
                       const float *grad_cost, float *grad_a, float *grad_b, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Farthest-point sampling (csrc/fps.hip): the k points of a cloud of n that cover it best, chosen greedily -- what brings clouds of
 * any size to the common size the matching metrics above need.  Not a port: the reference has no FPS.  tests/fps_ref.py restates all
 * of this in numpy.
 *   Input: xyz holds B clouds of n points, fp32, read in place through three strides counted in floats: coordinate a of point i of
 *     cloud b is xyz[b * cloud_stride + i * point_stride + a * axis_stride].  (B, n, 3) point-major is (3n, 3, 1); (B, 3, N)
 *     channel-major, the networks' layout, is (3N, 1, N); cloud_stride == 0 broadcasts one cloud.  1 <= k <= n <= the max_points
 *     query's value = 8192, DPF_ENOSUP beyond; bad arguments (B < 0, n < 1, k < 1, k > n, a missing xyz or index, an unknown form)
 *     return DPF_EINVAL; B == 0 launches nothing.  start: (B) int32, the first selection of every cloud, or NULL = 0 for every cloud.
 *   Arithmetic: d(i, j) = (dx*dx + dy*dy) + dz*dz with dx = x_i - x_j and the same per axis, every fp32 operation rounded on its own
 *     (no contraction).  d >= +0, and +inf where finite coordinates overflow; from finite input no NaN arises.
 *   Selection: sel_0 = start[b], mind_0[i] = d(i, sel_0); for t >= 1 sel_t = the LOWEST index i that attains max_i mind_(t-1)[i],
 *     and mind_t[i] = min(mind_(t-1)[i], d(i, sel_t)).
 *   Outputs per cloud: index (B, k) int32 = sel_t; radius2 (B, k) fp32, optional (NULL: not written), radius2[t] = max_i mind_t[i],
 *     the squared covering radius of the first t + 1 selections: it never increases with t, radius2[k-1] is the squared one-sided
 *     Hausdorff distance from the cloud to its subset, and it is 0 from the point where every distinct position has been taken.  Once
 *     radius2 is 0 every mind is 0 and the rule above keeps selecting index 0: a caller who asks for more points than the cloud has
 *     distinct positions gets repeats of point 0.  status (B) int32, optional: 0 = done; DPF_FPS_REFUSED = a non-finite coordinate
 *     among the cloud's n points or a start outside [0, n), and then index is -1 and radius2 NaN for that cloud.  Finite coordinates
 *     whose squared distance overflows to +inf are NOT refused: the rule is well defined on them (+inf is an ordinary maximum).
 *   Determinism: every output is bit-identical from run to run and depends on nothing but the cloud's own n points, k and start[b]
 *     -- not on the batch, the strides, the form or the launch shape.  One cloud's refusal touches no other cloud.
 *   form: 0 = by size (dispatch.h: fps_form: one wave up to 512 points, four waves up to 4096, sixteen above); 1 = one wave per
 *     cloud, n <= 512; 2 = a workgroup of four waves; 3 = of sixteen waves (the points per thread are a compile-time parameter of
 *     the kernel, a power of two).  A form forced past its limit returns DPF_ENOSUP, an unknown form DPF_EINVAL.
 *   One workgroup per cloud (the cloud index on grid.x: B may exceed 65535), one launch, the caller's stream, no synchronisation, no
 *     workspace, no memset nodes.  Every loop runs over n, over k or over a fixed number of waves: no input makes a launch spin. */
#define DPF_FPS_REFUSED (-1)
int dpf_fps_max_points(void);
int dpf_fps(int B, int n, const float *xyz, long cloud_stride, long point_stride, long axis_stride, int k, const int *start, int form,
            int *index, float *radius2, int *status, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Sliced 2-Wasserstein distance (csrc/swd.hip): project two clouds on L directions, sort each projection, and the 1-D optimal
 * transport of a direction is the rank-to-rank match -- a transport distance at O(L n log n) per CLOUD and O(L n) per PAIR, since the
 * sort belongs to a cloud and not to a pair.  Not a port: the reference has no such metric.  tests/swd_ref.py restates all of this in
 * numpy.
 * dpf_swd_tables
 *   Input: xyz holds B clouds of n points, fp32, read in place through three strides counted in floats, exactly as dpf_fps reads them
 *     ((B, n, 3) is (3n, 3, 1); (B, 3, N) is (3N, 1, N); cloud_stride == 0 broadcasts one cloud).  dirs: (L, 3) fp32, dense; they are
 *     NOT normalised here.  1 <= n <= the max_points query's value = 8192 (n need not be a power of two), DPF_ENOSUP beyond; L >= 1 and
 *     B * L < 2^31; bad arguments (B < 0, n < 1, L < 1, B * L too large, a missing xyz, dirs or sorted, an unknown form) return
 *     DPF_EINVAL; B == 0 launches nothing.
 *   Projection: p(b, l, i) = ((x * tx + y * ty) + z * tz) + 0.0f with (tx, ty, tz) = dirs[l], every fp32 operation rounded on its own
 *     (no contraction).  The final + 0.0f turns -0 into +0, so equal values have equal bits.
 *   Order: order(b, l, .) is the permutation of 0..n-1 that sorts the keys (p, i) ascending -- the value compared as a float, the
 *     LOWEST index first among equal values; sorted(b, l, r) = p(b, l, order(b, l, r)).
 *   Outputs: sorted (B, L, n) fp32; order (B, L, n) int32, optional (NULL: not written -- the pair sums do not need it); status (B)
 *     int32, optional: 0 or DPF_SWD_REFUSED.
 *   Refusal: a cloud is refused when any of its 3n coordinates, any of the 3L direction components or any of its L * n projections is
 *     not finite (overflow of finite input included).  Its L rows of sorted are then NaN and of order -1.  One cloud's refusal touches
 *     no other cloud (a non-finite direction refuses every cloud: it is part of every cloud's projections).
 *   Determinism: every output is bit-identical from run to run and depends on nothing but the cloud's own points and dirs -- not on
 *     the batch, the strides, the form or the launch shape.
 *   form: 0 = by size (dispatch.h: swd_form); 1 = one wave per sort, n <= 512; 2 = a workgroup of four waves; 3 = of sixteen waves
 *     (the keys per thread are a compile-time parameter, a power of two).  A form forced past its limit returns DPF_ENOSUP.
 *   One workgroup per (cloud, direction), one launch (one per 2^32 threads beyond that), the caller's stream, no synchronisation, no
 *     workspace, no memset nodes.  Every loop is bounded by n, log n or L.
 * dpf_swd_pairs / dpf_swd_pairwise read only sorted and status.  A table row is one cloud's (L, n) block.
 *   sumsq = sum_l sum_r (double) fl32(sa(l, r) - sb(l, r))^2, accumulated in float64 (the order of the additions is the kernel's; the
 *     result is within L * n * 2^-53 relative of the exact sum whatever it is).  Output float64: (B) for dpf_swd_pairs -- cloud
 *     b * a_stride of table A against cloud b * b_stride of table B, strides in table rows, 0 broadcasts -- and (N1, N2) row-major for
 *     dpf_swd_pairwise.  accumulate: 0 overwrites sumsq, 1 adds to what is there (one owner thread per pair, no atomics): a caller
 *     can walk the directions in chunks and never hold more than a chunk of the tables.  A pair with a refused side gives NaN.
 *     The distance is sumsq / (L * n), the Monte-Carlo SW2^2: no square root.  Bit-identical from run to run.
 * dpf_swd_grad: the permutations are constants.  With g(l, i) = fl32(sa(l, r) - sb(l, r)) at r = the rank of point i of a in
 *   direction l,  grad_a(b, i, axis) = fl32((double) grad_cost(b) * (2 / ((double) L * n)) * sum_l (double) g(l, i) * (double)
 *   dirs(l, axis)), the sum in float64 in ascending l; grad_b is the same with the sign reversed, at the ranks of b's points.  grad_a,
 *   grad_b: (B, n, 3) fp32 dense, either may be NULL (then its order may be too); grad_cost (B) fp32.  Refused pairs give 0.  No
 *   atomics: g is scattered through order into the workspace ((B, L, n) fp32, dpf_swd_grad_workspace_bytes; the targets are a
 *   permutation) and reduced over l per point.  B <= 65535.  Bit-identical from run to run.  No gradient for the directions. */
#define DPF_SWD_REFUSED (-1)
int dpf_swd_max_points(void);
int dpf_swd_tables(int B, int n, const float *xyz, long cloud_stride, long point_stride, long axis_stride, int L, const float *dirs,
                   int form, float *sorted, int *order, int *status, dpf_stream_t stream);
int dpf_swd_pairs(int B, int L, int n, const float *sorted_a, const int *status_a, long a_stride, const float *sorted_b,
                  const int *status_b, long b_stride, int accumulate, double *sumsq, dpf_stream_t stream);
int dpf_swd_pairwise(int N1, int N2, int L, int n, const float *sorted1, const int *status1, const float *sorted2, const int *status2,
                     int accumulate, double *sumsq, dpf_stream_t stream);
size_t dpf_swd_grad_workspace_bytes(int B, int L, int n);
int dpf_swd_grad(int B, int L, int n, const float *dirs, const float *sorted_a, const int *order_a, const int *status_a,
                 const float *sorted_b, const int *order_b, const int *status_b, const float *grad_cost, float *grad_a, float *grad_b,
                 void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * k nearest neighbours (csrc/knn.hip): for every query point the k points of its slot's cloud that are nearest to it, with their
 * squared distances, ascending -- the neighbourhood a spacing statistic, a repulsion term or a local feature needs, without the
 * (B, n, m) distance tensor.  Not a port: the reference has no point-level k-NN.  tests/knn_ref.py restates all of this in numpy.
 *   Input: query holds B sets of n points and cloud B sets of m points, fp32, each read in place through three strides counted in
 *     floats, exactly as dpf_fps reads a cloud: coordinate a of point i of slot b is p[b * cloud_stride + i * point_stride + a *
 *     axis_stride].  (B, n, 3) point-major is (3n, 3, 1); (B, 3, N) channel-major is (3N, 1, N); a cloud stride of 0 broadcasts one
 *     set over the batch.  query and cloud may be the same memory (a self-search); neither is written.
 *   Arithmetic: d(i, j) = (dx*dx + dy*dy) + dz*dz with dx = c_j.x - q_i.x and the same per axis, every fp32 operation rounded on its
 *     own (no contraction): dpf_nndistance's formula and bits.
 *   Eligible candidates of query i: every j in [0, m); with exclude_same_index != 0 all of them but j == i.  The exclusion goes by
 *     INDEX, not by distance: it is meant for a self-search, and a duplicate of the query at another index stays a neighbour at
 *     distance 0.  (A query with i >= m has nothing to exclude.)
 *   Result: the k eligible candidates with the smallest key (d, j), in ascending key order -- equal distances are ordered by the
 *     LOWEST index first, among the listed ones and at the cut after the k-th.  dist (B, n, k) fp32 and index (B, n, k) int32, both
 *     dense; status (B) int32, optional (NULL: not written): 0 or DPF_KNN_REFUSED.
 *   Arguments: 1 <= k <= dpf_knn_max_k() = 32, DPF_ENOSUP above; k above the number of eligible candidates (m, or m - 1 with
 *     exclude_same_index) returns DPF_EINVAL, as do B < 0, n < 1, m < 1, k < 1, a missing query, cloud, dist or index and an unknown
 *     form; B == 0 launches nothing.
 *   Refusal: a slot is refused when any coordinate of its n query points or its m cloud points is not finite or is larger in
 *     magnitude than 2^61.  Within that bound |dx| <= 2^62 and d <= 3 * 2^124 < the largest fp32, so no distance overflows: +inf is
 *     the value of an empty list slot and never ties with a real distance.  A refused slot gets dist NaN, index -1 and status
 *     DPF_KNN_REFUSED; no other slot is touched (a refused broadcast set refuses every slot: it is part of each).
 *   Determinism: every output is bit-identical from run to run and depends on nothing but the slot's own points, k and the flag --
 *     not on B, the strides, the form or the launch shape.
 *   form: 0 = by k (dispatch.h: knn_form: the smallest list capacity >= k); 1, 2, 3, 4 = a lane's list has capacity 4, 8, 16, 32 (a
 *     compile-time parameter of the kernel).  A forced capacity below k returns DPF_ENOSUP.
 *   One workgroup per 256 queries of a slot, one launch (cut by dispatch::chunk_grid past 32768 slots or 2^22 workgroups a slot), the
 *     caller's stream, no synchronisation, no workspace, no atomics, no memset nodes.  Every loop runs over n, m, k or a fixed
 *     queue depth: no input makes a launch spin. */
#define DPF_KNN_REFUSED (-1)
int dpf_knn_max_k(void);
int dpf_knn(int B, int n, const float *query, long q_cloud_stride, long q_point_stride, long q_axis_stride, int m, const float *cloud,
            long c_cloud_stride, long c_point_stride, long c_axis_stride, int k, int exclude_same_index, int form, float *dist,
            int *index, int *status, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Point-cloud normals by local PCA (csrc/normals.hip): per query point the covariance of its k listed neighbours, the eigenvalues of
 * that 3 x 3 matrix and the unit eigenvector of the smallest one -- the surface normal of the neighbourhood -- with a defined sign.
 * Not a port: the reference has no normals.  tests/normals_ref.py restates all of this in numpy float64.  No gradient.
 *   Input: cloud holds B sets of m points, fp32, read in place through the three strides dpf_knn takes (counted in floats; a cloud
 *     stride of 0 broadcasts one set).  index: (B, n, k) int32, dense -- what dpf_knn writes: row (b, i) lists the neighbourhood of
 *     query point i of slot b.  viewpoint: fp32, 3 values per slot at viewpoint + b * viewpoint_stride (in floats; 0 broadcasts one),
 *     or NULL for none.  Nothing is written but the outputs.
 *   Arguments: 3 <= k <= 32.  k < 3 returns DPF_EINVAL, as do B < 0, n < 1, m < 1 and a missing cloud, index, normal, eigenvalues or
 *     flag; k > 32 returns DPF_ENOSUP; B == 0 launches nothing.  k may exceed m (a list may repeat a point).
 *   Outputs, all dense: normal (B, n, 3) and eigenvalues (B, n, 3, ascending) float64; cov (B, n, 6) float64 in the order xx, xy, xz,
 *     yy, yz, zz, optional (NULL: not written); flag (B, n) int32.
 *   Validity is per POINT: point i is flagged when any of its k indices lies outside [0, m), or any gathered coordinate is not finite
 *     or exceeds 2^61 in magnitude.  A flagged point gets flag 1 and NaN in every floating output; a valid one flag 0; no other point
 *     is touched.  Every index is range-checked BEFORE it is used as an address: a table full of -1 (dpf_knn's refused slot) gives a
 *     table full of flags, never a load outside the cloud.  The call still returns 0.
 *   Covariance, bit-defined -- every operation a separately rounded float64 operation (no contraction), on the gathered fp32
 *     coordinates converted to float64:
 *       centroid  c_a = (p_0,a + p_1,a + ... + p_k-1,a) / (double) k     added in ascending s starting from p_0; one IEEE division
 *       C_ab = sum_s (p_s,a - c_a) * (p_s,b - c_b)                       each product rounded on its own; added in ascending s
 *                                                                        starting from the s = 0 term
 *     The two-pass form: clouds sit at offsets like 100 with 1e-3 of local spread, where sum(pp) - sum(p) sum(p) / k cancels.  No
 *     division by k or k - 1: the scale changes no eigenvector.  Within the 2^61 bound nothing overflows: (2^62)^2 * 32 < 2^130.
 *   Eigen-decomposition: cyclic Jacobi on the symmetric matrix, a FIXED 6 sweeps over the pairs (0, 1), (0, 2), (1, 2), no convergence
 *     test.  A rotation is skipped where its off-diagonal entry a_pq is exactly 0; else theta = (a_qq - a_pp) / (2 a_pq),
 *     t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with sgn(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq,
 *     a_pq = 0; with r the third index (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq), and the columns p and q of the accumulated
 *     rotations (initially the identity) turn the same way.  4 sweeps reach the rounding floor on every kind of neighbourhood
 *     measured; the eigenvalues and the vector are accurate to a few units of 2^-52 * the largest eigenvalue, they are
 *     not bit-defined against another implementation.
 *   Which vector: the three diagonal entries are sorted ascending by the stable three-element compare network (0, 1), (1, 2), (0, 1),
 *     swapping only where the left is strictly greater -- the lower column goes first among equals.  The normal is the column of the
 *     smallest, divided once by its norm sqrt((x^2 + y^2) + z^2).
 *   Sign, bit-defined given the vector: canonically the component of largest magnitude is positive, the lowest axis among equal
 *     magnitudes.  With a viewpoint w whose three coordinates are finite, t = ((n_x (w_x - c_x)) + n_y (w_y - c_y)) + n_z (w_z - c_z)
 *     in float64 against the neighbourhood's centroid, every product rounded on its own: t < 0 flips the canonical normal, t == 0
 *     keeps it.  A viewpoint with a non-finite coordinate counts as none for its slot.
 *   Determinism: every output of point i is bit-identical from run to run and depends on its own k gathered points and its slot's
 *     viewpoint alone -- not on B, n, the strides or the launch shape.
 *   One lane per point, one wave per workgroup, one launch (cut by dispatch::chunk_grid past 32768 slots or 2^22 workgroups a slot),
 *     the caller's stream, no synchronisation, no LDS, no workspace, no atomics, no memset nodes.  Every loop runs over k, over 3 or
 *     over the sweep count: no input makes a launch spin. */
int dpf_normals(int B, int n, int m, const float *cloud, long cloud_stride, long point_stride, long axis_stride, const int *index,
                int k, const float *viewpoint, long viewpoint_stride, double *normal, double *eigenvalues, double *cov, int *flag,
                dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Rigid alignment (csrc/align.hip): the weighted Procrustes fit of given correspondences (dpf_rigid_fit) and trimmed point-to-point
 * ICP (dpf_icp) -- what makes the metrics above usable on clouds that do not arrive in one frame.  Not a port: the reference has no
 * registration.  tests/align_ref.py restates all of this in numpy.  No gradient.
 *   Both minimise sum_i w_i |s R p_i + t - q_i|^2 over a proper rotation R (det = +1), a translation t and a scale s (s = 1 unless
 *     with_scale != 0).  A transform is 13 float64 values: R row-major (9), t (3), s.
 *   Input: src holds B sets of n points and dst B sets of m points (dpf_rigid_fit: n), fp32, each read in place through the three
 *     strides dpf_knn takes (counted in floats; a cloud stride of 0 broadcasts one set).  Neither is written.
 *     dpf_rigid_fit: point i of src belongs to point i of dst; weights (B, n) fp32 dense, optional (NULL: every weight 1).
 *     dpf_icp: init (B, 13) float64 dense, optional (NULL: the identity for every slot); max_dist2 the squared trim distance
 *     (<= 0, +inf or NaN: no trim).
 *   dpf_icp, iteration k = 0 .. iters - 1: (1) MATCH every source point, under the current transform, to its nearest target point;
 *     (2) SOLVE for the absolute transform from the ORIGINAL source points to their matches -- increments are never composed, so
 *     nothing drifts.  After the last solve one more match runs under the returned transform, and a last reduction of it: index,
 *     dist, sums and the last rmse and inliers belong to what is returned.  2 (iters + 1) launches (dpf_rigid_fit: 2).
 *   Match, bit-defined:
 *     y_a = fp32( ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) * s + t_a )   float64 on the fp32 coordinates converted to float64, every
 *                                                                    product and sum rounded on its own, ONE rounding to fp32
 *     A y with a component that is not finite or exceeds 2^61 in magnitude has no match: index -1, dist +inf, weight 0.
 *     d(i, j) = (dx*dx + dy*dy) + dz*dz with dx = c_j.x - y.x, fp32, no contraction: dpf_nndistance's bits.  The match is the smallest
 *     key (d, j), the LOWEST index among equal distances.  With a trim a match with d > max_dist2 becomes index -1 and weight 0
 *     (dist keeps d).  Matched points have weight 1.  changed = the number of points whose index differs from the one the iteration
 *     before wrote (an inlier turning outlier or back is a change: the outlier is -1); iteration 0 counts every point.
 *   Sums, bit-defined: eighteen float64 quantities per slot over the pivoted points p' = p - a, q' = q - c in float64, a = source
 *     point 0 of the slot and c = target point 0 (dpf_rigid_fit: point 0 of either set), in this order:
 *       [0] W = sum w   [1..3] S_p = sum (w p'_a)   [4..6] S_q = sum (w q'_a)   [7 + 3a + b] S_pq = sum ((w p'_a) q'_b)
 *       [16] S_pp = sum w ((p'_0^2 + p'_1^2) + p'_2^2)   [17] dpf_icp: S_d = sum w (double) d;  dpf_rigid_fit: S_qq, [16]'s form on q'
 *     every product rounded on its own; a point without a match contributes +0.0 to all eighteen.  One pass over pivoted points: a
 *     cloud at offset 100 with 1e-3 of spread keeps its digits.  ORDER: a block is 256 consecutive points; its sum is the pairwise
 *     tree  for stride = 128, 64, ..., 1: x[i] += x[i + stride]  over the block's terms (+0.0 past n); the block sums are added in
 *     ascending block order starting from block 0's.  The inlier count (w > 0) and changed are integer sums.
 *   Solve, float64, every operation rounded on its own: with W > 0,
 *       M_ab = S_pq_ab - (S_p_a S_q_b) / W      v = S_pp - ((S_p0^2 + S_p1^2) + S_p2^2) / W
 *     Horn's closed form: the symmetric 4 x 4 matrix
 *       N = [[(Mxx+Myy)+Mzz, Myz-Mzy,        Mzx-Mxz,         Mxy-Myx        ],
 *            [ .             (Mxx-Myy)-Mzz,  Mxy+Myx,         Mzx+Mxz        ],
 *            [ .             .               (-Mxx+Myy)-Mzz,  Myz+Mzy        ],
 *            [ .             .               .                (-Mxx-Myy)+Mzz ]]
 *     is diagonalised by cyclic Jacobi with dpf_normals' rotation over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a FIXED 7 sweeps,
 *     no convergence test (5 reach the rounding floor: DESIGN 4.5i).  The column of the largest diagonal entry (the lowest column
 *     among equals), divided once by its norm sqrt(((q0^2 + q1^2) + q2^2) + q3^2), its sign fixed so that its component of largest
 *     magnitude is positive (the lowest among equals), is the unit quaternion (q0; q1, q2, q3) = (w; x, y, z) of
 *       R = [[((ww+xx)-yy)-zz, 2(xy-wz),         2(xz+wy)       ],
 *            [2(xy+wz),        ((ww-xx)+yy)-zz,  2(yz-wx)       ],
 *            [2(xz-wy),        2(yz+wx),         ((ww-xx)-yy)+zz]]
 *     so det R = +1 always: there is no reflection to fix.  s = (sum_ab R_ab M_ba) / v with with_scale, else 1;
 *     t_a = (c_a + S_q_a / W) - s * ((R_a0 g_0 + R_a1 g_1) + R_a2 g_2) with g = a + S_p / W.  R, t and s are accurate to
 *     ALIGN_BOUND (tests/align_ref.py) relative to their scales; they are not bit-defined against another implementation, but they
 *     are bit-identical from run to run.
 *   Degenerate: fewer than 3 inliers, W = 0, v <= 0 under with_scale, or a non-finite entry in the result.  The slot keeps the
 *     transform it had (the init, or the identity), gets status DPF_ALIGN_DEGENERATE and stops iterating.
 *   Refused: a slot with a coordinate of src or dst, an entry of its init or a weight that is not finite or exceeds 2^30 in magnitude,
 *     or a negative weight (every product then stays below 2^61 and every sum finite).  It gets NaN in R, t, s, rmse, sums and
 *     dist, index -1, inliers 0, iterations 0 and status DPF_ALIGN_REFUSED; no other slot is touched.
 *   Convergence: when a match after the first finds changed == 0 the next solve would return the same bits; the slot is done and
 *     iterations = the number of solves that gave its transform.  Later launches leave a done slot's outputs in place; the rmse and
 *     inliers entries after it repeat the last value.  A slot that never converges has iterations = iters.
 *   Outputs, all dense: R (B, 3, 3), t (B, 3), s (B) float64; status (B) int32: 0, DPF_ALIGN_DEGENERATE or DPF_ALIGN_REFUSED; sums
 *     (B, 18) float64, optional (NULL: not written).  dpf_icp: index (B, n) int32 and dist (B, n) fp32 of the final match; rmse
 *     (B, iters + 1) float64 = sqrt(S_d / W) per match (NaN where W = 0); inliers (B, iters + 1) int32; iterations (B) int32.
 *     dpf_rigid_fit: rmse (B) = sqrt(e / W) from the closed form e = max(0, ((s s) v + v_q) - (2 s) sum_ab R_ab M_ba), v_q as v from
 *     S_qq and S_q: it cancels, so it is good to about 2^-26 of the clouds' spread (NaN for a degenerate slot).
 *   Arguments: B < 0, n < 1, m < 1, iters < 0, a missing pointer other than weights, init or sums, a workspace that is not 8-byte
 *     aligned or smaller than dpf_align_workspace_bytes(B, n) return DPF_EINVAL; B == 0 launches nothing.  The workspace is
 *     caller-owned and need not be cleared: iteration 0 takes "everything changed" from an argument.
 *   Determinism: every output is bit-identical from run to run and depends on the slot's own inputs alone -- not on B, the strides
 *     or the launch shape.  The caller's stream, no synchronisation, no memset nodes, no atomics; launches are cut by
 *     dispatch::chunk_grid.  Every loop runs over n, m, the block count, the sweep count or six pairs: no input makes a launch spin. */
#define DPF_ALIGN_DEGENERATE 1
#define DPF_ALIGN_REFUSED (-1)
size_t dpf_align_workspace_bytes(int B, int n);
int dpf_rigid_fit(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride, const float *dst,
                  long d_cloud_stride, long d_point_stride, long d_axis_stride, const float *weights, int with_scale, double *R,
                  double *t, double *s, double *rmse, double *sums, int *status, void *workspace, size_t workspace_bytes,
                  dpf_stream_t stream);
int dpf_icp(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride, int m, const float *dst,
            long d_cloud_stride, long d_point_stride, long d_axis_stride, int iters, float max_dist2, int with_scale,
            const double *init, double *R, double *t, double *s, int *index, float *dist, double *rmse, int *inliers,
            int *iterations, double *sums, int *status, void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* Point-to-plane ICP (csrc/align.hip, dpf_icp_plane): dpf_icp's match with a Gauss-Newton step on the distances to the target's
 * tangent planes in place of the closed form -- for two samplings of one surface, where point-to-point stalls at the sampling
 * density.  tests/align_plane_ref.py restates all of this in numpy.  No scale is fitted (s = 1), no gradient.
 *   Input: src, dst, the strides, max_dist2 and init as dpf_icp's; an init whose s entry is not exactly 1 refuses its slot.
 *     normals (B, m, 3) float64 dense: one normal per target point, used AS GIVEN -- not normalised, and every output below is
 *     unchanged, bit for bit, when any subset of them is negated (dpf_normals' unoriented normals are what it wants).
 *     tol >= 0: the convergence threshold on the step (below).
 *   Iteration k = 0 .. iters - 1: (1) MATCH as dpf_icp with s = 1 -- the bits of y = fp32(R p + t), the fp32 distance, the lowest
 *     index among ties, the trim, changed and the 2^61 rule are dpf_icp's (one kernel text); (2) one SOLVE of the linearised problem
 *     and the COMPOSITION of its increment onto the current transform.  After the last solve one more match runs under the returned
 *     transform: index, dist, sums and the last rmse, rmse_plane and inliers belong to what is returned.  2 (iters + 1) launches.
 *   Weights: a matched point has w = 1.  A trimmed match or a point with no match has index -1 and w = 0; a match j whose normal n_j
 *     has a component that is not finite (the NaN dpf_normals writes for a flagged point) KEEPS index j and has w = 0.  inliers
 *     counts w > 0; changed compares indices.
 *   Terms of a pair with w = 1, float64, every operation rounded on its own; y and q = c_j are the fp32 values converted to float64,
 *     c = target point 0 (the pivot), n = n_j:
 *       y'_a = y_a - c_a        r = (n_0 (y_0 - q_0) + n_1 (y_1 - q_1)) + n_2 (y_2 - q_2)
 *       a = (y'_1 n_2 - y'_2 n_1,  y'_2 n_0 - y'_0 n_2,  y'_0 n_1 - y'_1 n_0,  n_0, n_1, n_2)           (y' x n ; n)
 *   Sums, thirty-one float64 quantities per slot, in this order:
 *       [0] W = sum w        [1 + tri(i, j)] sum (a_i a_j + 0.0), i <= j, tri(i, j) = 6 i - i (i - 1) / 2 + (j - i): the upper
 *       triangle of A = sum a a^T row-major, (0,0) (0,1) .. (0,5) (1,1) .. (5,5)        [22 + i] b_i = sum (a_i r + 0.0)
 *       [28] S_d = sum (double) d        [29] S_r = sum r r        [30] S_yy = sum ((y'_0^2 + y'_1^2) + y'_2^2)
 *     (the + 0.0 makes a zero product +0.0 whatever the normal's sign).  A pair with w = 0 contributes +0.0 to all of them.  ORDER:
 *     dpf_icp's -- blocks of 256 consecutive points, the pairwise tree stride = 128 .. 1 (+0.0 past n), the block sums added in
 *     ascending block order starting from block 0's.
 *   Solve, float64, every operation one of + - * / sqrt, rounded on its own: A x = -b for x = (omega ; tau).
 *       A_jj <- A_jj * (1 + 2^-40)                                            (Marquardt damping, scale-free)
 *       LDL^T without pivoting, for j = 0 .. 5:
 *         d = A_jj;  for c = 0 .. j - 1: d = d - (L_jc L_jc) D_c;     ok_j = d > 0;     D_j = ok_j ? d : 0
 *         for i = j + 1 .. 5:  e = A_ji;  for c = 0 .. j - 1: e = e - (L_ic L_jc) D_c;     L_ij = ok_j ? e / d : 0
 *       for i = 0 .. 5:   y_i = -b_i;  for c = 0 .. i - 1: y_i = y_i - L_ic y_c;     y_i = ok_i ? y_i : 0
 *       z_i = ok_i ? y_i / D_i : 0
 *       for i = 5 .. 0:   x_i = z_i;   for c = i + 1 .. 5: x_i = x_i - L_ci x_c;     x_i = ok_i ? x_i : 0
 *     A pivot that is not > 0 drops its unknown (the rank-deficient case, such as a planar target: not an error).
 *     Increment: h = 0.5 omega;  norm = sqrt(((1 + h_0 h_0) + h_1 h_1) + h_2 h_2);  the unit quaternion (1 / norm; h / norm) through
 *     dpf_icp's quaternion-to-R formula gives dR, a proper rotation by construction that agrees with I + [omega]x to first order.
 *       R_ab <- (dR_a0 R_0b + dR_a1 R_1b) + dR_a2 R_2b        u = t - c        t_a <- (((dR_a0 u_0 + dR_a1 u_1) + dR_a2 u_2) + c_a) + tau_a
 *     Increments are COMPOSED (Gauss-Newton has no absolute solve).  |R^T R - I| <= |R0^T R0 - I| + 40 * 2^-53 per composition
 *     (DESIGN 4.5k counts the operations).
 *       step^2 = ((omega_0^2 + omega_1^2) + omega_2^2) + ((tau_0^2 + tau_1^2) + tau_2^2) / (S_yy / W)
 *   Per match k: rmse[k] = sqrt(S_d / W), rmse_plane[k] = sqrt(S_r / W) (NaN where W = 0), inliers[k], and step[k] = sqrt(step^2) of
 *     the solve that FOLLOWS match k -- 0 where none does (the last match, a converged or a degenerate slot).
 *   Convergence: a slot is done when a match k > 0 finds changed == 0 and the solve before it had step^2 <= tol * tol; tol = 0 stops
 *     only on an exactly zero step.  iterations = the number of solves that gave the transform; the entries of rmse, rmse_plane, step
 *     and inliers after a done match repeat its values.
 *   Degenerate: fewer than 6 inliers, W = 0, or a result (R, t or step^2) that is not finite.  The slot keeps its transform, gets
 *     DPF_ALIGN_DEGENERATE and stops.  Refused: as dpf_icp, or an init s other than 1, or a FINITE normal component above 2^30 in
 *     magnitude; the outputs are dpf_icp's for a refused slot, with NaN in rmse_plane and step.
 *   Outputs, dense: R, t, s (written as 1), index, dist, rmse, inliers, iterations, status as dpf_icp's; rmse_plane and step
 *     (B, iters + 1) float64; sums (B, 31) float64, optional (NULL: not written).
 *   Arguments: as dpf_icp's; tol < 0 or NaN, a missing normals, rmse_plane or step, a workspace smaller than
 *     dpf_icp_plane_workspace_bytes(B, n) return DPF_EINVAL.  The workspace need not be cleared.
 *   Determinism and launches: as dpf_icp -- no memset node, no atomics, no synchronisation; a done slot returns on a block-uniform
 *     branch; every loop runs over n, m, the block count or a compile-time count. */
size_t dpf_icp_plane_workspace_bytes(int B, int n);
int dpf_icp_plane(int B, int n, const float *src, long s_cloud_stride, long s_point_stride, long s_axis_stride, int m,
                  const float *dst, long d_cloud_stride, long d_point_stride, long d_axis_stride, const double *normals, int iters,
                  float max_dist2, double tol, const double *init, double *R, double *t, double *s, int *index, float *dist,
                  double *rmse, double *rmse_plane, double *step, int *inliers, int *iterations, double *sums, int *status,
                  void *workspace, size_t workspace_bytes, dpf_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Density-aware Chamfer distance (csrc/dcd.hip): DCD of Wu et al., "Balanced Chamfer Distance as a Comprehensive Metric for Point
 * Cloud Completion" (NeurIPS 2021), the published calc_dcd, from ONE nn_distance result per cloud: the counts, the loss and the
 * coefficients of its gradient.  Not a port: the reference has no DCD.  tests/dcd_ref.py restates all of this in numpy.
 *   Input, dense, per cloud b of B: dist1 (B, n) fp32 and idx1 (B, n) int32, the squared distance and the index of the nearest of the
 *     second set's m points for every point of the first set (what dpf_nndistance returns); dist2 (B, m), idx2 (B, m) the other way,
 *     indices into the first set.  alpha > 0 and n_lambda >= 0, both finite; non_reg 0 or not.  Nothing is read but these.
 *   Counts: c1[i] = the number of i' in [0, n) with idx1[i'] == idx1[i] (at least 1: i itself); c2[j] the same over idx2.  Exact.
 *   Terms, float64, every operation rounded on its own (no contraction), for side 1 (side 2: n and m swapped, dist2, c2):
 *       frac1 = (double) n / (double) m, under non_reg max(frac1, 1.0)
 *       p = (double) c1[i] when n_lambda == 1;  1.0 when n_lambda == 0;  pow((double) c1[i], n_lambda) otherwise
 *       W = frac1 / (p + 1e-6)          e = exp(-(alpha * (double) dist1[i]))          q = e * W          term[i] = 1.0 - q
 *       coef1[i] = fp32( h1 * q ),  h1 = (0.5 * alpha) / (double) n
 *     coef1[i] is d loss[b] / d dist1[i] with the weights W held constant, which is how the published loss detaches them.
 *   Sums, ORDER as dpf_icp's: a block is 256 consecutive queries; its sum is the pairwise tree  for stride = 128, 64, ..., 1:
 *     x[i] += x[i + stride]  over the block's terms (+0.0 past the end); the block sums are added in ascending block order starting
 *     from block 0's: S1.  L1 = S1 / (double) n, L2 = S2 / (double) m, loss[b] = 0.5 * (L1 + L2).
 *     exp and pow are the device library's (not correctly rounded): loss and halves are accurate to DCD_BOUND (tests/dcd_ref.py)
 *     relative to max(1, frac1, frac2) for finite distances >= 0, bit-identical from run to run and between the two forms.
 *   Refused: a cloud with an index outside [0, m) in idx1 or outside [0, n) in idx2.  It gets NaN in loss, halves and both coefs,
 *     -1 in both counts and status DPF_DCD_REFUSED; such an index is never used as an address and no other cloud is touched.
 *     Distances that are negative or not finite are NOT refused: they go through the arithmetic above.
 *   Outputs, dense: loss (B) float64 and status (B) int32 (0 or DPF_DCD_REFUSED), both required; halves (B, 2) float64 = L1, L2;
 *     count1 (B, n), count2 (B, m) int32; coef1 (B, n), coef2 (B, m) fp32 -- each of these optional (NULL: not written).
 *   form: 0 by size (dispatch::dcd_form), 1 the one-workgroup form (counts in LDS, one launch; n, m <= 32768, DPF_ENOSUP above),
 *     2 the workspace form (counts in the workspace: four launches).  The outputs do not depend on it.
 *   Arguments: B < 0, n < 1, m < 1, an alpha that is not positive and finite, an n_lambda that is negative or not finite, an unknown
 *     form, a missing required pointer, a workspace that is not 8-byte aligned or smaller than dpf_dcd_workspace_bytes(B, n, m)
 *     return DPF_EINVAL; B == 0 launches nothing.  The workspace is caller-owned, may come in dirty and is left dirty.
 *   The caller's stream, no allocation, no synchronisation, no memset node, no floating-point atomic (the counts are integer
 *     atomics: order-independent); capture-safe.  Every loop runs over n, m or the block count. */
#define DPF_DCD_REFUSED (-1)
size_t dpf_dcd_workspace_bytes(int B, int n, int m);
int dpf_dcd(int B, int n, int m, const float *dist1, const int *idx1, const float *dist2, const int *idx2, double alpha,
            double n_lambda, int non_reg, int form, double *loss, double *halves, int *count1, int *count2, float *coef1,
            float *coef2, int *status, void *workspace, size_t workspace_bytes, dpf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPF_HIP_H */
