"""The structural-loss CALLERS of the reference's lib/metrics/evaluation_metrics.py, over the HIP entry points:

  distChamferCUDA (:22-23), emd_approx (:26-31)     -- re-exported from networks.utils
  EMD_CD (:48-82)                                   -- per-pair Chamfer of two equally long sets, batched
  _pairwise_EMD_CD_ (:85-121)                       -- the (N_sample, N_ref) Chamfer and EMD matrices; the only caller of
                                                       match_cost in the reference
  knn (:125-154), lgan_mmd_cov (:157-169)           -- 1-NN accuracy, MMD and COV over those matrices (tensor arithmetic)
  compute_all_metrics (:172-200)                    -- the generation metrics (MMD / COV / 1-NNA, CD and EMD), its three matrix
                                                       pairs from networks.utils.pairwise_CD + pairwise_EMD
  unit_cube_grid_point_cloud, jsd_between_point_cloud_sets, entropy_of_occupancy_grid, jensen_shannon_divergence, _jsdiv
  (:206-321)                                        -- the occupancy-grid JSD; the nearest-centre binning of every point runs
                                                       on the device (dpf_occupancy_grid, metrics/occupancy.py) instead of a
                                                       scikit-learn tree query per cloud, the statistics stay host numpy / scipy

Same signatures, return structures and values as the reference's loops.  What differs is how a row is fed: the reference
expands sample i to (batch, n, 3) and copies it (`.contiguous()`) for every block of references; here the Chamfer launch
reads the one cloud through a zero batch stride (dpf_nndistance_strided_auto, same bits) and reduces to the per-pair CD
in one more launch; the EMD entry point needs a dense batch, so only that operand is materialised.
`accelerated_cd=False` asks the reference for its pure-PyTorch distChamfer (the O(N^2)-memory bmm form, :35-45); there
is no CPU or tensor-op fallback in this package, so both values of the flag run the exact HIP Chamfer."""
import warnings

import numpy as np
import torch

from ..networks.utils import distChamferCUDA, emd_approx, chamfer_per_cloud, chamfer_cd_per_cloud  # noqa: F401
from ..networks.utils import pairwise_CD, pairwise_EMD, pairwise_EMD_exact, emd_exact  # noqa: F401
from .._lib import lib, check, current_stream


def EMD_CD(sample_pcs, ref_pcs, batch_size, accelerated_cd=False, reduced=True):
    N_sample, N_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    assert N_sample == N_ref, "REF:%d SMP:%d" % (N_ref, N_sample)
    cd_lst = []
    for b_start in range(0, N_sample, batch_size):
        b_end = min(N_sample, b_start + batch_size)
        smp, ref = sample_pcs[b_start:b_end].contiguous(), ref_pcs[b_start:b_end].contiguous()
        if smp.is_cuda and smp.dtype == torch.float32 and ref.dtype == torch.float32 and not (torch.is_grad_enabled() and (smp.requires_grad or ref.requires_grad)):
            cd_lst.append(chamfer_cd_per_cloud(smp, ref))              # search + dl.mean(1) + dr.mean(1): ONE launch (ChamferEvaluator)
        else:
            dl, dr = distChamferCUDA(smp, ref)
            cd_lst.append(chamfer_per_cloud(dl, dr))                   # dl.mean(1) + dr.mean(1), one more launch
    cd = torch.cat(cd_lst).mean() if reduced else torch.cat(cd_lst)
    return {"MMD-CD": cd}


def _pairwise_EMD_CD_(sample_pcs, ref_pcs, batch_size, accelerated_cd=True):
    if not (sample_pcs.is_cuda and ref_pcs.is_cuda):
        raise RuntimeError("_pairwise_EMD_CD_ needs CUDA tensors (there is no CPU fallback)")
    sample_pcs, ref_pcs = sample_pcs.contiguous().float(), ref_pcs.contiguous().float()
    N_sample, n = sample_pcs.shape[0], sample_pcs.shape[1]
    N_ref, m = ref_pcs.shape[0], ref_pcs.shape[1]
    dev = sample_pcs.device
    all_cd = torch.empty((N_sample, N_ref), dtype=torch.float32, device=dev)
    all_emd = torch.empty((N_sample, N_ref), dtype=torch.float32, device=dev)
    bs = max(1, min(batch_size, N_ref))
    d1 = torch.empty((bs, n), dtype=torch.float32, device=dev)
    d2 = torch.empty((bs, m), dtype=torch.float32, device=dev)
    i1 = torch.empty((bs, n), dtype=torch.int32, device=dev)
    i2 = torch.empty((bs, m), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for i in range(N_sample):
            for r0 in range(0, N_ref, batch_size):
                r1 = min(N_ref, r0 + batch_size)
                nb = r1 - r0
                st = current_stream()
                check(lib().dpf_nndistance_strided_auto(nb, n, sample_pcs[i].data_ptr(), 0, m, ref_pcs[r0].data_ptr(), m * 3,
                                                        d1.data_ptr(), i1.data_ptr(), d2.data_ptr(), i2.data_ptr(), st),
                      "nndistance_strided")
                check(lib().dpf_chamfer_reduce(nb, n, m, d1.data_ptr(), d2.data_ptr(), all_cd[i, r0:r1].data_ptr(), st),
                      "chamfer_reduce")
                all_emd[i, r0:r1] = emd_approx(sample_pcs[i].unsqueeze(0).expand(nb, -1, -1).contiguous(), ref_pcs[r0:r1])
    return all_cd, all_emd


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """k-NN two-sample classifier, leave-one-out (:125-154): the clouds of x are labelled 1, those of y 0, and every cloud is
    predicted 1 when at least k / 2 of its k nearest other clouds (smallest entries of its column of the joint distance
    matrix) carry label 1.  Returns the confusion counts tp / fp / fn / tn, precision, recall, the per-class accuracies acc_t
    (of x) and acc_f (of y) and the overall accuracy acc, each a 0-d tensor of Mxx's dtype and device -- the same float32
    operations as the reference, in the same order."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.transpose(0, 1), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    self_excluded = M + torch.diag(float("inf") * torch.ones(n0 + n1).to(Mxx))
    _, idx = self_excluded.topk(k, 0, False)                               # (k, n0 + n1): every column's k nearest rows
    votes = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        votes = votes + label.index_select(0, idx[i])
    pred = torch.ge(votes, (float(k) / 2) * torch.ones(n0 + n1).to(Mxx)).float()
    tp, fp = (pred * label).sum(), (pred * (1 - label)).sum()
    fn, tn = ((1 - pred) * label).sum(), ((1 - pred) * (1 - label)).sum()
    return {
        'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn,
        'precision': tp / (tp + fp + 1e-10),
        'recall': tp / (tp + fn + 1e-10),
        'acc_t': tp / (tp + fn + 1e-10),
        'acc_f': tn / (tn + fp + 1e-10),
        'acc': torch.eq(label, pred).float().mean(),
    }


def lgan_mmd_cov(all_dist):
    """MMD and coverage of an (N_sample, N_ref) distance matrix (:157-169): lgan_mmd = mean over the references of the distance
    to the nearest sample, lgan_mmd_smp = mean over the samples of the distance to the nearest reference, lgan_cov = share of
    the references that are the nearest reference of some sample.  0-d tensors of all_dist's dtype and device."""
    N_ref = all_dist.size(1)
    nearest_ref_val, nearest_ref = torch.min(all_dist, dim=1)
    nearest_smp_val, _ = torch.min(all_dist, dim=0)
    covered = float(nearest_ref.unique().view(-1).size(0))
    return {
        'lgan_mmd': nearest_smp_val.mean(),
        'lgan_cov': torch.tensor(covered / float(N_ref)).to(all_dist),
        'lgan_mmd_smp': nearest_ref_val.mean(),
    }


def _pairwise_matrices(clouds1, clouds2, batch_size, emd="approx"):
    """(CD, EMD) matrices of every cloud of clouds1 against every cloud of clouds2: one matrix launch per chunk for each, both
    sets read in place (what _pairwise_EMD_CD_ returns, without its per-row loop and without forming any matching).
    emd: "approx" -- pairwise_EMD, the reference's matcher; "exact" -- pairwise_EMD_exact, the optimal matching."""
    if emd not in ("approx", "exact"):
        raise ValueError("emd must be 'approx' or 'exact', got %r" % (emd,))
    emd_matrix = pairwise_EMD if emd == "approx" else pairwise_EMD_exact
    return pairwise_CD(clouds1, clouds2, bs=batch_size), emd_matrix(clouds1, clouds2, bs=batch_size)


def _reduce_to(clouds, n_points, name):
    """the n_points farthest-point samples of every cloud, from index 0 (metrics/fps.py)"""
    from .fps import farthest_point_sample
    if not (isinstance(n_points, int) and not isinstance(n_points, bool)) or n_points < 1:
        raise ValueError("n_points must be a positive integer or None, got %r" % (n_points,))
    if n_points > clouds.shape[1]:
        raise ValueError("n_points = %d exceeds the %d points of %s" % (n_points, clouds.shape[1], name))
    with torch.no_grad():
        return farthest_point_sample(clouds.float(), n_points)


def compute_all_metrics(sample_pcs, ref_pcs, batch_size, accelerated_cd=False, emd="approx", n_points=None, swd=None, dcd=None):
    """The generation metrics of the reference (:172-200): MMD and COV (lgan_mmd_cov) from the (sample, reference) matrices
    and 1-NN accuracy (knn, k = 1) from those plus the (reference, reference) and (sample, sample) matrices, for Chamfer and
    approximate EMD.  Keys "lgan_mmd-CD", "lgan_cov-CD", "lgan_mmd_smp-CD", the same for EMD, "1-NN-CD-acc_t",
    "1-NN-CD-acc_f", "1-NN-CD-acc" and the same for EMD.  The reference's orientation is kept: the cross matrices are computed
    as (reference, sample) and transposed for lgan_mmd_cov, and approx-EMD is not symmetric in its operands.  `batch_size`
    bounds the pairs per launch; `accelerated_cd` is accepted and ignored (module docstring).  No autograd (pairwise_EMD).
    emd="exact" builds the three EMD matrices from pairwise_EMD_exact (the optimal matching; same keys); the default is the
    reference's approximate matcher.
    n_points: None -- the clouds as they are; an integer -- both sets are first reduced to that many points per cloud by
    farthest-point sampling from index 0 (farthest_point_sample: the subset that covers a cloud best for its size), which brings
    sets of different cloud sizes to the common size the EMD halves need and cuts the cost of the three EMD matrices; raises
    ValueError if it exceeds either set's cloud size.
    swd: None -- the keys and values above, nothing else; an integer L -- also "lgan_mmd-SWD", "lgan_cov-SWD", "lgan_mmd_smp-SWD"
    and "1-NN-SWD-acc_t" / "-acc_f" / "-acc" from three pairwise_SWD matrices (metrics/sliced.py: the sliced 2-Wasserstein distance
    with L directions of seed 0), in the same orientation, computed after n_points has been applied.
    dcd: None -- nothing more; a positive alpha -- also "lgan_mmd-DCD", "lgan_cov-DCD", "lgan_mmd_smp-DCD" and "1-NN-DCD-acc_t" /
    "-acc_f" / "-acc" from three pairwise_DCD matrices (metrics/dcd.py: the density-aware Chamfer distance at that alpha, n_lambda
    1), in the same orientation, computed after n_points has been applied."""
    if swd is not None and (not isinstance(swd, int) or isinstance(swd, bool) or swd < 1):
        raise ValueError("swd must be a positive number of directions or None, got %r" % (swd,))
    if dcd is not None and (isinstance(dcd, bool) or not isinstance(dcd, (int, float)) or not (0 < dcd < float("inf"))):
        raise ValueError("dcd must be a positive finite alpha or None, got %r" % (dcd,))
    if n_points is not None:
        sample_pcs, ref_pcs = _reduce_to(sample_pcs, n_points, "sample_pcs"), _reduce_to(ref_pcs, n_points, "ref_pcs")
    results = {}
    M_rs_cd, M_rs_emd = _pairwise_matrices(ref_pcs, sample_pcs, batch_size, emd)
    for metric, M in (("CD", M_rs_cd), ("EMD", M_rs_emd)):
        results.update({"%s-%s" % (k, metric): v for k, v in lgan_mmd_cov(M.t()).items()})
    M_rr_cd, M_rr_emd = _pairwise_matrices(ref_pcs, ref_pcs, batch_size, emd)
    M_ss_cd, M_ss_emd = _pairwise_matrices(sample_pcs, sample_pcs, batch_size, emd)
    for metric, (M_rr, M_rs, M_ss) in (("CD", (M_rr_cd, M_rs_cd, M_ss_cd)), ("EMD", (M_rr_emd, M_rs_emd, M_ss_emd))):
        results.update({"1-NN-%s-%s" % (metric, k): v for k, v in knn(M_rr, M_rs, M_ss, 1, sqrt=False).items() if 'acc' in k})
    if swd is not None:
        from .sliced import pairwise_SWD
        M_rs, M_rr, M_ss = (pairwise_SWD(a.float(), b.float(), n_directions=swd, seed=0)
                            for a, b in ((ref_pcs, sample_pcs), (ref_pcs, ref_pcs), (sample_pcs, sample_pcs)))
        results.update({"%s-SWD" % k: v for k, v in lgan_mmd_cov(M_rs.t()).items()})
        results.update({"1-NN-SWD-%s" % k: v for k, v in knn(M_rr, M_rs, M_ss, 1, sqrt=False).items() if 'acc' in k})
    if dcd is not None:
        from .dcd import pairwise_DCD
        M_rs, M_rr, M_ss = (pairwise_DCD(a.float(), b.float(), batch_size, alpha=float(dcd))
                            for a, b in ((ref_pcs, sample_pcs), (ref_pcs, ref_pcs), (sample_pcs, sample_pcs)))
        results.update({"%s-DCD" % k: v for k, v in lgan_mmd_cov(M_rs.t()).items()})
        results.update({"1-NN-DCD-%s" % k: v for k, v in knn(M_rr, M_rs, M_ss, 1, sqrt=False).items() if 'acc' in k})
    return results


#######################################################
# JSD (:203-321; from https://github.com/optas/latent_3d_points)
#######################################################
def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """The centre coordinates of each cell of a 3D grid of resolution^3 cells placed in the unit cube (:206-224), float32, and
    the spacing.  clip_sphere drops the cells whose centre lies outside the unit sphere (norm of the float32 centre > 0.5)."""
    from .occupancy import unit_cube_grid
    return unit_cube_grid(resolution, clip_sphere)


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """The JSD between two sets of point clouds (:227-238) over the sphere-clipped grid: (S1, n1, 3) and (S2, n2, 3), numpy
    arrays or CUDA float32 tensors."""
    in_unit_sphere = True
    sample_grid_var = entropy_of_occupancy_grid(sample_pcs, resolution, in_unit_sphere)[1]
    ref_grid_var = entropy_of_occupancy_grid(ref_pcs, resolution, in_unit_sphere)[1]
    return jensen_shannon_divergence(sample_grid_var, ref_grid_var)


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """The entropy of the occupancy-grid activation patterns of a collection of clouds (:241-280): every point counts for the
    grid cell whose centre is nearest, a cell's Bernoulli variable is the share of the clouds that touch it.  Returns
    (acc_entropy / n_cells, grid_counters): grid_counters float64 over the kept cells in unit_cube_grid_point_cloud's order.
    pclouds: (S, n, 3) numpy array (uploaded to the current device as float32) or CUDA float32 tensor (read in place).  The
    assignment is one launch (metrics/occupancy.py); a NaN or infinite point raises ValueError, as scikit-learn's query does."""
    from scipy.stats import entropy
    from .occupancy import nearest_grid_counts
    if verbose:
        epsilon = 10e-4
        bound = 0.5 + epsilon
        host = pclouds.detach().cpu().numpy() if isinstance(pclouds, torch.Tensor) else np.asarray(pclouds)
        if abs(np.max(host)) > bound or abs(np.min(host)) > bound:
            warnings.warn('Point-clouds are not in unit cube.')
        if in_sphere and np.max(np.sqrt(np.sum(host ** 2, axis=2))) > bound:
            warnings.warn('Point-clouds are not in unit sphere.')
    counts, touching = nearest_grid_counts(pclouds, grid_resolution, in_sphere)
    grid_counters = counts.astype(np.float64)
    acc_entropy = 0.0
    n = float(len(pclouds))
    per_count = {}                                    # entropy([p, 1 - p]) once per distinct count; summed in the cells' order
    for g in touching[touching > 0].tolist():
        e = per_count.get(g)
        if e is None:
            p = float(g) / n
            e = per_count[g] = entropy([p, 1.0 - p])
        acc_entropy += e
    return acc_entropy / len(grid_counters), grid_counters


def jensen_shannon_divergence(P, Q):
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError('Negative values.')
    if len(P) != len(Q):
        raise ValueError('Non equal size.')
    from scipy.stats import entropy

    P_ = P / np.sum(P)  # Ensure probabilities.
    Q_ = Q / np.sum(Q)

    e1 = entropy(P_, base=2)
    e2 = entropy(Q_, base=2)
    e_sum = entropy((P_ + Q_) / 2.0, base=2)
    res = e_sum - ((e1 + e2) / 2.0)

    res2 = _jsdiv(P_, Q_)

    if not np.allclose(res, res2, atol=10e-5, rtol=0):
        warnings.warn('Numerical values of two JSD methods don\'t agree.')

    return res


def _jsdiv(P, Q):
    """another way of computing JSD"""

    def _kldiv(A, B):
        a = A.copy()
        b = B.copy()
        idx = np.logical_and(a > 0, b > 0)
        a = a[idx]
        b = b[idx]
        return np.sum([v for v in a * np.log2(a / b)])

    P_ = P / np.sum(P)
    Q_ = Q / np.sum(Q)

    M = 0.5 * (P_ + Q_)

    return 0.5 * (_kldiv(P_, M) + _kldiv(Q_, M))
