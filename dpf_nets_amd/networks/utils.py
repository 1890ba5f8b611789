"""Chamfer call sites of the reference's lib/networks/utils.py (metrics half):
distChamferCUDA (:34-35), f_score (:38-42), pairwise_CD (:90-117), and
emd_approx (lib/metrics/evaluation_metrics.py:26-31) with its pairwise matrix, pairwise_EMD (the EMD half of :85-121)."""
import torch

from ..metrics.StructuralLosses.nn_distance import nn_distance
from ..metrics.StructuralLosses.match_cost import match_cost, match_cost_lean


def distChamferCUDA(x, y):
    return nn_distance(x, y)


def chamfer_distance(pred, true):
    """cd = (dl.mean(1) + dr.mean(1)).mean() as evaluating.py:110-113 reduces it."""
    dl, dr = distChamferCUDA(pred, true)
    return (dl.mean(1) + dr.mean(1)).mean()


def chamfer_per_cloud(dl, dr):
    """(B,) dl.mean(1) + dr.mean(1) in one deterministic HIP launch (evaluating.py:112)."""
    from .._lib import lib, check, current_stream
    if not (dl.is_cuda and dr.is_cuda and dl.is_contiguous() and dr.is_contiguous()):
        raise RuntimeError("dl, dr must be contiguous CUDA tensors")
    cd = torch.empty((dl.shape[0],), dtype=torch.float32, device=dl.device)
    with torch.cuda.device(dl.device):
        check(lib().dpf_chamfer_reduce(dl.shape[0], dl.shape[1], dr.shape[1], dl.data_ptr(), dr.data_ptr(),
                                       cd.data_ptr(), current_stream()), "chamfer_reduce")
    return cd


class ChamferEvaluator:
    """The evaluation loop's Chamfer call (evaluating.py:110-113: `nn_distance` both ways, then `dl.mean(1) + dr.mean(1)`) as
    ONE launch per batch: distances, indices and the per-cloud CD from the search kernel's own workgroups (NNDistanceCD).  The
    evaluator OWNS the scratch that call needs -- one CDWorkspace per (batch shape, device, stream), created outside any stream
    capture, as the interface's ownership rule asks (StructuralLossesBackend.CDWorkspace) -- so a caller that keeps one
    evaluator per evaluation loop gets the single-launch path with nothing cached behind its back.  r05: the
    package's own evaluation helpers (metrics.evaluation_metrics.EMD_CD, chamfer_cd_per_cloud) and bench.py's step go through
    this class; before, only the benchmark created a workspace."""

    MAX_WORKSPACES = 8          # (a ragged last batch and every new shape used to add a buffer for good)

    def __init__(self):
        import collections
        import threading
        self._ws = collections.OrderedDict()            # least recently used first
        self._lock = threading.Lock()

    def __call__(self, pred, true):
        """(B, n, 3), (B, m, 3) contiguous CUDA tensors -> dist1, idx1, dist2, idx2, cd (B,)"""
        from ..metrics.StructuralLosses import StructuralLossesBackend as BK
        # keyed by the stream OBJECT (held alive by the key: its handle cannot be recycled for another stream while the
        # workspace lives) and the calling thread (two threads on one stream would share tickets)
        import threading
        stream = torch.cuda.current_stream(pred.device)
        key = (pred.shape[0], pred.shape[1], true.shape[1], pred.device, stream, threading.get_ident())
        with self._lock:
            ws = self._ws.get(key)
            if ws is not None:
                self._ws.move_to_end(key)
            elif not torch.cuda.is_current_stream_capturing():
                ws = self._ws[key] = BK.CDWorkspace(key[0], key[1], key[2], pred.device)
                while len(self._ws) > self.MAX_WORKSPACES:
                    self._ws.popitem(last=False)
        return BK.NNDistanceCD(pred, true, ws)        # (no workspace while capturing a first call: fresh scratch, tickets cleared in-call)

    def cd(self, pred, true):
        return self(pred, true)[4]


_default_evaluator = None


def chamfer_cd_per_cloud(pred, true):
    """(B,) Chamfer distance of each pair of clouds, cd[b] = dist1[b].mean() + dist2[b].mean(), in one launch (no autograd:
    the evaluation path).  Uses a process-wide ChamferEvaluator; loops that run on several streams should keep their own."""
    global _default_evaluator
    if _default_evaluator is None:
        _default_evaluator = ChamferEvaluator()
    return _default_evaluator.cd(pred, true)


class ChamferLossFunction(torch.autograd.Function):
    """cd (B,) as ONE autograd node: forward = the evaluator's single launch (the bits of chamfer_cd_per_cloud), backward = one
    dpf_chamfer_cd_backward call for the inputs that need a gradient, its additions in a fixed order (the same bits every run)."""

    @staticmethod
    def forward(ctx, pred, true, evaluator):
        dist1, idx1, dist2, idx2, cd = evaluator(pred, true)
        ctx.save_for_backward(pred, true)
        ctx.idx1, ctx.idx2 = idx1, idx2          # indices ride on ctx, as in NNDistanceFunction
        return cd

    @staticmethod
    def backward(ctx, grad_cd):
        from ..metrics.StructuralLosses.StructuralLossesBackend import ChamferCDBackward
        pred, true = ctx.saved_tensors
        g1, g2 = ChamferCDBackward(pred, true, ctx.idx1, ctx.idx2, grad_cd.contiguous(),
                                   need1=ctx.needs_input_grad[0], need2=ctx.needs_input_grad[1])
        return g1, g2, None


def chamfer_loss(pred, true, evaluator=None):
    """(B,) Chamfer distance of each pair of clouds, cd[b] = dist1[b].mean() + dist2[b].mean(), WITH autograd: the value of
    chamfer_cd_per_cloud (one launch) and a deterministic one-call backward that computes only the gradients that are asked for.
    (B, n, 3), (B, m, 3) contiguous float32 CUDA tensors, anything else raises; evaluator: a ChamferEvaluator (default: the process-wide one)."""
    global _default_evaluator
    from ..metrics.StructuralLosses.StructuralLossesBackend import _check_input
    _check_input(pred, "pred"); _check_input(true, "true")          # (as NNDistanceCD: RuntimeError for a CPU tensor or another dtype)
    if evaluator is None:
        if _default_evaluator is None:
            _default_evaluator = ChamferEvaluator()
        evaluator = _default_evaluator
    return ChamferLossFunction.apply(pred, true, evaluator)


def f_score(predicted_clouds, true_clouds, threshold=0.001):
    """lib/networks/utils.py:38-42.  Without autograd the thresholds, means and the F1 formula are one launch over the two
    distance rows (dpf_fscore_reduce: integer counts, the float arithmetic in the reference's order)."""
    ld, rd = distChamferCUDA(predicted_clouds, true_clouds)
    if ld.is_cuda and not (torch.is_grad_enabled() and (ld.requires_grad or rd.requires_grad)):
        from .._lib import lib, check, current_stream
        out = torch.empty((ld.shape[0],), dtype=torch.float32, device=ld.device)
        ldc, rdc = ld.contiguous(), rd.contiguous()                       # locals: they must outlive the launch's enqueue
        with torch.cuda.device(ld.device):
            check(lib().dpf_fscore_reduce(ld.shape[0], ld.shape[1], rd.shape[1], ldc.data_ptr(), rdc.data_ptr(),
                                          float(threshold), out.data_ptr(), current_stream()), "fscore_reduce")
        return out
    precision = 100.0 * (rd < threshold).float().mean(1)
    recall = 100.0 * (ld < threshold).float().mean(1)
    return 2.0 * precision * recall / (precision + recall + 1e-7)


def pairwise_CD(clouds1, clouds2, bs=2048, shard_rows=False):
    """(N1, N2) matrix of Chamfer distances, cds[i, j] = CD(clouds1[i], clouds2[j]) (lib/networks/utils.py:90-117; three
    calls per generative evaluation, evaluating.py:245-247).

    ONE launch for the whole matrix (dpf_pairwise_cd: grid over (query tile, j, 2 i + direction), both clouds read in
    place, the per-point distances summed in the kernel) plus a finish over the workgroups' fixed-order partial sums --
    instead of the reference's loop of N1 `expand + contiguous + nn_distance + mean` calls.  `bs` (the reference's
    batching of the second set) only bounds the workspace here: rows are processed in chunks of at most bs pairs' worth.
    shard_rows: under torch.distributed every rank computes its contiguous block of rows (distributed.shard_bounds) and
    the (N1, N2) matrix is all-gathered -- no other communication.
    Clouds of fewer than 32 points fall back to one strided launch + one reduction per row."""
    from .._lib import lib, check, current_stream
    if not (clouds1.is_cuda and clouds2.is_cuda):
        raise RuntimeError("pairwise_CD needs CUDA tensors")
    clouds1, clouds2 = clouds1.contiguous(), clouds2.contiguous()
    if clouds1.dtype != torch.float32 or clouds2.dtype != torch.float32:
        raise RuntimeError("pairwise_CD needs float32 clouds")
    N1, n = clouds1.shape[0], clouds1.shape[1]
    N2, m = clouds2.shape[0], clouds2.shape[1]
    dev = clouds1.device
    lo, hi = 0, N1
    if shard_rows:
        from .. import distributed as D
        lo, hi = D.shard_bounds(N1)
    cds = torch.empty((hi - lo, N2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = current_stream()
        if n >= 32 and m >= 32 and N2 <= 65535:
            rows = max(1, min(hi - lo, 32767, max(1, (bs * 64) // max(N2, 1))))
            nbytes = lib().dpf_pairwise_cd_workspace_bytes(rows, N2, n, m)
            ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            for r0 in range(lo, hi, rows):
                nr = min(rows, hi - r0)
                check(lib().dpf_pairwise_cd(nr, N2, n, m, clouds1[r0].data_ptr(), clouds2.data_ptr(), cds[r0 - lo].data_ptr(),
                                            ws.data_ptr(), nbytes, st), "pairwise_cd")
        else:
            bs = max(1, min(bs, N2))
            d1 = torch.empty((bs, n), dtype=torch.float32, device=dev)
            d2 = torch.empty((bs, m), dtype=torch.float32, device=dev)
            i1 = torch.empty((bs, n), dtype=torch.int32, device=dev)
            i2 = torch.empty((bs, m), dtype=torch.int32, device=dev)
            for i in range(lo, hi):
                for j_l in range(0, N2, bs):
                    nb = min(N2, j_l + bs) - j_l
                    check(lib().dpf_nndistance_strided_auto(nb, n, clouds1[i].data_ptr(), 0, m, clouds2[j_l].data_ptr(), m * 3,
                                                            d1.data_ptr(), i1.data_ptr(), d2.data_ptr(), i2.data_ptr(), st),
                          "nndistance_strided")
                    check(lib().dpf_chamfer_reduce(nb, n, m, d1.data_ptr(), d2.data_ptr(),
                                                   cds[i - lo, j_l:j_l + nb].data_ptr(), st), "chamfer_reduce")
    if shard_rows:
        from .. import distributed as D
        cds = D.gather_clouds(cds)
    return cds


def emd_approx(sample, ref):
    B, N, N_ref = sample.size(0), sample.size(1), ref.size(1)
    assert N == N_ref, "Not sure what would EMD do in this case"
    return match_cost(sample, ref) / float(N)


def emd_approx_lean(sample, ref):
    """emd_approx through match_cost_lean: the same value, and a backward that rebuilds the matching's weights instead of
    reading a stored (B, N, N) matching (metrics/StructuralLosses/match_cost.py, MatchCostLeanFunction)."""
    B, N, N_ref = sample.size(0), sample.size(1), ref.size(1)
    assert N == N_ref, "Not sure what would EMD do in this case"
    return match_cost_lean(sample, ref) / float(N)


def pairwise_EMD(clouds1, clouds2, bs=512, shard_rows=False):
    """(N1, N2) matrix of approximate EMDs, out[i, j] = emd_approx(clouds1[i:i+1], clouds2[j:j+1]) to the approx-EMD tolerance
    contract (the EMD half of lib/metrics/evaluation_metrics.py:85-121, what compute_all_metrics builds its EMD numbers on).

    dpf_pairwise_emd: every pair of a launch is one cloud pair of the approx-EMD passes, both sets read in place, and no matching
    is written (the reference's loop expands a copy of clouds1[i] per block and writes a (b, n, n) matching per call).  The cost
    is divided by float(n) in fp32 as emd_approx does.  `bs` bounds the pairs per launch, and with them the workspace (about
    1.2 MB per pair at 2 048 points); an entry's bits do not depend on it.  Each pair chooses its kernel family from its own
    two clouds: an out-of-range or NaN cloud changes only its own entries.
    shard_rows: under torch.distributed every rank computes its contiguous block of rows (distributed.shard_bounds) and the
    matrix is all-gathered, as pairwise_CD does.
    No autograd: the pairwise entry keeps no state for a backward -- inputs that would record a graph raise.  (The batched
    function no longer needs a stored matching for its gradients: emd_approx_lean / match_cost_lean rebuild the weights from the
    forward's workspace.  The pairwise entry has no such backward.)"""
    from .._lib import lib, check, current_stream
    if not (clouds1.is_cuda and clouds2.is_cuda):
        raise RuntimeError("pairwise_EMD needs CUDA tensors")
    if clouds1.dtype != torch.float32 or clouds2.dtype != torch.float32:
        raise RuntimeError("pairwise_EMD needs float32 clouds")
    if torch.is_grad_enabled() and (clouds1.requires_grad or clouds2.requires_grad):
        raise RuntimeError("pairwise_EMD has no backward (it never forms the matching): call it under torch.no_grad() or on "
                           "tensors that do not require grad")
    if clouds1.dim() != 3 or clouds2.dim() != 3 or clouds1.shape[2] != 3 or clouds2.shape[2] != 3:
        raise RuntimeError("pairwise_EMD needs point-major (N, n, 3) clouds, got %s and %s"
                           % (tuple(clouds1.shape), tuple(clouds2.shape)))
    clouds1, clouds2 = clouds1.contiguous(), clouds2.contiguous()
    N1, n = clouds1.shape[0], clouds1.shape[1]
    N2, m = clouds2.shape[0], clouds2.shape[1]
    assert n == m, "Not sure what would EMD do in this case"
    dev = clouds1.device
    lo, hi = 0, N1
    if shard_rows:
        from .. import distributed as D
        lo, hi = D.shard_bounds(N1)
    emds = torch.empty((hi - lo, N2), dtype=torch.float32, device=dev)
    if hi > lo and N2 > 0 and n > 0:
        cols = max(1, min(N2, bs, 65535))                       # rows * cols pairs per launch: <= bs, and <= 65535 (grid y)
        rows = max(1, min(hi - lo, bs // cols, 65535 // cols))
        with torch.cuda.device(dev):
            st = current_stream()
            nbytes = lib().dpf_pairwise_emd_workspace_bytes(rows, cols, n, m)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            blk = torch.empty((rows * cols,), dtype=torch.float32, device=dev) if cols < N2 else None
            for r0 in range(lo, hi, rows):
                nr = min(rows, hi - r0)
                for c0 in range(0, N2, cols):
                    nc = min(cols, N2 - c0)
                    dst = emds[r0 - lo] if blk is None else blk
                    check(lib().dpf_pairwise_emd(nr, nc, n, m, clouds1[r0].data_ptr(), clouds2[c0].data_ptr(), dst.data_ptr(),
                                                 ws.data_ptr(), nbytes, st), "pairwise_emd")
                    if blk is not None:
                        emds[r0 - lo:r0 - lo + nr, c0:c0 + nc] = blk[:nr * nc].view(nr, nc)
        emds.div_(float(n))                                     # (the fp32 division of emd_approx, in place)
    if shard_rows:
        from .. import distributed as D
        emds = D.gather_clouds(emds)
    return emds


EMD_EXACT_MAX_ROUNDS = 1 << 20      # rounds per pair over all phases: ~100 times what Gaussian clouds of 2 048 points need (10 780)
EMD_EXACT_STATUS = {-1: "refused input (a non-finite coordinate or an extent whose square is not a normal float32)",
                    -2: "round cap reached (max_rounds)", -3: "bid range exceeded"}


def _emd_exact_check(x, name):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == 3 and x.is_contiguous()):
        raise RuntimeError("emd_exact: %s must be a contiguous float32 CUDA tensor of shape (B, n, 3); there is no CPU path" % name)


def _emd_exact_sizes(n, m, bits, max_rounds):
    from .._lib import lib
    if n != m:
        raise RuntimeError("emd_exact needs clouds of equal size, got %d and %d points" % (n, m))
    limit = lib().dpf_emd_exact_max_points()
    if n > limit:
        raise RuntimeError("emd_exact serves clouds of up to %d points, got %d" % (limit, n))
    if not 1 <= int(bits) <= 24 or int(max_rounds) < 0 or int(max_rounds) > 0x7fffffff:
        raise RuntimeError("emd_exact: bits must be in 1..24 and max_rounds in 0..2^31-1")


def _emd_exact_warn(status, what):
    """one RuntimeWarning naming the status of every unsolved pair (reads the statuses: a device synchronisation)"""
    bad = status[status < 0]
    if bad.numel():
        import warnings
        codes = sorted(set(bad.tolist()), reverse=True)
        warnings.warn("%s: %d of %d pairs not solved and set to NaN -- %s" % (
            what, bad.numel(), status.numel(), "; ".join("status %d: %s" % (c, EMD_EXACT_STATUS.get(c, "?")) for c in codes)),
            RuntimeWarning, stacklevel=3)


def _emd_exact_workspace(pairs, n, dev):
    from .._lib import lib
    nbytes = lib().dpf_emd_exact_workspace_bytes(pairs, n)
    return torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev), nbytes


def _emd_exact_normalise(cost, n):
    """cost <- fl32(cost / n), the correctly rounded fp32 quotient, in place.  Not cost.div_(n): for a Python scalar torch multiplies
    by fl32(1 / n) on the device, an ulp off for some costs unless n is a power of two (tests/test_gpu_emd_exact_edges.py: 3 of 15
    entries at n = 129).  In float64 the product with 1 / n is within 2^-52 (relative) of the quotient, while the quotient of a
    float32 by an integer n < 2^14 is never closer than 2^-38 to the midpoint of two float32 neighbours (the difference is a
    non-zero integer over 2 n 2^k): rounding the float64 result to float32 gives the quotient's own float32 rounding."""
    cost.copy_(cost.double().div_(float(n)))


class EMDExactFunction(torch.autograd.Function):
    """cost (B,) of the optimal matching as ONE autograd node: forward = one dpf_emd_exact launch, the assignment and its inverse
    kept for the backward, which is one dpf_emd_exact_grad launch for the inputs that need a gradient (the assignment is a constant,
    as in the reference's match_cost backward)."""

    @staticmethod
    def forward(ctx, sample, ref, bits, max_rounds, form, normalise):
        from .._lib import lib, check, current_stream
        B, n = sample.shape[0], sample.shape[1]
        dev = sample.device
        assignment = torch.empty((B, n), dtype=torch.int32, device=dev)
        inverse = torch.empty((B, n), dtype=torch.int32, device=dev)
        qcost = torch.empty((B,), dtype=torch.int64, device=dev)
        cost = torch.empty((B,), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        if B > 0 and n > 0:
            with torch.cuda.device(dev):
                ws, nbytes = _emd_exact_workspace(B, n, dev)
                check(lib().dpf_emd_exact(B, n, sample.data_ptr(), n * 3, ref.data_ptr(), n * 3, int(bits), int(max_rounds), int(form),
                                          assignment.data_ptr(), inverse.data_ptr(), qcost.data_ptr(), cost.data_ptr(),
                                          status.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "emd_exact")
        else:
            cost.zero_(); qcost.zero_(); status.zero_()
        ctx.scale = 1.0 / float(n) if normalise and n > 0 else 1.0
        if normalise and n > 0:
            _emd_exact_normalise(cost, n)
        ctx.save_for_backward(sample, ref)
        ctx.assignment, ctx.inverse = assignment, inverse          # indices ride on ctx, as in NNDistanceFunction
        ctx.mark_non_differentiable(assignment, qcost, status)
        return cost, assignment, qcost, status

    @staticmethod
    def backward(ctx, grad_cost, _ga, _gq, _gs):
        from .._lib import lib, check, current_stream
        sample, ref = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ga = torch.empty_like(sample) if need_a else None
        gb = torch.empty_like(ref) if need_b else None
        B, n = sample.shape[0], sample.shape[1]
        if (need_a or need_b) and B > 0 and n > 0:
            g = (grad_cost.float() * ctx.scale).contiguous()
            with torch.cuda.device(sample.device):
                check(lib().dpf_emd_exact_grad(B, n, sample.data_ptr(), ref.data_ptr(), ctx.assignment.data_ptr(), ctx.inverse.data_ptr(),
                                               g.data_ptr(), ga.data_ptr() if need_a else None, gb.data_ptr() if need_b else None,
                                               current_stream()), "emd_exact_grad")
        return ga, gb, None, None, None, None


def emd_exact_full(sample, ref, bits=20, max_rounds=EMD_EXACT_MAX_ROUNDS, form=0, normalise=False):
    """(cost (B,) fp32 -- divided by n only with normalise --, assignment (B, n) int32, qcost (B,) int64, status (B,) int32) of dpf_emd_exact
    (include/dpf_hip.h states the contract), with autograd through cost; no warning, no synchronisation.  form: 0 by size,
    1 / 2 force the resident / streamed kernel (tests and tools)."""
    _emd_exact_check(sample, "sample"); _emd_exact_check(ref, "ref")
    if sample.shape[0] != ref.shape[0]:
        raise RuntimeError("emd_exact needs as many clouds in both operands, got %d and %d" % (sample.shape[0], ref.shape[0]))
    _emd_exact_sizes(sample.shape[1], ref.shape[1], bits, max_rounds)
    return EMDExactFunction.apply(sample, ref, bits, max_rounds, form, normalise)


def emd_exact(sample, ref, return_assignment=False, bits=20, max_rounds=EMD_EXACT_MAX_ROUNDS):
    """(B,) exact EMD of equally sized clouds: the cost of the optimal one-to-one matching divided by n, emd_approx's normalisation.

    The matching is the exact optimum on an integer grid of 2^bits steps over the pair's extent (include/dpf_hip.h):
    its Euclidean cost is within 1.25 grid steps per point of the true optimum.  One autograd node; the backward treats the
    matching as a constant and computes only the gradients that are asked for.  return_assignment: also the (B, n) int32
    matching, point i of sample -> point assignment[i] of ref.
    sample, ref: contiguous float32 CUDA (B, n, 3), anything else raises RuntimeError -- there is no CPU path.
    max_rounds bounds the bidding rounds of a pair (default 2^20, about a hundred times what clouds of 2 048 points use).  A pair
    that is refused (non-finite or overflowing coordinates) or reaches the cap gives NaN (assignment -1) and one RuntimeWarning
    per call that names the status; looking at the statuses synchronises with the device."""
    out, assignment, _, status = emd_exact_full(sample, ref, bits, max_rounds, normalise=True)
    _emd_exact_warn(status, "emd_exact")
    return (out, assignment) if return_assignment else out


def pairwise_EMD_exact(clouds1, clouds2, bs=512, shard_rows=False, bits=20, max_rounds=EMD_EXACT_MAX_ROUNDS):
    """(N1, N2) matrix of exact EMDs, out[i, j] = emd_exact(clouds1[i:i+1], clouds2[j:j+1]) bit for bit: pairwise_EMD's shape,
    sharding and refusals with the exact matcher.  dpf_pairwise_emd_exact: one workgroup per pair, both sets read in place, no
    assignment written.  `bs` bounds the pairs of a launch (whole rows, at least one); an entry's bits do not depend on it.  Unsolved pairs are NaN
    and are named in one RuntimeWarning.  No autograd: inputs that would record a graph raise."""
    from .._lib import lib, check, current_stream
    if not (torch.is_tensor(clouds1) and torch.is_tensor(clouds2) and clouds1.is_cuda and clouds2.is_cuda):
        raise RuntimeError("pairwise_EMD_exact needs CUDA tensors")
    if clouds1.dtype != torch.float32 or clouds2.dtype != torch.float32:
        raise RuntimeError("pairwise_EMD_exact needs float32 clouds")
    if torch.is_grad_enabled() and (clouds1.requires_grad or clouds2.requires_grad):
        raise RuntimeError("pairwise_EMD_exact has no backward: call it under torch.no_grad() or on tensors that do not require grad")
    if clouds1.dim() != 3 or clouds2.dim() != 3 or clouds1.shape[2] != 3 or clouds2.shape[2] != 3:
        raise RuntimeError("pairwise_EMD_exact needs point-major (N, n, 3) clouds, got %s and %s"
                           % (tuple(clouds1.shape), tuple(clouds2.shape)))
    clouds1, clouds2 = clouds1.contiguous(), clouds2.contiguous()
    N1, n = clouds1.shape[0], clouds1.shape[1]
    N2 = clouds2.shape[0]
    _emd_exact_sizes(n, clouds2.shape[1], bits, max_rounds)
    dev = clouds1.device
    lo, hi = 0, N1
    if shard_rows:
        from .. import distributed as D
        lo, hi = D.shard_bounds(N1)
    emds = torch.empty((hi - lo, N2), dtype=torch.float32, device=dev)
    if hi > lo and N2 > 0 and n > 0:
        rows = max(1, min(hi - lo, max(1, int(bs)) // N2 if N2 <= bs else 1))
        status = torch.empty((hi - lo, N2), dtype=torch.int32, device=dev)
        qcost = torch.empty((rows, N2), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ws, nbytes = _emd_exact_workspace(rows * N2, n, dev)
            for r0 in range(lo, hi, rows):
                nr = min(rows, hi - r0)
                check(lib().dpf_pairwise_emd_exact(nr, N2, n, clouds1[r0].data_ptr(), clouds2.data_ptr(), int(bits), int(max_rounds), 0,
                                                   qcost.data_ptr(), emds[r0 - lo].data_ptr(), status[r0 - lo].data_ptr(),
                                                   ws.data_ptr(), nbytes, current_stream()), "pairwise_emd_exact")
        _emd_exact_normalise(emds, n)                           # (the division of emd_exact, in place)
        _emd_exact_warn(status, "pairwise_EMD_exact")
    if shard_rows:
        from .. import distributed as D
        emds = D.gather_clouds(emds)
    return emds


# ----------------------------------------------------------------------------------------------------------------
# The consumers of pairwise_CD in the reference's generative evaluation (evaluating.py:245-262): coverage, minimum matching
# distance and the 1-NN two-sample accuracy over the (N1, N2) Chamfer matrices, the voxel-occupancy Jensen-Shannon divergence
# over the clouds themselves, and the running-average helper of both loops.  Same names, arguments and values as
# lib/networks/utils.py:8-22, 45-87, 120-146; tensor / numpy plumbing -- the one kernel is the voxel binning of CUDA clouds.
# ----------------------------------------------------------------------------------------------------------------
class AverageMeter:
    """lib/networks/utils.py:8-22: last value, running sum / count / mean."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def COV(dists, axis=1):
    """Coverage (utils.py:120-121): the share of the clouds along `axis` that are the nearest neighbour of some cloud of the
    other set."""
    nearest = torch.argmin(dists, dim=axis)
    return float(torch.unique(nearest).numel()) / float(dists.shape[axis])


def MMD(dists, axis=1):
    """Minimum matching distance (utils.py:124-125): every cloud along `axis` to its nearest cloud of the other set, averaged."""
    return float(torch.amin(dists, dim=(axis + 1) % 2).float().mean())


def KNN(Mxx, Mxy, Myy, k, sqrt=False):
    """Leave-one-out k-NN two-sample accuracy (utils.py:128-146): the two sets are labelled -1 / +1, every cloud is classified
    by the sign of the label sum of its k nearest other clouds (ties go to +1); returns the share classified correctly."""
    n0, n1 = Mxx.shape[0], Myy.shape[0]
    label = torch.cat((-torch.ones(n0), torch.ones(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.t(), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    M = M + torch.diag(torch.full((n0 + n1,), float("inf")).to(Mxx))       # a cloud is not its own neighbour
    idx = torch.topk(M, k, dim=0, largest=False).indices                   # (k, n0 + n1): neighbours of every column
    votes = label[idx].sum(0)
    pred = torch.where(votes >= 0, torch.ones_like(votes), -torch.ones_like(votes))
    return float((pred == label).float().mean())


def get_voxel_occ_dist(all_clouds, clouds_flag='gen', res=28, bound=0.5, bs=128, warning=True):
    """Occupancy distribution of the points of all clouds over the res^3 voxels of [-0.5, 0.5)^3 (utils.py:45-80).
    all_clouds: (K, n, 3) numpy array.  A point outside the cube (or NaN) is not counted.  The bin edges are the reference's
    doubles -0.5 + i / res and the intervals half-open on the right, so every point lands in the voxel the reference
    picks; the counting is one bincount instead of batched comparison tables (`bs` is accepted and ignored).
    A CUDA float32 tensor (what evaluating.py:249 holds before its `.cpu().numpy()`) is binned where it is: one launch
    against the same table of edges (metrics/occupancy.py, dpf_occupancy_grid mode 0), and only the res^3 counts and the two
    diagnostics' flags come back.  Same return value, same two printed lines."""
    import numpy as np
    if isinstance(all_clouds, torch.Tensor) and all_clouds.is_cuda:
        from ..metrics.occupancy import cube_grid_counts
        counts, n_nans, out_of_bounds = cube_grid_counts(all_clouds, res, warn_bound=bound)
        if out_of_bounds and warning:
            print('{} clouds out of cube bounds: [-{}; {}]'.format(clouds_flag, bound, bound))
        if n_nans > 0:
            print('{} NaN values in point cloud tensors.'.format(n_nans))
        counts = counts.astype(np.uint64).reshape(res, res, res)
        return counts.astype(np.float64) / counts.sum()
    all_clouds = np.asarray(all_clouds)
    if np.any(np.fabs(all_clouds) > bound) and warning:
        print('{} clouds out of cube bounds: [-{}; {}]'.format(clouds_flag, bound, bound))
    n_nans = np.isnan(all_clouds).sum()
    if n_nans > 0:
        print('{} NaN values in point cloud tensors.'.format(n_nans))
    edges = -0.5 + np.arange(res + 1) * (1. / res)
    pts = all_clouds.reshape(-1, 3)
    cell = np.searchsorted(edges, pts, side='right') - 1                    # edges[c] <= x < edges[c + 1]; NaN sorts past the end
    inside = np.all((cell >= 0) & (cell < res), axis=1)
    cell = cell[inside]
    flat = (cell[:, 0] * res + cell[:, 1]) * res + cell[:, 2]
    counts = np.bincount(flat, minlength=res ** 3).astype(np.uint64).reshape(res, res, res)
    return np.float64(counts) / counts.sum()


def JSD(clouds1, clouds2, clouds1_flag='gen', clouds2_flag='ref', warning=True):
    """Jensen-Shannon divergence (base 2) between the voxel occupancy distributions of two sets of clouds (utils.py:83-87)."""
    from scipy.stats import entropy
    d1 = get_voxel_occ_dist(clouds1, clouds_flag=clouds1_flag, warning=warning).flatten()
    d2 = get_voxel_occ_dist(clouds2, clouds_flag=clouds2_flag, warning=warning).flatten()
    return entropy((d1 + d2) / 2.0, base=2) - 0.5 * (entropy(d1, base=2) + entropy(d2, base=2))


def save_model(state, model_name):
    """utils.py:25-27 (training.py's checkpoint writer): pickle protocol 4, one line on stdout."""
    torch.save(state, model_name, pickle_protocol=4)
    print('Model saved to ' + model_name)


def cnt_params(params):
    """utils.py:30-31: number of trainable scalars."""
    return sum(p.numel() for p in params if p.requires_grad)
