"""Same five functions the reference's pybind module exports
(lib/metrics/pytorch_structural_losses/pybind/bind.cpp:9-15), same argument and
return conventions as its ATen glue (src/structural_loss.cpp:22-124): the caller
side allocates every output with torch.empty on the input's device, inputs must
be contiguous device tensors (CHECK_INPUT, structural_loss.cpp:10-12), launches
go to the current stream and do not synchronise.  The kernels live in
libdpf_hip.so (csrc/chamfer.hip, csrc/emd.hip)."""
import os

import torch

from ..._lib import lib, check, current_stream


# Chamfer forward implementation; all return identical bits (tests/test_gpu_chamfer.py):
#   "auto"   (default) dpf_nndistance_auto: "mfma" for big problems (>= 1e8 pair evaluations, >= 64 workgroups of 256 queries),
#            "brute" otherwise
#   "brute"  O(n*m) exact VALU scan at ~80 % of its issue bound, data-independent cost
#   "mfma"   matrix-core filter (one bf16 MFMA per 32x32 pairs) + exact verification of the few candidates that can
#            win, fragments built in the kernel; r01: 25 us vs 52 us brute on cfg-2, 76 vs 190 us at B=8, N=8192
NN_IMPL = os.environ.get("DPF_CHAMFER_IMPL", "auto")
EMD_GRAD_TWO_PASS = bool(int(os.environ.get("DPF_EMD_GRAD_TWO_PASS", "0")))   # 1: separate grad1 / grad2 kernels
EMD_RMW = bool(int(os.environ.get("DPF_EMD_RMW", "0")))   # 1: the reference's per-level read-modify-write of `match`
EMD_LEAN_GRAD = bool(int(os.environ.get("DPF_EMD_LEAN_GRAD", "0")))   # 1: match_cost never stores the matching (match_cost_lean)


def nn_impl_entry(impl):
    """(workspace_bytes, launcher) of a workspace-taking Chamfer implementation"""
    L = lib()
    return {"mfma": (L.dpf_nndistance_mfma_workspace_bytes, L.dpf_nndistance_mfma)}[impl]


def _check_input(x, name, dtype=torch.float32):
    # mirrors CHECK_CUDA / CHECK_CONTIGUOUS (AT_ASSERTM -> RuntimeError)
    if not x.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not x.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if x.dtype != dtype:
        raise RuntimeError("%s must be %s" % (name, dtype))


def _dims(set_d, set_q):
    if set_d.dim() != 3 or set_q.dim() != 3 or set_d.shape[2] != 3 or set_q.shape[2] != 3 \
            or set_d.shape[0] != set_q.shape[0]:
        raise RuntimeError("expected (B, n, 3) and (B, m, 3) point clouds")
    return set_d.shape[0], set_d.shape[1], set_q.shape[1]


def NNDistance(set_d, set_q):
    """-> [dist1 (B,n), idx1 (B,n) int32, dist2 (B,m), idx2 (B,m) int32]   structural_loss.cpp:80-99"""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    b, n, m = _dims(set_d, set_q)
    dev = set_d.device
    dist1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        args = (b, n, set_d.data_ptr(), m, set_q.data_ptr(), dist1.data_ptr(), idx1.data_ptr(), dist2.data_ptr(),
                idx2.data_ptr())
        if NN_IMPL == "auto":
            check(lib().dpf_nndistance_auto(*args, current_stream()), "nndistance_auto")
        elif NN_IMPL == "brute":
            check(lib().dpf_nndistance(*args, current_stream()), "nndistance")
        else:   # same bits; scratch is caller-owned like every other buffer
            sized, fn = nn_impl_entry(NN_IMPL)
            nbytes = sized(b, n, m)
            ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
            check(fn(*args, ws.data_ptr(), nbytes, current_stream()), "nndistance_" + NN_IMPL)
    return [dist1, idx1, dist2, idx2]


class CDWorkspace:
    """Caller-owned scratch of NNDistanceCD for one problem size: one ticket per cloud (zero between calls -- the kernel's
    last arriver resets its own) and the workgroups' partial sums.  Owned like every other buffer of this interface
    (SURVEY 8b "ownership"): create it once per (shape, stream) OUTSIDE any stream capture, pass it to every call, use it
    from one stream at a time, and drop it with the stream.  A call that raises marks it dirty and the next call clears
    the tickets first.  Without one NNDistanceCD takes a fresh workspace per call and lets the library clear the tickets
    in-call (one tiny extra kernel, csrc/zero_fill.h): nothing is cached behind the caller's back, so an asynchronous
    fault or a recycled stream handle cannot leave a stale ticket for a later call."""

    def __init__(self, b, n, m, device):
        self.shape = (int(b), int(n), int(m))
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.nbytes = lib().dpf_nndistance_cd_workspace_bytes(*self.shape)
        self.buf = torch.zeros((self.nbytes,), dtype=torch.uint8, device=self.device)
        self.dirty = False

    def tickets(self):
        return self.buf[:4 * self.shape[0]].view(torch.int32)


def NNDistanceCD(set_d, set_q, workspace=None):
    """NNDistance plus cd (B,) = dist1.mean(1) + dist2.mean(1) (evaluating.py:112) -> [dist1, idx1, dist2, idx2, cd]; the
    reduction rides on the search kernel's workgroups (dpf_nndistance_cd) instead of a pass over the distances.
    workspace: a CDWorkspace of this problem size (one launch per call), or None (fresh scratch, tickets cleared in-call)."""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    b, n, m = _dims(set_d, set_q)
    dev = set_d.device
    if workspace is not None and (workspace.shape != (b, n, m) or workspace.device != dev):
        raise RuntimeError("NNDistanceCD: the workspace was made for %r on %s" % (workspace.shape, workspace.device))
    dist1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    cd = torch.empty((b,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if workspace is None:
            nbytes = lib().dpf_nndistance_cd_workspace_bytes(b, n, m)
            ws, tickets_are_zero = torch.empty((nbytes,), dtype=torch.uint8, device=dev), 0
        else:
            nbytes, ws, tickets_are_zero = workspace.nbytes, workspace.buf, 0 if workspace.dirty else 1
            workspace.dirty = True                      # until the launch has been issued without an error
        check(lib().dpf_nndistance_cd(b, n, set_d.data_ptr(), m, set_q.data_ptr(), dist1.data_ptr(), idx1.data_ptr(),
                                      dist2.data_ptr(), idx2.data_ptr(), cd.data_ptr(), ws.data_ptr(), nbytes,
                                      tickets_are_zero, current_stream()), "nndistance_cd")
        if workspace is not None:
            workspace.dirty = False
    return [dist1, idx1, dist2, idx2, cd]


def _grad_scratch(b, n, m, dev):
    """the deterministic backward's caller-owned scratch (nothing in it has to be zero) -> (tensor or None, pointer, bytes)"""
    nbytes = lib().dpf_nndistancegrad_det_workspace_bytes(b, n, m)
    if not nbytes:
        return None, None, 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws, ws.data_ptr(), nbytes


def NNDistanceGrad(set_d, set_q, idx1, idx2, grad_dist1, grad_dist2, deterministic=False):
    """-> [grad1 (B,n,3), grad2 (B,m,3)]                                    structural_loss.cpp:101-124
    deterministic=True: the additions of the scattered term in ascending query order (dpf_nndistancegrad_det) instead of the
    reference's atomics -- the same bits on every run, within the same tolerances."""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    _check_input(idx1, "idx1", torch.int32); _check_input(idx2, "idx2", torch.int32)
    _check_input(grad_dist1, "grad_dist1"); _check_input(grad_dist2, "grad_dist2")
    b, n, m = _dims(set_d, set_q)
    if deterministic and (idx1.numel() != b * n or grad_dist1.numel() != b * n or idx2.numel() != b * m or grad_dist2.numel() != b * m):
        raise RuntimeError("expected idx1 / grad_dist1 (B, n) and idx2 / grad_dist2 (B, m)")
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=set_d.device)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=set_d.device)
    with torch.cuda.device(set_d.device):
        if deterministic:
            ws, wsp, nbytes = _grad_scratch(b, n, m, set_d.device)
            check(lib().dpf_nndistancegrad_det(b, n, set_d.data_ptr(), m, set_q.data_ptr(), grad_dist1.data_ptr(),
                                               idx1.data_ptr(), grad_dist2.data_ptr(), idx2.data_ptr(), grad1.data_ptr(),
                                               grad2.data_ptr(), wsp, nbytes, current_stream()), "nndistancegrad_det")
        else:
            check(lib().dpf_nndistancegrad(b, n, set_d.data_ptr(), m, set_q.data_ptr(), grad_dist1.data_ptr(),
                                           idx1.data_ptr(), grad_dist2.data_ptr(), idx2.data_ptr(), grad1.data_ptr(),
                                           grad2.data_ptr(), current_stream()), "nndistancegrad")
    return [grad1, grad2]


def ChamferCDBackward(set_d, set_q, idx1, idx2, grad_cd, need1=True, need2=True):
    """The backward of cd (B,) = dist1.mean(1) + dist2.mean(1) in one call -> [grad1 (B,n,3) | None, grad2 (B,m,3) | None]:
    NNDistanceGrad(deterministic=True) with grad_dist1 = grad_cd / n and grad_dist2 = grad_cd / m, neither of them materialised
    (dpf_chamfer_cd_backward).  An output that is not needed is neither computed nor allocated."""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    _check_input(idx1, "idx1", torch.int32); _check_input(idx2, "idx2", torch.int32)
    _check_input(grad_cd, "grad_cd")
    b, n, m = _dims(set_d, set_q)
    if idx1.numel() != b * n or idx2.numel() != b * m or grad_cd.numel() != b:
        raise RuntimeError("expected idx1 (B, n), idx2 (B, m) and grad_cd (B,)")
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if need1 else None
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if need2 else None
    if not (need1 or need2):
        return [None, None]
    with torch.cuda.device(dev):
        ws, wsp, nbytes = _grad_scratch(b, n, m, dev)
        check(lib().dpf_chamfer_cd_backward(b, n, set_d.data_ptr(), m, set_q.data_ptr(), idx1.data_ptr(), idx2.data_ptr(),
                                            grad_cd.data_ptr(), grad1.data_ptr() if need1 else None,
                                            grad2.data_ptr() if need2 else None, wsp, nbytes, current_stream()),
              "chamfer_cd_backward")
    return [grad1, grad2]


def ApproxMatch(set_d, set_q):
    """-> [match (B,m,n), temp (B, 2(n+m))]                                 structural_loss.cpp:22-37"""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    b, n, m = _dims(set_d, set_q)
    match = torch.empty((b, m, n), dtype=torch.float32, device=set_d.device)
    temp = torch.empty((b, (n + m) * 2), dtype=torch.float32, device=set_d.device)
    with torch.cuda.device(set_d.device):
        if EMD_RMW:
            check(lib().dpf_approxmatch(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(),
                                        temp.data_ptr(), current_stream()), "approxmatch")
        else:   # `match` written once (scratch for the per-level ratio vectors is caller-owned).  Within the 1e-4 cost contract of
                # the read-modify-write path, NOT bit-identical to it since r05: in range the passes run on the matrix cores
                # (include/dpf_hip.h at dpf_emd_set_matrix_path; dpf_emd_set_matrix_path(0) selects the bit-identical kernels)
            nbytes = lib().dpf_approxmatch_workspace_bytes(b, n, m)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=set_d.device)
            check(lib().dpf_approxmatch_ws(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(),
                                           temp.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "approxmatch_ws")
    return [match, temp]


def ApproxMatchCost(set_d, set_q):
    """ApproxMatch followed by MatchCost (match_cost.py:20-22) in one call -> [match (B,m,n), temp, cost (B,)]: the
    pass that materialises the matching also sums match * distance (dpf_approxmatch_cost_ws)."""
    if EMD_RMW:
        match, temp = ApproxMatch(set_d, set_q)
        return [match, temp, MatchCost(set_d, set_q, match)]
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    b, n, m = _dims(set_d, set_q)
    dev = set_d.device
    match = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    temp = torch.empty((b, (n + m) * 2), dtype=torch.float32, device=dev)
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib().dpf_approxmatch_workspace_bytes(b, n, m)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        check(lib().dpf_approxmatch_cost_ws(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(), temp.data_ptr(),
                                            cost.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "approxmatch_cost_ws")
    return [match, temp, cost]


def ApproxMatchCostOnly(set_d, set_q):
    """ApproxMatchCost without the matching -> [temp, cost (B,), saved]: same bits of `temp[:, :n+m]` and `cost`, nothing of size
    n*m allocated or written (dpf_approxmatch_costonly_ws).  `saved` is the call's workspace: the state MatchCostGradRecompute
    rebuilds the matching from -- keep it, and the two clouds, unchanged until then."""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q")
    b, n, m = _dims(set_d, set_q)
    dev = set_d.device
    temp = torch.empty((b, (n + m) * 2), dtype=torch.float32, device=dev)
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib().dpf_approxmatch_workspace_bytes(b, n, m)
        saved = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        check(lib().dpf_approxmatch_costonly_ws(b, n, m, set_d.data_ptr(), set_q.data_ptr(), temp.data_ptr(), cost.data_ptr(),
                                                saved.data_ptr(), nbytes, current_stream()), "approxmatch_costonly_ws")
    return [temp, cost, saved]


def MatchCostGradRecompute(set_d, set_q, saved):
    """MatchCostGrad without a stored matching -> [grad1 (B,n,3), grad2 (B,m,3)]: the weights are rebuilt in registers from
    `saved` (ApproxMatchCostOnly of the same clouds), which is only read (dpf_matchcostgrad_recompute_ws)."""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q"); _check_input(saved, "saved", torch.uint8)
    b, n, m = _dims(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if saved.device != dev or saved.numel() < lib().dpf_approxmatch_workspace_bytes(b, n, m):
            raise RuntimeError("MatchCostGradRecompute: `saved` is not ApproxMatchCostOnly's workspace of these clouds")
        nbytes = lib().dpf_matchcostgrad_recompute_workspace_bytes(b, n, m)
        scratch = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        check(lib().dpf_matchcostgrad_recompute_ws(b, n, m, set_d.data_ptr(), set_q.data_ptr(), saved.data_ptr(), saved.numel(),
                                                   grad1.data_ptr(), grad2.data_ptr(), scratch.data_ptr(), nbytes,
                                                   current_stream()), "matchcostgrad_recompute_ws")
    return [grad1, grad2]


def MatchCost(set_d, set_q, match):
    """-> cost (B,)                                                         structural_loss.cpp:39-52"""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q"); _check_input(match, "match")
    b, n, m = _dims(set_d, set_q)
    out = torch.empty((b,), dtype=torch.float32, device=set_d.device)
    with torch.cuda.device(set_d.device):
        check(lib().dpf_matchcost(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(), out.data_ptr(),
                                  current_stream()), "matchcost")
    return out


def MatchCostGrad(set_d, set_q, match):
    """-> [grad1 (B,n,3), grad2 (B,m,3)]                                    structural_loss.cpp:54-69"""
    _check_input(set_d, "set_d"); _check_input(set_q, "set_q"); _check_input(match, "match")
    b, n, m = _dims(set_d, set_q)
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=set_d.device)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=set_d.device)
    with torch.cuda.device(set_d.device):
        if EMD_GRAD_TWO_PASS:
            check(lib().dpf_matchcostgrad(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(),
                                          grad1.data_ptr(), grad2.data_ptr(), current_stream()), "matchcostgrad")
        else:   # `match` read once; partial sums in caller-owned scratch
            nbytes = lib().dpf_matchcostgrad_workspace_bytes(b, n, m)
            ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=set_d.device)
            check(lib().dpf_matchcostgrad_ws(b, n, m, set_d.data_ptr(), set_q.data_ptr(), match.data_ptr(),
                                             grad1.data_ptr(), grad2.data_ptr(), ws.data_ptr(), nbytes,
                                             current_stream()), "matchcostgrad_ws")
    return [grad1, grad2]
