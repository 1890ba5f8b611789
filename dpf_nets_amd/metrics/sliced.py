"""Sliced 2-Wasserstein distance on the device (dpf_swd_*, include/dpf_hip.h; csrc/swd.hip): both clouds are projected on L
directions, every projection is sorted, and the 1-D optimal transport of a direction is the rank-to-rank match.  The sort belongs to a
cloud, not to a pair: an (N1, N2) matrix sorts (N1 + N2) * L projections once and then a pair costs L * n subtract-square-adds -- the
transport distance cheap enough for a whole pairwise matrix at full cloud size, and an O(n log n) transport loss.  The value is the
Monte-Carlo SW2^2 = sum_l sum_r (sa - sb)^2 / (L n): no square root.  There is no CPU path."""
import torch

from .._lib import lib, check, current_stream
from .fps import _strides

SWD_REFUSED = -1
TABLE_BUDGET_BYTES = 1 << 30        # pairwise_SWD: the two sets' sorted tables of one direction chunk stay under this


def sliced_directions(n_directions=128, seed=0, device=None):
    """(L, 3) fp32 unit directions: float64 Gaussian rows from a CPU torch.Generator seeded with `seed`, normalised in float64,
    rounded once to fp32, then moved to `device` -- the same on every machine for a given torch."""
    L = int(n_directions)
    if L < 1:
        raise ValueError("sliced_directions: n_directions must be at least 1, got %d" % L)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    d = torch.randn((L, 3), generator=gen, dtype=torch.float64, device="cpu")
    d = (d / d.norm(dim=1, keepdim=True)).to(torch.float32)
    return d if device is None else d.to(device)


def _need_cloud(clouds, what):
    if not (torch.is_tensor(clouds) and clouds.is_cuda and clouds.dtype == torch.float32 and clouds.dim() == 3):
        raise RuntimeError("%s needs float32 CUDA tensors of shape (B, n, 3), or (B, 3, N) with channels_first; there is no CPU path"
                           % what)


def _need_dirs(directions, dev, what):
    if not (torch.is_tensor(directions) and directions.dtype == torch.float32 and directions.dim() == 2 and directions.shape[1] == 3
            and directions.shape[0] >= 1):
        raise RuntimeError("%s needs directions as a float32 tensor of shape (L, 3)" % what)
    return directions.detach().to(dev).contiguous()


def sliced_tables(clouds, directions, channels_first=False, return_order=False, form=0):
    """The raw tables of dpf_swd_tables, no check of the statuses and no synchronisation: (sorted (B, L, n) fp32, status (B,) int32),
    or (sorted, order (B, L, n) int32, status) with return_order.  clouds: float32 CUDA, any strides, read in place; directions
    (L, 3) fp32, used as they are (not normalised).  form: 0 by size, 1, 2, 3 force a kernel form (tests and tools)."""
    _need_cloud(clouds, "sliced_tables")
    dev = clouds.device
    dirs = _need_dirs(directions, dev, "sliced_tables")
    B, n, sc, sp, sa = _strides(clouds, channels_first)
    limit = lib().dpf_swd_max_points()
    if not 1 <= n <= limit:
        raise RuntimeError("sliced_tables serves clouds of 1 to %d points, got %d" % (limit, n))
    src = clouds.detach()
    if min(sc, sp, sa) < 0:
        src = src.contiguous()
        B, n, sc, sp, sa = _strides(src, channels_first)
    L = dirs.shape[0]
    sorted_ = torch.empty((B, L, n), dtype=torch.float32, device=dev)
    order = torch.empty((B, L, n), dtype=torch.int32, device=dev) if return_order else None
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(lib().dpf_swd_tables(B, n, src.data_ptr(), sc, sp, sa, L, dirs.data_ptr(), int(form), sorted_.data_ptr(),
                                       order.data_ptr() if return_order else None, status.data_ptr(), current_stream()), "swd_tables")
    return (sorted_, order, status) if return_order else (sorted_, status)


def sliced_pair_sums(sorted_a, status_a, sorted_b, status_b, out=None, accumulate=False):
    """dpf_swd_pairs: (B,) float64 sums of squared differences of two tables, cloud b against cloud b; a table of one cloud
    broadcasts.  out/accumulate: add to an earlier call's sums (another chunk of directions)."""
    Ba, L, n = sorted_a.shape
    Bb = sorted_b.shape[0]
    if sorted_b.shape[1:] != (L, n) or not (Ba == Bb or Ba == 1 or Bb == 1):
        raise ValueError("sliced_pair_sums: tables of shapes %s and %s do not pair" % (tuple(sorted_a.shape), tuple(sorted_b.shape)))
    B = max(Ba, Bb)
    if out is None:
        out = torch.empty((B,), dtype=torch.float64, device=sorted_a.device)
        accumulate = False
    if B > 0:
        with torch.cuda.device(sorted_a.device):
            check(lib().dpf_swd_pairs(B, L, n, sorted_a.data_ptr(), status_a.data_ptr(), int(Ba == B), sorted_b.data_ptr(),
                                      status_b.data_ptr(), int(Bb == B), int(bool(accumulate)), out.data_ptr(), current_stream()),
                  "swd_pairs")
    return out


def sliced_matrix_sums(sorted1, status1, sorted2, status2, out=None, accumulate=False):
    """dpf_swd_pairwise: (N1, N2) float64 sums of squared differences of every cloud of table 1 against every cloud of table 2"""
    N1, L, n = sorted1.shape
    N2 = sorted2.shape[0]
    if sorted2.shape[1:] != (L, n):
        raise ValueError("sliced_matrix_sums: tables of shapes %s and %s do not pair" % (tuple(sorted1.shape), tuple(sorted2.shape)))
    if out is None:
        out = torch.empty((N1, N2), dtype=torch.float64, device=sorted1.device)
        accumulate = False
    if N1 > 0 and N2 > 0:
        with torch.cuda.device(sorted1.device):
            check(lib().dpf_swd_pairwise(N1, N2, L, n, sorted1.data_ptr(), status1.data_ptr(), sorted2.data_ptr(), status2.data_ptr(),
                                         int(bool(accumulate)), out.data_ptr(), current_stream()), "swd_pairwise")
    return out


def sliced_grad(directions, table_a, table_b, grad_cost, want_a=True, want_b=True):
    """dpf_swd_grad on two (sorted, order, status) tables of B clouds each: (grad_a, grad_b), each (B, n, 3) fp32 or None"""
    (sa, oa, sta), (sb, ob, stb) = table_a, table_b
    B, L, n = sa.shape
    dev = sa.device
    ga = torch.empty((B, n, 3), dtype=torch.float32, device=dev) if want_a else None
    gb = torch.empty((B, n, 3), dtype=torch.float32, device=dev) if want_b else None
    if B > 0 and (want_a or want_b):
        gc = grad_cost.detach().to(torch.float32).reshape(B).contiguous()
        nbytes = lib().dpf_swd_grad_workspace_bytes(B, L, n)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        with torch.cuda.device(dev):
            check(lib().dpf_swd_grad(B, L, n, directions.data_ptr(), sa.data_ptr(), ptr(oa), sta.data_ptr(), sb.data_ptr(), ptr(ob),
                                     stb.data_ptr(), gc.data_ptr(), ptr(ga), ptr(gb), ws.data_ptr(), nbytes, current_stream()),
                  "swd_grad")
    return ga, gb


def _swd_check(status, what, name):
    """ValueError naming the first refused cloud (reads the statuses: a device synchronisation)"""
    bad = torch.nonzero(status < 0)
    if bad.numel():
        raise ValueError("%s: cloud %d of %d of %s refused (a non-finite coordinate, direction or projection); %d refused in all"
                         % (what, int(bad[0, 0]), status.numel(), name, bad.shape[0]))


class _SlicedWasserstein(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, dirs, channels_first):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        tx = sliced_tables(x, dirs, channels_first, return_order=True) if need_x else \
            (lambda s, st: (s, None, st))(*sliced_tables(x, dirs, channels_first))
        ty = sliced_tables(y, dirs, channels_first, return_order=True) if need_y else \
            (lambda s, st: (s, None, st))(*sliced_tables(y, dirs, channels_first))
        _swd_check(tx[2], "sliced_wasserstein", "x")
        _swd_check(ty[2], "sliced_wasserstein", "y")
        sums = sliced_pair_sums(tx[0], tx[2], ty[0], ty[2])
        L, n = tx[0].shape[1], tx[0].shape[2]
        ctx.tables = (tx, ty) if (need_x or need_y) else None
        ctx.dirs = dirs
        ctx.channels_first = channels_first
        return (sums / float(L * n)).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_cost):
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None, None, None
        tx, ty = ctx.tables
        gx, gy = sliced_grad(ctx.dirs, tx, ty, grad_cost, need_x, need_y)
        if ctx.channels_first:
            gx = gx.transpose(1, 2) if gx is not None else None
            gy = gy.transpose(1, 2) if gy is not None else None
        return gx, gy, None, None


def sliced_wasserstein(x, y, directions=None, n_directions=128, seed=0, channels_first=False):
    """(B,) fp32 sliced 2-Wasserstein distance SW2^2 of cloud b of x against cloud b of y: the mean over the directions and the
    ranks of the squared difference of the two sorted projections (float64 sum, one rounding to fp32).

    x, y: float32 CUDA tensors (B, n, 3), or (B, 3, N) with channels_first, of any strides and EQUAL cloud size n <= 8192 (bring
    clouds of different sizes to a common one with farthest_point_sample first: ValueError otherwise); a CPU tensor raises
    RuntimeError.  directions: (L, 3) fp32, used as given; None draws sliced_directions(n_directions, seed).
    One autograd node: the forward is two table launches and one pair launch, the backward dpf_swd_grad with the sorting
    permutations as constants (as the matching is in emd_exact), computing only the gradients asked for; no gradient for the
    directions.  A cloud with a non-finite coordinate or projection is refused: ValueError naming the first such cloud (looking
    at the statuses synchronises with the device)."""
    _need_cloud(x, "sliced_wasserstein")
    _need_cloud(y, "sliced_wasserstein")
    if x.device != y.device:
        raise RuntimeError("sliced_wasserstein: x and y lie on different devices")
    nx, ny = (x.shape[2], y.shape[2]) if channels_first else (x.shape[1], y.shape[1])
    if nx != ny:
        raise ValueError("sliced_wasserstein needs clouds of equal size, got %d and %d points: bring them to a common size with "
                         "farthest_point_sample" % (nx, ny))
    if x.shape[0] != y.shape[0]:
        raise ValueError("sliced_wasserstein pairs cloud b of x with cloud b of y: got %d and %d clouds" % (x.shape[0], y.shape[0]))
    if directions is None:
        directions = sliced_directions(n_directions, seed, x.device)
    dirs = _need_dirs(directions, x.device, "sliced_wasserstein")
    return _SlicedWasserstein.apply(x, y, dirs, bool(channels_first))


def pairwise_SWD(clouds1, clouds2, directions=None, n_directions=128, seed=0, dir_chunk=None):
    """(N1, N2) fp32 matrix of SW2^2 of every cloud of clouds1 against every cloud of clouds2 (float32 CUDA (N, n, 3), equal n), no
    autograd.  Each set's tables are built ONCE per chunk of directions -- (N1 + N2) * L sorts in all -- and the matrix kernel adds
    the chunk's float64 sums to the earlier chunks', in ascending order of the directions.  dir_chunk: directions per chunk;
    None takes the most for which the two sorted tables of a chunk ((N1 + N2) * chunk * n * 4 bytes) stay under
    TABLE_BUDGET_BYTES = 1 GiB.  A refused cloud gives NaN in its row or column (no exception: reading statuses would synchronise)."""
    _need_cloud(clouds1, "pairwise_SWD")
    _need_cloud(clouds2, "pairwise_SWD")
    if clouds1.shape[1] != clouds2.shape[1]:
        raise ValueError("pairwise_SWD needs clouds of equal size, got %d and %d points: bring them to a common size with "
                         "farthest_point_sample" % (clouds1.shape[1], clouds2.shape[1]))
    dev = clouds1.device
    if directions is None:
        directions = sliced_directions(n_directions, seed, dev)
    dirs = _need_dirs(directions, dev, "pairwise_SWD")
    N1, n, _ = clouds1.shape
    N2 = clouds2.shape[0]
    L = dirs.shape[0]
    if dir_chunk is None:
        dir_chunk = max(1, min(L, TABLE_BUDGET_BYTES // max(1, (N1 + N2) * n * 4)))
    dir_chunk = int(dir_chunk)
    if dir_chunk < 1:
        raise ValueError("pairwise_SWD: dir_chunk must be at least 1, got %d" % dir_chunk)
    with torch.no_grad():
        sums = torch.zeros((N1, N2), dtype=torch.float64, device=dev)
        same = clouds1 is clouds2
        for l0 in range(0, L, dir_chunk):
            d = dirs[l0:l0 + dir_chunk]
            s1, st1 = sliced_tables(clouds1, d)
            s2, st2 = (s1, st1) if same else sliced_tables(clouds2, d)
            sliced_matrix_sums(s1, st1, s2, st2, out=sums, accumulate=l0 > 0)
        return (sums / float(L * n)).to(torch.float32)
