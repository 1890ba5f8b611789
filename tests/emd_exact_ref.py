"""The contract of dpf_emd_exact (include/dpf_hip.h) restated in numpy: the integer cost grid, float32 operation by operation,
and an integer epsilon-scaling auction over it -- the oracle of tests/test_gpu_emd_exact.py, itself checked against brute force and
scipy in tests/test_emd_exact_ref_cpu.py.  No scipy here: the GPU tests import this module.

The auction is the kernel's, statement for statement: synchronous rounds (every unassigned point of `a` bids on the prices of the
round's start), the lowest object index among equal values, per object the highest bid and then the lowest bidder, prices kept and
the assignment reset from phase to phase, epsilon from EPS0_SHIFT below the largest scaled cost down by EPS_SHIFT bits per phase
to 1.  So it also reports the rounds and bids the kernel should need."""
import numpy as np

F32 = np.float32
BITS = 20
N_MAX = 8192
EPS0_SHIFT = 4        # the first epsilon: ((n + 1) << bits) >> EPS0_SHIFT, at least 1
EPS_SHIFT = 3         # epsilon >>= EPS_SHIFT per phase, at least 1; the phase with epsilon == 1 is the last
STATUS_REFUSED = -1
STATUS_CAP = -2
STATUS_RANGE = -3
BID_LIMIT = 1 << 50   # a bid at or above it ends the pair with STATUS_RANGE (the kernel packs bid << 13 | tag into 63 bits)


def grid_scale(a, b, bits=BITS):
    """(status, s): status 0 and the power of two s of the cost grid, or 0 and s = 0 for a pair of zero extent, or STATUS_REFUSED."""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    pts = np.concatenate([a, b], 0)
    if not np.isfinite(pts).all():
        return STATUS_REFUSED, F32(0)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ext = (pts.max(0) - pts.min(0)).astype(F32)                  # fl32(hi - lo) per axis
        E = F32(ext.max())
        if not np.isfinite(E):
            return STATUS_REFUSED, F32(0)
        if E == 0:
            return 0, F32(0)
        E2 = F32(E * E)
        if not (np.isfinite(E2) and E2 >= np.finfo(F32).tiny) or not np.isfinite(F32(F32(3) * E2)):
            return STATUS_REFUSED, F32(0)
    _, ex = np.frexp(E)
    return 0, F32(np.ldexp(F32(1), bits - 1 - int(ex)))


def dist_matrix(a, b):
    """(n, n) float32 sqrt(((dx*dx + dy*dy) + dz*dz)), every operation rounded on its own (numpy's float32 sqrt is correctly rounded)"""
    a = np.asarray(a, F32)
    b = np.asarray(b, F32)
    d = (a[:, None, :] - b[None, :, :]).astype(F32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    d2 = ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)
    d2 = (d2 + (dz * dz).astype(F32)).astype(F32)
    return np.sqrt(d2).astype(F32)


def cost_matrix(a, b, bits=BITS):
    """(status, c, s): c (n, n) int64 = rint(dist * s), ties to even; all zeros for a pair of zero extent"""
    status, s = grid_scale(a, b, bits)
    n = np.asarray(a).shape[0]
    if status != 0:
        return status, None, s
    if s == 0:
        return 0, np.zeros((n, n), np.int64), s
    c = np.rint((dist_matrix(a, b) * s).astype(F32)).astype(np.int64)
    # d < sqrt(3) E and E s < 2^(bits - 1): below 2^bits from 2 bits on; at bits == 1 a diagonal of the extent's box can round to 2
    assert c.max() < (1 << bits) or (bits == 1 and c.max() == 2)
    return 0, c, s


def auction(c, bits=BITS, max_rounds=1 << 20):
    """c (n, n) int64 costs below 2^bits -> (status, assignment (n,) int32, rounds, bids).  Minimises sum c[i, assignment[i]]."""
    n = c.shape[0]
    if n == 1:
        return 0, np.zeros(1, np.int32), 0, 0
    u0 = c.astype(np.int64) * (n + 1)                                # what the kernel minimises: (n + 1) c_ij + price_j
    price = np.zeros(n, np.int64)
    eps = max(1, ((n + 1) << bits) >> EPS0_SHIFT)
    rounds = bids = 0
    rows = np.arange(n)
    while True:
        owner = np.full(n, -1, np.int64)
        free = rows.copy()
        while free.size:
            if rounds >= max_rounds:
                return STATUS_CAP, np.full(n, -1, np.int32), rounds, bids
            rounds += 1
            bids += free.size
            k = np.arange(free.size)
            u = u0[free] + price[None, :]
            j = u.argmin(1)                                          # the first minimum: the lowest object index
            u1 = u[k, j]
            u[k, j] = np.iinfo(np.int64).max
            u2 = u.min(1)
            bid = price[j] + (u2 - u1) + eps
            if (bid >= BID_LIMIT).any():
                return STATUS_RANGE, np.full(n, -1, np.int32), rounds, bids
            order = np.lexsort((free, -bid, j))                      # per object: the highest bid, then the lowest bidder, first
            first = np.ones(order.size, bool)
            first[1:] = j[order][1:] != j[order][:-1]
            win = order[first]
            lost = np.ones(free.size, bool)
            lost[win] = False
            evicted = owner[j[win]]
            owner[j[win]] = free[win]
            price[j[win]] = bid[win]
            free = np.concatenate([free[lost], evicted[evicted >= 0]])
        if eps == 1:
            break
        eps = max(1, eps >> EPS_SHIFT)
    assignment = np.empty(n, np.int32)
    assignment[owner] = rows
    return rounds, assignment, rounds, bids


def solve(a, b, bits=BITS, max_rounds=1 << 20):
    """The outputs of one pair as the header states them: dict(status, assignment, qcost, cost (float32, summed in ascending i),
    s, c, rounds, bids)."""
    n = np.asarray(a).shape[0]
    status, c, s = cost_matrix(a, b, bits)
    out = dict(status=status, assignment=np.full(n, -1, np.int32), qcost=-1, cost=F32(np.nan), s=s, c=c, rounds=0, bids=0)
    if status != 0:
        return out
    if s == 0:
        out.update(assignment=np.arange(n, dtype=np.int32), qcost=0, cost=F32(0))
        return out
    status, asg, rounds, bids = auction(c, bits, max_rounds)
    out.update(status=status, rounds=rounds, bids=bids)
    if status < 0:
        return out
    d = dist_matrix(a, b)[np.arange(n), asg]
    cost = F32(0)
    for x in d:
        cost = F32(cost + x)
    out.update(assignment=asg, qcost=int(c[np.arange(n), asg].sum()), cost=cost)
    return out


def cost64(a, b, assignment):
    """the float64 Euclidean cost of an assignment"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b[np.asarray(assignment)]) ** 2).sum(1)).sum())


def grad64(a, b, assignment, g):
    """float64 d(g * cost) / da, / db for a constant assignment; 0 where the matched distance is 0"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    asg = np.asarray(assignment)
    diff = a - b[asg]
    d = np.sqrt((diff ** 2).sum(1, keepdims=True))
    ga = np.where(d > 0, g * diff / np.where(d > 0, d, 1.0), 0.0)
    gb = np.zeros_like(b)
    gb[asg] = -ga
    return ga, gb


# ---- the case list of the GPU test (and of the K measurement on the CPU) ------------------------------------------------------
KINDS = ("gauss", "collapsed", "collinear", "lattice", "perm", "shift", "same")
# the kinds of tests/test_gpu_emd_exact_edges.py only (KINDS is the parametrisation of the first suite and of the K measurement)
EDGE_KINDS = ("jitter", "point", "point_signed")
JITTER = 2.0          # the noise of "jitter" in standard deviations of the cloud: the largest of the amplitudes tried at which the
                      # oracle still solves 4 096 and 4 097 points in under ten seconds (tests/test_gpu_emd_exact_edges.py has the table)


def scaling_edges(a, b, bits=BITS):
    """(lo, hi): the smallest and the largest k at which the pair scaled by 2^k (in float32) is still served, not refused.  Below lo
    E * E is no normal float32; above hi 3 * (E * E), or a coordinate, overflows."""
    def served(k):
        f = np.ldexp(F32(1), k)
        with np.errstate(over="ignore"):
            return grid_scale((np.asarray(a, F32) * f).astype(F32), (np.asarray(b, F32) * f).astype(F32), bits)[0] == 0
    assert served(0)
    lo = hi = 0
    while lo > -200 and served(lo - 1):
        lo -= 1
    while hi < 200 and served(hi + 1):
        hi += 1
    return lo, hi


def make_case(kind, n, seed):
    """(a, b, extra): two (n, 3) float32 clouds; extra: the permutation of "perm" and "jitter", the offset of "shift", else None"""
    rng = np.random.RandomState(seed)
    extra = None
    a = rng.randn(n, 3).astype(F32)
    if kind == "gauss":
        b = (rng.randn(n, 3) * 0.7 + 0.2).astype(F32)
    elif kind == "collapsed":                                        # all of b equal, half of a equal
        b = np.repeat(rng.randn(1, 3).astype(F32), n, 0)
        a[: n // 2] = a[0]
    elif kind == "collinear":
        t = rng.randn(n, 1).astype(F32)
        a = (t * np.array([[1.0, 2.0, -0.5]], F32)).astype(F32)
        b = (rng.randn(n, 1).astype(F32) * np.array([[1.0, 2.0, -0.5]], F32) + F32(0.25)).astype(F32)
    elif kind == "lattice":                                          # a 4 x 4 x 4 integer lattice against itself shifted by half a cell
        g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F32)
        a = g[rng.permutation(64)[np.arange(n) % 64]]
        b = (g[rng.permutation(64)[np.arange(n) % 64]] + F32(0.5)).astype(F32)
    elif kind == "perm":
        extra = rng.permutation(n).astype(np.int32)                  # b[j] = a[inverse(extra)[j]]: assignment == extra
        b = np.empty_like(a)
        b[extra] = a
    elif kind == "shift":
        a = (np.rint(a * F32(256)) / F32(256)).astype(F32)           # multiples of 2^-8: a + c is exact in float32
        extra = np.array([0.5, -0.25, 2.0], F32)
        b = (a + extra).astype(F32)
    elif kind == "same":
        b = a.copy()
    elif kind == "jitter":                                           # a permuted copy moved by a little noise: the matching is mostly
        extra = rng.permutation(n).astype(np.int32)                  # the permutation, and where it is not, objects change hands
        b = np.empty_like(a)
        b[extra] = a
        b = (b + rng.randn(n, 3).astype(F32) * F32(JITTER)).astype(F32)
    elif kind == "point":                                            # every point of both clouds the same: E == 0
        a = np.repeat(a[:1], n, 0)
        b = a.copy()
    elif kind == "point_signed":                                     # the same with zeros of both signs: -0.0 == +0.0, E == 0
        a = np.repeat(a[:1], n, 0)
        a[:, 1] = F32(0)
        b = a.copy()
        a[0::2, 1] = F32(-0.0)
        b[1::3, 1] = F32(-0.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), extra
