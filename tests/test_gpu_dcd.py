"""dpf_dcd (csrc/dcd.hip) on the device against tests/dcd_ref.py, the numpy restatement of include/dpf_hip.h.  Counts and statuses are
compared for equality; loss and halves against the float64 restatement within dcd_ref.dcd_bound of the shape, relative to max(1, frac1,
frac2) (device exp / pow are not correctly rounded); the coefficients within one fp32 rounding: 2^-23 relative plus one fp32 subnormal.
The two forms, repeats, and a cloud alone against the same cloud in a batch are compared bit for bit.  The C ABI is called directly,
with sentinel guards around every output and the workspace; dist / idx are hand-made on the host, so hostile inputs need no search.
Failing without the feature: nothing exports metrics.density_aware_chamfer or dpf_dcd on the parent commit.

Worst deviation of loss / halves from the restatement measured on the MI355X over the cases of this file: 1.39e-16 relative to
max(1, frac1, frac2) (1.25 roundings of a float64; 0 in most cases), against bounds from 2.4e-15 (one point) to 3.4e-14 (32769)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dcd_ref as D                                                                          # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
ALPHAS = (1.0, 40.0, 1000.0)
OUTPUTS = ("loss", "halves", "count1", "count2", "coef1", "coef2", "status")
WORST = {"loss": 0.0}


def _dev():
    return torch.device("cuda", 0)


class Guarded:
    """an output with GUARD sentinel elements on either side"""

    def __init__(self, shape, dtype):
        count = int(np.prod(shape))
        self.sentinel = -77 if dtype in (torch.int32,) else -7.7e7
        self.buf = torch.full((count + 2 * GUARD,), self.sentinel, dtype=dtype, device=_dev())
        self.view = self.buf[GUARD:GUARD + count].view(*shape)

    def ptr(self):
        return self.view.data_ptr()

    def take(self):
        edge = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((edge == self.sentinel).all()), "an output was written outside its extent"
        return self.view.cpu().numpy()


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def raw(case, alpha=1000.0, n_lambda=1.0, non_reg=False, form=0, skip=(), fill=None, rc_only=False):
    """case: (dist1 (B, n), idx1, dist2 (B, m), idx2) numpy -> dict of numpy outputs, guards checked.  skip: optional outputs passed
    as NULL; fill: a byte the workspace is filled with (the sentinel otherwise: dirty either way)"""
    from dpf_nets_amd._lib import lib, check, current_stream
    d1, i1, d2, i2 = (cuda(a) for a in case)
    B, n = d1.shape
    m = d2.shape[1]
    o = dict(loss=Guarded((B,), torch.float64), halves=Guarded((B, 2), torch.float64), count1=Guarded((B, n), torch.int32),
             count2=Guarded((B, m), torch.int32), coef1=Guarded((B, n), torch.float32), coef2=Guarded((B, m), torch.float32),
             status=Guarded((B,), torch.int32))
    nbytes = lib().dpf_dcd_workspace_bytes(B, n, m)
    ws = Guarded(((nbytes + 7) // 8,), torch.float64)
    if fill is not None:
        ws.view.view(torch.uint8).fill_(fill)
    ptr = lambda k: None if k in skip else o[k].ptr()                                        # noqa: E731
    rc = lib().dpf_dcd(B, n, m, d1.data_ptr(), i1.data_ptr(), d2.data_ptr(), i2.data_ptr(), float(alpha), float(n_lambda), int(non_reg),
                       int(form), ptr("loss"), ptr("halves"), ptr("count1"), ptr("count2"), ptr("coef1"), ptr("coef2"), ptr("status"),
                       ws.ptr(), nbytes, current_stream())
    if rc_only:
        return rc
    check(rc, "dcd")
    torch.cuda.synchronize()
    ws.take()
    return {k: v.take() for k, v in o.items()}


def batch(kinds, n, m, seed):
    each = [D.make(kind, n, m, seed + 10 * b) for b, kind in enumerate(kinds)]
    return tuple(np.stack([e[k] for e in each]) for k in range(4))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def bit_equal(x, y, what, keys=OUTPUTS):
    for k in keys:
        assert x[k].dtype == y[k].dtype and same(x[k].view(np.uint8), y[k].view(np.uint8)), (what, k)


def against_the_restatement(got, case, alpha, n_lambda, non_reg, what):
    n, m = case[0].shape[1], case[2].shape[1]
    ref = D.dcd_batch(*case, alpha=alpha, n_lambda=n_lambda, non_reg=non_reg)
    for k in ("count1", "count2", "status"):
        assert same(got[k], ref[k]), (what, k)
    scale = max(1.0, n / m, m / n)
    bound = D.dcd_bound(n, m)
    dev = max(np.abs(got["loss"] - ref["loss"]).max(), np.abs(got["halves"] - ref["halves"]).max()) / scale
    WORST["loss"] = max(WORST["loss"], dev)
    print("%s: loss deviation %.3g (bound %.3g); worst so far %.3g" % (what, dev, bound, WORST["loss"]))
    assert dev <= bound, (what, dev, bound)
    for k in ("coef1", "coef2"):
        r = ref[k].astype(np.float64)
        assert (np.abs(got[k].astype(np.float64) - r) <= 2.0 ** -23 * np.abs(r) + 2.0 ** -149).all(), (what, k)
    return ref


@pytest.mark.parametrize("n", SIZES)
def test_every_block_edge_against_the_restatement_in_both_forms(n):
    """n, m over the edges of the 256-block and its tree, B in {1, 3}; the kinds, alpha and n_lambda rotate through the shapes"""
    for j, m in enumerate(SIZES):
        turn = SIZES.index(n) + j
        for B in (1, 3):
            kinds = [D.KINDS[(turn + b + B) % len(D.KINDS)] for b in range(B)]
            alpha, n_lambda, non_reg = ALPHAS[turn % 3], (1.0, 1.0, 0.5, 0.0, 2.0)[(turn + B) % 5], bool(turn & 1)
            case = batch(kinds, n, m, 1000 * n + m)
            what = "n %d m %d B %d %s alpha %g lambda %g non_reg %d" % (n, m, B, "/".join(kinds), alpha, n_lambda, non_reg)
            one = raw(case, alpha, n_lambda, non_reg, form=1)
            two = raw(case, alpha, n_lambda, non_reg, form=2)
            bit_equal(one, two, what)
            against_the_restatement(one, case, alpha, n_lambda, non_reg, what)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_kind_at_every_alpha_and_exponent(alpha):
    n, m = 257, 513
    case = batch(D.KINDS, n, m, 7)
    assert (case[1][0] == case[1][0, 0]).all() and (D.counts(case[1][0], m) == n).all()      # "one": count = n, the atomic worst case
    assert (D.counts(case[1][1], m) == 1).all()                                              # "perm" (n <= m): every count 1
    assert (np.exp(-(1.0 * case[0][4].astype(np.float64))) == 0).all() and (case[0][3] == 0).all()
    for n_lambda in (0.0, 0.5, 1.0, 2.0):
        for non_reg in (False, True):
            what = "kinds at alpha %g lambda %g non_reg %d" % (alpha, n_lambda, non_reg)
            one = raw(case, alpha, n_lambda, non_reg, form=1)
            bit_equal(one, raw(case, alpha, n_lambda, non_reg, form=2), what)
            ref = against_the_restatement(one, case, alpha, n_lambda, non_reg, what)
            assert (one["halves"][4] == 1.0).all() and (one["coef1"][4] == 0).all()           # e underflows: every term is 1
            if n_lambda in (0.0, 1.0):
                assert same(one["halves"][3], ref["halves"][3])                              # distances of 0 and no pow: exp(-0) = 1 in any library


def test_the_cap_of_the_one_workgroup_form_and_one_past_it():
    cap = D.LDS_TARGETS
    for n, m, kind in ((cap, cap, "one"), (cap + 1, cap, "random"), (cap, cap + 1, "one")):
        case = batch((kind,), n, m, 5)
        by_size = raw(case, 40.0, form=0)
        against_the_restatement(by_size, case, 40.0, 1.0, False, "n %d m %d by size" % (n, m))
        bit_equal(by_size, raw(case, 40.0, form=2), "n %d m %d, the workspace form" % (n, m))
        if max(n, m) <= cap:
            bit_equal(by_size, raw(case, 40.0, form=1), "the cap, the one-workgroup form")
            assert (by_size["count1"] == n).all() and (by_size["count2"] == m).all()
        else:
            assert raw(case, 40.0, form=1, rc_only=True) == -2                               # DPF_ENOSUP: forced past its cap


def test_repeats_a_cloud_alone_and_a_dirty_workspace_give_the_same_bits():
    n, m = 513, 257
    case = batch(("random", "one", "perm"), n, m, 3)
    for form in (1, 2):
        first = raw(case, 40.0, 0.5, form=form)
        bit_equal(first, raw(case, 40.0, 0.5, form=form), "a repeat, form %d" % form)
        for fill in (0x00, 0xFF, 0x5A):
            bit_equal(first, raw(case, 40.0, 0.5, form=form, fill=fill), "workspace filled with %#x, form %d" % (fill, form))
        for b in range(3):
            alone = raw(tuple(a[b:b + 1] for a in case), 40.0, 0.5, form=form)
            for k in OUTPUTS:
                assert same(first[k][b:b + 1].view(np.uint8), alone[k].view(np.uint8)), (form, b, k)


def test_one_index_out_of_range_refuses_its_cloud_alone():
    n, m = 300, 257
    clean = batch(("random", "random", "perm"), n, m, 9)
    for which, value in ((1, m), (1, -1), (3, n), (3, 2 ** 31 - 1)):
        case = tuple(a.copy() for a in clean)
        case[which][1, 299 if which == 1 else 256] = value
        for form in (1, 2):
            got = raw(case, 40.0, form=form)
            assert got["status"].tolist() == [0, D.REFUSED, 0]
            assert np.isnan(got["loss"][1]) and np.isnan(got["halves"][1]).all() and np.isnan(got["coef1"][1]).all() and np.isnan(got["coef2"][1]).all()
            assert (got["count1"][1] == -1).all() and (got["count2"][1] == -1).all()
            for b in (0, 2):
                alone = raw(tuple(a[b:b + 1] for a in clean), 40.0, form=form)
                for k in OUTPUTS:
                    assert same(got[k][b:b + 1].view(np.uint8), alone[k].view(np.uint8)), (which, value, form, b, k)
            ref = D.dcd_batch(*case, alpha=40.0)
            assert same(got["status"], ref["status"]) and same(got["count1"], ref["count1"]) and same(got["count2"], ref["count2"])
    # distances that are negative or not finite are served: they go through the arithmetic
    odd = tuple(a.copy() for a in clean)
    odd[0][0, 3], odd[0][0, 4], odd[2][2, 5] = np.nan, -1.0, np.inf
    one, two = raw(odd, 1.0, form=1), raw(odd, 1.0, form=2)
    for k in OUTPUTS:
        assert same(one[k], two[k]), k                                                       # (NaN equals NaN: its payload is not part of the contract)
    ref = D.dcd_batch(*odd, alpha=1.0)
    assert one["status"].tolist() == [0, 0, 0] and np.isnan(one["loss"][0]) and np.isnan(one["coef1"][0, 3]) and one["coef2"][2, 5] == 0
    assert same(np.isnan(one["halves"]), np.isnan(ref["halves"])) and abs(one["loss"][2] - ref["loss"][2]) <= D.dcd_bound(n, m) * max(n / m, 1.0)
    assert abs(one["coef1"][0, 4] - ref["coef1"][0, 4]) <= 2.0 ** -23 * ref["coef1"][0, 4]


def test_null_outputs_and_return_codes():
    from dpf_nets_amd._lib import lib
    n, m = 65, 255
    case = batch(("random", "one"), n, m, 4)
    for form in (1, 2):
        full = raw(case, 40.0, form=form)
        for skip in (("halves",), ("count1", "count2"), ("coef1", "coef2"), ("halves", "count1", "count2", "coef1", "coef2")):
            part = raw(case, 40.0, form=form, skip=skip)
            bit_equal(full, part, "without %s" % (skip,), [k for k in OUTPUTS if k not in skip])
            for k in skip:
                assert (part[k] == (-77 if part[k].dtype == np.int32 else -7.7e7)).all()     # nothing was written there
    assert raw(case, 40.0, skip=("loss",), rc_only=True) == -1 and raw(case, 40.0, skip=("status",), rc_only=True) == -1
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("inf")), dict(alpha=float("nan")), dict(n_lambda=-1.0),
               dict(n_lambda=float("nan")), dict(n_lambda=float("inf")), dict(form=3), dict(form=-1)):
        assert raw(case, **kw, rc_only=True) == -1, kw
    L = lib()
    null = [None] * 7
    assert L.dpf_dcd(1, 0, 4, None, None, None, None, 1.0, 1.0, 0, 0, *null, None, 0, None) == -1
    assert L.dpf_dcd(1, 4, 0, None, None, None, None, 1.0, 1.0, 0, 0, *null, None, 0, None) == -1
    assert L.dpf_dcd(-1, 4, 4, None, None, None, None, 1.0, 1.0, 0, 0, *null, None, 0, None) == -1
    assert L.dpf_dcd(0, 4, 4, None, None, None, None, 1.0, 1.0, 0, 0, *null, None, 0, None) == 0             # no clouds: nothing is launched
    assert L.dpf_dcd(1, 4, 4, None, None, None, None, 1.0, 1.0, 0, 0, *null, None, 0, None) == -1            # missing pointers
    assert L.dpf_dcd_workspace_bytes(0, 4, 4) == 0 and L.dpf_dcd_workspace_bytes(2, 0, 4) == 0
    assert L.dpf_dcd_workspace_bytes(2, 300, 257) == ((2 * (300 + 257 + 1) * 4 + 7) // 8) * 8 + 2 * (2 + 2) * 8


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def clouds(seed=0, B=3, n=512, m=400, noise=None):
    """(uniform prediction, collapsed prediction, target): a Gaussian target; the uniform prediction is an independent Gaussian cloud,
    or with `noise` a reconstruction (the target's points, cycled to n of them, moved by Gaussian noise of that size); the collapsed one
    is the uniform one with half its points on 8 spots of the target"""
    rng = np.random.default_rng(seed)
    y = (0.3 * rng.standard_normal((B, m, 3))).astype(np.float32)
    x = (0.3 * rng.standard_normal((B, n, 3))).astype(np.float32)
    if noise is not None:
        x = (y[:, np.arange(n) % m] + noise * rng.standard_normal((B, n, 3))).astype(np.float32)
    c = x.copy()
    c[:, n // 2:] = y[:, rng.integers(0, m, size=n - n // 2) % 8]
    return cuda(x), cuda(c), cuda(y)


def tensor_op_dcd(x, y, idx1, idx2, alpha, n_lambda, non_reg):
    """the published formulation on tensor ops in float64, on GIVEN indices: differentiable in x and y, the weights detached"""
    def half(a, b, idx, frac):
        d = ((a - torch.gather(b, 1, idx[:, :, None].expand(-1, -1, 3))) ** 2).sum(-1)
        count = torch.stack([torch.bincount(i, minlength=b.shape[1]).gather(0, i) for i in idx]).double()
        return (1 - torch.exp(-alpha * d) * (frac / (count ** n_lambda + 1e-6))).mean(1)
    n, m = x.shape[1], y.shape[1]
    f1, f2 = (max(1.0, n / m), max(1.0, m / n)) if non_reg else (n / m, m / n)
    return (half(x, y, idx1, f1) + half(y, x, idx2, f2)) / 2


@pytest.mark.parametrize("alpha,n_lambda,non_reg", [(1000.0, 1.0, False), (40.0, 0.5, True)])
def test_density_aware_chamfer_on_real_clouds(alpha, n_lambda, non_reg):
    from dpf_nets_amd.metrics import density_aware_chamfer, density_aware_chamfer_raw
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    x, c, y = clouds(noise=0.005)                                                            # a good reconstruction, and the same with a pile-up
    n, m = x.shape[1], y.shape[1]
    losses = []
    for pred in (x, c):
        loss, (halves, count1, count2, idx1, idx2) = density_aware_chamfer(pred, y, alpha, n_lambda, non_reg, return_raw=True)
        d1, i1, d2, i2 = BK.NNDistance(pred, y)                                              # the DEVICE'S OWN dist / idx: ties cannot differ
        assert torch.equal(i1, idx1) and torch.equal(i2, idx2) and loss.dtype == torch.float32 and loss.shape == (3,)
        ref = D.dcd_batch(d1.cpu().numpy(), i1.cpu().numpy(), d2.cpu().numpy(), i2.cpu().numpy(), alpha, n_lambda, non_reg)
        assert same(count1.cpu().numpy(), ref["count1"]) and same(count2.cpu().numpy(), ref["count2"])
        h = halves.cpu().numpy()
        dev = np.abs(h - ref["halves"]).max() / max(1.0, n / m)
        WORST["loss"] = max(WORST["loss"], dev)
        print("real clouds: halves deviation %.3g (bound %.3g)" % (dev, D.dcd_bound(n, m)))
        assert dev <= D.dcd_bound(n, m)
        assert same(loss.cpu().numpy(), (0.5 * (h[:, 0] + h[:, 1])).astype(np.float32))      # one rounding of the float64 loss
        rawout = density_aware_chamfer_raw(d1, i1, d2, i2, alpha, n_lambda, non_reg)
        assert same(rawout[1].cpu().numpy(), h) and int(rawout[6].abs().max()) == 0
        losses.append(loss.cpu().numpy())
    assert int(count1.max()) >= 8                                                            # the pile-up was seen
    assert (losses[1] > losses[0]).all(), losses                                             # ... and costs: collapsed above uniform


@pytest.mark.parametrize("alpha,spread", [(40.0, None), (1000.0, 0.01)])
def test_the_gradient_against_float64_autograd_on_the_devices_indices(alpha, spread):
    """the tolerance of tests/test_gpu_chamfer_grad_det.py for the deterministic backward: rtol 1e-5, atol 1e-5"""
    from dpf_nets_amd.metrics import density_aware_chamfer
    x, c, y = clouds(seed=2)
    if spread is not None:                                                                   # alpha 1000: a prediction close to the target, so that e is not 0
        y = y[:, :400].contiguous()
        c = (y + spread * torch.randn_like(y)).contiguous()
        c = torch.cat([c, c[:, :112] + spread], dim=1).contiguous()
    grads = []
    for _ in range(2):
        p, t = c.clone().requires_grad_(True), y.clone().requires_grad_(True)
        loss, (_, _, _, idx1, idx2) = density_aware_chamfer(p, t, alpha, return_raw=True)
        w = torch.tensor([1.0, -2.0, 0.5], device=_dev())
        (loss * w).sum().backward()
        grads.append((p.grad.clone(), t.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*grads))                                   # two backward runs: the same bits
    p64, t64 = c.double().requires_grad_(True), y.double().requires_grad_(True)
    (tensor_op_dcd(p64, t64, idx1.long(), idx2.long(), alpha, 1.0, False) * w.double()).sum().backward()
    for got, want in zip(grads[0], (p64.grad, t64.grad)):
        assert float(want.abs().max()) > 1e-3                                                # (a gradient worth comparing)
        assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5), float((got.double() - want).abs().max())
    # only the gradient that is asked for
    p = c.clone().requires_grad_(True)
    density_aware_chamfer(p, y, alpha).mul(w).sum().backward()
    assert torch.equal(p.grad, grads[0][0])
    t = y.clone().requires_grad_(True)
    density_aware_chamfer(c, t, alpha).mul(w).sum().backward()
    assert torch.equal(t.grad, grads[0][1]) and c.grad is None
    with torch.no_grad():
        assert density_aware_chamfer(p, y, alpha).grad_fn is None


def test_pairwise_dcd_is_the_twelve_single_calls():
    from dpf_nets_amd.metrics import density_aware_chamfer, pairwise_DCD
    rng = np.random.default_rng(4)
    a, b = cuda((0.3 * rng.standard_normal((3, 257, 3))).astype(np.float32)), cuda((0.3 * rng.standard_normal((4, 300, 3))).astype(np.float32))
    M = pairwise_DCD(a, b, 5, alpha=40.0, n_lambda=0.5)
    assert M.shape == (3, 4) and M.dtype == torch.float32 and not M.requires_grad
    for i in range(3):
        for j in range(4):
            assert torch.equal(M[i, j], density_aware_chamfer(a[i:i + 1], b[j:j + 1], 40.0, 0.5)[0]), (i, j)
    assert torch.equal(M, pairwise_DCD(a, b, 2048, alpha=40.0, n_lambda=0.5))


def test_a_refused_cloud_raises_naming_it(monkeypatch):
    from dpf_nets_amd.metrics import density_aware_chamfer
    from dpf_nets_amd.metrics import dcd as module
    x, _, y = clouds(seed=6)
    search = module.BK.NNDistance

    def broken(a, b):
        out = search(a, b)
        out[1][1, 5] = b.shape[1]                                                           # a search gone wrong: one index past the cloud
        return out

    monkeypatch.setattr(module.BK, "NNDistance", broken)
    with pytest.raises(ValueError, match="cloud 1 of 3 refused"):
        density_aware_chamfer(x, y)
