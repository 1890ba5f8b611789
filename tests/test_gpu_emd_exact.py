"""dpf_emd_exact on the GPU against the numpy oracle of its contract (tests/emd_exact_ref.py; the oracle itself is checked against
brute force and scipy in tests/test_emd_exact_ref_cpu.py).  Sizes 1, 2, 63, 64, 65 (one wave), 256 (four waves, late rounds cut
into slices) and 2 048 (sixteen waves); every kind of the case list at B = 3 with three different clouds per operand.  The oracle
of a case is computed once and shared."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import emd_exact_ref as R                                                                   # noqa: E402
from emd_exact_common import U, check_pair, clouds, dev, run, same_bits                     # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 256)
_ORACLE, _DEVICE = {}, {}


def oracle(kind, n, B=3):
    key = (kind, n, B)
    if key not in _ORACLE:
        a, b, _ = clouds(kind, n, B)
        _ORACLE[key] = [R.solve(a[k], b[k]) for k in range(B)]
    return _ORACLE[key]


def device(kind, n, B=3):
    key = (kind, n, B)
    if key not in _DEVICE:
        a, b, _ = clouds(kind, n, B)
        _DEVICE[key] = run(a, b)
    return _DEVICE[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_values_against_the_oracle(kind, n):
    a, b, extra = clouds(kind, n)
    cost, asg, qcost, status = device(kind, n)
    for k, o in enumerate(oracle(kind, n)):
        check_pair(a[k], b[k], o, cost[k], asg[k], qcost[k], status[k], (kind, n, k))
        if kind == "perm":                                                                  # 6
            assert len({tuple(p) for p in a[k].tolist()}) == n
            assert np.array_equal(asg[k], extra[k]) and cost[k] == 0 and qcost[k] == 0
        if kind == "shift":                                                                 # 7
            norm = float(np.sqrt((extra[k].astype(np.float64) ** 2).sum()))
            assert abs(float(cost[k]) / n - norm) <= (n + 8) * 2.0 ** -24 * norm
        if kind == "same":
            assert cost[k] == 0 and qcost[k] == 0


def test_two_clouds_of_2048_points():
    a, b, _ = clouds("gauss", 2048, 2)
    cost, asg, qcost, status = device("gauss", 2048, 2)
    for k, o in enumerate(oracle("gauss", 2048, 2)):
        check_pair(a[k], b[k], o, cost[k], asg[k], qcost[k], status[k], ("gauss", 2048, k))


def test_power_of_two_scaling_keeps_the_matching_and_scales_the_cost():                    # 8
    a, b, _ = clouds("gauss", 65)
    base = device("gauss", 65)
    for k in (10, -10):
        f = np.float32(2.0 ** k)
        cost, asg, qcost, status = run(a * f, b * f)
        assert same_bits((asg, qcost, status), base[1:])
        assert same_bits((cost,), ((base[0] * f).astype(np.float32),))


def test_bit_identical_across_runs_batches_forms_strides_and_the_pairwise_entry():         # 9
    from dpf_nets_amd._lib import lib, check, current_stream
    for kind, n in (("gauss", 65), ("lattice", 256), ("collapsed", 64)):
        a, b, _ = clouds(kind, n)
        base = device(kind, n)
        assert same_bits(run(a, b), base), (kind, n, "second run")
        for form in (1, 2):
            assert same_bits(run(a, b, form=form), base), (kind, n, "form", form)
        for k in range(3):
            assert same_bits(run(a[k:k + 1], b[k:k + 1]), [x[k:k + 1] for x in base]), (kind, n, "alone", k)
        ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
        with torch.no_grad():
            M = U().pairwise_EMD_exact(ta, tb).cpu().numpy()
            M1 = U().pairwise_EMD_exact(ta, tb, bs=1).cpu().numpy()
            diag = U().emd_exact(ta, tb).cpu().numpy()
        assert same_bits((M,), (M1,)) and same_bits((np.diagonal(M).copy(),), (diag,)), (kind, n, "pairwise")
        # row 0 of the matrix again: stride 0 over a[0] against the materialised copies
        rep = ta[0:1].expand(3, -1, -1).contiguous()
        want = run(rep.cpu().numpy(), b)
        outs = [torch.empty((3, n), dtype=torch.int32, device=dev()), torch.empty((3, n), dtype=torch.int32, device=dev()),
                torch.empty((3,), dtype=torch.int64, device=dev()), torch.empty((3,), dtype=torch.float32, device=dev()),
                torch.empty((3,), dtype=torch.int32, device=dev())]
        nbytes = lib().dpf_emd_exact_workspace_bytes(3, n)
        ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev())
        check(lib().dpf_emd_exact(3, n, ta.data_ptr(), 0, tb.data_ptr(), n * 3, 20, 1 << 20, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                  outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), ws.data_ptr(), nbytes, current_stream()),
              "emd_exact")
        got = (outs[3].cpu().numpy(), outs[0].cpu().numpy(), outs[2].cpu().numpy(), outs[4].cpu().numpy())
        assert same_bits(got, want), (kind, n, "stride 0")
        assert same_bits(((got[0] / np.float32(n)).astype(np.float32),), (M[0],)), (kind, n, "stride 0 against the matrix row")
        inv = outs[1].cpu().numpy()
        assert all(np.array_equal(inv[k][got[1][k]], np.arange(n)) for k in range(3)), (kind, n, "inverse")


def test_a_bad_pair_touches_only_itself():                                                  # 10
    a, b, _ = clouds("gauss", 65)
    clean = device("gauss", 65)
    for where, value in (("a", np.nan), ("b", np.inf), ("a", -np.inf), ("extent", 3e38), ("square", 1e20)):
        x, y = a.copy(), b.copy()
        if where == "extent" or where == "square":
            x[1, 0, 0], y[1, 5, 0] = value, -value
        else:
            (x if where == "a" else y)[1, 7, 2] = value
        assert R.solve(x[1], y[1])["status"] == R.STATUS_REFUSED
        cost, asg, qcost, status = run(x, y)
        assert status[1] == R.STATUS_REFUSED and np.isnan(cost[1]) and qcost[1] == -1 and (asg[1] == -1).all(), (where, value)
        for k in (0, 2):
            assert same_bits([t[k] for t in (cost, asg, qcost, status)], [t[k] for t in clean]), (where, value, k)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = U().emd_exact(torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())).cpu().numpy()
        assert np.isnan(out[1]) and np.isfinite(out[[0, 2]]).all()
        mine = [m for m in w if issubclass(m.category, RuntimeWarning)]
        assert len(mine) == 1 and "status -1" in str(mine[0].message), [str(m.message) for m in w]


def test_the_round_cap_ends_a_pair_with_its_status():                                       # 11
    a, b, _ = clouds("gauss", 64)
    cost, asg, qcost, status = run(a, b, max_rounds=1)
    assert (status == R.STATUS_CAP).all() and np.isnan(cost).all() and (qcost == -1).all() and (asg == -1).all()
    needed = int(device("gauss", 64)[3][0])
    assert run(a[:1], b[:1], max_rounds=needed)[3][0] == needed and run(a[:1], b[:1], max_rounds=needed - 1)[3][0] == R.STATUS_CAP
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = U().emd_exact(torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev()), max_rounds=1)
    mine = [m for m in w if issubclass(m.category, RuntimeWarning)]
    assert torch.isnan(out).all() and len(mine) == 1 and "status -2" in str(mine[0].message)


def test_gradient():                                                                        # 12
    for kind, n in (("gauss", 65), ("collapsed", 64), ("same", 63)):
        a, b, _ = clouds(kind, n)
        asg = device(kind, n)[1]
        g = np.array([0.75, -2.0, 1.0], np.float32)
        grads = []
        for _ in range(2):
            ta = torch.from_numpy(a).to(dev()).requires_grad_(True)
            tb = torch.from_numpy(b).to(dev()).requires_grad_(True)
            out = U().emd_exact(ta, tb)
            assert out.grad_fn is not None and type(out.grad_fn).__name__ == "EMDExactFunctionBackward"
            out.backward(torch.from_numpy(g).to(dev()))
            grads.append((ta.grad.cpu().numpy(), tb.grad.cpu().numpy()))
        assert same_bits(grads[0], grads[1]), (kind, n)
        for k in range(3):
            wa, wb = R.grad64(a[k], b[k], asg[k], float(g[k]) / n)
            # unit vectors times g / n: the difference, three products, two sums, a root, a quotient and a product -- 8 roundings
            tol = 8 * 2.0 ** -24 * abs(float(g[k])) / n
            assert np.abs(grads[0][0][k] - wa).max() <= tol and np.abs(grads[0][1][k] - wb).max() <= tol, (kind, n, k)
            zero = (a[k] == b[k][asg[k]]).all(1)
            assert (grads[0][0][k][zero] == 0).all() and (grads[0][1][k][asg[k][zero]] == 0).all()
        if kind == "same":
            assert (grads[0][0] == 0).all() and (grads[0][1] == 0).all()
    # an input that needs no gradient gets none, and its launch argument is NULL
    ta = torch.from_numpy(a).to(dev()).requires_grad_(True)
    tb = torch.from_numpy(b).to(dev())
    U().emd_exact(ta, tb).sum().backward()
    assert ta.grad is not None and tb.grad is None
    fn = U().EMDExactFunction

    class Ctx:
        needs_input_grad = (False, False, False, False, False, False)
        saved_tensors = (ta.detach(), tb)
        assignment = inverse = None                     # (would fail if a launch read them)
        scale = 1.0
    assert fn.backward(Ctx, torch.ones(3, device=dev()), None, None, None) == (None,) * 6


def test_gradient_against_finite_differences_on_well_separated_points():
    """(tests/gradcheck.py bounds golden projections of the model's parameters and does not fit here.)  Far-apart matches keep the
    matching constant under the step: central differences of the float64 cost of the device's matching."""
    a, b, _ = clouds("shift", 5)
    asg = device("shift", 5)[1]
    ta = torch.from_numpy(a).to(dev()).requires_grad_(True)
    U().emd_exact(ta, torch.from_numpy(b).to(dev())).sum().backward()
    got = ta.grad.cpu().numpy()
    h = 1e-4
    for k in range(3):
        for i in range(5):
            for ax in range(3):
                p, m = a[k].astype(np.float64), a[k].astype(np.float64)
                p[i, ax] += h
                m[i, ax] -= h
                fd = (R.cost64(p, b[k], asg[k]) - R.cost64(m, b[k], asg[k])) / (2 * h) / 5
                assert abs(got[k, i, ax] - fd) <= 1e-6, (k, i, ax, got[k, i, ax], fd)


def test_refusals():                                                                        # 13
    u = U()
    a = torch.randn(2, 16, 3, device=dev())
    b = torch.randn(2, 16, 3, device=dev())
    limit = 8192
    bad = [(a.cpu(), b), (a, b.cpu()), (a.double(), b.double()), (a.half(), b), (a, b[:, :15].contiguous()),
           (a.transpose(0, 1).contiguous().transpose(0, 1), b), (a[:, :, :2].contiguous(), b[:, :, :2].contiguous()), (a[0], b[0]),
           (a, b[:1]), (torch.zeros(1, limit + 1, 3, device=dev()), torch.zeros(1, limit + 1, 3, device=dev()))]
    for x, y in bad:
        with pytest.raises(RuntimeError):
            u.emd_exact(x, y)
    with pytest.raises(RuntimeError, match="8192"):
        u.pairwise_EMD_exact(torch.zeros(1, limit + 1, 3, device=dev()), torch.zeros(1, limit + 1, 3, device=dev()))
    for x, y in ((a.cpu(), b), (a.double(), b), (a, b[:, :15].contiguous()), (a.clone().requires_grad_(True), b)):
        with pytest.raises(RuntimeError):
            u.pairwise_EMD_exact(x, y)
    for kw in (dict(bits=0), dict(bits=25), dict(max_rounds=-1)):
        with pytest.raises(RuntimeError):
            u.emd_exact(a, b, **kw)
    out, asg = u.emd_exact(a, b, return_assignment=True)
    assert out.shape == (2,) and asg.shape == (2, 16) and asg.dtype == torch.int32


def test_the_largest_served_size_runs_in_the_streamed_form():
    """8 192 points: the second cloud from global memory, the bids in the workspace.  b = a[perm]: 13 rounds, cost 0."""
    a, b, perm = R.make_case("perm", 8192, 3)
    cost, asg, qcost, status = run(a[None], b[None])
    assert np.array_equal(asg[0], perm) and cost[0] == 0 and qcost[0] == 0 and 0 < status[0] < 64


def test_compute_all_metrics_with_the_exact_matcher():                                      # 14
    from dpf_nets_amd.metrics import evaluation_metrics as EM
    rng = np.random.RandomState(11)
    smp = torch.from_numpy(rng.randn(5, 64, 3).astype(np.float32)).to(dev())
    ref = torch.from_numpy((rng.randn(6, 64, 3) * 0.8).astype(np.float32)).to(dev())
    with torch.no_grad():
        default = EM.compute_all_metrics(smp, ref, 4)
        exact = EM.compute_all_metrics(smp, ref, 4, emd="exact")

        def build(emd_matrix):                          # the function's body before the option existed, on the given EMD matrices
            res = {}
            rs = (u.pairwise_CD(ref, smp, bs=4), emd_matrix(ref, smp, bs=4))
            rr = (u.pairwise_CD(ref, ref, bs=4), emd_matrix(ref, ref, bs=4))
            ss = (u.pairwise_CD(smp, smp, bs=4), emd_matrix(smp, smp, bs=4))
            for i, metric in enumerate(("CD", "EMD")):
                res.update({"%s-%s" % (k, metric): v for k, v in EM.lgan_mmd_cov(rs[i].t()).items()})
            for i, metric in enumerate(("CD", "EMD")):
                res.update({"1-NN-%s-%s" % (metric, k): v for k, v in EM.knn(rr[i], rs[i], ss[i], 1, sqrt=False).items() if "acc" in k})
            return res
        u = U()
        want_default, want_exact = build(u.pairwise_EMD), build(u.pairwise_EMD_exact)
    assert list(default) == list(exact) == list(want_default)
    for k in default:
        assert same_bits((default[k].cpu().numpy(),), (want_default[k].cpu().numpy(),)), k
        assert same_bits((exact[k].cpu().numpy(),), (want_exact[k].cpu().numpy(),)), k
    assert float(exact["lgan_mmd-EMD"]) != float(default["lgan_mmd-EMD"])
    with pytest.raises(ValueError):
        EM.compute_all_metrics(smp, ref, 4, emd="best")
