"""approx-EMD without a stored matching: the cost-only forward (dpf_approxmatch_costonly_ws) against the storing one, bit for bit,
and the recomputing backward (dpf_matchcostgrad_recompute_ws) against the gradients read off the stored matching -- the same
weights, so the project's bound for "the same sums in a different order" (test_one_pass_gradients_match_two_pass: rtol 1e-4,
atol 1e-5) on every kind of cloud, both kernel families."""
import numpy as np
import pytest
import torch

from oracle import structural as S
from oracle.gen_golden import chamfer_inputs
from tests.emd_cases import KINDS, emd_clouds, matrix_path

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
ORACLE_SHAPES = ((2, 64, 64), (3, 300, 257), (128, 1024, 500), (70, 2048, 700), (600, 200, 129), (1100, 200, 90))


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    return BK


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in arrays]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _forward_cases():
    for (B, n, m) in ((2, 64, 64), (3, 300, 257), (2, 1024, 2048), (1, 100, 37), (16, 2048, 2048), (2, 1, 1), (3, 33, 130)):
        yield "uniform %s" % ((B, n, m),), chamfer_inputs(900 + n, B, n, m)
    a, b = chamfer_inputs(41, 4, 300, 257)
    b[2] += 5.0                                       # one cloud beyond the matrix path's range: the call's verdict is packed-VALU
    yield "one cloud out of range", (a, b)
    a, b = chamfer_inputs(42, 3, 257, 300)
    a[1, 17, 2] = np.nan
    yield "one NaN point", (a, b)


@pytest.mark.parametrize("matrix", [True, False])
def test_cost_only_forward_has_the_storing_forward_bits(matrix):
    BK = _gpu()
    with matrix_path(matrix):
        for tag, (a, b) in _forward_cases():
            ta, tb = _cuda(a, b)
            nm = a.shape[1] + b.shape[1]
            _match, temp, cost = BK.ApproxMatchCost(ta, tb)
            for rep in range(2):
                t2, c2, saved = BK.ApproxMatchCostOnly(ta, tb)
                assert torch.equal(_bits(c2), _bits(cost)), (tag, rep, c2, cost)
                assert torch.equal(_bits(t2[:, :nm]), _bits(temp[:, :nm])), (tag, rep)
                assert saved.dtype == torch.uint8 and saved.numel() >= 16


def _check_grads(BK, a, b, tag, oracle=False):
    ta, tb = _cuda(a, b)
    match, _ = BK.ApproxMatch(ta, tb)
    g1, g2 = BK.MatchCostGrad(ta, tb, match)
    _t, _c, saved = BK.ApproxMatchCostOnly(ta, tb)
    h1, h2 = BK.MatchCostGradRecompute(ta, tb, saved)
    torch.cuda.synchronize()
    for name, h, g in (("grad1", h1, g1), ("grad2", h2, g2)):
        h, g = h.cpu().numpy(), g.cpu().numpy()
        print("%s %s: max |lean - stored| = %.3g (max |stored| %.3g)" % (tag, name, np.abs(h - g).max(), np.abs(g).max()))
        np.testing.assert_allclose(h, g, rtol=RTOL, atol=ATOL, err_msg="%s %s" % (tag, name))
    if oracle:
        r1, r2 = S.matchcostgrad(a, b, match.cpu().numpy())
        np.testing.assert_allclose(h1.cpu().numpy(), r1, rtol=RTOL, atol=ATOL, err_msg=tag + " grad1 vs oracle")
        np.testing.assert_allclose(h2.cpu().numpy(), r2, rtol=RTOL, atol=ATOL, err_msg=tag + " grad2 vs oracle")


@pytest.mark.parametrize("matrix", [True, False])
def test_lean_gradients_equal_stored_matching_gradients_uniform(matrix):
    """the shape list of test_one_pass_gradients_match_two_pass: also against the CPU oracle fed the GPU's matching"""
    BK = _gpu()
    with matrix_path(matrix):
        for (B, n, m) in ORACLE_SHAPES:
            a, b = chamfer_inputs(900 + n, B, n, m)
            _check_grads(BK, a, b, "uniform %s matrix=%d" % ((B, n, m), matrix), oracle=True)


@pytest.mark.parametrize("matrix", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_lean_gradients_equal_stored_matching_gradients_kinds(kind, matrix):
    """every kind of the fuzz (dup, grid and line bring exact ties and coincident points), GPU against GPU on identical weights"""
    BK = _gpu()
    with matrix_path(matrix):
        for i, (B, n, m) in enumerate(((2, 300, 257), (2, 1024, 1024))):
            a, b = emd_clouds(np.random.default_rng(7000 + 10 * KINDS.index(kind) + i), kind, B, n, B, m)
            _check_grads(BK, a, b, "%s %s matrix=%d" % (kind, (B, n, m), matrix))


@pytest.mark.parametrize("matrix", [True, False])
def test_lean_gradients_of_a_cloud_against_itself(matrix):
    BK = _gpu()
    with matrix_path(matrix):
        for (B, n) in ((2, 300), (2, 1024)):
            a, _ = chamfer_inputs(77 + n, B, n, n)
            _check_grads(BK, a, a.copy(), "self %s matrix=%d" % ((B, n), matrix))


def test_backward_is_deterministic_and_leaves_the_saved_state_alone():
    BK = _gpu()
    for matrix in (True, False):
        with matrix_path(matrix):
            for (B, n, m) in ((3, 300, 257), (2, 1024, 2048)):
                ta, tb = _cuda(*chamfer_inputs(300 + n, B, n, m))
                _t, _c, saved = BK.ApproxMatchCostOnly(ta, tb)
                before = saved.clone()
                g = BK.MatchCostGradRecompute(ta, tb, saved)
                h = BK.MatchCostGradRecompute(ta, tb, saved)
                torch.cuda.synchronize()
                assert torch.equal(saved, before)
                assert torch.equal(_bits(g[0]), _bits(h[0])) and torch.equal(_bits(g[1]), _bits(h[1]))
                # the family is the forward's: the setting at the time of the backward does not enter
                with matrix_path(not matrix):
                    f = BK.MatchCostGradRecompute(ta, tb, saved)
                assert torch.equal(_bits(g[0]), _bits(f[0])) and torch.equal(_bits(g[1]), _bits(f[1]))
                assert torch.equal(saved, before)


def test_lean_forward_and_backward_repeat_bit_for_bit_at_16_x_8192():
    BK = _gpu()
    ta, tb = _cuda(*chamfer_inputs(5, 16, 8192, 8192))
    runs = []
    for _ in range(3):
        _t, c, saved = BK.ApproxMatchCostOnly(ta, tb)
        g1, g2 = BK.MatchCostGradRecompute(ta, tb, saved)
        runs.append((c, g1, g2))
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert torch.equal(_bits(x), _bits(y))
    assert torch.isfinite(runs[0][1]).all() and torch.isfinite(runs[0][2]).all()


def _grads(fn, a, b, w, req_a, req_b):
    ta, tb = _cuda(a, b)
    ta.requires_grad_(req_a); tb.requires_grad_(req_b)
    cost = fn(ta, tb)
    (cost * w).sum().backward()
    return cost.detach(), ta.grad, tb.grad


def test_autograd_lean_against_stored():
    BK = _gpu()
    from dpf_nets_amd.metrics.StructuralLosses.match_cost import match_cost, match_cost_lean
    from dpf_nets_amd.networks import utils as U
    for (B, n, m) in ((3, 300, 257), (2, 1024, 1024)):
        a, b = chamfer_inputs(1200 + n, B, n, m)
        w = torch.rand(B, generator=torch.Generator().manual_seed(n)).cuda() + 0.5
        for req_a, req_b in ((True, True), (True, False), (False, True)):
            c0, ga0, gb0 = _grads(match_cost, a, b, w, req_a, req_b)
            c1, ga1, gb1 = _grads(match_cost_lean, a, b, w, req_a, req_b)
            assert torch.equal(_bits(c0), _bits(c1))
            for g0, g1, req in ((ga0, ga1, req_a), (gb0, gb1, req_b)):
                if not req:
                    assert g0 is None and g1 is None
                    continue
                np.testing.assert_allclose(g1.cpu().numpy(), g0.cpu().numpy(), rtol=RTOL, atol=ATOL)
            BK.EMD_LEAN_GRAD = True                       # the switch routes match_cost itself: the lean path's bits
            try:
                c2, ga2, gb2 = _grads(match_cost, a, b, w, req_a, req_b)
            finally:
                BK.EMD_LEAN_GRAD = False
            assert torch.equal(_bits(c2), _bits(c1))
            for g1, g2 in ((ga1, ga2), (gb1, gb2)):
                assert (g1 is None and g2 is None) or torch.equal(_bits(g1), _bits(g2))
        ta, tb = _cuda(a, b)
        want = BK.ApproxMatchCost(ta, tb)[2]
        with torch.no_grad():
            assert torch.equal(_bits(match_cost(ta.clone().requires_grad_(True), tb)), _bits(want))
        assert torch.equal(_bits(match_cost(ta, tb)), _bits(want))
    a, b = chamfer_inputs(8, 2, 512, 512)
    ta, tb = _cuda(a, b)
    assert torch.equal(_bits(U.emd_approx_lean(ta, tb)), _bits(U.emd_approx(ta, tb)))
    ta.requires_grad_(True)
    lean, stored = U.emd_approx_lean(ta, tb), U.emd_approx(ta, tb)
    assert torch.equal(_bits(lean.detach()), _bits(stored.detach()))
    lean.sum().backward()
    g_lean = ta.grad.clone()
    ta.grad = None
    stored.sum().backward()
    np.testing.assert_allclose(g_lean.cpu().numpy(), ta.grad.cpu().numpy(), rtol=RTOL, atol=ATOL)


def test_memory_holds_no_matching():
    """B = 8, n = m = 4096: one cloud's matching is 4 n m = 67 MB and the stored path holds eight.  The no-grad match_cost and
    the lean forward + backward stay within what the library reports, and below ONE matching."""
    _gpu()
    from dpf_nets_amd._lib import lib
    from dpf_nets_amd.metrics.StructuralLosses.match_cost import match_cost, match_cost_lean
    B, n = 8, 4096
    ta, tb = _cuda(*chamfer_inputs(3, B, n, n))
    w = torch.rand(B, device="cuda") + 0.5
    r512 = lambda v: (v + 511) // 512 * 512                           # noqa: E731 (the caching allocator's rounding)
    ws = lib().dpf_approxmatch_workspace_bytes(B, n, n)
    scratch = lib().dpf_matchcostgrad_recompute_workspace_bytes(B, n, n)
    temp, cost, grad = B * 4 * n * 4, B * 4, B * n * 3 * 4

    def rise_of(fn):
        """-> (rise of the peak of the bytes the call REQUESTED, rise of the peak of the bytes the allocator handed out).  The
        bound by the library's reported sizes is held against the first: the caching allocator rounds a request above 10 MB up
        to a multiple of 2 MiB (measured: 18 629 392 -> 18 874 368), which says nothing about the code under test.  The second,
        with that rounding in it, must still stay below one matching."""
        fn()                                                          # (library loaded, kernels resident)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before, before_req = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["requested_bytes.all.current"]
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.memory_stats()["requested_bytes.all.peak"] - before_req, torch.cuda.max_memory_allocated() - before)

    def nograd():
        with torch.no_grad():
            match_cost(ta, tb)

    req, rise = rise_of(nograd)
    print("no-grad match_cost: requested %d, allocated %d, workspace %d" % (req, rise, ws))
    assert req <= r512(ws) + r512(temp) + r512(cost), (req, ws)
    assert rise < 4 * n * n, rise

    def lean():
        xa, xb = ta.clone().requires_grad_(True), tb.clone().requires_grad_(True)
        (match_cost_lean(xa, xb) * w).sum().backward()

    req, rise = rise_of(lean)
    print("lean forward + backward: requested %d, allocated %d, workspace %d, scratch %d" % (req, rise, ws, scratch))
    clones_and_grads = 4 * r512(grad)                                  # xa, xb and their .grad
    products = 3 * r512(cost) + 2 * r512(grad)                         # cost * w, its sum, grad_output; a broadcast product per gradient
    assert req <= r512(ws) + r512(scratch) + r512(temp) + r512(cost) + clones_and_grads + products, (req, ws, scratch)
    assert rise < 4 * n * n, rise


def test_lean_runs_at_64_x_8192():
    _gpu()
    from dpf_nets_amd.metrics.StructuralLosses.match_cost import match_cost_lean
    B, n = 64, 8192
    ta, tb = _cuda(*chamfer_inputs(11, B, n, n))
    ta.requires_grad_(True); tb.requires_grad_(True)
    cost = match_cost_lean(ta, tb)
    cost.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(cost).all()
    assert torch.isfinite(ta.grad).all() and torch.isfinite(tb.grad).all()
    assert (ta.grad.abs().sum(2) > 0).all()
