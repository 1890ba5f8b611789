"""The deterministic Chamfer backward on the GPU (csrc/chamfer_grad.hip: dpf_nndistancegrad_det, dpf_chamfer_cd_backward) and the
layers above it, BIT FOR BIT against the contract's numpy restatement (tests/chamfer_grad_ref.py): both entries, both outputs and
each output NULL, both kernel forms, lists of every length class, a dirty workspace, a busy neighbour stream, graph replay, the
one-node loss networks.utils.chamfer_loss, nn_distance under torch's deterministic flag and the compiled extension.
Indices always come from the project's own NNDistance."""
import numpy as np
import pytest
import torch

from tests import chamfer_grad_ref as R

pytestmark = pytest.mark.gpu

LONG = 64              # dispatch::CG_LONG_LIST (tests/test_chamfer_grad_ref_cpu.py pins it): longer lists go to a wave


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK
    return BK


def _clouds(seed, b, n, m, kind=None):
    rng = np.random.default_rng(seed)
    x1 = rng.standard_normal((b, n, 3)).astype(np.float32)
    x2 = rng.standard_normal((b, m, 3)).astype(np.float32)
    if kind == "collapsed":                    # the target cloud one point: first-minimum rule -> idx1 == 0, ONE list of length n
        x2[:] = x2[:, :1]
    if kind == "halves":                       # cloud 1 = its first half twice: every list of cloud 2's targets in g2 ... and
        x1[:, n // 2:] = x1[:, :n // 2]        # cloud 2 = cloud 1's first half: lists of exactly 2
        x2 = np.ascontiguousarray(x1[:, :n // 2])
    return x1, x2


class Case:
    """clouds on the GPU, the search's indices, rows with mixed signs and a few zeros, a per-cloud gradient -- and the restatement's
    results, computed once"""

    def __init__(self, seed, b, n, m, kind=None):
        BK = _gpu()
        self.shape = (b, n, m)
        x1, x2 = _clouds(seed, b, n, m, kind)
        m = x2.shape[1]
        self.shape = (b, n, m)
        rng = np.random.default_rng(seed + 1)
        gd1 = rng.standard_normal((b, n)).astype(np.float32)
        gd2 = rng.standard_normal((b, m)).astype(np.float32)
        gd1[:, ::5] = 0
        gd2[:, 1::9] = 0
        gcd = rng.standard_normal((b,)).astype(np.float32)
        self.x1, self.x2, self.gd1, self.gd2, self.gcd = (torch.from_numpy(a).cuda() for a in (x1, x2, gd1, gd2, gcd))
        _, self.i1, _, self.i2 = BK.NNDistance(self.x1, self.x2)
        i1, i2 = self.i1.cpu().numpy(), self.i2.cpu().numpy()
        if kind == "collapsed":
            assert not i1.any()
        if kind == "halves":
            assert (np.bincount(i1[0], minlength=m) == 2).all()
        self.ref_row = R.nndistancegrad_det(x1, x2, i1, i2, gd1, gd2)
        self.ref_cd = R.chamfer_cd_backward(x1, x2, i1, i2, gcd)


_cases = {}


def case(*key):
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def call(c, form, need1=True, need2=True, fill=0xFF, outs=None):
    """the raw entry (NULL outputs are part of the contract) with a DIRTY workspace -> [g1 | None, g2 | None]"""
    from dpf_nets_amd._lib import lib, check, current_stream
    L = lib()
    b, n, m = c.shape
    nbytes = L.dpf_nndistancegrad_det_workspace_bytes(b, n, m)
    ws = torch.full((max(nbytes, 8),), fill, dtype=torch.uint8, device="cuda")
    if outs is None:
        outs = [torch.full((b, k, 3), float("nan"), device="cuda") for k in (n, m)]
    p1, p2 = outs[0].data_ptr() if need1 else None, outs[1].data_ptr() if need2 else None
    if form == "row":
        check(L.dpf_nndistancegrad_det(b, n, c.x1.data_ptr(), m, c.x2.data_ptr(), c.gd1.data_ptr(), c.i1.data_ptr(), c.gd2.data_ptr(),
                                       c.i2.data_ptr(), p1, p2, ws.data_ptr(), nbytes, current_stream()), "nndistancegrad_det")
    else:
        check(L.dpf_chamfer_cd_backward(b, n, c.x1.data_ptr(), m, c.x2.data_ptr(), c.i1.data_ptr(), c.i2.data_ptr(), c.gcd.data_ptr(),
                                        p1, p2, ws.data_ptr(), nbytes, current_stream()), "chamfer_cd_backward")
    c.keep = ws                                 # (alive until the caller has synchronised)
    return [outs[0] if need1 else None, outs[1] if need2 else None]


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def assert_bits(got, ref, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        if g is None:
            continue
        g, r = bits(g), np.ascontiguousarray(r).view(np.int32)
        bad = int((g != r).sum())
        assert bad == 0, "%s, output %d: %d of %d words differ from the restatement" % (what, k + 1, bad, g.size)


class workspace_form:
    """every output through the workspace form (dpf_chamfer_grad_lds_mode(0)), whatever its size"""

    def __enter__(self):
        from dpf_nets_amd._lib import lib
        self.old = lib().dpf_chamfer_grad_lds_mode(0)

    def __exit__(self, *a):
        from dpf_nets_amd._lib import lib
        lib().dpf_chamfer_grad_lds_mode(self.old)


def check_all_forms(c, what):
    for form, ref in (("row", c.ref_row), ("cd", c.ref_cd)):
        for need1, need2 in ((True, True), (True, False), (False, True)):
            assert_bits(call(c, form, need1, need2), ref, "%s, %s form, outputs %d%d" % (what, form, need1, need2))


SHAPES = [
    (1, 1, 1, None), (2, 7, 3, None),                      # degenerate
    (1, 64, 8, None),                                      # every target of cloud 2 has a list
    (3, 257, 257, None), (2, 130, 515, None),              # ragged; n != m
    (2, 2500, 2048, None),                                 # larger, n != m
    (2, LONG - 1, 5, "collapsed"), (2, LONG, 5, "collapsed"), (2, LONG + 1, 5, "collapsed"),     # one list at the long-list threshold
    (1, 4100, 33, "collapsed"),                            # a very long single list
    (2, 600, 300, "halves"),                               # lists of exactly 2
]


@pytest.mark.parametrize("b,n,m,kind", SHAPES)
def test_bit_exact_against_the_restatement(b, n, m, kind):
    check_all_forms(case(100 + n, b, n, m, kind), "LDS form")


@pytest.mark.parametrize("b,n,m,kind", [(2, 7, 3, None), (2, 2500, 2048, None), (2, LONG + 1, 5, "collapsed"),
                                        (1, 4100, 33, "collapsed"), (2, 600, 300, "halves")])
def test_workspace_form_forced_gives_the_same_bits(b, n, m, kind):
    c = case(100 + n, b, n, m, kind)
    with workspace_form():
        from dpf_nets_amd._lib import lib
        assert lib().dpf_nndistancegrad_det_workspace_bytes(b, *c.shape[1:]) > 0
        check_all_forms(c, "workspace form (forced)")


def test_workspace_form_past_the_lds_limit():
    """9000 and 8200 queries: neither output fits the LDS form (8192); 16384 key slots = four LDS-sorted chunks and the network's
    two widest stages in global memory"""
    from dpf_nets_amd._lib import lib
    c = case(7, 1, 9000, 8200, None)
    assert lib().dpf_nndistancegrad_det_workspace_bytes(1, 9000, 8200) == 2 * 16384 * 8 + 12 * (9000 + 8200)
    check_all_forms(c, "workspace form")


def test_one_form_each():
    """12000 targets with 700 queries sort in LDS, the other output's 12000 queries in the workspace: one call, both forms"""
    c = case(8, 1, 12000, 700, None)
    check_all_forms(c, "mixed forms")


def test_dirty_workspace():
    c = case(100 + 2500, 2, 2500, 2048, None)
    with workspace_form():
        for fill in (0xFF, 0x00, 0x5A):
            assert_bits(call(c, "row", fill=fill), c.ref_row, "workspace filled with %#x" % fill)


@pytest.mark.parametrize("b,n,m,kind", [(4, 2048, 2048, None), (1, 4100, 33, "collapsed")])
def test_repeatable_beside_a_busy_stream(b, n, m, kind):
    """20 calls, the search kernel of other clouds running on a second stream meanwhile: identical bytes, and the restatement's"""
    BK = _gpu()
    c = case(100 + n, b, n, m, kind)
    other = torch.randn(8, 2048, 3, device="cuda"), torch.randn(8, 2048, 3, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    first = None
    for r in range(20):
        with torch.cuda.stream(side):
            BK.NNDistance(*other)
            BK.NNDistance(*other)
        got = [bits(t) for t in call(c, "row")]
        if first is None:
            first = got
        assert all(np.array_equal(a, f) for a, f in zip(got, first)), "call %d differs from the first" % r
    torch.cuda.synchronize()
    assert_bits([torch.from_numpy(f.view(np.float32)) for f in first], c.ref_row, "beside a busy stream")


def test_graph_capture_replays_the_eager_bits():
    c = case(100 + 257, 3, 257, 257, None)
    eager = [bits(t) for t in call(c, "cd")]
    outs = [torch.zeros(3, 257, 3, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(c, "cd", outs=outs)
    for replay in range(2):
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(bits(o), e) for o, e in zip(outs, eager)), "replay %d" % replay


def test_chamfer_loss_value_and_gradient():
    _gpu()
    from dpf_nets_amd.networks.utils import chamfer_cd_per_cloud, chamfer_loss
    from dpf_nets_amd.metrics.StructuralLosses.nn_distance import nn_distance
    c = case(100 + 130, 2, 130, 515, None)
    pred, true = c.x1.clone().requires_grad_(True), c.x2.clone().requires_grad_(True)
    cd = chamfer_loss(pred, true)
    assert cd.shape == (2,) and cd.grad_fn is not None
    assert np.array_equal(bits(cd), bits(chamfer_cd_per_cloud(c.x1, c.x2)))
    cd.sum().backward()
    ones = R.chamfer_cd_backward(c.x1.cpu().numpy(), c.x2.cpu().numpy(), c.i1.cpu().numpy(), c.i2.cpu().numpy(), np.ones(2, np.float32))
    assert_bits([pred.grad, true.grad], ones, "chamfer_loss(...).sum().backward()")
    # ... and the composition it replaces
    p2, t2 = c.x1.clone().requires_grad_(True), c.x2.clone().requires_grad_(True)
    d1, d2 = nn_distance(p2, t2)
    (d1.mean(1) + d2.mean(1)).sum().backward()
    assert torch.allclose(pred.grad, p2.grad, rtol=1e-5, atol=1e-5) and torch.allclose(true.grad, t2.grad, rtol=1e-5, atol=1e-5)
    # only the prediction requires a gradient: the other one is not computed
    p3 = c.x1.clone().requires_grad_(True)
    chamfer_loss(p3, c.x2).sum().backward()
    assert np.array_equal(bits(p3.grad), bits(pred.grad))
    t4 = c.x2.clone().requires_grad_(True)
    chamfer_loss(c.x1, t4).sum().backward()
    assert t4.grad is not None and np.array_equal(bits(t4.grad), bits(true.grad)) and c.x1.grad is None
    with torch.no_grad():
        assert chamfer_loss(pred, true).grad_fn is None
    with pytest.raises(RuntimeError):
        chamfer_loss(c.x1.cpu(), c.x2.cpu())
    with pytest.raises(RuntimeError):
        chamfer_loss(c.x1.double(), c.x2.double())


def test_nn_distance_under_the_deterministic_flag():
    _gpu()
    import importlib
    ND = importlib.import_module("dpf_nets_amd.metrics.StructuralLosses.nn_distance")     # (the package exports the function under this name)
    c = case(100 + 2500, 2, 2500, 2048, None)

    def backward():
        a, b = c.x1.clone().requires_grad_(True), c.x2.clone().requires_grad_(True)
        d1, d2 = ND.nn_distance(a, b)
        torch.autograd.backward([d1, d2], [c.gd1, c.gd2])
        return [a.grad, b.grad]

    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        first, second = backward(), backward()
    finally:
        torch.use_deterministic_algorithms(was)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(first, second))
    assert_bits(first, c.ref_row, "nn_distance backward under torch.use_deterministic_algorithms(True)")
    # the module attribute overrides the flag either way
    assert not ND.deterministic_backward()
    try:
        ND.DETERMINISTIC_BACKWARD = True
        assert_bits(backward(), c.ref_row, "DETERMINISTIC_BACKWARD = True")
        ND.DETERMINISTIC_BACKWARD = False
        torch.use_deterministic_algorithms(True)
        assert not ND.deterministic_backward()
    finally:
        ND.DETERMINISTIC_BACKWARD = None
        torch.use_deterministic_algorithms(was)


def test_compiled_extension_gives_the_ctypes_backends_bits():
    BK = _gpu()
    from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend_native as native
    c = case(100 + 130, 2, 130, 515, None)
    args = (c.x1, c.x2, c.i1, c.i2, c.gd1, c.gd2)
    got, ref = native.NNDistanceGrad(*args, deterministic=True), BK.NNDistanceGrad(*args, deterministic=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(got, ref))
    assert_bits(got, c.ref_row, "native.NNDistanceGrad(deterministic=True)")
    for x, y in zip(native.NNDistanceGrad(*args), got):              # the reference's six arguments: the reference's (atomic) path
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-5)
    got = native.ChamferCDBackward(c.x1, c.x2, c.i1, c.i2, c.gcd, need2=False)
    ref = BK.ChamferCDBackward(c.x1, c.x2, c.i1, c.i2, c.gcd, need2=False)
    assert got[1] is None and ref[1] is None and np.array_equal(bits(got[0]), bits(ref[0]))
    assert_bits(got, c.ref_cd, "native.ChamferCDBackward")
    with pytest.raises(RuntimeError, match="contiguous"):
        BK.ChamferCDBackward(c.x1[:, ::2], c.x2, c.i1, c.i2, c.gcd)
    with pytest.raises(RuntimeError, match="int32"):
        BK.NNDistanceGrad(c.x1, c.x2, c.i1.long(), c.i2, c.gd1, c.gd2, deterministic=True)
