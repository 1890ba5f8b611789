"""csrc/encoder_train.hip where the seeded states of tests/test_gpu_encoder_train.py never take it, against the float64 restatement
of tests/encoder_train_ref.py (which makes the kernel's tie choice and is pinned by tests/test_encoder_train_ref_cpu.py):

  * negative BatchNorm scales -- the `!up` half of et_pool_kernel with the tile minima of the layer-3 epilogue, c0 < 0 in the FWD
    prologue, the sign of c2 in et_bn_bwd_finish --, zero scales (every point ties) and dead features, in every layer, with exact
    zeros where the gradient is zero by structure;
  * exact ties of the maximum (duplicate points, inside a tile and across a tile boundary): the lowest index takes the gradient;
  * running statistics: two consecutive calls, momentum 0.5 and 1.0, the unbiased variance at its smallest count (B N = 2), clouds
    far from the origin;
  * train_precision = "bf16x3" (the NS = 2 forward GEMMs), forward only; torch.no_grad() in train().

Every call goes through PointNetCloudEncoder.train() and torch.max(feats, dim=2)[0].  Bars: those of tests/test_gpu_encoder_train.py,
relative to the tensor's largest magnitude.  Seeds: picked on the float64 restatement alone (encoder_train_ref.SEEDS)."""
import functools

import pytest
import torch

from tests import encoder_train_ref as R
from tests.encoder_train_ref import TOL_OUT, TOL_GRAD, TOL_STAT, rel

pytestmark = pytest.mark.gpu

HOSTILE = ("signs", "all_down", "dead_mid")
TIE_SHAPES = R.SHAPES[1:]


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd import networks
    return networks


def _encoder(nets, st, momentum=None, precision=None):
    enc = nets.PointNetCloudEncoder(3, 64, [128, 256, 512])
    R.load_module(enc, st, torch.float32)
    if momentum is not None:
        for name in R.LAYERS:
            getattr(enc.features, name + "_bn").momentum = momentum
    if precision is not None:
        enc.train_precision = precision
    return enc.cuda().train()


def _step(enc, x, r):
    for p in enc.parameters():
        p.grad = None
    x.grad = None
    feats = enc(x)
    pooled = torch.max(feats, dim=2)[0]
    (pooled * r).sum().backward()
    return feats, pooled


@functools.lru_cache(maxsize=None)
def _case(B, N, state, kind="plain", momentum=0.1):
    """the case's inputs and its float64 restatement, computed once and shared"""
    _, st, xs, g = R.case_inputs(B, N, state, kind)
    return st, xs, g, R.restate(st, xs, g, momentum=momentum)


def _run(nets, B, N, state, kind="plain", momentum=0.1, **kw):
    st, xs, g, ref = _case(B, N, state, kind, momentum)
    enc = _encoder(nets, st, momentum=momentum, **kw)
    r = g.cuda()
    for x in xs:
        xg = x.cuda().requires_grad_(True)
        feats, pooled = _step(enc, xg, r)
        assert isinstance(feats, nets.TrainPointFeatures) and feats._full is None
    return enc, xg, pooled, ref


def _errors(enc, x, pooled, ref):
    """{quantity: (relative error, bar)} of pooled, dx, the twelve gradients and the eight running statistics"""
    err = {"pooled": (rel(pooled, ref["pooled"]), TOL_OUT), "dx": (rel(x.grad, ref["dx"]), TOL_GRAD)}
    grads = dict(enc.named_parameters())
    assert set(grads) == set(ref["grads"])
    for k, v in ref["grads"].items():
        assert grads[k].grad is not None and torch.isfinite(grads[k].grad).all()
        err[k] = (rel(grads[k].grad, v), TOL_GRAD)
    sd = enc.state_dict()
    for k, v in ref["stats"].items():
        err[k] = (rel(sd[k], v), TOL_STAT)
    assert len(err) == 22
    return err


def _hold(label, err, check=True):
    worst = {}
    for k, (e, bar) in err.items():
        kind = "pooled" if k == "pooled" else "dx" if k == "dx" else "stat" if "running" in k else "grad"
        worst[kind] = max(worst.get(kind, 0.0), e)
    print("%s: " % (label,) + "  ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    for k, (e, bar) in err.items():
        assert e <= bar or not check, (label, k, e, bar)


def _exact_zeros(enc, pooled, st, ref):
    """exactly 0.0 wherever the restatement is zero by structure; -> how many features of each kind were checked"""
    dead_pooled, dead, zero_gamma = R.structural_zeros(st, ref["fw"])
    grad = {k: p.grad.cpu() for k, p in enc.named_parameters()}
    assert (pooled.cpu()[ref["pooled"] == 0] == 0).all()
    for l, name in enumerate(R.LAYERS):
        W = grad["features.%s.weight" % name][0]
        gone = dead_pooled if l == 3 else dead[l]
        assert (W[gone] == 0).all(), name
        assert (grad["features.%s_bn.weight" % name][gone] == 0).all() and (grad["features.%s_bn.bias" % name][gone] == 0).all(), name
        assert (W[zero_gamma[l]] == 0).all(), name                        # d y = gamma rstd (...) = 0
        if l > 0:
            assert (W[:, dead[l - 1]] == 0).all(), name                   # an all-zero row of the packed a_{l-1} operand
    return int(dead_pooled.sum()), [int(d.sum()) for d in dead], [int(z.sum()) for z in zero_gamma]


@pytest.mark.parametrize("B,N", R.SHAPES)
@pytest.mark.parametrize("state", HOSTILE)
def test_hostile_states(state, B, N):
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, B, N, state)
    st = _case(B, N, state)[0]
    gam3 = ref["fw"]["gam"][3]
    down = int((gam3 < 0).sum())
    assert down == (512 if state == "all_down" else 97 if state == "signs" else 0)        # 1::5 of 512 less the six that 3::16 zeroes
    n_pool, n_dead, n_zero = _exact_zeros(enc, pooled, st, ref)
    if state == "signs":
        assert n_pool >= 57 and all(n >= 4 for n in n_zero)
    if state == "dead_mid":
        assert all(n >= 5 for n in n_dead) and all(n >= 5 for n in n_zero[:3])
    print("%s (%d,%d): %d features pool through the minima, %d pooled dead, hidden dead %s, zero gamma %s" % (state, B, N, down, n_pool, n_dead, n_zero))
    _hold((state, B, N), _errors(enc, x, pooled, ref))
    assert all(int(getattr(enc.features, n + "_bn").num_batches_tracked) == 1 for n in R.LAYERS)


@pytest.mark.parametrize("B,N", TIE_SHAPES)
@pytest.mark.parametrize("state", ["plain", "signs"])
def test_ties_give_the_gradient_to_the_lowest_index(state, B, N):
    """with_duplicates: point N-1 is point 0 (same tile at N = 33, the last tile's ragged end at N = 700) and point 35 is point 3
    (across a tile boundary).  dx elementwise: right only if the lowest index took the sparse part of the gradient (the wrong choice
    is more than 100 x TOL_GRAD away, tests/test_encoder_train_ref_cpu.py)."""
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, B, N, state, "dup")
    wins = int(((ref["arg"] == 0) | ((ref["arg"] == 3) if N > 40 else False)).sum())
    assert wins > 0 and not (ref["arg"] == N - 1).any()
    print("ties %s (%d,%d): %d (cloud, feature) winners have a copy" % (state, B, N, wins))
    _hold(("ties", state, B, N), _errors(enc, x, pooled, ref))


def test_two_consecutive_calls_compound_the_statistics():
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, 3, 33, "plain", "pair")
    assert len(_case(3, 33, "plain", "pair")[1]) == 2
    _hold("two calls", _errors(enc, x, pooled, ref))
    assert all(int(getattr(enc.features, n + "_bn").num_batches_tracked) == 2 for n in R.LAYERS)


@pytest.mark.parametrize("momentum", [0.5, 1.0])
def test_momentum_on_all_four_layers(momentum):
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, 3, 33, "plain", momentum=momentum)
    _hold(("momentum", momentum), _errors(enc, x, pooled, ref))
    if momentum == 1.0:                                                    # running = the batch statistic
        for l, name in enumerate(R.LAYERS):
            bn = getattr(enc.features, name + "_bn")
            assert rel(bn.running_mean, ref["fw"]["mean"][l]) <= TOL_STAT
            assert rel(bn.running_var, ref["fw"]["var"][l] * (99.0 / 98.0)) <= TOL_STAT


def test_smallest_count_takes_the_unbiased_factor_of_two():
    """(1,2): the smallest count the module sends to HIP; running_var takes var n / (n - 1) = 2 var"""
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, 1, 2, "plain")
    _hold("(1,2)", _errors(enc, x, pooled, ref))
    for l, name in enumerate(R.LAYERS):
        bn, rv0 = getattr(enc.features, name + "_bn"), R._t(_case(1, 2, "plain")[0], "features.%s_bn.running_var" % name)
        assert rel(bn.running_var, 0.9 * rv0 + 0.1 * 2.0 * ref["fw"]["var"][l]) <= TOL_STAT


@pytest.mark.parametrize("B,N", TIE_SHAPES)
def test_clouds_far_from_the_origin(B, N):
    """+8.0 on every axis: the variance of y0 is far below its squared mean (the case of the Chan / M2 statistics of et_l0 and
    et_bn_finish).  |y0| / std(y0) is ~40 here, so fp32 rounding of y0 alone moves xhat0 by ~3e-6 -- more than the 1e-6 the seeds
    keep clear of zero -- and at (5,700) a ReLU at an argmax point takes the other subgradient than float64's in ANY fp32 arithmetic.

    The bars of tests/test_gpu_encoder_train.py apply first.  A quantity that misses one is held to 2 x the error of the fp32
    tensor-op path (hip_training = False, the arithmetic the reference runs; 2 for its run-to-run reduction order) on the same
    quantity against the same restatement, measured here: the kernel is never worse than that.  Measured on an MI355X:
      (3,33)   kernel: pooled 3.2e-6, dx 2.7e-5, gradients <= 1.4e-4, statistics 3.4e-7 -- all within the bars;
               fp32 tensor ops: pooled 8.1e-5, dx 7.8e-3, gradients <= 2.7e-2, statistics 4.9e-6
      (5,700)  kernel: pooled 3.3e-6, statistics 1.8e-7, ten gradients within TOL_GRAD; dx 9.88e-4 and d beta of layer 0 1.26e-3 miss
               it.  fp32 tensor ops on those two: 2.74e-2 and 1.97e-2 (bars 5.5e-2 and 3.9e-2); its worst gradient 8.5e-2, pooled
               8.6e-5, statistics 8.4e-6"""
    nets = _gpu()
    enc, x, pooled, ref = _run(nets, B, N, "plain", "shift")
    st, xs, g, _ = _case(B, N, "plain", "shift")
    t32 = _encoder(nets, st)
    t32.hip_training = False
    x32 = xs[0].cuda().requires_grad_(True)
    feats32, pooled32 = _step(t32, x32, g.cuda())
    assert torch.is_tensor(feats32)
    err, err32 = _errors(enc, x, pooled, ref), _errors(t32, x32, pooled32, ref)
    _hold(("fp32 tensor ops, shifted", B, N), err32, check=False)
    _hold(("shifted", B, N), err, check=False)
    for k, (e, bar) in err.items():
        if e > bar:
            print("  %s misses %.3g: kernel %.3g, fp32 tensor ops %.3g" % (k, bar, e, err32[k][0]))
            bar = 2.0 * err32[k][0]
        assert e <= bar, (B, N, k, e, bar)


@pytest.mark.parametrize("B,N", R.SHAPES)
@pytest.mark.parametrize("state", ["plain", "signs"])
def test_bf16x3_forward(state, B, N):
    """train_precision = "bf16x3": the NS = 2 instantiation of every forward GEMM.  Pooled and the running statistics against float64;
    two runs bit-identical; the gradients are NOT held to float64 (this precision trades ReLU-decision parity,
    docs/DESIGN_history_r01_r03.md 4.7) -- they are finite, of the right shapes, and backward runs."""
    nets = _gpu()
    st, xs, g, ref = _case(B, N, state)
    runs = []
    for _ in range(2):
        enc = _encoder(nets, st, precision="bf16x3")
        x = xs[0].cuda().requires_grad_(True)
        feats, pooled = _step(enc, x, g.cuda())
        assert isinstance(feats, nets.TrainPointFeatures) and feats._full is None
        runs.append([pooled.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in enc.parameters()] +
                    [v.clone() for k, v in enc.state_dict().items() if "running" in k])
    assert len(runs[0]) == 22 and all(torch.equal(a, b) for a, b in zip(*runs))
    err = {k: v for k, v in _errors(enc, x, pooled, ref).items() if k == "pooled" or "running" in k}
    _hold(("bf16x3", state, B, N), err)
    assert x.grad.shape == x.shape and torch.isfinite(x.grad).all()
    for p in enc.parameters():
        assert p.grad.shape == p.shape and torch.isfinite(p.grad).all()
    rm = enc.features.sd2_bn.running_mean.clone()
    full = feats.tensor()
    assert full.shape == (B, 512, N) and torch.equal(enc.features.sd2_bn.running_mean, rm)
    assert rel(full.max(dim=2)[0], pooled) <= TOL_OUT


def test_no_grad_in_train_mode_on_signs():
    nets = _gpu()
    B, N = 3, 33
    enc, x, pooled, ref = _run(nets, B, N, "signs")
    st, xs, g, _ = _case(B, N, "signs")
    enc2 = _encoder(nets, st)
    with torch.no_grad():
        p2 = torch.max(enc2(xs[0].cuda()), dim=2)[0]
    assert torch.equal(p2, pooled) and not p2.requires_grad
    for n in R.LAYERS:
        a, b = getattr(enc.features, n + "_bn"), getattr(enc2.features, n + "_bn")
        assert int(b.num_batches_tracked) == 1
        assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
        assert rel(b.running_mean, ref["stats"]["features.%s_bn.running_mean" % n]) <= TOL_STAT
