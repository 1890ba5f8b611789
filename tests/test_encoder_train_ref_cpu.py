"""The float64 restatement of the training-mode encoder (tests/encoder_train_ref.py) that checks csrc/encoder_train.hip on the GPU,
checked itself without one:

  * against float64 autograd of the package's module in train() (tensor ops), pooled through a gather at the restatement's arg;
  * against the vectors captured from the REFERENCE's module in train() mode (tests/golden/encoder.npz, keys *_train_*), at the bars
    tests/test_gpu_encoder_train.py holds the kernel to -- the helper is pinned to the reference, not to this package;
  * every seed of the GPU cases satisfies seed_is_clean;
  * four deliberately wrong restatements differ from the true one, on the case meant to catch each, by more than 100 x the GPU bar:
    the hostile inputs can tell a wrong kernel from a right one."""
import json
import os

import numpy as np
import pytest
import torch

from dpf_nets_amd.networks.encoders import PointNetCloudEncoder
from oracle import detrng
from oracle import encoder_oracle as EO
from tests import encoder_train_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TIGHT = 1e-10
FACTOR = 100.0


def _module_reference(st, xs, g, arg, momentum):
    """float64 autograd of the module in train(), hip_training = False; the last call pooled by gather at `arg`"""
    enc = R.load_module(PointNetCloudEncoder(3, 64, [128, 256, 512]), st)
    enc.hip_training = False
    for name in R.LAYERS:
        getattr(enc.features, name + "_bn").momentum = momentum
    assert enc.training
    for x in xs[:-1]:
        with torch.no_grad():
            enc(x.double())
    xin = xs[-1].double().clone().requires_grad_(True)
    feat = enc(xin)
    assert torch.is_tensor(feat) and feat.dtype == torch.float64
    pooled = torch.gather(feat, 2, arg[:, :, None])[..., 0]
    (pooled * g.double()).sum().backward()
    return enc, pooled.detach(), xin.grad, {k: p.grad for k, p in enc.named_parameters()}


CASES = [(B, N, s, "plain", 0.1) for s in R.STATES for (B, N) in R.SHAPES] + \
        [(3, 33, "signs", "dup", 0.1), (5, 700, "plain", "dup", 0.1), (3, 33, "plain", "pair", 0.5), (1, 2, "plain", "plain", 1.0),
         (3, 33, "plain", "shift", 0.1)]


@pytest.mark.parametrize("B,N,state,kind,momentum", CASES)
def test_restatement_vs_float64_autograd_of_the_module(B, N, state, kind, momentum):
    seed, st, xs, g = R.case_inputs(B, N, state, kind)
    out = R.restate(st, xs, g, momentum=momentum)
    enc, pooled, dx, grads = _module_reference(st, xs, g, out["arg"], momentum)
    assert R.rel(out["pooled"], pooled) <= TIGHT and R.rel(out["dx"], dx) <= TIGHT
    assert set(grads) == set(out["grads"]) == set(R.param_names())
    for k, v in grads.items():
        assert R.rel(out["grads"][k], v) <= TIGHT, k
    sd = enc.state_dict()
    assert len(out["stats"]) == 8
    for k, v in out["stats"].items():
        assert R.rel(v, sd[k]) <= TIGHT, k
    assert all(int(sd["features.%s_bn.num_batches_tracked" % n]) == len(xs) for n in R.LAYERS)
    # the gather is the maximum: no other point of the cloud has a larger feature
    with torch.no_grad():
        enc2 = R.load_module(PointNetCloudEncoder(3, 64, [128, 256, 512]), st)
        enc2.hip_training = False
        assert torch.equal(enc2(xs[-1].double()).max(dim=2)[0], pooled)
    # the states cover what they say they cover
    gam3 = out["fw"]["gam"][3]
    if state == "all_down":
        assert (gam3 < 0).all()
    if state == "signs":
        assert all((g_ < 0).any() and (g_ == 0).sum() >= 3 for g_ in out["fw"]["gam"]) and (out["pooled"][:, 2::9] == 0).all()
    dead_pooled, dead, zero_gamma = R.structural_zeros(st, out["fw"])
    if state == "dead_mid":
        for l in range(3):
            want = torch.zeros_like(dead[l])
            want[2::11] = True
            want[5::13] = False                                            # index 57 is in both: gamma = 0, beta = +0.7 holds
            assert dead[l][want].all() and want.sum() >= 5 and zero_gamma[l][5::13].all()
            assert (out["fw"]["a"][l + 1][:, 5::13] == float(np.float32(0.7))).all()
    # the structural zeros are exact zeros of the restatement
    for l, name in enumerate(R.LAYERS):
        W = out["grads"]["features.%s.weight" % name][0]
        off = zero_gamma[l] | (dead_pooled if l == 3 else dead[l])
        assert (W[off] == 0).all()
        gone = dead_pooled if l == 3 else dead[l]
        assert (out["grads"]["features.%s_bn.weight" % name][gone] == 0).all() and (out["grads"]["features.%s_bn.bias" % name][gone] == 0).all()
        if l > 0:
            assert (W[:, dead[l - 1]] == 0).all()


def test_duplicates_tie_and_the_lowest_index_wins():
    B, N = 5, 700
    seed = R.SEEDS[(B, N, "signs", "dup")]
    x = R.case_clouds(seed, B, N, "dup")[0]
    assert torch.equal(x[:, :, 0], x[:, :, N - 1]) and torch.equal(x[:, :, 3], x[:, :, 35])
    fw = R.forward(R.make_state("signs", seed), x)
    assert not (fw["arg"] == N - 1).any() and not (fw["arg"] == 35).any()
    hit = (fw["arg"] == 0) | (fw["arg"] == 3)
    assert hit.any()                                                       # the duplicated points do win features
    last = R.forward(R.make_state("signs", seed), x, rule="last")
    assert torch.equal(last["arg"][hit], torch.where(fw["arg"][hit] == 0, N - 1, 35)) and torch.equal(last["arg"][~hit], fw["arg"][~hit])
    assert R.rel(last["pooled"], fw["pooled"]) <= 1e-14


@pytest.mark.parametrize("case", ["a", "b"])
def test_restatement_vs_reference_fixture(case):
    """pooled, dx, gradient projections and running statistics of the reference's own module in train() mode, at the bars of
    tests/test_gpu_encoder_train.py"""
    from oracle.gen_golden import _grad_projection
    gold = np.load(os.path.join(HERE, "golden", "encoder.npz"))
    with open(os.path.join(HERE, "golden", "encoder.json")) as f:
        seed, B, N = json.load(f)["cases"][case]
    st = EO.make_encoder_state(seed)
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N))
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512)))
    out = R.restate(st, [x], g)
    tag = case + "_train"
    assert R.rel(out["pooled"], torch.from_numpy(gold[tag + "_max"])) <= R.TOL_OUT
    assert R.rel(out["dx"], torch.from_numpy(gold[tag + "_dx"])) <= R.TOL_GRAD
    proj = _grad_projection([(k, out["grads"][k]) for k in R.param_names()], seed)
    assert len(proj) == 12
    for k, v in proj.items():
        ref = gold[tag + "_gproj_" + k]
        for i in range(3):
            assert abs(v[i] - ref[i]) <= 1e-3 * (ref[2] + 1e-6) + 1e-5, (k, v, ref)
    for k, v in out["stats"].items():
        assert R.rel(v, torch.from_numpy(gold[tag + "_stat_" + k])) <= R.TOL_STAT, k


def test_every_seed_is_clean():
    for (B, N, state, kind), seed in R.SEEDS.items():
        st = R.make_state(state, seed)
        for x in R.case_clouds(seed, B, N, kind):
            ok, near, narrow = R.seed_is_clean(st, x)
            assert ok, (B, N, state, kind, seed, near, narrow)
    assert not set(R.SEEDS) & set(R.LEAST_UNCLEAN)
    for (B, N, state, kind), (seed, near, narrow) in R.LEAST_UNCLEAN.items():      # the one case without a clean seed: the record is true
        (x,) = R.case_clouds(seed, B, N, kind)
        assert R.seed_is_clean(R.make_state(state, seed), x) == (False, near, narrow)


def test_seed_is_clean_rejects_what_it_should():
    """a pre-activation moved onto zero at an argmax point, and a runner-up moved next to the winner, are both seen; the copy of a
    winner is not a runner-up"""
    B, N, seed = 3, 33, R.SEEDS[(3, 33, "plain", "plain")]
    st = R.make_state("plain", seed)
    x = R.case_clouds(seed, B, N, "plain")[0]
    assert R.seed_is_clean(st, x) == (True, 0, 0)
    fw = R.forward(st, x)
    p = int(fw["arg"][0, 0])
    bad = {k: np.array(v, copy=True) for k, v in st.items()}               # beta moves z0[point p, feature 5] to ~0
    bad["features.init_sd_bn.bias"][5] -= np.float32(fw["z"][0][p, 5])
    ok, near, _ = R.seed_is_clean(bad, x)
    assert not ok and near >= 1
    x2 = x.clone()                                                         # a second point next to the winner of feature 0
    q = (p + 1) % N
    x2[0, :, q] = x2[0, :, p] * (1 + 2.0 ** -22)
    ok, _, narrow = R.seed_is_clean(st, x2)
    assert not ok and narrow >= 1
    x3 = x.clone()
    x3[0, :, q] = x3[0, :, p]
    assert R.seed_is_clean(st, x3)[2] == 0


def _diffs(true, wrong):
    """{quantity: (relative difference, GPU bar)}"""
    d = {"pooled": (R.rel(wrong["pooled"], true["pooled"]), R.TOL_OUT), "dx": (R.rel(wrong["dx"], true["dx"]), R.TOL_GRAD)}
    for k in true["grads"]:
        d[k] = (R.rel(wrong["grads"][k], true["grads"][k]), R.TOL_GRAD)
    for k in true["stats"]:
        d[k] = (R.rel(wrong["stats"][k], true["stats"][k]), R.TOL_STAT)
    return d


def _told_apart(d):
    return [k for k, (diff, bar) in d.items() if diff > FACTOR * bar]


@pytest.mark.parametrize("B,N", R.SHAPES)
def test_sensitivity_pool_by_max_y3_regardless_of_sign(B, N):
    for state in ("all_down", "signs"):
        _, st, xs, g = R.case_inputs(B, N, state)
        d = _diffs(R.restate(st, xs, g), R.restate(st, xs, g, rule="max_y3"))
        assert "pooled" in _told_apart(d) and "dx" in _told_apart(d), (state, d)


@pytest.mark.parametrize("state", ["plain", "signs"])
@pytest.mark.parametrize("B,N", R.SHAPES[1:])
def test_sensitivity_last_winning_point(B, N, state):
    _, st, xs, g = R.case_inputs(B, N, state, "dup")
    d = _diffs(R.restate(st, xs, g), R.restate(st, xs, g, rule="last"))
    assert "dx" in _told_apart(d), d
    assert d["pooled"][0] <= 1e-12                                         # only the gradient's place tells them apart


def test_sensitivity_biased_variance_into_running_var():
    _, st, xs, g = R.case_inputs(1, 2, "plain")
    for m in (0.1, 0.5, 1.0):
        d = _diffs(R.restate(st, xs, g, momentum=m), R.restate(st, xs, g, momentum=m, unbiased=False))
        assert all("features.%s_bn.running_var" % n in _told_apart(d) for n in R.LAYERS), (m, d)


def test_sensitivity_momentum_applied_once_for_two_calls():
    _, st, xs, g = R.case_inputs(3, 33, "plain", "pair")
    assert len(xs) == 2
    d = _diffs(R.restate(st, xs, g), R.restate(st, xs, g, once=True))
    assert all(k in _told_apart(d) for k in d if "running" in k), d
