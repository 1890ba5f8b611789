"""The checkers of tests/test_gpu_film_edges.py, pinned without a GPU (tests/film_ref.py):

  * `film_train_ref` in float64 against float64 autograd through the module's own layers of one sub-net (Linear without bias,
    BatchNorm1d in train(), Swish, Linear, as networks/flows.py builds them), its running statistics update included, at 1e-12;
  * `film_frozen_ref` in float64 against frozen_engine._film_forward / _film_backward in float64 at 1e-12;
  * the class A precondition: at every class A case, training and frozen, the fp32 formulation's own error against float64 under
    `rel_per_net` is at most a quarter of the class A bar of that tensor, film_ref.BARS (measured here: training 7.8e-7 forward, 5.6e-7 statistics,
    2.0e-6 backward -- dW0 at (3,5,128); frozen 5.3e-7, 9.5e-8, 1.8e-6), so a class A bar is never met by fp32 rounding alone;
  * the r32 rule is capped: class B is exactly the enumerated tuple, nothing outside it may use the rule;
  * `make_case` builds the hostile and scaled states it promises, `rel_per_net` sees one wrong sub-net and one non-zero behind a zero."""
import pytest
import torch
import torch.nn as nn

from tests import film_ref as R
from tests.film_ref import F, EPS

AGREE = 1e-12


def _inputs(K, B, G, variant="seeded", offset=0.0):
    c = R.make_case(K, B, G, R.case_seed(K, B, G), variant, offset)
    return c, (c["g"], c["W0"], c["gam"], c["bet"], c["W1"], c["b1"], c["dfm"])


def _ref(mode, dtype, c, a):
    if mode == "train":
        return R.film_train_ref(dtype, *a, EPS)
    return R.film_frozen_ref(dtype, *a, c["rm"], c["rv"], EPS)


@pytest.mark.parametrize("K,B,G,variant", [(3, 5, 128, "seeded"), (2, 17, 260, "hostile"), (5, 4, 68, "scaled")])
def test_training_reference_vs_the_modules_own_layers(K, B, G, variant):
    from dpf_nets_amd.networks.layers import Swish
    c, a = _inputs(K, B, G, variant)
    ref = R.film_train_ref(torch.float64, *a, EPS)
    for k in range(K):
        net = nn.Sequential(nn.Linear(G, F, bias=False), nn.BatchNorm1d(F), Swish(), nn.Linear(F, F, bias=True)).double().train()
        with torch.no_grad():
            net[0].weight.copy_(c["W0"][k]); net[1].weight.copy_(c["gam"][k]); net[1].bias.copy_(c["bet"][k])
            net[3].weight.copy_(c["W1"][k]); net[3].bias.copy_(c["b1"][k])
        assert net[1].eps == EPS
        g = c["g"].double().requires_grad_(True)
        fm = net(g)
        (fm * c["dfm"][k].double()).sum().backward()
        got = dict(fm=fm, dW0=net[0].weight.grad, dgam=net[1].weight.grad, dbet=net[1].bias.grad, dW1=net[3].weight.grad,
                   db1=net[3].bias.grad, dg_part=g.grad)
        for name, v in got.items():
            r = R.rel_per_net(v, ref[name][k], False)
            assert r <= AGREE, (k, name, r)
        m = net[1].momentum
        assert R.rel_per_net(net[1].running_mean, m * ref["mean"][k], False) <= AGREE
        assert R.rel_per_net(net[1].running_var, (1 - m) + m * ref["uvar"][k], False) <= AGREE
    assert R.rel_per_net(ref["dg_part"].sum(0), ref["dg"], False) <= AGREE


@pytest.mark.parametrize("K,B,G,variant", [(3, 5, 128, "seeded"), (7, 1, 128, "seeded"), (2, 17, 260, "hostile"), (5, 4, 68, "scaled")])
def test_frozen_reference_vs_the_frozen_formulas(K, B, G, variant):
    from dpf_nets_amd.networks.frozen_engine import _film_forward, _film_backward
    c, a = _inputs(K, B, G, variant)
    ref = R.film_frozen_ref(torch.float64, *a, c["rm"], c["rv"], EPS)
    d = {k: v.double() for k, v in c.items()}
    col = lambda t: t.unsqueeze(1)
    rstd = torch.rsqrt(col(d["rv"]) + EPS)
    fm, xhat, y, sig, sw = _film_forward(d["g"], d["W0"], col(d["gam"]), col(d["bet"]), d["W1"], col(d["b1"]), col(d["rm"]), rstd)
    back = _film_backward(d["dfm"], d["g"], d["W0"], col(d["gam"]), d["W1"], rstd, xhat, y, sig, sw, True)
    got = dict(zip(("dW0", "dgam", "dbet", "dW1", "db1", "dg"), back), fm=fm, xhat=xhat, rstd=rstd)
    for name, v in got.items():
        r = R.rel_per_net(v, ref[name], name != "dg")
        assert r <= AGREE, (name, r)
    du = torch.rsqrt(d["rv"] + EPS).unsqueeze(1) * d["gam"].unsqueeze(1) * (torch.matmul(d["dfm"], d["W1"]) * (sig * (1.0 + y * (1.0 - sig))))
    assert R.rel_per_net(torch.bmm(du, d["W0"]), ref["dg_part"]) <= AGREE
    assert R.rel_per_net(ref["dg_part"].sum(0), ref["dg"], False) <= AGREE


@pytest.mark.parametrize("mode", R.MODES)
def test_class_a_precondition(mode):
    seen = 0
    for case in R.cases(mode):
        if R.is_class_b(mode, *case):
            continue
        K, B, G, variant, offset = case
        c, a = _inputs(K, B, G, variant, offset)
        r64, r32 = _ref(mode, torch.float64, c, a), _ref(mode, torch.float32, c, a)
        for name, kind in R.KIND.items():
            if name in r64:
                r = R.rel_per_net(r32[name], r64[name], name != "dg")
                print("R32", R.case_id(mode, *case), name, "%.3e" % r)
                assert r <= R.BARS[mode][kind] / 4, (case, name, r)
        seen += 1
    assert seen == (8 if mode == "train" else 15)


def test_the_r32_rule_is_capped():
    every = [(mode,) + case for mode in R.MODES for case in R.cases(mode)]
    assert len(every) == len(set(every)) == 21 + 23
    assert len(R.CLASS_B) == len(set(R.CLASS_B)) == 21 and set(R.CLASS_B) <= set(every)
    for case in every:
        assert (case in R.CLASS_B) == R.is_class_b(*case), case
        mode, K, B, G, variant, offset = case
        assert R.is_class_b(*case) == (variant in ("hostile", "scaled") or offset != 0 or (mode == "train" and B < 4))
        for name, kind in R.KIND.items():
            a = R.BARS[mode][kind]
            assert a <= R.CLASS_A_BARS[mode][kind]                                                # tightened, never widened
            huge = R.bar_for(R.BARS, *case, name, 1.0)
            assert huge == (R.R32_FACTOR if case in R.CLASS_B else a), (case, name)            # r32 enters for class B alone
            assert R.bar_for(R.BARS, *case, name, 0.0) == a                                # and never lowers a bar
    assert not any(off and B < 4 for (_, _, B, _, _, off) in every)                                # offset at B < 4 says nothing
    assert R.bar_for(R.BARS, "train", 2, 64, 516, "seeded", 0.0, "dW0", 1e-3) == 2e-5
    assert R.bar_for(R.BARS, "train", 2, 64, 516, "seeded", 50.0, "dW0", 1e-3) == 8e-3


def test_make_case_builds_what_it_promises():
    K, B, G = 9, 63, 196
    c, a = _inputs(K, B, G, "hostile")
    s = R.make_case(K, B, G, R.case_seed(K, B, G), "seeded")
    assert bool((c["gam"][:, 0::4] == -s["gam"][:, 0::4]).all()) and bool((c["gam"][:, 1] == 0).all()) and bool((c["W0"][:, 2] == 0).all())
    assert bool((c["bet"][:, 3] == -30).all()) and bool((c["bet"][:, 5] == 30).all()) and bool((c["gam"][:, 7] == 40 * s["gam"][:, 7]).all())
    ref = R.film_train_ref(torch.float64, *a, EPS)
    assert float(ref["y"].min()) < -88 and float(ref["y"].max()) > 88
    assert bool((ref["xhat"][:, :, 2] == 0).all()) and bool((ref["dW0"][:, 1] == 0).all()) and float(ref["dW0"][:, 2].abs().max()) > 0
    assert torch.allclose(ref["rstd"][:, 2], torch.full((K,), EPS ** -0.5, dtype=torch.float64), rtol=1e-12)
    c = R.make_case(K, B, G, R.case_seed(K, B, G), "scaled")
    assert torch.equal(c["W0"][0], s["W0"][0] * 2.0 ** -10) and torch.equal(c["W0"][K - 1], s["W0"][K - 1] * 2.0 ** 10)
    assert torch.equal(c["dfm"][0], s["dfm"][0] * 2.0 ** 8) and torch.equal(c["dfm"][K - 1], s["dfm"][K - 1] * 2.0 ** -8)
    assert torch.equal(R.make_case(2, 16, 128, 5, "seeded", 50.0)["g"], R.make_case(2, 16, 128, 5, "seeded")["g"] + 50.0)


def test_rel_per_net_sees_one_small_sub_net_and_a_broken_zero():
    ref = torch.randn(4, 5, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref[2] *= 1e-6                                             # a sub-net of small magnitude
    ref[2, 0, 0] = 1e-5                                       # (its largest entry)
    ref[1, :, 3] = 0
    got = ref.clone()
    got[2, 0, 0] *= 1.5
    whole = float((got - ref).abs().max() / ref.abs().max())
    assert whole < 1e-5 and R.rel_per_net(got, ref, False) == whole              # invisible in one number over all sub-nets
    assert abs(R.rel_per_net(got, ref) - 0.5) < 1e-12
    got = ref.clone()
    got[1, 0, 3] = 1e-30
    with pytest.raises(AssertionError):
        R.rel_per_net(got, ref)
    got = ref.clone()
    got[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        R.rel_per_net(got, ref)
    zero = torch.zeros(2, 3, dtype=torch.float64)
    assert R.rel_per_net(zero.float(), zero) == 0.0
