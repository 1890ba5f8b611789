"""The checkers of tests/test_gpu_gprior_train.py, pinned without a GPU (tests/gprior_train_ref.py):

  * `oracle64_train` against what the reference's own GlobalRNVPDecoder gave under train() (the `*_train_*` vectors of
    tests/golden/gprior.npz): the three lists and d/dg at 1e-4 (measured: lists <= 7e-7, d/dg <= 2e-6; the goldens are fp32), the
    projections of every parameter gradient by tests/test_gpu_gprior.py's rule, the running statistics at 1e-5;
  * `step64`, the explicit-codes float64 step of the C-ABI tests, against `oracle64_train` on the module's own code sequence in both
    block layouts at 1e-12 (two float64 evaluations of the same arithmetic);
  * the state mutators produce the hostile states they promise."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gprior_oracle as GO
from tests import gprior_train_ref as R
from tests.gprior_train_ref import NAMES, rel

TOL = 1e-4
MODES = ("direct", "inverse")


def test_float64_training_oracle_vs_reference_golden(golden_dir):
    from oracle.gen_golden import _grad_projection
    gold = np.load(os.path.join(golden_dir, "gprior.npz"))
    meta = json.load(open(os.path.join(golden_dir, "gprior.json")))
    cases = {c: v for c, v in meta["cases"].items() if v[4] >= 2}
    assert sorted(cases) == ["a", "b", "c"]
    for case, (seed, n_flows, nf, G, B) in cases.items():
        for mode in MODES:
            tag = "%s_train_%s_" % (case, mode)
            ref = R.oracle64_train(seed, n_flows, nf, G, B, mode)
            for name in NAMES:
                r = rel(ref[name], gold[tag + name])
                print("REL", case, mode, name, r)
                assert r <= TOL, (case, mode, name, r)
            r = rel(ref["dg"], gold[tag + "dg"])
            print("REL", case, mode, "dg", r)
            assert r <= TOL, (case, mode, r)
            proj = _grad_projection([(k, torch.from_numpy(v)) for k, v in ref["grads"].items()], seed)
            assert len(proj) == 10 * 2 * n_flows
            for k, v in proj.items():
                g = gold[tag + "gproj_" + k]
                np.testing.assert_allclose(v, g, rtol=1e-3, atol=1e-4 * max(1.0, float(g[2])), err_msg=case + mode + k)
            assert len(ref["stats"]) == 4 * 2 * n_flows
            for k, v in ref["stats"].items():
                assert rel(v, gold[tag + "stat_" + k]) <= 1e-5, (case, mode, k)


@pytest.mark.parametrize("mutate", [None, R.hostile_bn, R.floor_active])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_flows,nf,G,B", [(2, 40, 6, 9), (1, 8, 2, 3), (2, 24, 20, 31)])
def test_explicit_codes_step_agrees_with_the_oracle(n_flows, nf, G, B, mode, mutate):
    seed, S = 900 + G + B, 2 * n_flows
    ref = R.oracle64_train(seed, n_flows, nf, G, B, mode, mutate)
    state = R.make_state(seed, n_flows, nf, G, mutate)
    g = R.inputs(seed, B, G)
    w = [t.numpy() for t in R.projection_weights(seed, S, B, G)]
    for params_only in (0, 1):
        blocks, total, stat_slots = R.param_blocks(S, nf, G, params_only)
        block = R.canon_block(state, S, G, params_only)
        assert block.size == total
        got = R.step64(block, params_only, R.module_codes(n_flows), G, nf, g, mode, w)
        for name in NAMES + ("dg",):
            assert rel(got[name], ref[name]) <= 1e-12, (params_only, name, rel(got[name], ref[name]))
        assert sorted(k for k, _, _ in blocks) == sorted(ref["grads"])
        for k, o, shape in blocks:
            piece = got["dcanon"][o:o + int(np.prod(shape))].reshape(shape)
            assert rel(piece, ref["grads"][k]) <= 1e-12, (params_only, k, rel(piece, ref["grads"][k]))
        for o, n in stat_slots:
            assert not got["dcanon"][o:o + n].any()
        # the batch statistics the step returns are the ones behind the oracle's running statistics
        for s, (prefix, _, _) in enumerate(GO.step_plan(n_flows, G)):
            for net, br in enumerate(("mu", "logvar")):
                base = "%sT_%s_0.%s_mlp0_bn." % (prefix, br, br)
                mean, var = got["stats"][s, 0, net * nf:(net + 1) * nf], got["stats"][s, 1, net * nf:(net + 1) * nf]
                rm, rv = (state[base + k].astype(np.float64) for k in ("running_mean", "running_var"))
                assert rel(0.9 * rm + 0.1 * mean, ref["stats"][base + "running_mean"]) <= 1e-12
                assert rel(0.9 * rv + 0.1 * var * B / (B - 1.0), ref["stats"][base + "running_var"]) <= 1e-12


def test_explicit_codes_step_null_tables_and_code_indices():
    assert R.code_indices(0, 6) == ([0, 2, 4], [1, 3, 5]) and R.code_indices(1, 6) == ([1, 3, 5], [0, 2, 4])
    assert R.code_indices(2, 6) == ([0, 1, 2], [3, 4, 5]) and R.code_indices(3, 6) == ([3, 4, 5], [0, 1, 2])
    assert [R.code_indices(c, 2)[0] for c in range(4)] == [[0], [1], [0], [1]]
    for n_flows in (1, 2, 3):
        assert [R.code_indices(c, 8)[0] for c in R.module_codes(n_flows)] == [w for _, w, _ in GO.step_plan(n_flows, 8)]
    nf, G, B, codes = 8, 6, 4, [3, 0, 1]
    state = R.make_state(5, 2, nf, G)
    block = R.canon_block(state, 3, G, 1)
    got = R.step64(block, 1, codes, G, nf, R.inputs(5, B, G), "direct", [None, None, None])
    assert not got["dg"].any() and not got["dcanon"].any() and got["gs"].shape == (3, B, G)
    for s, c in enumerate(codes):
        keep = R.code_indices(c, G)[1]
        assert not got["mus"][s][:, keep].any() and not got["lvs"][s][:, keep].any()


@pytest.mark.parametrize("n_flows,nf,G,B", [(2, 40, 6, 9), (2, 24, 20, 31), (1, 8, 2, 3)])
def test_mutators_make_the_states_they_promise(n_flows, nf, G, B):
    seed = 900 + G + B
    plain = R.make_state(seed, n_flows, nf, G)
    host = R.make_state(seed, n_flows, nf, G, R.hostile_bn)
    assert sorted(plain) == sorted(host) and host is not plain
    nets = [k for k in host if k.endswith("mlp0_bn.weight")]
    assert len(nets) == 4 * n_flows
    for k in nets:
        w, w0 = host[k], host[k.replace("mlp0_bn.weight", "mlp0.weight")]
        assert w[0] == 0 and (w < 0).sum() == max(1, round(0.4 * nf)) and (w == 0).sum() == 1
        assert np.array_equal(np.abs(w[1:]), np.abs(plain[k][1:]))
        assert not w0[-1].any() and w0[:-1].any(axis=1).all()
    assert all(np.array_equal(plain[k], host[k]) for k in plain if "mlp0_bn.weight" not in k and "mlp0.weight" not in k)
    # the dead unit has exactly zero batch variance in every net, in the oracle's own evaluation
    block = R.canon_block(host, 2 * n_flows, G, 1)
    st = R.step64(block, 1, R.module_codes(n_flows), G, nf, R.inputs(seed, B, G), "direct", [None] * 3)["stats"]
    assert st.shape == (2 * n_flows, 2, 2 * nf)
    assert not st[:, :, nf - 1].any() and not st[:, :, 2 * nf - 1].any() and (st[:, 1, :nf - 1] > 0).all()
    ref = R.oracle64_train(seed, n_flows, nf, G, B, "direct", R.hostile_bn)
    assert all(np.isfinite(v).all() for v in ref["grads"].values())
    # the floor
    fl = R.make_state(seed, n_flows, nf, G, R.floor_active)
    for k in fl:
        if k.endswith("logvar_mlp1.bias"):
            assert fl[k][0] == -20 and (G < 6 or fl[k][2] == -14) and np.array_equal(fl[k][1::2], plain[k][1::2])
        else:
            assert np.array_equal(fl[k], plain[k])
    modes = MODES if n_flows <= 2 else ("direct",)
    for mode in modes:
        ref = R.oracle64_train(seed, n_flows, nf, G, B, mode, R.floor_active)
        assert ref["lvs"].min() < -13 and ref["lvs"].min() > np.log(GO.EPS) and np.isfinite(ref["gs"]).all()
        assert all(np.isfinite(v).all() for v in ref["grads"].values())
