"""knn, lgan_mmd_cov and compute_all_metrics (lib/metrics/evaluation_metrics.py:125-200) as mirrored by
dpf_nets_amd.metrics.evaluation_metrics, against values the reference's own functions returned on the same fixed matrices
(tools/gen_golden_eval_all_metrics.py -> tests/golden/eval_all_metrics.npz).  compute_all_metrics is fed the fixture matrices
by replacing the module's matrix functions, as the generator replaced the reference's _pairwise_EMD_CD_: the same float32
operations on the same inputs, so every value must be EQUAL.  The cases hold tied distances (duplicated rows and columns,
small-integer matrices) and N_sample != N_ref."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_all_metrics.npz")
CASES = (("a", 12, 10), ("b", 16, 16), ("c", 7, 19), ("d", 9, 9))
KNN_KEYS = ("tp", "fp", "fn", "tn", "precision", "recall", "acc_t", "acc_f", "acc")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def E():
    from dpf_nets_amd.metrics import evaluation_metrics
    return evaluation_metrics


def _fixture(gold, tag):
    return {k: torch.from_numpy(gold["%s/%s" % (tag, k)]) for k in ("rs_cd", "rr_cd", "ss_cd", "rs_emd", "rr_emd", "ss_emd")}


def _equal(got, want, what):
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.dim() == 0, what
    assert np.array_equal(got.numpy(), want), (what, float(got), float(want))


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_knn_vs_reference_golden(gold, E, tag):
    fx = _fixture(gold, tag)
    for k, sq in ((1, False), (3, False), (2, True)):
        got = E.knn(fx["rr_emd"], fx["rs_emd"], fx["ss_emd"], k, sqrt=sq)
        assert tuple(got.keys()) == KNN_KEYS
        for key in KNN_KEYS:
            _equal(got[key], gold["%s/knn%d%s/%s" % (tag, k, "_sqrt" if sq else "", key)], (tag, k, sq, key))


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_lgan_mmd_cov_vs_reference_golden(gold, E, tag):
    got = E.lgan_mmd_cov(_fixture(gold, tag)["rs_emd"].t())
    assert tuple(got.keys()) == ("lgan_mmd", "lgan_cov", "lgan_mmd_smp")
    for key, v in got.items():
        _equal(v, gold["%s/lgan/%s" % (tag, key)], (tag, key))


@pytest.mark.parametrize("tag,ns,nr", CASES)
def test_compute_all_metrics_vs_reference_golden(gold, E, monkeypatch, tag, ns, nr):
    fx = _fixture(gold, tag)
    sample, ref = torch.zeros(ns, 4, 3), torch.zeros(nr, 4, 3)
    lookup = {(id(ref), id(sample)): "rs", (id(ref), id(ref)): "rr", (id(sample), id(sample)): "ss"}
    calls = []

    def matrices(metric):
        def fn(a, b, bs=None, shard_rows=False):
            which = lookup[(id(a), id(b))]                 # (a KeyError here: a matrix in the wrong orientation)
            calls.append((metric, which, bs))
            return fx[which + "_" + metric]
        return fn

    monkeypatch.setattr(E, "pairwise_CD", matrices("cd"))
    monkeypatch.setattr(E, "pairwise_EMD", matrices("emd"))
    got = E.compute_all_metrics(sample, ref, 5, accelerated_cd=True)
    assert list(got.keys()) == [str(k) for k in gold[tag + "/all_keys"]]
    for key, v in got.items():
        _equal(v, gold["%s/all/%s" % (tag, key)], (tag, key))
    assert sorted(calls) == sorted((m, w, 5) for m in ("cd", "emd") for w in ("rs", "rr", "ss"))


def test_knn_one_nn_accuracy_by_hand(E):
    """Two well separated sets: every cloud's nearest other cloud is in its own set -> 1-NN accuracy 1 (a two-sample test that
    can tell the sets apart); one set against a copy of itself -> the nearest neighbour is always the copy -> accuracy 0."""
    x = torch.tensor([[0.0], [0.1], [0.2]])
    y = torch.tensor([[5.0], [5.1]])
    d = lambda a, b: (a - b.t()).abs()                              # noqa: E731
    res = E.knn(d(x, x), d(x, y), d(y, y), 1)
    assert float(res["acc"]) == 1.0 and float(res["tp"]) == 3.0 and float(res["tn"]) == 2.0
    res = E.knn(d(x, x), d(x, x) * 0.5, d(x, x), 1)
    assert float(res["acc"]) == 0.0
