"""Host parts of the occupancy-grid JSD (lib/metrics/evaluation_metrics.py:203-321) as mirrored by
dpf_nets_amd.metrics.evaluation_metrics, against vectors captured from the reference's own functions
(tools/gen_golden_occupancy.py -> tests/golden/occupancy_jsd.npz).  The binning itself runs on the device
(tests/test_gpu_occupancy.py)."""
import os
import warnings

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occupancy_jsd.npz")
NAMES = ("unit_cube_grid_point_cloud", "jsd_between_point_cloud_sets", "entropy_of_occupancy_grid", "jensen_shannon_divergence",
         "_jsdiv")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def EM():
    from dpf_nets_amd.metrics import evaluation_metrics
    return evaluation_metrics


def counters(gold, tag, res, sph):
    key = "%s/%d/%d" % (tag, res, sph)
    out = np.zeros(len(gold["grid/%d/%d" % (res, sph)].reshape(-1, 3)))
    out[gold["counters_idx/" + key]] = gold["counters_val/" + key]
    return out


def test_the_five_names_import_from_the_mirror(EM):
    for name in NAMES:
        assert callable(getattr(EM, name)), name


def test_no_scikit_learn_import_in_the_package():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpf_nets_amd")
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(d, f)).read()
                assert "import sklearn" not in text and "from sklearn" not in text, os.path.join(d, f)


@pytest.mark.parametrize("res", [8, 28])
@pytest.mark.parametrize("sph", [False, True])
def test_unit_cube_grid_is_bit_equal_to_the_reference(gold, EM, res, sph):
    grid, spacing = EM.unit_cube_grid_point_cloud(res, sph)
    ref = gold["grid/%d/%d" % (res, sph)]
    assert grid.dtype == np.float32 and grid.shape == ref.shape
    assert grid.tobytes() == ref.tobytes()
    assert spacing == float(gold["spacing/%d" % res])


def test_the_golden_inputs_have_no_near_ties(gold):
    """the generator's condition on the inputs: scikit-learn's choice on a tie is unspecified"""
    assert float(gold["min_gap"]) >= 1e-7


@pytest.mark.parametrize("res", [8, 28])
def test_jsd_of_the_golden_counters(gold, EM, res):
    P, Q = counters(gold, "sample", res, True), counters(gold, "ref", res, True)
    want = float(gold["jsd/%d" % res])
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the two methods agree: no cross-check warning
        assert abs(EM.jensen_shannon_divergence(P, Q) - want) <= 1e-12
    assert abs(EM._jsdiv(P, Q) - want) <= 1e-12
    assert abs(EM.jensen_shannon_divergence(P, P)) <= 1e-12


def test_jsd_argument_checks(EM):
    with pytest.raises(ValueError):
        EM.jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError):
        EM.jensen_shannon_divergence(np.array([1.0, 1.0]), np.array([1.0, 1.0, 1.0]))
