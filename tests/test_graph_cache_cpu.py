"""csrc/graph_cache.h keys a training call by what its `fill` lambda adds.  A parameter the fill forgets is invisible to every
parity test (the eager and the recording call are right; the replay reads or writes another call's buffer), so the six
fills are read here against their C signatures, and against tests/graph_cases.py, whose argument list drives the GPU cases
of tests/test_gpu_graph_cache.py: a parameter added to an entry fails here until it is in the fill AND has a role there."""
import re

import pytest

from tests import graph_cases as GC


@pytest.mark.parametrize("entry", list(GC.ENTRIES))
def test_fill_names_every_parameter_and_graph_cases_lists_it(entry):
    params, fill = GC.signature_and_fill(entry)
    assert params[-1] == "stream", (entry, params)
    params = params[:-1]
    listed = [n for n, _ in GC.ENTRIES[entry][1]]
    for name in params:
        assert re.search(r"\b%s\b" % name, fill), "%s: parameter `%s` is not named in the fill of its graph key" % (entry, name)
        assert name in listed, "%s: parameter `%s` is not listed in tests/graph_cases.py" % (entry, name)
    for name in listed:
        assert name in params, "%s: tests/graph_cases.py lists `%s`, which the signature lacks" % (entry, name)
    assert listed == params, "%s: tests/graph_cases.py lists the parameters in another order than the signature" % entry


def test_every_listed_argument_reaches_a_gpu_case():
    """device pointers -> `one pointer moves`; host arrays -> the host-table cases; scalars -> a second value, or a reason"""
    roles = {GC.SCALAR, GC.HOST, GC.IN, GC.OUT, GC.INOUT, GC.SCRATCH}
    for entry, name, role in GC.ARGUMENTS:
        assert role in roles, (entry, name, role)
    assert len(GC.DEVICE_POINTERS) + len(GC.HOST_TABLES) + len(GC.SCALARS) == len(GC.ARGUMENTS)
    for entry, name in GC.SCALARS:
        kwargs = GC.BASE[GC.family(entry)]
        assert name in kwargs, (entry, name)
        second = GC.second_value(entry, name, kwargs)
        assert second is not None or (entry, name) in GC.NO_SECOND_VALUE, (entry, name)
        assert second is None or second[name] != kwargs[name], (entry, name)
    assert {n for _, n in GC.HOST_TABLES} == {"meta_host", "g_ps", "g_mus", "g_lvs", "running"}


def test_the_reader_sees_a_missing_name():
    """the guard itself: a fill without `dp_tmp` is reported"""
    params, fill = GC.signature_and_fill("dpf_flow_train_backward")
    assert "dp_tmp" in params
    cut = re.sub(r"\bdp_tmp\b,?", "", fill)
    assert not re.search(r"\bdp_tmp\b", cut) and re.search(r"\bdp_in\b", cut)
