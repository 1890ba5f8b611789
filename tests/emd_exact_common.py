"""What tests/test_gpu_emd_exact.py and tests/test_gpu_emd_exact_edges.py share: the batches of the case list, the launch through
emd_exact_full, the bit comparison and the assertions of one solved pair against the numpy oracle (tests/emd_exact_ref.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import emd_exact_ref as R                                                                   # noqa: E402

K_CAP = 1.25                                    # grid steps per point (tests/test_emd_exact_ref_cpu.py)


def dev():
    return torch.device("cuda", 0)


def U():
    from dpf_nets_amd.networks import utils
    return utils


def clouds(kind, n, B=3):
    cases = [R.make_case(kind, n, 100 * n + k) for k in range(B)]
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases]


def run(a, b, **kw):
    """numpy (B, n, 3) pair -> numpy cost, assignment, qcost, status"""
    out = U().emd_exact_full(torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev()), **kw)
    return tuple(t.detach().cpu().numpy() for t in out)


def same_bits(x, y):
    def raw(v):
        return np.ascontiguousarray(np.atleast_1d(np.asarray(v))).view(np.uint8)
    return all(np.array_equal(raw(p), raw(q)) for p, q in zip(x, y))


def check_pair(a, b, o, cost, asg, qcost, status, tag):
    """assertions 1-5 of one solved pair; o = R.solve(a, b, bits) carries the grid (s, c) of the bits in use"""
    n = a.shape[0]
    c64 = R.cost64(a, b, asg)
    q = 1.0 / float(o["s"]) if o["s"] else 0.0
    print(tag, "status", status, "oracle rounds", o["rounds"], "qcost", qcost, o["qcost"], "cost", cost, c64,
          "rel", abs(float(cost) - c64) / max(c64, 1e-300), "K", (c64 - R.cost64(a, b, o["assignment"])) / (n * q) if q else 0.0)
    assert status >= 0, tag
    assert sorted(asg.tolist()) == list(range(n)), tag                                     # 1
    assert int(qcost) == o["qcost"], tag                                                    # 2
    assert int(qcost) == int(o["c"][np.arange(n), asg].sum()), tag                          # 3
    assert abs(float(cost) - c64) <= (n + 8) * 2.0 ** -24 * c64, tag                        # 4
    assert c64 <= R.cost64(a, b, o["assignment"]) + K_CAP * n * q, tag                      # 5
    # the tie rules fix the outcome: the oracle's matching and its number of rounds
    assert np.array_equal(asg, o["assignment"]) and int(status) == o["rounds"], tag
