"""tests/loss_refs.py checked before anything is measured against it: every float64 reference against torch.autograd in
float64 on the gather / broadcast formulation of the same loss, at small ragged shapes; the error-bound quantities
(sums of absolute terms, counts) against explicit loops; chamfer_grad_ref against the fp32 C restatement
oracle.structural.nndistancegrad within that oracle's own rounding."""
import math

import numpy as np
import pytest
import torch

from oracle import detrng
from oracle import structural as S
from tests.loss_refs import cd_ref, chamfer_grad_ref, fscore_ref, nll_ref

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


def _chamfer_case(seed, b, n, m, hot=False):
    x1 = detrng.normal_f32(seed, (b, n, 3))
    x2 = detrng.normal_f32(seed + 1, (b, m, 3), 0.1, 0.8)
    gd1 = detrng.normal_f32(seed + 2, (b, n))
    gd2 = detrng.normal_f32(seed + 3, (b, m))
    if hot:
        idx1 = np.full((b, n), m - 1, np.int32)
        idx2 = np.full((b, m), 0, np.int32)
    else:
        idx1 = np.minimum((detrng.uniform(seed + 4, b * n) * m).astype(np.int32), m - 1).reshape(b, n)
        idx2 = np.minimum((detrng.uniform(seed + 5, b * m) * n).astype(np.int32), n - 1).reshape(b, m)
    return x1, x2, idx1, idx2, gd1, gd2


CHAMFER_SHAPES = [(2, 7, 3, False), (3, 57, 30, False), (1, 1, 1, False), (2, 1, 50, False), (2, 50, 1, False), (2, 33, 33, True)]


@pytest.mark.parametrize("b,n,m,hot", CHAMFER_SHAPES)
def test_chamfer_grad_ref_is_the_autograd_gradient_of_the_gathered_loss(b, n, m, hot):
    x1, x2, idx1, idx2, gd1, gd2 = _chamfer_case(11 + n, b, n, m, hot)
    t1 = torch.from_numpy(x1).double().requires_grad_(True)
    t2 = torch.from_numpy(x2).double().requires_grad_(True)
    i1 = torch.from_numpy(idx1).long()[:, :, None].expand(b, n, 3)
    i2 = torch.from_numpy(idx2).long()[:, :, None].expand(b, m, 3)
    d1 = (t1 - torch.gather(t2, 1, i1)).square().sum(2)            # the distance to the chosen neighbour, nndistance.cu:139-145
    d2 = (t2 - torch.gather(t1, 1, i2)).square().sum(2)
    ((d1 * torch.from_numpy(gd1).double()).sum() + (d2 * torch.from_numpy(gd2).double()).sum()).backward()
    g1, g2, a1, a2, k1, k2 = chamfer_grad_ref(x1, x2, idx1, idx2, gd1, gd2)
    assert np.all(np.abs(g1 - t1.grad.numpy()) <= 1e-13 * a1 + 1e-300)
    assert np.all(np.abs(g2 - t2.grad.numpy()) <= 1e-13 * a2 + 1e-300)
    # the bound's quantities, by explicit loops
    ea1, ea2 = np.zeros((b, n, 3)), np.zeros((b, m, 3))
    ek1, ek2 = np.zeros((b, n), np.int64), np.zeros((b, m), np.int64)
    for i in range(b):
        for j in range(n):
            t = np.abs(2.0 * float(gd1[i, j]) * (x1[i, j].astype(np.float64) - x2[i, idx1[i, j]].astype(np.float64)))
            ea1[i, j] += t; ea2[i, idx1[i, j]] += t; ek2[i, idx1[i, j]] += 1
        for j in range(m):
            t = np.abs(2.0 * float(gd2[i, j]) * (x2[i, j].astype(np.float64) - x1[i, idx2[i, j]].astype(np.float64)))
            ea2[i, j] += t; ea1[i, idx2[i, j]] += t; ek1[i, idx2[i, j]] += 1
    np.testing.assert_allclose(a1, ea1, rtol=1e-13, atol=0)
    np.testing.assert_allclose(a2, ea2, rtol=1e-13, atol=0)
    assert np.array_equal(k1, ek1) and np.array_equal(k2, ek2)
    assert int(k1.sum()) == b * m and int(k2.sum()) == b * n


@pytest.mark.parametrize("b,n,m,hot", CHAMFER_SHAPES)
def test_chamfer_grad_ref_vs_the_fp32_oracle(b, n, m, hot):
    """The oracle forms each term in fp32 (two roundings: the difference, the product; the factor 2 is exact), adds them in
    double and rounds the sum to fp32 once: |oracle - ref| <= 2 u sum|term| (1 + u) + u |ref|."""
    x1, x2, idx1, idx2, gd1, gd2 = _chamfer_case(23 + m, b, n, m, hot)
    o1, o2 = S.nndistancegrad(x1, x2, idx1, idx2, gd1, gd2)
    g1, g2, a1, a2, _, _ = chamfer_grad_ref(x1, x2, idx1, idx2, gd1, gd2)
    assert np.all(np.abs(o1 - g1) <= 2 * U * (1 + U) * a1 + U * np.abs(g1) + TINY)
    assert np.all(np.abs(o2 - g2) <= 2 * U * (1 + U) * a2 + U * np.abs(g2) + TINY)
    assert np.abs(o1 - g1).max() > 0 or n * m == 1                # (a float64 reference, not the oracle again)


def _nll_forms(seed, B, C, N):
    """mu0 / lv0 as numpy views of the stride forms the C entry point accepts."""
    r = lambda k, shape, lo, hi: detrng.uniform(detrng.key(seed, k), int(np.prod(shape)), lo, hi).astype(np.float32).reshape(shape)
    return {
        "1c1": lambda k, lo, hi: np.broadcast_to(r(k, (1, C, 1), lo, hi), (B, C, N)),
        "bc1": lambda k, lo, hi: np.broadcast_to(r(k, (B, C, 1), lo, hi), (B, C, N)),
        "dense": lambda k, lo, hi: r(k, (B, C, N), lo, hi),
        "bnc_t": lambda k, lo, hi: r(k, (B, N, C), lo, hi).transpose(0, 2, 1),
    }


@pytest.mark.parametrize("B,C,N,mu_form,lv_form,with_sum,grad_out", [
    (1, 3, 1, "dense", "dense", True, 1.0), (5, 3, 77, "1c1", "bc1", True, 1.0), (3, 5, 41, "bc1", "bnc_t", True, -0.37),
    (4, 1, 30, "bnc_t", "1c1", False, -0.37), (2, 3, 19, "dense", "dense", False, 1.0)])
def test_nll_ref_is_the_autograd_gradient_of_the_broadcast_loss(B, C, N, mu_form, lv_form, with_sum, grad_out):
    forms = _nll_forms(5, B, C, N)
    s0 = detrng.normal_f32(6, (B, C, N), 0.0, 0.5)
    mu0, lv0 = forms[mu_form]("mu", -0.5, 0.5), forms[lv_form]("lv", -6.0, 1.0)
    sl = detrng.normal_f32(7, (B, C, N), 0.0, 2.0) if with_sum else None
    leaves = [torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True)
              for v in (s0, np.zeros_like(s0) if sl is None else sl, mu0, lv0)]
    ts, tl, tm, tv = leaves
    out = 0.5 * ((tl + tv + (ts - tm) ** 2 / torch.exp(tv)).sum() / B + math.log(2.0 * math.pi) * C * N)
    out.backward(torch.tensor(grad_out, dtype=torch.float64))
    value, sum_abs, grads = nll_ref(s0, mu0, lv0, sl, B, grad_out)
    assert abs(value - float(out.detach())) <= 1e-13 * (sum_abs / B + abs(value))
    for got, leaf in zip(grads, leaves):
        assert got.shape == (B, C, N)
        np.testing.assert_allclose(got, leaf.grad.numpy(), rtol=1e-12, atol=1e-300)
    d = s0.astype(np.float64) - mu0.astype(np.float64)
    want_abs = sum(abs(float(x)) for x in (np.zeros(1) if sl is None else sl).ravel()) + float(np.abs(lv0.astype(np.float64)).sum()) \
        + float((d * d * np.exp(-lv0.astype(np.float64))).sum())
    assert abs(sum_abs - want_abs) <= 1e-12 * want_abs
    # a base distribution that is a learned per-cloud vector receives the full gradient summed over what it was expanded along
    if lv_form == "bc1":
        small = torch.from_numpy(np.array(lv0[:, :, :1])).double().requires_grad_(True)
        o2 = 0.5 * ((tl.detach() + small.expand(B, C, N) + (ts.detach() - tm.detach()) ** 2 / torch.exp(small.expand(B, C, N))).sum() / B)
        o2.backward(torch.tensor(grad_out, dtype=torch.float64))
        np.testing.assert_allclose(grads[3].sum(axis=2, keepdims=True), small.grad.numpy(), rtol=1e-11, atol=1e-300)


def test_fscore_ref_and_cd_ref_vs_torch_float64():
    t = np.float32(0.001)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))
    for (b, n, m) in ((3, 1, 1), (4, 7, 13), (2, 255, 257)):
        d1 = detrng.uniform_f32(31 + n, (b, n), 0.0, 0.002)
        d2 = detrng.uniform_f32(32 + m, (b, m), 0.0, 0.002)
        d1[0, 0], d2[0, 0] = t, below                              # exactly at the threshold: not a hit
        if n > 4:
            d1[1, :5] = (above, below, np.nan, np.inf, 0.0)
        f, r, p = fscore_ref(d1, d2, t)
        t1, t2 = torch.from_numpy(d1), torch.from_numpy(d2)
        prec = 100.0 * (t2 < float(t)).double().mean(1)            # utils.py:38-42 (float(t) is the float32 value, exactly)
        rec = 100.0 * (t1 < float(t)).double().mean(1)
        np.testing.assert_allclose(f, (2 * prec * rec / (prec + rec + 1e-7)).numpy(), rtol=1e-14, atol=0)
        assert np.array_equal(r, (t1 < float(t)).sum(1).numpy()) and np.array_equal(p, (t2 < float(t)).sum(1).numpy())
        assert not np.isnan(f).any()
        ok1, ok2 = np.nan_to_num(d1, nan=1.0, posinf=1.0), np.nan_to_num(d2, nan=1.0, posinf=1.0)
        cd, a1, a2 = cd_ref(ok1, ok2)
        want = torch.from_numpy(ok1).double().mean(1) + torch.from_numpy(ok2).double().mean(1)   # evaluating.py:112
        np.testing.assert_allclose(cd, want.numpy(), rtol=1e-14, atol=0)
        np.testing.assert_allclose(a1, ok1.astype(np.float64).sum(1), rtol=1e-14)
        np.testing.assert_allclose(a2, ok2.astype(np.float64).sum(1), rtol=1e-14)
    # no hits on a side: 0, never NaN; the threshold itself is not a hit, its lower neighbour is
    z = np.full((1, 4), t, np.float32)
    assert fscore_ref(z, z, t)[0][0] == 0.0
    assert fscore_ref(z, np.full((1, 4), below, np.float32), t)[0][0] == 0.0
    h = np.full((1, 4), below, np.float32)
    assert abs(fscore_ref(h, h, t)[0][0] - 100.0) < 1e-6
