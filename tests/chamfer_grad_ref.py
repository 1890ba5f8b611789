"""The deterministic Chamfer backward's contract (include/dpf_hip.h: dpf_nndistancegrad_det, dpf_chamfer_cd_backward) in numpy
float32: the direct term vectorised, then the scattered term with np.add.at -- ufunc.at is unbuffered and takes its operands one
after the other, so handing it the contributions in ascending query order IS the stated order.  Every intermediate is np.float32
(numpy rounds each operation separately: there is no contraction to switch off).  TEST INFRASTRUCTURE."""
import numpy as np

F = np.float32


def _one_output(xt, xq, idx_t, idx_q, gd_t, gd_q):
    """gradient of the `target` cloud xt (B,T,3): direct term from gd_t / idx_t, then the queries l = 0 .. Q-1 in ascending order"""
    B = xt.shape[0]
    two = F(2)
    g = np.empty_like(xt)
    for i in range(B):
        g[i] = (two * gd_t[i])[:, None] * (xt[i] - xq[i][idx_t[i]])                        # (2 gd_t[j]) (xt[j] - xq[idx_t[j]])
        contrib = -((two * gd_q[i])[:, None] * (xq[i] - xt[i][idx_q[i]]))                  # -((2 gd_q[l]) (xq[l] - xt[idx_q[l]]))
        assert g[i].dtype == F and contrib.dtype == F
        np.add.at(g[i], idx_q[i], contrib)                                                 # g[idx_q[l]] += contrib[l], l ascending
    return g


def nndistancegrad_det(xyz1, xyz2, idx1, idx2, gd1, gd2):
    """(B,n,3), (B,m,3), idx1 (B,n), idx2 (B,m), gd1 (B,n), gd2 (B,m) -> g1 (B,n,3), g2 (B,m,3), the defined result"""
    xyz1, xyz2 = np.ascontiguousarray(xyz1, F), np.ascontiguousarray(xyz2, F)
    gd1, gd2 = np.ascontiguousarray(gd1, F), np.ascontiguousarray(gd2, F)
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    return _one_output(xyz1, xyz2, idx1, idx2, gd1, gd2), _one_output(xyz2, xyz1, idx2, idx1, gd2, gd1)


def chamfer_cd_backward(xyz1, xyz2, idx1, idx2, grad_cd):
    """the same with gd1[i][j] = grad_cd[i] / (float)n and gd2[i][l] = grad_cd[i] / (float)m (fp32 divisions)"""
    grad_cd = np.ascontiguousarray(grad_cd, F)
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    gd1 = np.repeat((grad_cd / F(n))[:, None], n, axis=1)
    gd2 = np.repeat((grad_cd / F(m))[:, None], m, axis=1)
    assert gd1.dtype == F and gd2.dtype == F and gd1.shape == (b, n)
    return nndistancegrad_det(xyz1, xyz2, idx1, idx2, gd1, gd2)
