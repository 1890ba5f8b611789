"""float64 restatement of the SPARSE backward of the eval-mode PointNet encoder + max over the points, as csrc/encoder_frozen.hip
computes it: (b, f) with pooled[b, f] > 0 is a virtual point at x[b, :, arg[b, f]]; d z3 is one-hot; with the folded scale
s_l = gamma_l / sqrt(var_l + 1e-5)

    d a2 = g s3[f] W3[f, :]            d a_{l-1} = (s_l dz_l) W_l        dz_l = [a_l > 0] d a_l
    dbeta_l = sum dz_l                  dgamma_l = sum dz_l xhat_l,  xhat_l = (W_l a_{l-1} - mean_l) rstd_l
    dW_l = sum (s_l dz_l) a_{l-1}^T     dx[b, :, n] = sum over the features f with arg[b, f] = n of d x_v(b, f)

Checked against float64 autograd of the module and against a fixture of the reference's own module
(tests/test_encoder_frozen_cpu.py); the GPU tests (tests/test_gpu_encoder_frozen.py) use it with the kernel's own arg."""
import numpy as np
import torch

from oracle import encoder_oracle as EO

LAYERS = ("init_sd", "sd0", "sd1", "sd2")
EPS = 1e-5
TOL_OUT, TOL_GRAD = 1e-4, 5e-4           # the bars of tests/test_gpu_encoder_train.py
DX_SKIP_CAP = 0.10                       # bf16x3 dx: share of argmax points that may be left out (near-zero pre-activations)
GPU_SHAPES = ((1, 1), (2, 5), (2, 31), (3, 33), (2, 255), (1, 257), (5, 700))
EDGE_SHAPES = ((3, 33), (5, 700))


# seeds per (B, N, edge state), picked on the float64 reference alone so that the share of argmax points with a near-zero
# pre-activation (near_zero_points) stays under DX_SKIP_CAP; tests/test_encoder_frozen_cpu.py checks that without a GPU
SEEDS = {(1, 1, 0): 12, (2, 5, 0): 6, (2, 31, 0): 12, (3, 33, 0): 16, (2, 255, 0): 17, (1, 257, 0): 13, (5, 700, 0): 23,
         (3, 33, 1): 3, (5, 700, 1): 12}


def case_inputs(B, N, edge):
    """-> seed, numpy state, x (B,3,N) float32, g (B,512) float32 of a test case"""
    from oracle import detrng
    seed = SEEDS[(B, N, int(edge))]
    st = edge_state(seed) if edge else EO.make_encoder_state(seed)
    x = torch.from_numpy(EO.encoder_inputs(seed, B, N))
    g = torch.from_numpy(detrng.normal_f32(detrng.key(seed, "enc_r"), (B, 512)))
    return seed, st, x, g


def edge_state(seed):
    """The seeded state with, in EVERY layer, gamma < 0 on some features and gamma = 0 exactly on a few, and dead features in
    the last layer: beta so negative that no point's value is positive (pooled = 0)."""
    st = {k: np.array(v, copy=True) for k, v in EO.make_encoder_state(seed).items()}
    for name in LAYERS:
        g = st["features.%s_bn.weight" % name]
        g[1::5] *= -1.0
        g[3::16] = 0.0
    st["features.sd2_bn.bias"][2::9] = -50.0
    return st


def param_names():
    return ["features.%s%s.weight" % (n, suf) for n in LAYERS for suf in ("", "_bn")] + ["features.%s_bn.bias" % n for n in LAYERS]


def load_state(enc, st, dtype=torch.float64):
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}, strict=True)
    return enc.to(dtype).eval()


def _t(st, key):
    return torch.from_numpy(np.asarray(st[key])).to(torch.float64)


def sparse_backward(st, x, g, arg=None):
    """st: numpy state; x (B,3,N), g (B,512) float64 tensors; arg (B,512) integer tensor or None (then: the lowest point attaining
    the float64 maximum).  -> dict: pooled, arg, dx, grads {state key: gradient}, pre [z0, z1, z2] of the virtual points."""
    x, g = x.to(torch.float64), g.to(torch.float64)
    B, _, N = x.shape
    W = [_t(st, "features.%s.weight" % n)[0] for n in LAYERS]
    gam = [_t(st, "features.%s_bn.weight" % n) for n in LAYERS]
    bet = [_t(st, "features.%s_bn.bias" % n) for n in LAYERS]
    mean = [_t(st, "features.%s_bn.running_mean" % n) for n in LAYERS]
    rstd = [1.0 / torch.sqrt(_t(st, "features.%s_bn.running_var" % n) + EPS) for n in LAYERS]
    s = [gam[l] * rstd[l] for l in range(4)]

    def layer(l, a):                                      # a (..., cin) -> xhat, z
        xh = (a @ W[l].t() - mean[l]) * rstd[l]
        return xh, xh * gam[l] + bet[l]

    if arg is None:
        a = x.permute(0, 2, 1)                            # (B,N,3)
        for l in range(4):
            a = torch.relu(layer(l, a)[1])
        feat = a.permute(0, 2, 1)                         # (B,512,N)
        m = feat.max(dim=2, keepdim=True)[0]
        arg = (feat == m).to(torch.int64).argmax(dim=2)   # the first index attaining the maximum
    arg = arg.to(torch.int64)
    xv = torch.gather(x.unsqueeze(1).expand(B, 512, 3, N), 3, arg[:, :, None, None].expand(B, 512, 3, 1))[..., 0]   # (B,512,3)
    acts, xhs, pre = [xv], [], []
    for l in range(3):
        xh, z = layer(l, acts[-1])
        xhs.append(xh); pre.append(z); acts.append(torch.relu(z))
    a2 = acts[3]                                          # (B,512,256)
    xh3 = ((a2 * W[3][None]).sum(-1) - mean[3]) * rstd[3] # (B,512): feature f of virtual point (b, f)
    pooled = torch.relu(xh3 * gam[3] + bet[3])
    dz3 = torch.where(pooled > 0, g, torch.zeros_like(g))
    grads = {}
    grads["features.sd2_bn.bias"] = dz3.sum(0)
    grads["features.sd2_bn.weight"] = (dz3 * xh3).sum(0)
    grads["features.sd2.weight"] = (s[3][:, None] * (dz3[:, :, None] * a2).sum(0))[None]
    da = dz3[:, :, None] * s[3][None, :, None] * W[3][None]                 # (B,512,256)
    for l in (2, 1, 0):
        dz = torch.where(acts[l + 1] > 0, da, torch.zeros_like(da))
        name = LAYERS[l]
        grads["features.%s_bn.bias" % name] = dz.sum((0, 1))
        grads["features.%s_bn.weight" % name] = (dz * xhs[l]).sum((0, 1))
        u = dz * s[l]
        grads["features.%s.weight" % name] = torch.einsum("bvo,bvi->oi", u, acts[l])[None]
        da = u @ W[l]
    dx = torch.zeros_like(x)
    for b in range(B):
        dx[b].index_add_(1, arg[b], da[b].t().contiguous())
    return {"pooled": pooled, "arg": arg, "dx": dx, "grads": grads, "pre": pre}


def autograd_reference(enc64, x, g, arg=None):
    """float64 autograd of the module in eval(): pooled by gather at `arg` (or the module's own max), dx, {name: gradient}"""
    for p in enc64.parameters():
        p.grad = None
    xin = x.detach().to(torch.float64).clone().requires_grad_(True)
    feat = enc64.forward_torch(xin) if hasattr(enc64, "forward_torch") else enc64(xin)
    pooled = feat.max(dim=2)[0] if arg is None else torch.gather(feat, 2, arg.to(torch.int64)[:, :, None])[..., 0]
    (pooled * g.to(torch.float64)).sum().backward()
    return pooled.detach(), xin.grad, {k: p.grad.clone() for k, p in enc64.named_parameters()}


def near_zero_points(pre, arg, live):
    """(B,512) bool: virtual point (b, f) has one of its 448 pre-activations within TOL_OUT of zero, relative to its layer's largest
    magnitude; spread to every live feature sharing its point -> the argmax POINTS that may be left out of a bf16x3 dx comparison.
    -> (set of (b, n) that may be left out, set of all live (b, n))"""
    near = torch.zeros(arg.shape, dtype=torch.bool)
    for z in pre:
        near |= (z.abs() <= TOL_OUT * z.abs().max()).any(-1)
    skip, pts = set(), set()
    for b, f in zip(*torch.nonzero(live, as_tuple=True)):
        key = (int(b), int(arg[b, f]))
        pts.add(key)
        if near[b, f]:
            skip.add(key)
    return skip, pts


def projection(grad, key, seed):
    """oracle.gen_golden._grad_projection of one gradient"""
    from oracle import detrng
    v = np.asarray(grad.detach().cpu().numpy(), dtype=np.float64).ravel()
    r = detrng.normal(detrng.key(seed, "proj:" + key), v.size)
    return np.array([v.sum(), float(v @ r), float(np.abs(v).sum())])
