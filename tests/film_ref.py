"""References, cases and bars of the FiLM conditioner kernel tests (csrc/film_train.hip: tests/test_gpu_film_edges.py on the GPU,
pinned without one by tests/test_film_ref_cpu.py).  Plain torch, device- and dtype-agnostic: with torch.float64 the functions below
are the reference, with torch.float32 they are the project's fp32 tensor-op formulation (train_engine / frozen_engine), whose own
error against float64 on the same inputs is the yardstick `r32`.

The formulation is the one in the header of film_train.hip, per sub-net k of K:
    u = g W0^T ; xhat = (u - mean) * rstd ; y = gamma * xhat + beta ; fm = swish(y) W1^T + b1
training: mean / biased variance over the B clouds, rstd = rsqrt(var + eps); frozen: the running statistics, constants."""
import torch

F = 64
EPS = 1e-5
MODES = ("train", "frozen")

# ---- the cases: (K, B, G) ----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 4),                        # one sub-net, the smallest legal batch and width
          (3, 3, 132),                      # a full 128-column tile plus a 4-column tail
          (5, 4, 68),                       # one cloud per group; a 4-column second block in the d g pass
          (2, 16, 128), (2, 17, 260),       # the 16|17 NB dispatch edge
          (2, 32, 64), (2, 33, 36),         # the 32|33 NB dispatch edge
          (9, 63, 196),                     # K = 9 (the eight-at-a-time sum's tail of one), B = 63, ragged G
          (2, 64, 516),                     # the largest LDS carve-out, four tiles plus a tail
          (3, 5, 128)]                      # a small batch at the production width
FROZEN_ONLY = [(1, 1, 4), (7, 1, 128), (8, 4, 36), (17, 3, 68), (252, 1, 4)]          # the eight-at-a-time sum and the ticket
VARIANT_SHAPES = [(5, 4, 68), (2, 17, 260), (9, 63, 196), (2, 64, 516)]              # hostile and scaled, both modes
OFFSET_SHAPES = [(2, 16, 128), (2, 33, 36), (2, 64, 516)]                            # g + 50, training only
OFFSET = 50.0


def cases(mode):
    """Every (K, B, G, variant, offset) of `mode`."""
    out = [s + ("seeded", 0.0) for s in SHAPES + (FROZEN_ONLY if mode == "frozen" else [])]
    out += [s + (v, 0.0) for v in ("hostile", "scaled") for s in VARIANT_SHAPES]
    if mode == "train":
        out += [s + ("seeded", OFFSET) for s in OFFSET_SHAPES]
    return out


def case_id(mode, K, B, G, variant, offset):
    return "%s-%s%s(%d,%d,%d)" % (mode, variant, "+%g" % offset if offset else "", K, B, G)


# ---- the bars ----------------------------------------------------------------------------------------------------------------------
# kind of each compared tensor
KIND = dict(fm="fwd", xhat="fwd", rstd="stat", mean="stat", uvar="stat",
            dW0="bwd", dgam="bwd", dbet="bwd", dW1="bwd", db1="bwd", dg_part="bwd", dg="bwd")
# Class A (seeded, no offset; training B >= 4, frozen any B): the bars of tests/test_gpu_film_train.py and of
# test_film_frozen_entries_vs_tensor_ops, now per sub-net.  test_film_ref_cpu.py holds the fp32 formulation to a quarter of BARS below.
CLASS_A_BARS = {"train": {"fwd": 2e-5, "stat": 1e-5, "bwd": 5e-5}, "frozen": {"fwd": 1e-5, "stat": 1e-5, "bwd": 2e-5}}
# BARS, what class A is held to: where the kernels measured 10 x or more under a bar of CLASS_A_BARS on an MI355X (everywhere), 16 x
# the worst class A r32 measured there, rounded up to one digit -- if that is tighter.  It is for the training backward (r32 1.2e-6:
# 5e-5 -> 2e-5) and the frozen rstd (r32 5.6e-8: 1e-5 -> 9e-7); the other four stay (16 r32 = 1.4e-5 -> 2e-5, 9.8e-6 -> 1e-5,
# 1.2e-5 > 1e-5, 2.4e-5 > 2e-5).  The measured table is in tests/test_gpu_film_edges.py.
BARS = {"train": {"fwd": 2e-5, "stat": 1e-5, "bwd": 2e-5}, "frozen": {"fwd": 1e-5, "stat": 9e-7, "bwd": 2e-5}}
R32_FACTOR = 8                              # another summation order on a cancelling sum (tests/test_gpu_gprior_train.py)
# Class B, the ONLY cases held to max(class A bar, R32_FACTOR * r32): training at B < 4, hostile, scaled, offset.  Ill-conditioned for
# ANY fp32 evaluation once the error is taken per sub-net (fp32 tensor ops on the CPU: up to 1e-5 on dg_part in hostile and scaled --
# cancellation over the 64 features --, up to 4e-4 on dW0 with offset inputs).
CLASS_B = (
    ("train", 1, 2, 4, "seeded", 0.0), ("train", 3, 3, 132, "seeded", 0.0),
    ("train", 5, 4, 68, "hostile", 0.0), ("train", 2, 17, 260, "hostile", 0.0), ("train", 9, 63, 196, "hostile", 0.0), ("train", 2, 64, 516, "hostile", 0.0),
    ("train", 5, 4, 68, "scaled", 0.0), ("train", 2, 17, 260, "scaled", 0.0), ("train", 9, 63, 196, "scaled", 0.0), ("train", 2, 64, 516, "scaled", 0.0),
    ("train", 2, 16, 128, "seeded", 50.0), ("train", 2, 33, 36, "seeded", 50.0), ("train", 2, 64, 516, "seeded", 50.0),
    ("frozen", 5, 4, 68, "hostile", 0.0), ("frozen", 2, 17, 260, "hostile", 0.0), ("frozen", 9, 63, 196, "hostile", 0.0), ("frozen", 2, 64, 516, "hostile", 0.0),
    ("frozen", 5, 4, 68, "scaled", 0.0), ("frozen", 2, 17, 260, "scaled", 0.0), ("frozen", 9, 63, 196, "scaled", 0.0), ("frozen", 2, 64, 516, "scaled", 0.0),
)


def is_class_b(mode, K, B, G, variant, offset):
    """By the rule; the tests assert that it names exactly the cases of CLASS_B."""
    return variant != "seeded" or offset != 0.0 or (mode == "train" and B < 4)


def bar_for(bars, mode, K, B, G, variant, offset, name, r32):
    """The bar of tensor `name` in one case: the class A bar of its kind (`bars`: BARS), or for a case of
    CLASS_B max(that, R32_FACTOR * r32)."""
    a = bars[mode][KIND[name]]
    return max(a, R32_FACTOR * r32) if (mode, K, B, G, variant, float(offset)) in CLASS_B else a


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def case_seed(K, B, G):
    return K * 1000 + B * 10 + G


def make_case(K, B, G, seed, variant, offset=0.0):
    """fp32 CPU tensors g (B,G), W0 (K,F,G), gam, bet (K,F), W1 (K,F,F), b1 (K,F), dfm (K,B,F), and for the frozen kernels the
    running statistics rm, rv (K,F).
      seeded   the distributions of tests/test_gpu_film_train.py (running statistics: test_film_frozen_entries_vs_tensor_ops)
      hostile  per sub-net: every fourth BatchNorm scale negative, scale 1 zero, feature 2 dead (W0 row zero: zero batch variance,
               rstd = eps^-1/2, xhat exactly 0 in training), beta -30 / +30 on features 3 / 5 (Swish saturated either way), scale 7
               times 40 (|y| past 88, where expf(-y) overflows, for part of the batch)
      scaled   sub-net k's W0 times 2^(-10 + 20 k / (K - 1)), its dfm times 2^(8 - 16 k / (K - 1))
    offset is added to g: batch means far above the spread."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, G, generator=gen) + offset
    W0 = torch.randn(K, F, G, generator=gen) / G ** 0.5
    gam = 1.0 + 0.2 * torch.randn(K, F, generator=gen)
    bet = 0.3 * torch.randn(K, F, generator=gen)
    W1 = torch.randn(K, F, F, generator=gen) / 8.0
    b1 = 0.1 * torch.randn(K, F, generator=gen)
    dfm = torch.randn(K, B, F, generator=gen)
    rm = 0.1 * torch.randn(K, F, generator=gen)
    rv = 0.5 + torch.rand(K, F, generator=gen)
    if variant == "hostile":
        gam[:, 0::4] *= -1
        gam[:, 1] = 0
        W0[:, 2] = 0
        bet[:, 3] = -30
        bet[:, 5] = 30
        gam[:, 7] *= 40
    elif variant == "scaled":
        k = torch.arange(K, dtype=torch.float64) / max(K - 1, 1)
        W0 *= torch.pow(2.0, -10 + 20 * k).float().view(K, 1, 1)
        dfm *= torch.pow(2.0, 8 - 16 * k).float().view(K, 1, 1)
    else:
        assert variant == "seeded", variant
    return dict(g=g, W0=W0, gam=gam, bet=bet, W1=W1, b1=b1, dfm=dfm, rm=rm, rv=rv)


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _film(dtype, g, W0, gam, bet, W1, b1, dfm, eps, stats):
    g, W0, gam, bet, W1, b1 = (t.detach().to(dtype).clone().requires_grad_(True) for t in (g, W0, gam, bet, W1, b1))
    dfm = dfm.detach().to(dtype)
    B = g.shape[0]
    u = torch.matmul(g.unsqueeze(0), W0.transpose(1, 2))                        # (K, B, F)
    u.retain_grad()
    out = {}
    if stats is None:
        var, mean = torch.var_mean(u, dim=1, unbiased=False, keepdim=True)
        out["mean"], out["uvar"] = mean.detach().squeeze(1), var.detach().squeeze(1) * (B / (B - 1.0))
    else:
        mean, var = (t.detach().to(dtype).unsqueeze(1) for t in stats)
    rstd = torch.rsqrt(var + eps)
    xhat = (u - mean) * rstd
    y = xhat * gam.unsqueeze(1) + bet.unsqueeze(1)
    fm = torch.baddbmm(b1.unsqueeze(1), y * torch.sigmoid(y), W1.transpose(1, 2))
    (fm * dfm).sum().backward()
    dg_part = torch.bmm(u.grad, W0.detach())                                    # (K, B, G): sub-net k's share of d g
    out.update(fm=fm.detach(), xhat=xhat.detach(), rstd=rstd.detach().squeeze(1), y=y.detach(), dW0=W0.grad, dgam=gam.grad,
               dbet=bet.grad, dW1=W1.grad, db1=b1.grad, dg_part=dg_part, dg=g.grad)
    return out


def film_train_ref(dtype, g, W0, gam, bet, W1, b1, dfm, eps):
    """Training mode in `dtype`: fm, xhat (K,B,F), rstd, mean, uvar = var B / (B - 1) (K,F), the gradients of (fm * dfm).sum() --
    dW0, dgam, dbet, dW1, db1, dg -- and the per-sub-net dg_part[k] = du[k] @ W0[k] (K,B,G).  (`y` rides along for the tests'
    saturation check.)"""
    return _film(dtype, g, W0, gam, bet, W1, b1, dfm, eps, None)


def film_frozen_ref(dtype, g, W0, gam, bet, W1, b1, dfm, running_mean, running_var, eps):
    """The same with frozen statistics (du = rstd * gamma * dy): no mean / uvar."""
    return _film(dtype, g, W0, gam, bet, W1, b1, dfm, eps, (running_mean, running_var))


# ---- the measure -------------------------------------------------------------------------------------------------------------------
def rel_per_net(got, ref, per_net=True):
    """max-abs error over the reference's max-abs, taken for every slice k of the leading (K) axis on its own; the worst k.  per_net
    False (dg, which has no K axis): over the whole tensor.  Wherever the reference is exactly zero -- the dW0 row behind gamma = 0,
    xhat, mean and dgam of a dead feature, a slice that is zero altogether -- `got` must be exactly zero."""
    ref = ref.detach().double()
    got = got.detach().double().reshape(ref.shape)
    zero = ref == 0
    assert bool((got[zero] == 0).all()), "not exactly zero where the reference is: %d of %d elements" % (int((got[zero] != 0).sum()), int(zero.sum()))
    if not per_net:
        got, ref = got.unsqueeze(0), ref.unsqueeze(0)
    K = ref.shape[0]
    err = (got - ref).abs().reshape(K, -1).amax(1)
    scale = ref.abs().reshape(K, -1).amax(1)
    assert bool(torch.isfinite(err).all()), "not finite"
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max())
