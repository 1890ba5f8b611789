"""Shared by tests/test_flow_hostile_cpu.py, tests/test_gpu_flow_hostile.py, tests/test_gpu_flow_frozen.py and
tests/test_gpu_flow_train.py: a state mutator that takes the seeded coupling-stack states (oracle/flow_oracle.py: BatchNorm scales and
variances in [0.5, 1.5], FiLM factors near 1, no dead unit, small outputs) to where a trained checkpoint goes, the hostile input
clouds, the pack-time range bound of networks/engine.py restated on CPU tensors, and the float64 yardstick.

What `hostile_flow` changes, per coupling layer and per branch (features drawn from a seeded permutation, all distinct):

  sd0_bn.weight (gamma0)   every third hidden feature negated; one exactly 0.0 (its beta0 = +0.25, so the unit is the constant
                           relu(0.25) and d gamma0 = sum dh0 * xhat is live); one scaled up until its term of the range bound is
                           BIG_BOUND = 0.75 F16_LIMIT (the column of sd1.weight behind it is scaled down by the same factor, as
                           test_f16x3_large_activations does, so the layer's output keeps its scale)
  sd0_bn.running_var/mean  one variance 3e-3, one 50, four means +-3
  sd1_bn.running_var       10^u, u spread evenly over [-2, 2] in seeded order
  FiLM                     ..._film_w1.bias shifted per feature by linspace(-12, 6): FA = (eps + e^cw) / sqrt(rv1 + eps_bn) runs from
                           eps-dominated (7e-7) to several hundred; ..._film_b1.bias shifted by +-3 in seeded signs.  The sd2.weight
                           column of a feature whose nominal FA = e^shift / sqrt(rv1) exceeds 1 is divided by it, so that the stack's
                           points stay inside the coordinate range the guard assumes (F16_COORD_MAX).  The folded output rows W2' = w2 FA
                           therefore run from 1e-8 up to |w2| only: the LARGE side of W2' is NOT reached by these states (one row of
                           W2' in the hundreds throws the points out of the guard's range; rows of 10 |w2| put the fp32 tensor
                           operations themselves at 1e-6 of float64, half of bf16x6's bar).  The shift D = FC / FA and the
                           accumulator it is preloaded into keep their full range, 1e-3 to 1e10
  dead / constant unit     an sd0.weight row of zeros with beta0 = -0.5 / +0.5 (running_mean0 = 0: the pre-activation is exactly beta0
                           in evaluation as it is under batch statistics)
  zero sd1 row             h1 == 0: that feature is relu(D)
  saturated layer          layer SAT_LAYER (two warped channels), logvar branch: sd2.weight times SAT_GAIN and sd2.bias = (+SAT_REACH,
                           -SAT_REACH): the pre-softsign output is +50 +- a few in one channel, -50 +- a few in the other, and
                           softsign saturates on both sides (an output CENTRED on 0 and stretched to +-50 would be a difference of
                           two numbers in the thousands: the units that are constant over the points dominate o)
  identity layer           layer ID_LAYER: sd2.weight and sd2.bias of both branches exactly zero

With running_stats=False (training mode: running statistics are not read) the running-statistics part and the gamma0 scaled to the
evaluation guard are left out."""
import math

import numpy as np
import torch

from oracle import detrng
from oracle import flow_oracle as FO

F16_LIMIT = 2048.0          # networks/engine.py
F16_COORD_MAX = 32.0
BIG_BOUND = 0.75 * F16_LIMIT
SAT_LAYER, ID_LAYER = 4, 1          # a layer that warps two channels; a layer the frozen tests' cross term ps[2] * mus[4] does not read
SAT_REACH, SAT_GAIN = 50.0, 10.0
WIDE = 8.0                  # a quarter of F16_COORD_MAX
VARIANTS = ("plain", "same", "wide")
ROLES = ("zero", "big", "small_var", "large_var", "mean0", "mean1", "mean2", "mean3", "dead", "const", "zero_row1")


def layer_prefixes(state):
    """State-dict prefixes of the coupling layers in the state's (direct) order; [""] for a single layer's state."""
    out = []
    for k in state:
        i = k.find("T_")
        pre = k[:i] if i >= 0 else k[:-len("eps")]
        if pre not in out:
            out.append(pre)
    return out


def roles(seed, prefix, br, F=64):
    """{role: feature} of one (layer, branch), and the seeded permutation behind it."""
    perm = np.argsort(detrng.uniform(detrng.key(seed, "hostile:" + prefix + br), F), kind="stable")
    return {name: int(perm[i]) for i, name in enumerate(ROLES)}, perm


def hostile_flow(state, seed, running_stats=True):
    st = {k: np.array(v, copy=True) for k, v in state.items()}
    for li, pre in enumerate(layer_prefixes(st)):
        for br in FO.BRANCHES:
            t0 = "%sT_%s_0.%s_" % (pre, br, br)
            w0, g0, b0 = st[t0 + "sd0.weight"], st[t0 + "sd0_bn.weight"], st[t0 + "sd0_bn.bias"]
            rm0, rv0 = st[t0 + "sd0_bn.running_mean"], st[t0 + "sd0_bn.running_var"]
            w1, rv1 = st[t0 + "sd1.weight"], st[t0 + "sd1_bn.running_var"]
            w2, b2 = st["%sT_%s_1.%s_sd2.weight" % (pre, br, br)], st["%sT_%s_1.%s_sd2.bias" % (pre, br, br)]
            F = g0.shape[0]
            r, perm = roles(seed, pre, br, F)
            # ---- running statistics
            if running_stats:
                rv0[r["small_var"]] = 3e-3
                rv0[r["large_var"]] = 50.0
                for i in range(4):
                    rm0[r["mean%d" % i]] = 3.0 if i % 2 == 0 else -3.0
                order = np.argsort(detrng.uniform(detrng.key(seed, "hostile_rv1:" + pre + br), F), kind="stable")
                rv1[order] = (10.0 ** np.linspace(-2.0, 2.0, F)).astype(np.float32)
            # ---- dead and constant units
            for name, beta in (("dead", -0.5), ("const", 0.5)):
                w0[0, r[name], :] = 0.0
                b0[r[name]] = beta
                rm0[r[name]] = 0.0
            # ---- gamma0: signs, the exact zero, the one at the guard
            g0[int(perm[F - 1]) % 3::3] *= np.float32(-1.0)
            g0[r["zero"]] = 0.0
            b0[r["zero"]] = 0.25
            if running_stats:
                f = r["big"]
                rm0[f] = 0.0                        # the unit switches with the sign of W0 x: on for part of the points
                reach = float(np.abs(w0[0, f]).sum()) * F16_COORD_MAX + abs(float(rm0[f]))
                s0 = (BIG_BOUND - abs(float(b0[f]))) / reach
                new = math.copysign(s0 * math.sqrt(float(rv0[f]) + FO.BN_EPS), float(g0[f]))
                w1[0, :, f] *= np.float32(abs(float(g0[f]) / new))
                g0[f] = new
            # ---- zero sd1 row
            w1[0, r["zero_row1"], :] = 0.0
            # ---- FiLM: cw over [-12, +6], cb at +-3; W2' = w2 FA kept O(w2)
            order = np.argsort(detrng.uniform(detrng.key(seed, "hostile_cw:" + pre + br), F), kind="stable")
            shift = np.empty(F)
            shift[order] = np.linspace(-12.0, 6.0, F)
            st["%sT_%s_0_cond_w.%s_sd1_film_w1.bias" % (pre, br, br)] += shift.astype(np.float32)
            sign = np.where(detrng.uniform(detrng.key(seed, "hostile_cb:" + pre + br), F) < 0.5, -3.0, 3.0)
            st["%sT_%s_0_cond_b.%s_sd1_film_b1.bias" % (pre, br, br)] += sign.astype(np.float32)
            fa = np.exp(shift) / np.sqrt(rv1.astype(np.float64) + FO.BN_EPS)
            w2[0] *= (1.0 / np.maximum(1.0, fa)).astype(np.float32)[None, :]
            # ---- the saturated and the identity layer
            if li == SAT_LAYER and br == "logvar":
                w2 *= np.float32(SAT_GAIN)
                b2[0, :] = (SAT_REACH, -SAT_REACH)
            if li == ID_LAYER:
                w2[...] = 0.0
                b2[...] = 0.0
    return st


def hostile_flow_train(state, seed):
    """The parameter part alone (training mode)."""
    return hostile_flow(state, seed, running_stats=False)


def guard_bound(state):
    """networks/engine.py f16_in_range restated on the numpy state in fp32: (max over layers / branches / features of
    sum_k |s0 W0[f][k]| F16_COORD_MAX + |beta0 - running_mean0 s0|,  max |W1|)."""
    hb, wb = [], []
    for pre in layer_prefixes(state):
        for br in FO.BRANCHES:
            t0 = "%sT_%s_0.%s_" % (pre, br, br)
            g0, b0 = torch.from_numpy(state[t0 + "sd0_bn.weight"]), torch.from_numpy(state[t0 + "sd0_bn.bias"])
            rm0, rv0 = torch.from_numpy(state[t0 + "sd0_bn.running_mean"]), torch.from_numpy(state[t0 + "sd0_bn.running_var"])
            s0 = g0 / torch.sqrt(rv0 + FO.BN_EPS)
            w = torch.from_numpy(state[t0 + "sd0.weight"])[0].abs().sum(1) * s0.abs()
            T = (b0 - rm0 * s0).abs()
            hb.append(float((w * F16_COORD_MAX + T).max()))
            wb.append(float(torch.from_numpy(state[t0 + "sd1.weight"]).abs().max()))
    return max(hb), max(wb)


def hostile_inputs(seed, B, N, G, variant="plain"):
    """FO.synthetic_inputs as they are ("plain"); with every point of cloud min(1, B - 1) equal to its first ("same"); with cloud 0
    scaled so that its largest coordinate is WIDE ("wide").  -> (targets, base samples, g), fp32 numpy."""
    tgt, z, g = (np.array(a, copy=True) for a in FO.synthetic_inputs(seed, B, N, G))
    for a in (tgt, z):
        if variant == "same":
            b = min(1, B - 1)
            a[b] = a[b, :, :1]
        elif variant == "wide":
            a[0] *= np.float32(WIDE / float(np.abs(a[0]).max()))
        elif variant != "plain":
            raise ValueError(variant)
    return tgt, z, g


SEED = 91
_STATES = {}


def decoder_state(G, n_flows=2, seed=SEED, train=False):
    """The hostile numpy state of the cases below, made once; callers must not write into it."""
    key = (G, n_flows, seed, train)
    if key not in _STATES:
        _STATES[key] = hostile_flow(FO.make_decoder_state(seed, n_flows, 64, G), seed, running_stats=not train)
    return _STATES[key]


def decoder_case(G, B, N, mode, variant, n_flows=2, seed=SEED, train=False):
    """(hostile numpy state, source points (B,3,N), g (B,G)) of one case of the GPU tests."""
    tgt, z, g = hostile_inputs(seed, B, N, G, variant)
    return decoder_state(G, n_flows, seed, train), (tgt if mode == "inverse" else z), g


_REF = {}


def reference64(G, B, N, mode, variant, n_flows=2, seed=SEED):
    """FO.decoder in float64 on the CPU: (ps, mus, lvs) lists of float64 tensors in direct order.  Computed once per case and
    shared; callers must not write into it."""
    key = (G, B, N, mode, variant, n_flows, seed)
    if key not in _REF:
        state, src, g = decoder_case(G, B, N, mode, variant, n_flows, seed)
        st = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in FO.to_torch(state).items()}
        with torch.no_grad():
            _REF[key] = FO.decoder(st, n_flows, torch.from_numpy(src).double(), torch.from_numpy(g).double(), mode)
    return _REF[key]
