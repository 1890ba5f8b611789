"""The four fused FiLM conditioner kernels (csrc/film_train.hip: training-mode forward / backward, frozen-statistics forward /
backward) through the C ABI against float64, PER SUB-NET, at the edges the kernels have (tests/film_ref.py: the references, the
cases and the bars; pinned without a GPU by tests/test_film_ref_cpu.py):

  shapes    K = 1, 7, 8, 9, 17, 252 (the last-arriver sum loads the shares eight at a time with a guarded tail); B on either side of
            the NB dispatch (16|17, 32|33), B = 1 .. 4, 63, 64 (the largest LDS carve-out); G = 4, 36, 64, 68, 132, 196, 260, 516 (a
            full 128-column tile plus a tail, a partial second 64-column block in the d g pass);
  values    `hostile` (negative, zero and 40-fold BatchNorm scales, a dead feature with rstd = eps^-1/2, Swish saturated either way),
            `scaled` (sub-nets whose weights and gradients differ by 2^20 and 2^16 inside one launch), `offset` (g + 50, training);
  per case  a. every output NaN-filled with a sentinel region behind it inside the same allocation: the sentinel intact, every
               element written and finite;  b. fm, xhat, rstd (training: mean, uvar);  c. accumulate = 0: the five parameter
               gradients per sub-net, the shares of d g per sub-net and their sum (frozen: the workspace's shares and d g);
            d. accumulate = 1 onto seeded random contents P: P + (c) in fp32, BITWISE -- put() and tile_store() add a value that is
               already rounded (a sum read back from LDS or the last of a chain of adds), so there is no product for the compiler to
               contract into the add;  f. a second call gives the same bits;  frozen: the ticket is 0 after every call, and every
               frozen case of this module runs on ONE ticket word;
  e.        training with dg_part = NULL, frozen with dg = NULL: the five parameter gradients bitwise as with it, the ticket 0, a
            NaN-filled workspace untouched.

Measure: film_ref.rel_per_net -- for every tensor with a leading K axis the max-abs error of sub-net k over the max-abs of the
reference's sub-net k, the worst k (d g whole); wherever the reference is exactly zero the GPU must be exactly zero.  Every
comparison prints `REL <case> <tensor> <kernel> <r32>`; r32 is the fp32 tensor-op formulation (film_ref with torch.float32) on the
GPU on the same inputs against float64 -- the yardstick is never the kernel itself.

Bars.  Class A (seeded, no offset; training B >= 4, frozen any B): film_ref.BARS -- training 2e-5 forward, 1e-5 statistics and
rstd, 2e-5 backward; frozen 1e-5, 9e-7, 2e-5.  They are the bars of tests/test_gpu_film_train.py and of
test_film_frozen_entries_vs_tensor_ops (film_ref.CLASS_A_BARS), now per sub-net; the kernels measured 10 x or more under every one of
them, so each was set to 16 x the worst class A r32 measured on the GPU, rounded up to one digit, where that is tighter: the training
backward 5e-5 -> 2e-5, the frozen rstd 1e-5 -> 9e-7; for the other four 16 r32 is the old bar or above it, and they stay.
Class B (film_ref.CLASS_B, 21 enumerated cases: training at B < 4, hostile, scaled, offset): max(class A bar, 8 r32) per tensor
(8: another summation order on a cancelling sum).  No other case uses that rule.

MEASURED on an MI355X, worst `rel_per_net` of the kernel per class and tensor kind (beside it the worst r32 of the class); every one
of the 44 cases passed as first written, no kernel change:
  training          fm, xhat           rstd, mean, uvar   parameter gradients  dg_part, its sum
  A  seeded B >= 4  7.9e-7 (9.0e-7)    6.6e-7 (6.1e-7)    1.8e-6 (1.2e-6)      1.0e-6 (7.6e-7)
  B  B < 4          5.1e-6 (1.8e-6)    8.1e-7 (2.7e-6)    6.7e-5 (1.8e-5)      3.8e-5 (2.0e-5)
  B  hostile        7.9e-7 (9.0e-7)    6.6e-7 (6.1e-7)    1.6e-6 (7.1e-7)      3.1e-6 (2.6e-6)
  B  scaled         8.5e-7 (8.8e-7)    6.6e-7 (6.1e-7)    1.6e-6 (1.2e-6)      9.0e-7 (1.2e-6)
  B  offset         5.8e-5 (5.8e-5)    1.4e-5 (1.4e-5)    2.8e-4 (2.3e-4)      2.4e-5 (2.2e-5)
  frozen            fm, xhat           rstd               parameter gradients  shares, dg
  A  seeded         7.2e-7 (7.4e-7)    9.5e-8 (5.6e-8)    6.8e-7 (6.7e-7)      1.1e-6 (1.5e-6)
  B  hostile        7.2e-7 (7.4e-7)    7.8e-8 (5.3e-8)    2.5e-6 (3.0e-6)      6.1e-6 (6.1e-6)
  B  scaled         5.9e-7 (5.9e-7)    7.8e-8 (5.3e-8)    1.6e-5 (4.1e-5)      1.8e-5 (3.7e-5)
The largest kernel / r32 ratio of any single class B comparison is 4.2 (dW0 at training (1,2,4): 6.7e-5 against 1.8e-5), of the 8
allowed.  accumulate = 1 is bitwise P + (accumulate = 0) in every case.

The hostile recipe's 40-fold scale takes |y| past 88 (expf overflow) only where the batch is big enough: in training |xhat| <=
sqrt(B - 1), so B = 4 stops at |y| ~ 70 and B = 17 reaches 83 on these seeds; it is asserted, both signs, at B = 63 and 64 (measured
|y| up to 155 in training, 270 frozen).  The -30 / +30 shifts keep y beyond -15 / +15 at every B (asserted): 1 - sigmoid(y) is below fp32's rounding of 1.
"""
import pytest
import torch

from tests import film_ref as R
from tests.film_ref import F, EPS, BARS

pytestmark = pytest.mark.gpu

GUARD = 64 + 128                # the sentinel behind every output (and behind W0): 64 floats and one more 128-column tile
SENTINEL = 12345.0
GRADS = ("dW0", "dgam", "dbet", "dW1", "db1")
_TICKET = []                    # the one ticket word of every frozen call in this module


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from dpf_nets_amd._lib import lib, check, current_stream
    return lib(), check, current_stream()


def _ticket():
    if not _TICKET:
        _TICKET.append(torch.zeros(1, dtype=torch.int32, device="cuda"))
    return _TICKET[0]


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _guarded(shape, src=None):
    """A NaN-filled (or src-filled) buffer of `shape` with GUARD sentinel floats behind it inside the same allocation."""
    n = _numel(shape)
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = SENTINEL
    if src is not None:
        buf[:n] = src.reshape(-1)
    return buf


def _ptr(buf):
    return None if buf is None else buf.data_ptr()


def _collect(what, bufs, shapes):
    """After a launch: every sentinel intact, every element written and finite -> the outputs as tensors of their own shapes."""
    torch.cuda.synchronize()
    out = {}
    for name, buf in bufs.items():
        if buf is None:
            continue
        n = _numel(shapes[name])
        assert buf.numel() == n + GUARD and bool((buf[n:] == SENTINEL).all()), (what, name, "written past the output")
        assert bool(torch.isfinite(buf[:n]).all()), (what, name, "an element was left unwritten or is not finite")
        out[name] = buf[:n].view(shapes[name])
    return out


def _shapes(K, B, G):
    return dict(fm=(K, B, F), xhat=(K, B, F), rstd=(K, F), mean=(K, F), uvar=(K, F), dW0=(K, F, G), dgam=(K, F), dbet=(K, F),
                dW1=(K, F, F), db1=(K, F), dg_part=(K, B, G), dg=(B, G))


def _inputs(K, B, G, variant, offset):
    c = R.make_case(K, B, G, R.case_seed(K, B, G), variant, offset)
    d = {k: v.cuda() for k, v in c.items()}
    d["W0"] = _guarded((K, F, G), d["W0"])[:K * F * G].view(K, F, G)          # a read past a W0 row stays inside the allocation
    return d


def _forward(mode, d, K, B, G):
    L, check, st = _gpu()
    shapes = _shapes(K, B, G)
    names = ("fm", "xhat", "rstd") + (("mean", "uvar") if mode == "train" else ())
    o = {n: _guarded(shapes[n]) for n in names}
    p = [d[k].data_ptr() for k in ("g", "W0", "gam", "bet", "W1", "b1")]
    if mode == "train":
        check(L.dpf_film_train_forward(K, B, G, *p, EPS, *(o[n].data_ptr() for n in names), st), "film_train_forward")
    else:
        check(L.dpf_film_frozen_forward(K, B, G, *p, d["rm"].data_ptr(), d["rv"].data_ptr(), EPS, *(o[n].data_ptr() for n in names), st),
              "film_frozen_forward")
    return _collect(mode + " forward", o, shapes)


def _backward(mode, d, fwd, K, B, G, accumulate=0, prior=None, want_dg=True):
    """One backward launch.  prior: the contents the five gradient buffers hold before it (accumulate = 1).  Frozen: the workspace is
    NaN-filled and handed over even when d g is not wanted, and the ticket is 0 afterwards."""
    L, check, st = _gpu()
    shapes = _shapes(K, B, G)
    o = {n: _guarded(shapes[n], None if prior is None else prior[n]) for n in GRADS}
    p = [t.data_ptr() for t in (d["g"], d["W0"], d["gam"], d["bet"], d["W1"], fwd["xhat"], fwd["rstd"], d["dfm"])]
    if mode == "train":
        o["dg_part"] = _guarded(shapes["dg_part"]) if want_dg else None
        check(L.dpf_film_train_backward(K, B, G, *p, *(o[n].data_ptr() for n in GRADS), _ptr(o["dg_part"]), accumulate, st),
              "film_train_backward")
        return _collect("train backward", o, shapes)
    assert L.dpf_film_frozen_workspace_floats(K, B, G) == K * B * G
    o["dg"] = _guarded(shapes["dg"]) if want_dg else None
    work, ticket = _guarded(shapes["dg_part"]), _ticket()
    check(L.dpf_film_frozen_backward(K, B, G, *p, *(o[n].data_ptr() for n in GRADS), _ptr(o["dg"]), work.data_ptr(), ticket.data_ptr(),
                                     accumulate, st), "film_frozen_backward")
    if want_dg:
        o["dg_part"] = work
    out = _collect("frozen backward", o, shapes)
    assert int(ticket) == 0, "the ticket did not return to zero"
    if not want_dg:
        assert bool(torch.isnan(work[:K * B * G]).all()) and bool((work[K * B * G:] == SENTINEL).all()), "d g unwanted, workspace touched"
    return out


def _references(mode, d):
    a = (d["g"], d["W0"], d["gam"], d["bet"], d["W1"], d["b1"], d["dfm"])
    if mode == "train":
        return R.film_train_ref(torch.float64, *a, EPS), R.film_train_ref(torch.float32, *a, EPS)
    return R.film_frozen_ref(torch.float64, *a, d["rm"], d["rv"], EPS), R.film_frozen_ref(torch.float32, *a, d["rm"], d["rv"], EPS)


def _case(mode, K, B, G, variant="seeded", offset=0.0):
    _gpu()
    case = (mode, K, B, G, variant, float(offset))
    cid = R.case_id(*case)
    assert (case in R.CLASS_B) == R.is_class_b(*case), "the r32 rule is for the cases of CLASS_B and no others"
    d = _inputs(K, B, G, variant, offset)
    ref, r32 = _references(mode, d)
    if variant == "hostile":
        assert float(ref["y"][:, :, 3].max()) < -15 and float(ref["y"][:, :, 5].min()) > 15
        if B >= 63:
            assert float(ref["y"].min()) < -88 and float(ref["y"].max()) > 88, "the hostile state does not reach expf's overflow"

    def compare(name, got, ref_name=None):
        ref_name = ref_name or name
        per_net = ref_name != "dg"
        r, r3 = R.rel_per_net(got, ref[ref_name], per_net), R.rel_per_net(r32[ref_name], ref[ref_name], per_net)
        print("REL", cid, name, "%.3e" % r, "%.3e" % r3)
        bar = R.bar_for(BARS, *case, ref_name, r3)
        assert r <= bar, (cid, name, r, r3, bar)

    # a, b: the forward
    fwd = _forward(mode, d, K, B, G)
    for name in fwd:
        compare(name, fwd[name])
    # a, c: the backward, accumulate = 0
    got = _backward(mode, d, fwd, K, B, G)
    for name in GRADS + ("dg_part",):
        compare(name, got[name])
    if mode == "train":
        compare("sum(dg_part)", got["dg_part"].sum(0), "dg")
    else:
        compare("dg", got["dg"])
    # f: the same bits on a second call
    fwd2 = _forward(mode, d, K, B, G)
    got2 = _backward(mode, d, fwd, K, B, G)
    assert all(torch.equal(fwd[n], fwd2[n]) for n in fwd), (cid, "forward, second call")
    assert all(torch.equal(got[n], got2[n]) for n in got), (cid, "backward, second call")
    # d: accumulate = 1 onto random contents is one fp32 add per element
    gen = torch.Generator().manual_seed(R.case_seed(K, B, G) + 1)
    shapes = _shapes(K, B, G)
    prior = {n: (torch.randn(shapes[n], generator=gen) * float(got[n].abs().max())).cuda() for n in GRADS}
    acc = _backward(mode, d, fwd, K, B, G, accumulate=1, prior=prior)
    for n in GRADS:
        assert torch.equal(acc[n], prior[n] + got[n]), (cid, n, "accumulate = 1 is not P + (accumulate = 0), bitwise",
                                                        float((acc[n] - (prior[n] + got[n])).abs().max()))
    for n in ("dg_part",) + (("dg",) if mode == "frozen" else ()):
        assert torch.equal(acc[n], got[n]), (cid, n, "accumulate = 1 changed d g")


@pytest.mark.parametrize("K,B,G,variant,offset", R.cases("train"), ids=lambda v: str(v))
def test_training_kernels_vs_float64(K, B, G, variant, offset):
    _case("train", K, B, G, variant, offset)


@pytest.mark.parametrize("K,B,G,variant,offset", R.cases("frozen"), ids=lambda v: str(v))
def test_frozen_kernels_vs_float64(K, B, G, variant, offset):
    _case("frozen", K, B, G, variant, offset)


def test_frozen_sub_net_counts_one_after_another_on_one_ticket():
    """K = 1, 7, 8, 17, 252 back to back: fewer than eight sub-nets, exactly eight, a tail of one, many -- every call finds the ticket
    the previous one left and leaves it 0 (asserted inside _backward after each of the three backward launches of a case)."""
    _gpu()
    before = _ticket().data_ptr()
    for K, B, G in R.FROZEN_ONLY:
        _case("frozen", K, B, G)
    assert _ticket().data_ptr() == before and int(_ticket()) == 0


@pytest.mark.parametrize("mode", R.MODES)
def test_optional_d_g(mode):
    """e: (2, 17, 260) -- NB = 8, two tiles and a 4-column tail.  Without d g (training: dg_part = NULL; frozen: dg = NULL, the early
    return in front of the ticket) the five parameter gradients have the same bits, the ticket stays 0 and the workspace NaN."""
    _gpu()
    K, B, G = 2, 17, 260
    d = _inputs(K, B, G, "seeded", 0.0)
    fwd = _forward(mode, d, K, B, G)
    full = _backward(mode, d, fwd, K, B, G)
    bare = _backward(mode, d, fwd, K, B, G, want_dg=False)
    assert set(bare) == set(GRADS)
    for n in GRADS:
        assert torch.equal(full[n], bare[n]), n
    if mode == "frozen":
        assert int(_ticket()) == 0
        again = _backward(mode, d, fwd, K, B, G)                   # and the next call that wants d g finds the ticket in order
        assert torch.equal(again["dg"], full["dg"])
