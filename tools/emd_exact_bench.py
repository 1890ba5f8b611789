"""Timing of dpf_emd_exact (csrc/emd_exact.hip) at the evaluation shapes, the rounds it needs, the same assignment problems on
the host where scipy is installed, and -- for information -- how far the approximate matcher sits from the optimum.  Not part of
bench.py.

    python tools/emd_exact_bench.py [--out FILE]

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  Rounds are the
kernel's own status; bids per pair come from the numpy oracle (tests/emd_exact_ref.py), which the kernel follows round for round
(tests/test_gpu_emd_exact.py asserts equal round counts), on --oracle-pairs pairs.  The host figure is one thread building the
float64 distance matrix and calling scipy.optimize.linear_sum_assignment on it, per pair."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import emd_exact_ref as R                                                                   # noqa: E402
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd.networks import utils as U                                                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--oracle-pairs", type=int, default=2)
    ap.add_argument("--host-pairs", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = 2048
    gen = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn((256, n, 3), device=dev, generator=gen)
    b = torch.randn((256, n, 3), device=dev, generator=gen) * 0.7 + 0.2
    say("# Gaussian clouds of n = %d points; ms per call, median of %d after %d warm-ups" % (n, args.repeats, args.warmup))
    for B in (1, 32, 256):
        ms = timed(lambda: U.emd_exact_full(a[:B], b[:B]), args.warmup, args.repeats)
        status = U.emd_exact_full(a[:B], b[:B])[3].cpu().numpy()
        say("  emd_exact  B = %3d   %10.3f ms   rounds per pair: min %d  median %d  max %d" % (B, ms, status.min(), np.median(status), status.max()))
    with torch.no_grad():
        ms = timed(lambda: U.pairwise_EMD_exact(a[:64], b[:64], bs=4096), 1, args.repeats)
    say("  pairwise_EMD_exact 64 x 64 x %d   %10.3f ms   %.0f pairs/s" % (n, ms, 4096 / (ms * 1e-3)))
    req = a[:32].clone().requires_grad_(True)
    cost = U.emd_exact_full(req, b[:32])[0]
    g = torch.ones_like(cost)
    say("  backward (one gather launch), B = 32   %10.4f ms" % timed(lambda: torch.autograd.grad(cost, req, g, retain_graph=True), args.warmup, args.repeats))
    ah, bh = a[:max(args.oracle_pairs, args.host_pairs)].cpu().numpy(), b[:max(args.oracle_pairs, args.host_pairs)].cpu().numpy()
    for k in range(args.oracle_pairs):
        o = R.solve(ah[k], bh[k])
        say("  pair %d: %d rounds, %d bids (%.1f per round), %.1f bids per point" % (k, o["rounds"], o["bids"], o["bids"] / max(o["rounds"], 1), o["bids"] / n))
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        say("  host: scipy is not installed here, no host figure")
    else:
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        for k in range(args.host_pairs):
            d = np.sqrt(((ah[k].astype(np.float64)[:, None] - bh[k].astype(np.float64)[None]) ** 2).sum(-1))
            linear_sum_assignment(d)
        say("  host: distance matrix + scipy linear_sum_assignment, one thread: %.1f ms per pair (%d pairs)"
            % ((time.perf_counter() - t0) * 1e3 / args.host_pairs, args.host_pairs))

    say("# emd_approx / emd_exact (information only: approxmatch's weights are no feasible plan, neither direction is guaranteed)")
    ratios = []
    for kind in R.KINDS:
        for m in (63, 64, 65, 256):
            c = [R.make_case(kind, m, 100 * m + k) for k in range(3)]
            ratios.append((kind, m, np.stack([x[0] for x in c]), np.stack([x[1] for x in c])))
    report(say, "the GPU test's case list", ratios, dev)
    import emd_cases as EC
    rng = np.random.default_rng(7)
    report(say, "the approx-EMD fuzz kinds, n = m = 512", [(kind, 512) + EC.emd_clouds(rng, kind, 3, 512, 3, 512) for kind in EC.KINDS], dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def report(say, title, cases, dev):
    allr = []
    for kind, m, x, y in cases:
        tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        with torch.no_grad():
            ex, ap = U.emd_exact(tx, ty).cpu().numpy().astype(np.float64), U.emd_approx(tx, ty).cpu().numpy().astype(np.float64)
        ok = ex > 0
        allr += (ap[ok] / ex[ok]).tolist()
    r = np.array(allr)
    say("  %s: %d pairs with a non-zero optimum -- min %.4f  median %.4f  max %.4f" % (title, r.size, r.min(), np.median(r), r.max()))


if __name__ == "__main__":
    main()
