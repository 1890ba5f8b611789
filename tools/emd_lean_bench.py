"""approx-EMD with and without a stored matching, in one process, the legs alternating, timed with device events after a warm-up
of every shape:
  forward              ApproxMatchCost (writes the (B, n, n) matching) against ApproxMatchCostOnly; the stored leg runs twice per
                       round ("fwd_stored", "fwd_stored_again"): the difference of two identical legs is the run-to-run spread
  forward + backward   match_cost (stored matching, read once by dpf_matchcostgrad_ws) against match_cost_lean (the matching
                       rebuilt in registers by dpf_matchcostgrad_recompute_ws)
plus each leg's peak allocation rise and the largest difference of the costs (expected 0) and of the gradients.
One JSON line per shape.   usage: emd_lean_bench.py [B n ...] [--reps R]      (default shapes: 16 8192, 32 2048, 64 8192)"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpf_nets_amd.metrics.StructuralLosses import StructuralLossesBackend as BK      # noqa: E402
from dpf_nets_amd.metrics.StructuralLosses.match_cost import match_cost, match_cost_lean      # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def fwd_bwd(fn, a, b, w):
    xa, xb = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    cost = fn(xa, xb)
    (cost * w).sum().backward()
    return cost.detach(), xa.grad, xb.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    shapes = [tuple(args.shape[i:i + 2]) for i in range(0, len(args.shape), 2)] if args.shape else [(16, 8192), (32, 2048), (64, 8192)]
    legs = {"fwd_stored": lambda a, b, w: BK.ApproxMatchCost(a, b)[2],
            "fwd_costonly": lambda a, b, w: BK.ApproxMatchCostOnly(a, b)[1],
            "fwd_stored_again": lambda a, b, w: BK.ApproxMatchCost(a, b)[2],
            "fwdbwd_stored": lambda a, b, w: fwd_bwd(match_cost, a, b, w),
            "fwdbwd_lean": lambda a, b, w: fwd_bwd(match_cost_lean, a, b, w)}
    cases = []
    for B, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        a = torch.randn(B, n, 3, device="cuda", generator=g) * 0.2
        b = torch.randn(B, n, 3, device="cuda", generator=g) * 0.2
        w = torch.rand(B, device="cuda", generator=g) + 0.5
        cases.append((B, n, a, b, w))
    for B, n, a, b, w in cases:                                         # warm-up of every shape and leg
        for fn in legs.values():
            timed(lambda: fn(a, b, w))
    for B, n, a, b, w in cases:
        times = {k: [] for k in legs}
        outs = {}
        for _ in range(max(5, args.reps)):                              # alternating
            for k, fn in legs.items():
                outs[k], ms = timed(lambda: fn(a, b, w))
                times[k].append(ms)
        mem = {k: peak_rise(lambda: fn(a, b, w)) for k, fn in legs.items() if k != "fwd_stored_again"}
        best = {k: min(v) for k, v in times.items()}
        cs, g1s, g2s = outs["fwdbwd_stored"]
        cl, g1l, g2l = outs["fwdbwd_lean"]
        spread = max(abs(x - y) for x, y in zip(times["fwd_stored"], times["fwd_stored_again"])) / best["fwd_stored"]
        line = {"B": B, "n": n, "reps": len(times["fwd_stored"])}
        for k in legs:
            line[k + "_ms"] = round(best[k], 3)
            line[k + "_ms_all"] = [round(v, 3) for v in times[k]]
        line.update({"fwd_costonly_over_stored": round(best["fwd_costonly"] / best["fwd_stored"], 4),
                     "fwd_stored_spread": round(spread, 4),
                     "fwdbwd_lean_over_stored": round(best["fwdbwd_lean"] / best["fwdbwd_stored"], 4),
                     "peak_rise_bytes": mem, "matching_bytes": 4 * B * n * n,
                     "max_cost_diff_fwd": float((outs["fwd_costonly"] - outs["fwd_stored"]).abs().max()),
                     "max_cost_diff_fwdbwd": float((cl - cs).abs().max()),
                     "max_grad1_diff": float((g1l - g1s).abs().max()), "max_grad2_diff": float((g2l - g2s).abs().max()),
                     "max_grad_abs": float(max(g1s.abs().max(), g2s.abs().max()))})
        print(json.dumps(line), flush=True)
        del outs, cs, g1s, g2s, cl, g1l, g2l


if __name__ == "__main__":
    main()
