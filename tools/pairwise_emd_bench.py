"""pairwise_EMD (dpf_pairwise_emd: no matching written) against the EMD half of _pairwise_EMD_CD_ (per row an expanded copy of
the sample cloud and one emd_approx = match_cost call over the reference block, which writes the (b, n, n) matching), in one
process, alternating the two, timed with device events after a warm-up of every shape.  Also compares the two matrices: max
relative difference and whether any per-row / per-column argmin changes.
usage: pairwise_emd_bench.py [N1 N2 n ...] [--reps R] [--bs BS]      (default shapes: 128 128 2048 and 16 16 8192)"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpf_nets_amd.networks.utils import pairwise_EMD, emd_approx      # noqa: E402


def row_loop(a, b, batch_size):
    """the EMD half of metrics.evaluation_metrics._pairwise_EMD_CD_ (evaluation_metrics.py:85-121), verbatim in its calls"""
    N1, N2 = a.shape[0], b.shape[0]
    out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    for i in range(N1):
        for r0 in range(0, N2, batch_size):
            r1 = min(N2, r0 + batch_size)
            out[i, r0:r1] = emd_approx(a[i].unsqueeze(0).expand(r1 - r0, -1, -1).contiguous(), b[r0:r1])
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bs", type=int, default=512, help="pairwise_EMD's pairs per launch")
    args = ap.parse_args()
    shapes = [tuple(args.shape[i:i + 3]) for i in range(0, len(args.shape), 3)] if args.shape else [(128, 128, 2048), (16, 16, 8192)]
    cases = []
    for N1, N2, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        a = torch.randn(N1, n, 3, device="cuda", generator=g) * 0.2
        b = torch.randn(N2, n, 3, device="cuda", generator=g) * 0.2
        cases.append((N1, N2, n, a, b))
    legs = {"pairwise_EMD": lambda a, b: pairwise_EMD(a, b, bs=args.bs),
            "row_loop": lambda a, b: row_loop(a, b, b.shape[0])}
    with torch.no_grad():
        for N1, N2, n, a, b in cases:                                     # warm-up of every shape and leg
            for fn in legs.values():
                timed(lambda: fn(a, b))
        for N1, N2, n, a, b in cases:
            times = {k: [] for k in legs}
            outs = {}
            for _ in range(args.reps):                                    # alternating
                for k, fn in legs.items():
                    outs[k], ms = timed(lambda: fn(a, b))
                    times[k].append(ms)
            p, r = outs["pairwise_EMD"], outs["row_loop"]
            rel = float(((p - r).abs() / r.abs()).max())
            row_flips = int((p.argmin(1) != r.argmin(1)).sum())
            col_flips = int((p.argmin(0) != r.argmin(0)).sum())
            best = {k: min(v) for k, v in times.items()}
            print(json.dumps({"N1": N1, "N2": N2, "n": n, "bs": args.bs,
                              "pairwise_EMD_ms": round(best["pairwise_EMD"], 3), "row_loop_ms": round(best["row_loop"], 3),
                              "speedup": round(best["row_loop"] / best["pairwise_EMD"], 3),
                              "pairwise_EMD_ms_all": [round(v, 3) for v in times["pairwise_EMD"]],
                              "row_loop_ms_all": [round(v, 3) for v in times["row_loop"]],
                              "max_rel_diff": rel, "finite": bool(torch.isfinite(p).all()),
                              "argmin_changes_rows": row_flips, "argmin_changes_cols": col_flips}), flush=True)


if __name__ == "__main__":
    main()
