"""Timing of dpf_fps (csrc/fps.hip): every kernel form beside the by-size pick, and what a user did before it existed -- a
farthest-point loop on tensor ops, per round a gather of the last pick, a distance, `minimum` and `argmax` -- on the same GPU in
the same process.  Not part of bench.py.

    python tools/fps_bench.py [--out FILE]

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  Before anything is
timed the loop's indices are compared with the kernel's on a cloud where the comparison is fair: Gaussian points rounded to
multiples of 2^-6, on which every fp32 operation of either side is exact whatever the order of its sums, and the rounds with more
than one point at the maximum are counted (0: tie-free; on a tie both sides take the lowest index).
Per shape: ms per call; at B = 1 also the time per round (call time / k), the number dispatch.h's thresholds are set from; the
ratio of the loop's time to the by-size pick's."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd.metrics.fps import farthest_point_index                                   # noqa: E402

FORMS = ((1, "1 wave"), (2, "4 waves"), (3, "16 waves"))
SHAPES = ((2048, 512), (2500, 2048), (8192, 2048))
BATCHES = (1, 32, 256, 1024)


def tensor_op_fps(pts, k, count_ties=False):
    """(B, n, 3) -> (B, k) int64 indices from index 0 (and the number of rounds with a tie at the maximum)"""
    B, n, _ = pts.shape
    index = torch.empty((B, k), dtype=torch.long, device=pts.device)
    mind = torch.full((B, n), float("inf"), device=pts.device)
    sel = torch.zeros((B,), dtype=torch.long, device=pts.device)
    rows = torch.arange(B, device=pts.device)
    ties = torch.zeros((), dtype=torch.long, device=pts.device)
    for t in range(k):
        index[:, t] = sel
        mind = torch.minimum(mind, ((pts - pts[rows, sel].unsqueeze(1)) ** 2).sum(-1))
        sel = mind.argmax(1)
        if count_ties:
            ties += ((mind == mind.max(1, keepdim=True)[0]).sum(1) > 1).any()
    return (index, int(ties)) if count_ties else index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="the forms between 64 and 1024 points too (where the thresholds sit)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator(device=dev).manual_seed(3)
    cloud = torch.randn((max(BATCHES), max(n for n, _ in SHAPES), 3), device=dev, generator=gen)

    exact = torch.round(cloud[:4, :2048] * 64.0) / 64.0
    want, ties = tensor_op_fps(exact, 512, count_ties=True)
    got = farthest_point_index(exact, 512)[0].long()
    same = bool((want == got).all())
    say("# check: tensor-op loop vs dpf_fps, 4 clouds of 2048 points on the 2^-6 grid, k = 512: indices %s, rounds with a tie at the maximum: %d"
        % ("EQUAL" if same else "DIFFER", ties))
    if not same:
        raise SystemExit("the baseline and the kernel disagree: nothing timed")

    def forms_of(pts, k):
        out = []
        for force, name in ((0, "by size"),) + FORMS:
            try:
                farthest_point_index(pts, k, form=force)
            except RuntimeError:
                continue                                                                    # (forced past its limit)
            out.append((name, timed(lambda: farthest_point_index(pts, k, form=force), args.warmup, args.repeats)))
        return out

    say("# Gaussian clouds; ms per call, median of %d after %d warm-ups (the tensor-op loop: %d after 1)" % (args.repeats, args.warmup, args.loop_repeats))
    for n, k in SHAPES:
        for B in BATCHES:
            pts = cloud[:B, :n].contiguous()
            res = forms_of(pts, k)
            loop = timed(lambda: tensor_op_fps(pts, k), 1, args.loop_repeats)
            pick = res[0][1]
            say("  n = %4d  k = %4d  B = %4d   %s   tensor-op loop %10.3f ms = %7.1f x the pick%s"
                % (n, k, B, "   ".join("%s %9.4f ms" % r for r in res), loop, loop / pick,
                   "   per round: %s" % "  ".join("%s %.3f us" % (nm, ms * 1e3 / k) for nm, ms in res) if B == 1 else ""))
    if args.small:
        say("# the forms where their thresholds sit: us per round at k = n, B = 1 | ms per call at B = 1024")
        for n in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
            say("  n = %4d   %s" % (n, "   ".join("%s %.3f us | %.4f ms" % (nm, a * 1e3 / n, b) for (nm, a), (_, b) in
                                                  zip(forms_of(cloud[:1, :n].contiguous(), n), forms_of(cloud[:1024, :n].contiguous(), n)))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
