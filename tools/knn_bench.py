"""Timing of dpf_knn (csrc/knn.hip): the by-k pick beside every forced list capacity, and two baselines on the same GPU in the same
process -- what a user did before it existed (the expanded squared distance |q|^2 + |c|^2 - 2 q.c as a (B, n, m) tensor, the
diagonal masked, then `topk`), and dpf_nndistance_auto at the same sizes as the k = 1 floor (for information, not a bar).  Not part
of bench.py.

    python tools/knn_bench.py [--out FILE]

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  Every case is a
self-search with the exclusion.  Before anything is timed the tensor-op route's indices are compared with the kernel's on a cloud
where the comparison is fair: integer coordinates in [-512, 512), on which every fp32 operation of either side is exact; rows whose
k + 1 smallest distances hold a tie are left out of the index comparison (topk does not say which of two equals it lists) and
counted."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd import _lib                                                               # noqa: E402
from dpf_nets_amd.metrics.knn import knn_index                                              # noqa: E402

FORMS = ((1, "cap 4"), (2, "cap 8"), (3, "cap 16"), (4, "cap 32"))
CASES = ((32, 2048, 8), (32, 2048, 16), (32, 2048, 32), (4, 8192, 16), (256, 512, 8))


def tensor_op_knn(pts, k):
    """(B, n, 3) -> (dist, index) of the k nearest OTHER points by the expanded distance and topk"""
    sq = (pts * pts).sum(-1)
    d = sq[:, :, None] + sq[:, None, :] - 2.0 * torch.bmm(pts, pts.transpose(1, 2))
    d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    return torch.topk(d, k, dim=2, largest=False, sorted=True)


def nn_floor(pts):
    B, n, _ = pts.shape
    r = torch.empty((2, B, n), device=pts.device)
    i = torch.empty((2, B, n), dtype=torch.int32, device=pts.device)
    return lambda: _lib.check(_lib.lib().dpf_nndistance_auto(B, n, pts.data_ptr(), n, pts.data_ptr(), r[0].data_ptr(), i[0].data_ptr(),
                                                             r[1].data_ptr(), i[1].data_ptr(), _lib.current_stream()), "nndistance_auto")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator(device=dev).manual_seed(3)
    exact = torch.randint(-512, 512, (4, 2048, 3), device=dev, generator=gen).float()
    k = 16
    wd, wi = tensor_op_knn(exact, k + 1)
    gd, gi, _ = knn_index(exact, exact, k, True)
    clear = (wd[:, :, 1:] != wd[:, :, :-1]).all(-1)
    same = bool((wd[:, :, :k] == gd).all()) and bool((wi[:, :, :k][clear] == gi.long()[clear]).all())
    say("# check: tensor-op route vs dpf_knn, 4 clouds of 2048 integer points, k = %d: distances %s; indices compared on %d of %d rows "
        "(the rest hold a tie among their %d smallest distances)" % (k, "and indices EQUAL" if same else "or indices DIFFER",
                                                                      int(clear.sum()), clear.numel(), k + 1))
    if not same:
        raise SystemExit("the baseline and the kernel disagree: nothing timed")

    say("# Gaussian clouds, self-search with the exclusion; ms per call, median of %d after %d warm-ups" % (args.repeats, args.warmup))
    for B, n, k in CASES:
        pts = torch.randn((B, n, 3), device=dev, generator=gen)
        res = [("by k", timed(lambda: knn_index(pts, pts, k, True), args.warmup, args.repeats))]
        for force, name in FORMS:
            if (4 << (force - 1)) >= k:
                res.append((name, timed(lambda: knn_index(pts, pts, k, True, form=force), args.warmup, args.repeats)))
        base = timed(lambda: tensor_op_knn(pts, k), args.warmup, args.repeats)
        floor = timed(nn_floor(pts), args.warmup, args.repeats)
        say("  B = %3d  n = m = %4d  k = %2d   %s   tensor ops %8.4f ms = %5.1f x the pick   dpf_nndistance_auto (k = 1, both ways) %7.4f ms"
            % (B, n, k, "   ".join("%s %8.4f ms" % r for r in res), base, base / res[0][1], floor))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
