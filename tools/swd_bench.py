"""Timing of the sliced-Wasserstein kernels (csrc/swd.hip): every form of the per-(cloud, direction) sort, the (N1, N2) matrix at
n = 2048, L = 128, and beside them what a user would do without them -- the same result from tensor ops on the same device
(`clouds @ dirs.T`, `torch.sort`, subtract, square, mean) -- and pairwise_EMD_exact's time for a matrix of the same shape.  Not part
of bench.py.

    python tools/swd_bench.py [--out profiles/swd_forms.txt] [--emd 256]

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  Before anything is
timed the tensor-op matrix is compared with pairwise_SWD's on a small case.
Sort: us per sort = ms per dpf_swd_tables call / (B * L) with 8192 sorts in flight (every CU busy), and the latency of one sort
alone.  Matrix: ms of the matrix kernel over tables already built, ms of the table builds, and pairwise_SWD end to end.
--emd N: pairwise_EMD_exact on an N x N matrix (one run; the auction's time does not depend on the matrix's shape but on its pairs,
so larger matrices are scaled by their pair count and marked as such); 0 skips it."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd.metrics import sliced as S                                                # noqa: E402

FORMS = ((0, "by size"), (1, "1 wave"), (2, "4 waves"), (3, "16 waves"))
SORT_SIZES = (64, 256, 512, 1024, 2048, 4096, 8192)
SORTS_IN_FLIGHT = 8192
N_POINTS, N_DIRS = 2048, 128
MATRICES = (256, 1000)


def tensor_op_tables(clouds, dirs):
    return torch.sort((clouds @ dirs.t()).transpose(1, 2), dim=2)[0]                        # (N, L, n)


def tensor_op_matrix(c1, c2, dirs):
    """(N1, N2) fp32 from tensor ops alone: project, sort, then a row of the matrix at a time (the (N1, N2, L, n) block of
    differences would not fit)"""
    s1, s2 = tensor_op_tables(c1, dirs), tensor_op_tables(c2, dirs)
    return torch.stack([((s1[i][None] - s2) ** 2).mean((1, 2)) for i in range(s1.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--emd", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator(device=dev).manual_seed(3)
    cloud = torch.randn((2 * max(MATRICES), max(SORT_SIZES), 3), device=dev, generator=gen)
    dirs = S.sliced_directions(N_DIRS, 0, dev)

    a, b = cloud[:20, :500].contiguous(), cloud[20:50, :500].contiguous()
    got, want = S.pairwise_SWD(a, b, dirs[:16]), tensor_op_matrix(a, b, dirs[:16])
    err = float(((got - want).abs() / want).max())
    say("# check: tensor ops vs pairwise_SWD, 20 x 30 clouds of 500 points, 16 directions: largest relative difference %.2e" % err)
    if not err < 1e-4:
        raise SystemExit("the baseline and the kernels disagree: nothing timed")

    say("# the sort by form: us per (cloud, direction) sort with %d sorts in flight | us for one sort alone; median of %d after %d warm-ups"
        % (SORTS_IN_FLIGHT, args.repeats, args.warmup))
    for n in SORT_SIZES:
        many, one = cloud[:SORTS_IN_FLIGHT // N_DIRS, :n].contiguous(), cloud[:1, :n].contiguous()
        row = []
        for force, name in FORMS:
            try:
                S.sliced_tables(one, dirs[:1], form=force)
            except RuntimeError:
                continue                                                                    # (forced past its limit)
            t_many = timed(lambda: S.sliced_tables(many, dirs, form=force), args.warmup, args.repeats)
            t_one = timed(lambda: S.sliced_tables(one, dirs[:1], form=force), args.warmup, args.repeats)
            row.append("%s %7.3f us | %6.1f us" % (name, t_many * 1e3 / SORTS_IN_FLIGHT, t_one * 1e3))
        t_ops = timed(lambda: tensor_op_tables(many, dirs), args.warmup, args.repeats)
        say("  n = %4d   %s   tensor ops (matmul + torch.sort) %7.3f us" % (n, "   ".join(row), t_ops * 1e3 / SORTS_IN_FLIGHT))

    say("# the matrix at n = %d, L = %d: ms; the tensor-op path once after one warm-up at the smaller shape" % (N_POINTS, N_DIRS))
    pairs_per_ms = None
    for N in MATRICES:
        c1, c2 = cloud[:N, :N_POINTS].contiguous(), cloud[N:2 * N, :N_POINTS].contiguous()
        chunk = max(1, min(N_DIRS, S.TABLE_BUDGET_BYTES // (2 * N * N_POINTS * 4)))
        d = dirs[:chunk].contiguous()
        t_tab = timed(lambda: (S.sliced_tables(c1, d), S.sliced_tables(c2, d)), args.warmup, args.repeats)
        (s1, st1), (s2, st2) = S.sliced_tables(c1, d), S.sliced_tables(c2, d)
        t_mat = timed(lambda: S.sliced_matrix_sums(s1, st1, s2, st2), args.warmup, args.repeats)
        del s1, s2
        t_all = timed(lambda: S.pairwise_SWD(c1, c2, dirs), 1, 3)
        t_ops = timed(lambda: tensor_op_matrix(c1, c2, dirs), 1 if N == MATRICES[0] else 0, 1)
        elems = float(N) * N * chunk * N_POINTS
        say("  %4d x %4d   tables of %3d directions (both sets) %8.3f ms   matrix kernel over them %8.3f ms = %.2f T pair-elements/s   "
            "pairwise_SWD, all %d directions %9.3f ms   tensor ops %10.1f ms = %6.1f x pairwise_SWD"
            % (N, N, chunk, t_tab, t_mat, elems / t_mat * 1e-9, N_DIRS, t_all, t_ops, t_ops / t_all))
        if args.emd > 0:
            from dpf_nets_amd.networks.utils import pairwise_EMD_exact
            if pairs_per_ms is None:
                e1, e2 = c1[:args.emd], c2[:args.emd]
                with torch.no_grad():
                    t_emd = timed(lambda: pairwise_EMD_exact(e1, e2), 0, 1)
                pairs_per_ms = args.emd * args.emd / t_emd
                say("  pairwise_EMD_exact, %d x %d at n = %d, one run: %.1f ms = %.0f pairs/s" % (args.emd, args.emd, N_POINTS, t_emd,
                                                                                                   pairs_per_ms * 1e3))
            t_emd_N = N * N / pairs_per_ms
            say("  %4d x %4d   pairwise_EMD_exact %s %.0f ms = %.0f x pairwise_SWD"
                % (N, N, "measured" if N == args.emd else "SCALED by pairs from the run above:", t_emd_N, t_emd_N / t_all))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
