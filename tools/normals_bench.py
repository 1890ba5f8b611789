"""Timing of dpf_normals (csrc/normals.hip) beside the dpf_knn launch in front of it, and the route a user took before it existed, on
the same GPU in the same process: knn_gather -> a (B, n, k, 3) float64 tensor -> centred covariance -> torch.linalg.eigh on B * n
3 x 3 matrices.  Both routes start from the same index table.  Not part of bench.py.

    python tools/normals_bench.py [--out FILE]

Events on the launch stream, warm-up first, the median of the timed repeats (tools/point_mesh_bench.py: timed).  Before anything is
timed the tensor-op route is compared with the kernel on Gaussian clouds, so that the comparison is like for like: every eigenvalue
within 2^-46 lambda_max, and |v x u_0| (lambda_1 - lambda_0) / lambda_max <= 2^-46 where the gap exceeds 2^-20 lambda_max (the
bounds of tests/test_gpu_normals.py; the two covariances differ by the order of their additions, a few units of 2^-52)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from point_mesh_bench import timed                                                          # noqa: E402
from dpf_nets_amd.metrics.knn import knn_index, knn_gather                                  # noqa: E402
from dpf_nets_amd.metrics.normals import normals_from_index                                 # noqa: E402

CASES = ((32, 2048, 16), (256, 512, 16), (4, 8192, 32))
BOUND = 2.0 ** -46


def tensor_op_normals(pts, index):
    """(B, n, 3) fp32, (B, n, k) int64 -> (eigenvalues ascending (B, n, 3), the smallest one's vector (B, n, 3)), float64"""
    nb = knn_gather(pts, index).double()                                                    # (B, n, k, 3)
    d = nb - nb.mean(2, keepdim=True)
    lam, vec = torch.linalg.eigh(d.transpose(2, 3) @ d)
    return lam, vec[..., 0]


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
    pts = torch.randn((4, 2048, 3), device=dev, generator=gen)
    k = 16
    index = knn_index(pts, pts, k, False)[1]
    normal, lam, flag = normals_from_index(pts, index)
    wl, wv = tensor_op_normals(pts, index.long())
    lmax = wl[..., 2]
    ev = ((lam - wl).abs().max(-1)[0] / lmax).max().item()
    gap = wl[..., 1] - wl[..., 0]
    clear = gap > 2.0 ** -20 * lmax
    angle = (torch.linalg.cross(normal, wv).norm(dim=-1) * gap / lmax)[clear].max().item()
    ok = int(flag.sum()) == 0 and ev <= BOUND and angle <= BOUND
    say("# check: tensor-op route vs dpf_normals, 4 clouds of 2048 Gaussian points, k = %d: eigenvalues within %.2f x 2^-52 lambda_max, "
        "sin(angle) * gap / lambda_max %.2f x 2^-52 on %d of %d points (bound: 64 x 2^-52 each): %s"
        % (k, ev * 2.0 ** 52, angle * 2.0 ** 52, int(clear.sum()), clear.numel(), "AGREE" if ok else "DISAGREE"))
    if not ok:
        raise SystemExit("the baseline and the kernel disagree: nothing timed")

    say("# Gaussian clouds, the k nearest points of the cloud itself (the point included); ms per call, median of %d after %d warm-ups"
        % (args.repeats, args.warmup))
    for B, n, k in CASES:
        pts = torch.randn((B, n, 3), device=dev, generator=gen)
        index = knn_index(pts, pts, k, False)[1]
        wide = index.long()
        t_knn = timed(lambda: knn_index(pts, pts, k, False), args.warmup, args.repeats)
        t_nrm = timed(lambda: normals_from_index(pts, index), args.warmup, args.repeats)
        t_both = timed(lambda: normals_from_index(pts, knn_index(pts, pts, k, False)[1]), args.warmup, args.repeats)
        t_ops = timed(lambda: tensor_op_normals(pts, wide), args.warmup, args.repeats)
        say("  B = %3d  n = %4d  k = %2d   dpf_knn %8.4f ms   dpf_normals %8.4f ms (%4.2f x dpf_knn)   both %8.4f ms   "
            "tensor ops from the same index %9.4f ms = %6.1f x dpf_normals"
            % (B, n, k, t_knn, t_nrm, t_nrm / t_knn, t_both, t_ops, t_ops / t_nrm))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
