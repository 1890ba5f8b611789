"""Timings of the rigid-alignment kernels (csrc/align.hip) on the device -> profiles/align_forms.txt.  Not part of bench.py.

    python tools/align_bench.py [--out profiles/align_forms.txt] [--reps 20]

Every step is a child process of its own under its own time limit (a step that exceeds it is reported and the rest is skipped):
    icp          metrics.icp at 32 x 2048 x 2048 and at 50 x 2500 x 2500 (the SVR evaluation shape), 30 iterations, from an 8 degree turn
    match        one match launch alone (dpf_icp with iters = 0) beside dpf_knn at k = 1 on the same clouds
    tensor_ops   the cdist / argmin / batched svd loop on the same inputs, 30 iterations
    icp_plane    metrics.icp_plane beside metrics.icp on the same inputs, 30 iterations each, the target's normals (estimate_normals,
                 k = 16) computed once outside the timed region: median, lowest and highest of --reps runs
Times are medians of --reps runs after 3 warm-up runs, between two stream synchronisations."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((32, 2048, 2048), (50, 2500, 2500))
ITERS = 30
LIMITS = {"icp": 240, "match": 180, "tensor_ops": 300, "icp_plane": 240}


def clouds(B, n, m, seed=0):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import align_ref as A
    rng = np.random.default_rng(seed)
    src = rng.uniform(-1.0, 1.0, size=(B, n, 3)).astype(np.float32)
    dst = (src.astype(np.float64) @ A.KNOWN_R.T + A.KNOWN_T)[:, rng.permutation(n)[:m] if m <= n else np.arange(n)]
    dev = torch.device("cuda", 0)
    return torch.from_numpy(src).to(dev), torch.from_numpy(dst.astype(np.float32)).to(dev)


def sorted_ms(fn, reps):
    import torch
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times


def median_ms(fn, reps):
    times = sorted_ms(fn, reps)
    return times[len(times) // 2]


def tensor_icp(src, dst, iters):
    """the loop the kernels replace: it writes the (B, n, m) distance tensor every iteration"""
    import torch
    B = src.shape[0]
    R = torch.eye(3, device=src.device, dtype=src.dtype).expand(B, 3, 3)
    t = torch.zeros((B, 3), device=src.device, dtype=src.dtype)
    for _ in range(iters):
        moved = src @ R.transpose(1, 2) + t[:, None]
        near = torch.cdist(moved, dst).argmin(2)
        q = torch.gather(dst, 1, near[:, :, None].expand(-1, -1, 3))
        pm, qm = src.mean(1, keepdim=True), q.mean(1, keepdim=True)
        U, _, Vt = torch.linalg.svd((q - qm).transpose(1, 2) @ (src - pm))
        fix = torch.ones((B, 3), device=src.device, dtype=src.dtype)
        fix[:, 2] = torch.sign(torch.det(U) * torch.det(Vt))
        R = U @ torch.diag_embed(fix) @ Vt
        t = qm[:, 0] - (R @ pm.transpose(1, 2))[:, :, 0]
    return R, t


def step(name, reps):
    import torch
    from dpf_nets_amd.metrics import icp
    from dpf_nets_amd.metrics.align import icp_raw, icp_plane_raw
    from dpf_nets_amd.metrics.knn import knn_index
    for B, n, m in SHAPES:
        src, dst = clouds(B, n, m)
        shape = "%d x %d x %d" % (B, n, m)
        if name == "icp":
            T, info = icp(src, dst, iters=ITERS, return_info=True)
            its = info.iterations.cpu().numpy()
            ms = median_ms(lambda: icp_raw(src, dst, ITERS), reps)
            print("icp          %-16s %8.3f ms  (%d iterations asked; the slots converged after %d..%d; final rmse %.2e)"
                  % (shape, ms, ITERS, its.min(), its.max(), float(info.rmse[:, -1].max())))
        elif name == "match":
            a = median_ms(lambda: icp_raw(src, dst, 0), reps)
            b = median_ms(lambda: knn_index(src, dst, 1), reps)
            print("match        %-16s %8.3f ms  one match + its reduction (dpf_icp, iters = 0);  dpf_knn k = 1: %8.3f ms" % (shape, a, b))
        elif name == "tensor_ops":
            ms = median_ms(lambda: tensor_icp(src, dst, ITERS), max(3, reps // 4))
            print("tensor_ops   %-16s %8.3f ms  cdist / argmin / batched svd, %d iterations, fp32, no early stop" % (shape, ms, ITERS))
        elif name == "icp_plane":
            from dpf_nets_amd.metrics import icp_plane, estimate_normals
            nrm = estimate_normals(dst, 16, double=True)[0]
            T, info = icp_plane(src, dst, nrm, iters=ITERS, return_info=True)
            its = info.iterations.cpu().numpy()
            a = sorted_ms(lambda: icp_plane_raw(src, dst, nrm, ITERS), reps)
            b = sorted_ms(lambda: icp_raw(src, dst, ITERS), reps)
            print("icp_plane    %-16s %8.3f ms  (low %.3f, high %.3f; %d iterations asked, tol 1e-7; the slots stopped after %d..%d; final "
                  "rmse_plane %.2e);  icp on the same inputs: %8.3f ms (low %.3f, high %.3f)"
                  % (shape, a[len(a) // 2], a[0], a[-1], ITERS, its.min(), its.max(), float(info.rmse_plane[:, -1].max()),
                     b[len(b) // 2], b[0], b[-1]))
        else:
            raise SystemExit("unknown step " + name)
    print("device: " + torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_forms.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", default=None)
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    lines = ["rigid alignment (csrc/align.hip): tools/align_bench.py, medians of %d runs" % args.reps]
    for name in ("icp", "match", "tensor_ops", "icp_plane"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)], capture_output=True,
                               text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            lines.append("%s: exceeded its limit of %d s; the remaining steps were not run" % (name, LIMITS[name]))
            break
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append("%s: exit status %d; the remaining steps were not run\n%s" % (name, r.returncode, r.stderr[-2000:]))
            break
    text = "\n".join(dict.fromkeys(lines)) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if "not run" not in text else 1


if __name__ == "__main__":
    sys.exit(main())
