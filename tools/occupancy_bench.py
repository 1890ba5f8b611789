"""Times dpf_occupancy_grid (csrc/occupancy.hip) at an evaluation's shapes -- by default 1 000 clouds x 2 048 points, 28^3 cells --
in both modes, with device events on the launch stream around the entry point alone (buffers allocated before, nothing copied
back inside the window), and the whole Python call (upload excluded, the counters' copy to the host included) on the host clock.
Beside them, on the same host: the numpy cube path of networks.utils.get_voxel_occ_dist, and the reference-style scikit-learn
tree query per cloud when scikit-learn is importable (it is not a dependency of the package).
Two inputs: randn * 0.27 (about a third of the points leave the fast path of the sphere grid) and the same points pulled inside
the sphere (what a normalised data set looks like).  Prints one JSON line.
usage: python tools/occupancy_bench.py [--clouds 1000] [--points 2048] [--res 28] [--reps 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpf_nets_amd._lib import lib, check, current_stream          # noqa: E402
from dpf_nets_amd.metrics import occupancy as OC                    # noqa: E402
from dpf_nets_amd.networks import utils as U                        # noqa: E402


def device_ms(x, mode, res, sph, reps):
    t = OC._tables(mode, res, sph, x.device)
    S, n, cells = x.shape[0], x.shape[1], t["cells"]
    counts = torch.empty((cells,), dtype=torch.int64, device=x.device)
    touching = torch.empty((cells,), dtype=torch.int32, device=x.device)
    flags = torch.empty((4,), dtype=torch.int32, device=x.device)
    nbytes = lib().dpf_occupancy_grid_workspace_bytes(S, n, res)
    ws = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=x.device)
    ptr = lambda k: t[k].data_ptr() if k in t else None            # noqa: E731

    def call():
        check(lib().dpf_occupancy_grid(S, n, x.data_ptr(), res, mode, ptr("edges"), ptr("centres"), ptr("kept"), ptr("kept_xyz"),
                                       cells if mode == 1 else 0, 0.5, counts.data_ptr(), touching.data_ptr(), flags.data_ptr(),
                                       ws.data_ptr(), nbytes, current_stream()), "occupancy_grid")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}


def host_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1000)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--res", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sklearn-clouds", type=int, default=20, help="clouds given to the scikit-learn query (scaled to the set)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "occupancy_bench needs a GPU (there is no fallback)"
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    wide = (rng.randn(a.clouds, a.points, 3) * 0.27).astype(np.float32)
    norm = np.linalg.norm(wide, axis=2, keepdims=True)
    inside = (wide * np.minimum(1.0, 0.45 / np.maximum(norm, 1e-9))).astype(np.float32)
    out = {"clouds": a.clouds, "points": a.points, "res": a.res, "reps": a.reps}
    for tag, c in (("randn027", wide), ("inside_sphere", inside)):
        x = torch.from_numpy(c).to(dev)
        r = {"cube_device_entry": device_ms(x, 0, a.res, False, a.reps),
             "sphere_device_entry": device_ms(x, 1, a.res, True, a.reps),
             "fullgrid_device_entry": device_ms(x, 1, a.res, False, a.reps),
             "cube_python_call": host_ms(lambda: U.get_voxel_occ_dist(x, res=a.res, warning=False), a.reps),
             "sphere_python_call": host_ms(lambda: OC.nearest_grid_counts(x, a.res, True), a.reps),
             "cube_numpy_host": host_ms(lambda: U.get_voxel_occ_dist(c, res=a.res, warning=False), max(2, a.reps // 3))}
        assert np.array_equal(U.get_voxel_occ_dist(x, res=a.res, warning=False), U.get_voxel_occ_dist(c, res=a.res, warning=False))
        try:
            from sklearn.neighbors import NearestNeighbors
            grid = OC.unit_cube_grid(a.res, True)[0]
            nn = NearestNeighbors(n_neighbors=1).fit(grid)
            k = min(a.sklearn_clouds, a.clouds)
            t0 = time.perf_counter()
            for pc in c[:k]:
                nn.kneighbors(pc)
            r["sklearn_tree_query_only"] = {"clouds_timed": k, "ms_scaled_to_set": (time.perf_counter() - t0) * 1e3 * a.clouds / k}
        except ImportError:
            r["sklearn_tree_query_only"] = "scikit-learn is not importable here"
        out[tag] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
