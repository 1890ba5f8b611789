"""Times the device-side mesh sampler (csrc/mesh_sample.hip, dpf_nets_amd/datasets) at the reference configs' batch: one
sample_clouds call of B = 64 slots x cloud_size 2048 with the eval cloud (4096 samples per slot), drawn path, for synthetic
meshes of 2 000, 20 000 and 200 000 faces -- device events around the call (variates + sampling kernels, outputs allocated
inside), and the same call on the host clock up to a synchronisation.  Also the one-time MeshStore construction (upload, CDF
build, the flag read-back) on the host clock and the CDF build's launches alone between device events.  Beside them, on the
same machine's CPU, one core: the reference-style numpy sampler per item (lib/datasets/cloud_sampling.py restated: areas,
np.random.choice, the fp32 point formula, the split), scaled to a batch of 64 and to the reference's 8 loader workers.
Writes a text table (default profiles/mesh_sampler.txt) and prints one JSON line.
usage: python tools/mesh_sampler_bench.py [--batch 64] [--cloud-size 2048] [--meshes 16] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dpf_nets_amd import datasets as DS                               # noqa: E402
from dpf_nets_amd._lib import lib, check, current_stream             # noqa: E402


def soup(F, seed):
    rng = np.random.RandomState(seed)
    V = F // 2 + 3
    v = (rng.random_sample((V, 3)) - 0.5).astype(np.float32)
    i0 = rng.randint(0, V, size=F)
    return v, np.stack([i0, (i0 + rng.randint(1, 4, size=F)) % V, (i0 + rng.randint(4, 8, size=F)) % V], axis=1).astype(np.uint32)


def numpy_sample_cloud(vertices_c, faces_vc, size):
    polygons = vertices_c[faces_vc]
    cross = np.cross(polygons[:, 2] - polygons[:, 0], polygons[:, 2] - polygons[:, 1])
    areas = np.sqrt((cross ** 2).sum(1)) / 2.0
    k = np.random.choice(np.arange(len(polygons)), size=2 * size, p=areas / areas.sum())
    sp = polygons[k]
    s1 = np.random.random((2 * size, 1)).astype(np.float32)
    s2 = np.random.random((2 * size, 1)).astype(np.float32)
    cond = (s1 + s2) > 1.
    s1[cond] = 1. - s1[cond]
    s2[cond] = 1. - s2[cond]
    cloud = (sp[:, 0] + s1 * (sp[:, 1] - sp[:, 0]) + s2 * (sp[:, 2] - sp[:, 0])).astype(np.float32)
    return cloud[::2].T, cloud[1::2].copy().T


def stats(times):
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cloud-size", type=int, default=2048)
    ap.add_argument("--meshes", type=int, default=16, help="distinct meshes in the store (the batch cycles through them)")
    ap.add_argument("--faces", type=int, nargs="+", default=[2000, 20000, 200000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sampler.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_sampler_bench needs a GPU (there is no fallback)"
    dev = torch.device("cuda", 0)
    B, N = a.batch, a.cloud_size
    rows, out = [], {"batch": B, "cloud_size": N, "eval_cloud": True, "meshes": a.meshes, "reps": a.reps, "faces": {}}
    for F in a.faces:
        meshes = [soup(F, 1000 + i) for i in range(a.meshes)]
        vb = np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.uint64)
        fb = np.cumsum([0] + [len(f) for _, f in meshes]).astype(np.uint64)
        vertices, faces = np.concatenate([v for v, _ in meshes]), np.concatenate([f for _, f in meshes])
        DS.MeshStore(vertices, vb, faces, fb, device=dev)                                   # (first touch: library load, allocator)
        build = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = DS.MeshStore(vertices, vb, faces, fb, device=dev)
            build.append((time.perf_counter() - t0) * 1e3)
        n_tiles = int(store.tile_bounds[-1])
        nbytes = lib().dpf_mesh_cdf_workspace_bytes(store.num_meshes, n_tiles)
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
        cdf, flags, kernels = torch.empty_like(store.cdf), torch.empty_like(store.flags), []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(lib().dpf_mesh_cdf_build(store.num_meshes, store.vertices.data_ptr(), store.vertex_bounds.data_ptr(),
                                           store.faces.data_ptr(), store.face_bounds.data_ptr(), store.tile_bounds.data_ptr(), n_tiles,
                                           cdf.data_ptr(), flags.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "mesh_cdf_build")
            e1.record()
            e1.synchronize()
            kernels.append(e0.elapsed_time(e1))
        assert torch.equal(cdf, store.cdf)
        idx = np.arange(B) % a.meshes
        for step in range(3):
            DS.sample_clouds(store, idx, N, return_eval_cloud=True, seed=1, step=step)
        torch.cuda.synchronize()
        device, host = [], []
        for step in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            batch = DS.sample_clouds(store, idx, N, return_eval_cloud=True, seed=1, step=10 + step)
            e1.record()
            e1.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            device.append(e0.elapsed_time(e1))
        assert bool(torch.isfinite(batch["cloud"]).all()) and batch["eval_cloud"].shape == (B, 3, N)
        cpu = []
        for i in range(max(3, min(8, a.meshes))):
            v, f = meshes[i % a.meshes]
            t0 = time.perf_counter()
            numpy_sample_cloud(v, f, N)
            cpu.append((time.perf_counter() - t0) * 1e3)
        r = {"sample_clouds_device": stats(device), "sample_clouds_host_clock": stats(host), "store_construction_host_clock": stats(build),
             "cdf_build_device": stats(kernels), "numpy_sample_cloud_per_item": stats(cpu)}
        r["clouds_per_second_device"] = B / (r["sample_clouds_device"]["median_ms"] * 1e-3)
        r["numpy_batch_ms_1_core"] = B * r["numpy_sample_cloud_per_item"]["median_ms"]
        r["numpy_batch_ms_8_workers"] = r["numpy_batch_ms_1_core"] / 8
        out["faces"][str(F)] = r
        rows.append("%9d  %12.4f  %12.4f  %14.0f  %12.3f  %12.3f  %12.3f  %12.2f" % (
            F, r["sample_clouds_device"]["median_ms"], r["sample_clouds_host_clock"]["median_ms"], r["clouds_per_second_device"],
            r["cdf_build_device"]["median_ms"], r["store_construction_host_clock"]["median_ms"],
            r["numpy_sample_cloud_per_item"]["median_ms"], r["numpy_batch_ms_8_workers"]))
    head = ["mesh sampler: one sample_clouds call, B = %d slots x cloud_size %d with the eval cloud (%d samples per slot), drawn path;"
            % (B, N, 2 * N),
            "store of %d synthetic meshes per row; medians of %d calls (3 for the store construction); %s"
            % (a.meshes, a.reps, torch.cuda.get_device_name(0)),
            "numpy columns: the reference-style sampler on this machine's CPU, one core per item; batch = %d items / 8 workers" % B,
            "",
            "%9s  %12s  %12s  %14s  %12s  %12s  %12s  %12s" % ("faces", "batch ms", "batch ms", "clouds/s", "CDF build ms", "store ms",
                                                               "numpy ms", "numpy batch"),
            "%9s  %12s  %12s  %14s  %12s  %12s  %12s  %12s" % ("per mesh", "(device)", "(host clock)", "(device)", "(device)", "(host clock)",
                                                               "per item", "ms, 8 workers")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
