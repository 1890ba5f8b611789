"""Device side of the two occupancy-grid Jensen-Shannon metrics: dpf_occupancy_grid (csrc/occupancy.hip) over (S, n, 3)
clouds, with the tables the kernel compares against built ON THE HOST by the reference's own numpy expressions.

  cube_grid_counts    -- half-open cube bins of lib/networks/utils.py:45-80 (mode 0)
  nearest_grid_counts -- nearest centre of the (optionally sphere-clipped) grid of lib/metrics/evaluation_metrics.py:206-280
                         (mode 1)

Both return integer numpy arrays; only those (and a four-word flag record) come back from the device."""
import numpy as np
import torch

from .._lib import lib, check, current_stream

_TABLES = {}


def max_resolution():
    return int(lib().dpf_occupancy_max_res())


def grid_centres(resolution):
    """The per-axis centre values of unit_cube_grid_point_cloud, `i * spacing - 0.5` in double stored to float32, and spacing."""
    spacing = 1.0 / float(resolution - 1)
    return (np.arange(resolution) * spacing - 0.5).astype(np.float32), spacing


def unit_cube_grid(resolution, clip_sphere=False):
    """lib/metrics/evaluation_metrics.py:206-224 without its three Python loops: the same float32 array and spacing."""
    from numpy.linalg import norm
    axis, spacing = grid_centres(resolution)
    grid = np.ndarray((resolution, resolution, resolution, 3), np.float32)
    grid[..., 0] = axis[:, None, None]
    grid[..., 1] = axis[None, :, None]
    grid[..., 2] = axis[None, None, :]
    if clip_sphere:
        grid = grid.reshape(-1, 3)
        grid = grid[norm(grid, axis=1) <= 0.5]
    return grid, spacing


def _check_resolution(resolution, lowest):
    resolution = int(resolution)
    if resolution < lowest or resolution > max_resolution():
        raise ValueError("occupancy grid: resolution %d is outside %d..%d (the per-cloud presence bitmap of resolution^3 bits is "
                         "held in LDS)" % (resolution, lowest, max_resolution()))
    return resolution


def _tables(mode, resolution, in_sphere, device):
    key = (mode, resolution, bool(in_sphere), device)
    t = _TABLES.get(key)
    if t is None:
        if mode == 0:
            edges = -0.5 + np.arange(resolution + 1) * (1. / resolution)
            t = {"edges": torch.from_numpy(edges).to(device), "cells": resolution ** 3}
        else:
            from numpy.linalg import norm
            axis, _ = grid_centres(resolution)
            full = unit_cube_grid(resolution, False)[0].reshape(-1, 3)
            t = {"centres": torch.from_numpy(axis).to(device)}
            if in_sphere:
                keep = norm(full, axis=1) <= 0.5
                kept = np.full(len(full), -1, np.int32)
                kept[keep] = np.arange(int(keep.sum()), dtype=np.int32)
                t["kept"] = torch.from_numpy(kept).to(device)
                full = full[keep]
            t["kept_xyz"] = torch.from_numpy(np.ascontiguousarray(full)).to(device)
            t["cells"] = len(full)
        _TABLES[key] = t
    return t


def _as_device_clouds(clouds, what):
    """(S, n, 3) float32 contiguous CUDA tensor: a CUDA tensor is read in place, a numpy array goes to the current device."""
    if isinstance(clouds, torch.Tensor):
        if not clouds.is_cuda:
            raise RuntimeError("%s: a tensor must be a CUDA tensor (pass host data as a numpy array)" % what)
        if clouds.dtype != torch.float32:
            raise RuntimeError("%s needs float32 clouds, got %s" % (what, clouds.dtype))
        x = clouds.detach().contiguous()
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(clouds), dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s needs (S, n, 3) clouds with S, n >= 1, got %s" % (what, tuple(x.shape)))
    return x


def _run(x, mode, resolution, t, warn_bound):
    dev, S, n, cells = x.device, x.shape[0], x.shape[1], t["cells"]
    counts = torch.empty((cells,), dtype=torch.int64, device=dev)
    touching = torch.empty((cells,), dtype=torch.int32, device=dev)
    flags = torch.empty((4,), dtype=torch.int32, device=dev)
    nbytes = lib().dpf_occupancy_grid_workspace_bytes(S, n, resolution)
    ws = torch.empty((max(nbytes, 4),), dtype=torch.uint8, device=dev)
    ptr = lambda name: t[name].data_ptr() if name in t else None                                    # noqa: E731
    with torch.cuda.device(dev):
        rc = lib().dpf_occupancy_grid(S, n, x.data_ptr(), resolution, mode, ptr("edges"), ptr("centres"), ptr("kept"), ptr("kept_xyz"),
                                      cells if mode == 1 else 0, float(warn_bound), counts.data_ptr(), touching.data_ptr(),
                                      flags.data_ptr(), ws.data_ptr(), nbytes, current_stream())
    if rc == -2:
        raise ValueError("occupancy grid: resolution %d is not supported" % resolution)
    check(rc, "occupancy_grid")
    return counts.cpu().numpy(), touching.cpu().numpy(), flags.cpu().numpy()


def cube_grid_counts(clouds, resolution, warn_bound=0.5):
    """counts (resolution^3,) int64 of the points per half-open voxel of [-0.5, 0.5)^3, the number of NaN coordinates, and
    whether some |coordinate| exceeds warn_bound."""
    resolution = _check_resolution(resolution, 1)
    x = _as_device_clouds(clouds, "cube_grid_counts")
    counts, _, flags = _run(x, 0, resolution, _tables(0, resolution, False, x.device), np.float32(warn_bound))
    return counts, int(flags[1]), bool(flags[2])


def nearest_grid_counts(clouds, resolution, in_sphere=False):
    """(counts, clouds_touching) over the kept cells of the grid, in the order of unit_cube_grid(resolution, in_sphere): every
    point goes to its nearest kept centre.  A NaN or infinite point raises ValueError."""
    resolution = _check_resolution(resolution, 2)
    x = _as_device_clouds(clouds, "nearest_grid_counts")
    counts, touching, flags = _run(x, 1, resolution, _tables(1, resolution, in_sphere, x.device), np.float32(np.inf))
    if flags[0]:
        raise ValueError("occupancy grid: %d points have a NaN or infinite coordinate" % int(flags[0]))
    return counts, touching
