"""Training clouds sampled from triangle meshes ON THE DEVICE (csrc/mesh_sample.hip): the collated batch the reference's
DataLoader builds on the host per item -- lib/datasets/datasets.py:69-106 = read a mesh, sample_cloud
(lib/datasets/cloud_sampling.py:4-32), split into cloud / eval_cloud, ComposeCloudTransformation
(lib/datasets/cloud_transformations.py) -- written where the model reads it.

  MeshStore       -- the meshes of one part of meshes.h5 on the device, with a per-mesh cumulative area distribution
  sample_clouds   -- one batch: {'cloud', 'eval_cloud'?, 'orig_c'?, 'orig_s'?, 'faces'?} as CUDA tensors
  host_variates   -- the uniforms a (seed, step) call draws on the device, as numpy arrays, bit for bit
  CloudTransform  -- the reference's cloud_* config keys: four go into the sampling kernel, noise and centring are tensor ops

The arithmetic is the reference's (fp32, every operation rounded on its own); the contract is in include/dpf_hip.h."""
import numpy as np
import torch

from .._lib import lib, check, current_stream

BAD_INDEX, BAD_AREA, BAD_TOTAL = 1, 2, 4            # the flag bits of dpf_mesh_cdf_build
_M64 = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _mix(x):
    """splitmix64 on uint64 arrays (as dpf_nets_amd/synthetic.py:_splitmix64; callers silence the wrap-around warnings)."""
    x = x + _GOLDEN
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def host_variates(seed, step, B, S):
    """(u, s1, s2) of a sample_clouds(seed=seed, step=step) call with B slots of S samples: u (B, S) float64 in [0, 1) with 53
    random bits, s1 / s2 (B, S) float32 = the double uniform rounded to float32.  Keyed by (seed, step, slot, sample, stream)."""
    B, S = int(B), int(S)
    if B < 1 or S < 1:
        raise ValueError("host_variates needs B, S >= 1, got %d, %d" % (B, S))
    with np.errstate(over="ignore"):
        base = _mix(_mix(np.array([int(seed) & _M64], np.uint64)) ^ np.uint64(int(step) & _M64))
        slot = _mix(base ^ np.arange(B, dtype=np.uint64))[:, None]
        i4 = np.arange(S, dtype=np.uint64)[None, :] * np.uint64(4)
        d = [(_mix(slot ^ (i4 + np.uint64(k))) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) for k in range(3)]
    return d[0], d[1].astype(np.float32), d[2].astype(np.float32)


def _bounds(b, total, what):
    b = np.asarray(b)
    if b.ndim != 1 or b.size < 2 or b.dtype.kind not in "iu":
        raise ValueError("MeshStore: %s must be a 1-D integer array of M + 1 entries" % what)
    b = b.astype(np.int64)
    if b[0] != 0 or b[-1] != total or np.any(np.diff(b) < 0):
        raise ValueError("MeshStore: %s must start at 0, never decrease and end at %d (the rows it indexes)" % (what, total))
    return b


class MeshStore(object):
    """The meshes of meshes.h5 on the device: `vertices` (sum V, 3) float32 (`<part>_vertices_c`), `faces` (sum F, 3) with vertex
    indices local to their mesh (`<part>_faces_vc`), and the two bounds arrays of M + 1 entries, as numpy arrays; optionally
    `orig_c` (M, 3) / `orig_s` (M,).  Construction uploads them, builds every mesh's cumulative area distribution and reads the
    validation flags back (the store's one synchronisation).  A bad mesh raises -- IndexError for a face index outside the
    mesh's vertices, ValueError for a non-finite area or a total area of zero -- unless strict=False, which records it in
    `store.bad` ({mesh: flag bits}); sample_clouds refuses to sample such a mesh."""

    def __init__(self, vertices, vertex_bounds, faces, face_bounds, orig_c=None, orig_s=None, device=None, strict=True):
        for name, x in (("vertices", vertices), ("faces", faces)):
            if isinstance(x, torch.Tensor):
                raise TypeError("MeshStore: %s must be a numpy array as the h5 file holds it, not a tensor" % name)
        vertices, faces = np.asarray(vertices), np.asarray(faces)
        if vertices.ndim != 2 or vertices.shape[1] != 3 or vertices.dtype.kind != "f":
            raise ValueError("MeshStore: vertices must be a (sum V, 3) floating array, got %s %s" % (vertices.dtype, vertices.shape))
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
            raise ValueError("MeshStore: faces must be a (sum F, 3) integer array, got %s %s" % (faces.dtype, faces.shape))
        vb = _bounds(vertex_bounds, len(vertices), "vertex_bounds")
        fb = _bounds(face_bounds, len(faces), "face_bounds")
        if len(vb) != len(fb):
            raise ValueError("MeshStore: vertex_bounds and face_bounds describe %d and %d meshes" % (len(vb) - 1, len(fb) - 1))
        nf = np.diff(fb)
        if np.any(nf < 1) or np.any(nf >= 2 ** 31):
            raise ValueError("MeshStore: every mesh needs between 1 and 2^31 - 1 faces (mesh %d has %d)"
                             % (int(np.flatnonzero((nf < 1) | (nf >= 2 ** 31))[0]), int(nf[(nf < 1) | (nf >= 2 ** 31)][0])))
        if faces.dtype != np.uint32:
            if faces.size and (faces.min() < 0 or faces.max() >= 2 ** 32):
                raise IndexError("MeshStore: a face index is negative or does not fit 32 bits")
            faces = faces.astype(np.uint32)
        self.num_meshes = M = len(fb) - 1
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MeshStore: the store lives on a GPU, got device %s" % self.device)
        self.tile = int(lib().dpf_mesh_cdf_tile())
        tb = np.concatenate([[0], np.cumsum((nf + self.tile - 1) // self.tile)]).astype(np.int64)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)        # noqa: E731
        self.face_counts = nf
        self.vertices, self.faces = up(vertices, np.float32), up(faces.view(np.int32), np.int32)
        self.vertex_bounds, self.face_bounds, self.tile_bounds = up(vb, np.int64), up(fb, np.int64), up(tb, np.int64)
        self.orig_c = self.orig_s = None
        if orig_c is not None:
            oc = np.asarray(orig_c, dtype=np.float32)
            if oc.shape != (M, 3):
                raise ValueError("MeshStore: orig_c must be (%d, 3), got %s" % (M, oc.shape))
            self.orig_c = up(oc, np.float32)
        if orig_s is not None:
            os_ = np.asarray(orig_s, dtype=np.float32).reshape(-1)
            if os_.shape != (M,):
                raise ValueError("MeshStore: orig_s must hold %d scales, got %s" % (M, np.shape(orig_s)))
            self.orig_s = up(os_, np.float32)
        self.cdf = torch.empty((len(faces),), dtype=torch.float64, device=self.device)
        self.flags = torch.empty((M,), dtype=torch.int32, device=self.device)
        n_tiles = int(tb[-1])
        nbytes = lib().dpf_mesh_cdf_workspace_bytes(M, n_tiles)
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().dpf_mesh_cdf_build(*self.abi_args()[:5], self.tile_bounds.data_ptr(), n_tiles, self.cdf.data_ptr(),
                                           self.flags.data_ptr(), ws.data_ptr(), nbytes, current_stream()), "mesh_cdf_build")
            flags = self.flags.cpu().numpy()                                                          # the one synchronisation
        self.bad = {int(m): int(flags[m]) for m in np.flatnonzero(flags)}
        if strict and self.bad:
            raise self._error(min(self.bad))

    def _error(self, m):
        bits = self.bad[m]
        more = "" if len(self.bad) == 1 else " (%d bad meshes in all: %s)" % (len(self.bad), sorted(self.bad)[:8])
        if bits & BAD_INDEX:
            return IndexError("MeshStore: mesh %d has a face index outside its %d vertices%s"
                              % (m, int(self.vertex_bounds[m + 1] - self.vertex_bounds[m]), more))
        if bits & BAD_AREA:
            return ValueError("MeshStore: mesh %d has a face of non-finite area (a NaN or infinite vertex)%s" % (m, more))
        return ValueError("MeshStore: mesh %d has a total area of zero: its area distribution does not exist%s" % (m, more))

    def __len__(self):
        return self.num_meshes

    def abi_args(self):
        """The store as the C ABI takes it: (M, vertices, vertex_bounds, faces, face_bounds, flags).  The entries that take no
        flags here (dpf_mesh_cdf_build, dpf_mesh_sample) pass the leading five."""
        return (self.num_meshes, self.vertices.data_ptr(), self.vertex_bounds.data_ptr(), self.faces.data_ptr(),
                self.face_bounds.data_ptr(), self.flags.data_ptr())


class CloudTransform(object):
    """ComposeCloudTransformation's config keys (lib/datasets/cloud_transformations.py:67-83), in its order: rescale / recentre
    to the original frame, translate, scale -- fused into the sampling kernel -- then noise and centring, which run as tensor
    ops on the batch (`tail`).  Unknown keys are ignored, as the reference's **kwargs do."""

    def __init__(self, **kwargs):
        self.rescale = bool(kwargs.get("cloud_rescale2orig"))
        self.recenter = bool(kwargs.get("cloud_recenter2orig"))
        self.translate = bool(kwargs.get("cloud_translate"))
        self.scale = bool(kwargs.get("cloud_scale"))
        self.noise = bool(kwargs.get("cloud_noise"))
        self.center = bool(kwargs.get("cloud_center"))
        self.shift = np.zeros(3, np.float32)
        if self.translate:
            self.shift = np.array(kwargs["cloud_translate_shift"], dtype=np.float32).reshape(-1)
            if self.shift.shape != (3,):
                raise ValueError("CloudTransform: cloud_translate_shift must hold 3 values, got %s" % (kwargs["cloud_translate_shift"],))
        self.scale_value = np.float32(kwargs["cloud_scale_scale"]) if self.scale else np.float32(1.0)
        self.noise_scale = np.float32(kwargs["cloud_noise_scale"]) if self.noise else np.float32(0.0)

    def order(self):
        """The names of the active steps in the order they are applied."""
        on = (("rescale2orig", self.rescale), ("recenter2orig", self.recenter), ("translate", self.translate),
              ("scale", self.scale), ("noise", self.noise), ("center", self.center))
        return [name for name, flag in on if flag]

    def fused(self):
        """(mask, shift, scale) of the part the kernel applies: bits 1 rescale, 2 recentre, 4 translate, 8 scale."""
        return (int(self.rescale) | int(self.recenter) << 1 | int(self.translate) << 2 | int(self.scale) << 3,
                self.shift, self.scale_value)

    def tail(self, sample, generator=None):
        """Noise (torch.randn on the clouds' device, cloud first, then eval_cloud) and centring (minus the mean over the points),
        in place on sample['cloud'] / sample['eval_cloud']."""
        names = [k for k in ("cloud", "eval_cloud") if k in sample]
        if self.noise:
            for k in names:
                x = sample[k]
                x += torch.randn(x.shape, dtype=x.dtype, device=x.device, generator=generator) * float(self.noise_scale)
        if self.center:
            for k in names:
                sample[k] -= sample[k].mean(dim=2, keepdim=True)
        return sample


def _variate(x, name, dtype, B, S, device):
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("sample_clouds: variates[%s] is a CPU tensor; pass a CUDA tensor or a numpy array" % name)
        if x.device != device:
            raise RuntimeError("sample_clouds: variates[%s] is on %s, the store on %s" % (name, x.device, device))
        if x.dtype != dtype:
            raise TypeError("sample_clouds: variates[%s] must be %s, got %s" % (name, dtype, x.dtype))
        x = x.detach().contiguous()
    else:
        x = np.asarray(x)
        want = np.float64 if dtype == torch.float64 else np.float32
        if x.dtype != want:
            raise TypeError("sample_clouds: variates[%s] must be %s, got %s" % (name, np.dtype(want), x.dtype))
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if tuple(x.shape) not in ((B, S), (B, S, 1)):
        raise ValueError("sample_clouds: variates[%s] must be (%d, %d), got %s" % (name, B, S, tuple(x.shape)))
    return x


def sample_clouds(store, mesh_indices, cloud_size, return_eval_cloud=False, seed=0, step=0, transform=None, variates=None,
                  return_faces=False):
    """One collated batch from the meshes `mesh_indices` (host integers: a list, a numpy array or a CPU tensor) of `store`:
    'cloud' (B, 3, cloud_size) float32 and, with return_eval_cloud, 'eval_cloud' of the same shape (2 * cloud_size samples per
    slot, even ones to cloud, odd ones to eval_cloud); 'orig_c' (B, 3) / 'orig_s' (B,) if the store has them; 'faces'
    (B, samples) int32 with return_faces.  (seed, step) select the drawn stream -- a training loop passes its iteration number --
    and every slot draws its own, also when two slots name one mesh.  variates=(u, s1, s2), each (B, samples) with u float64 in
    [0, 1) and s1 / s2 float32, replaces the draw.  transform: a CloudTransform.  No host synchronisation."""
    if not isinstance(store, MeshStore):
        raise TypeError("sample_clouds: store must be a MeshStore")
    if isinstance(mesh_indices, torch.Tensor):
        if mesh_indices.is_cuda:
            raise RuntimeError("sample_clouds: mesh_indices must be host integers (they are checked against the store before "
                               "anything is launched), got a CUDA tensor")
        mesh_indices = mesh_indices.numpy()
    idx = np.asarray(mesh_indices)
    if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
        raise TypeError("sample_clouds: mesh_indices must be a non-empty 1-D sequence of integers, got %s %s" % (idx.dtype, idx.shape))
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx.max() >= store.num_meshes:
        raise IndexError("sample_clouds: mesh index %d is outside the store's %d meshes"
                         % (int(idx[(idx < 0) | (idx >= store.num_meshes)][0]), store.num_meshes))
    for m in idx:
        if int(m) in store.bad:
            raise store._error(int(m))
    N = int(cloud_size)
    if N < 1 or N >= 2 ** 30:
        raise ValueError("sample_clouds: cloud_size %d is outside 1..2^30 - 1" % N)
    if transform is not None and not isinstance(transform, CloudTransform):
        raise TypeError("sample_clouds: transform must be a CloudTransform or None")
    mask, shift, scale = transform.fused() if transform is not None else (0, np.zeros(3, np.float32), np.float32(1.0))
    if (mask & 1 and store.orig_s is None) or (mask & 2 and store.orig_c is None):
        raise ValueError("sample_clouds: the transform rescales / recentres to the original frame but the store has no orig_s / orig_c")
    dev, B, split = store.device, len(idx), bool(return_eval_cloud)
    S = 2 * N if split else N
    L = lib()
    with torch.cuda.device(dev):
        if variates is None:
            u = torch.empty((B, S), dtype=torch.float64, device=dev)
            s1 = torch.empty((B, S), dtype=torch.float32, device=dev)
            s2 = torch.empty((B, S), dtype=torch.float32, device=dev)
            check(L.dpf_mesh_variates(B, S, int(seed) & _M64, int(step) & _M64, u.data_ptr(), s1.data_ptr(), s2.data_ptr(),
                                      current_stream()), "mesh_variates")
        else:
            if len(variates) != 3:
                raise ValueError("sample_clouds: variates must be (u, s1, s2)")
            u = _variate(variates[0], "u", torch.float64, B, S, dev)
            s1 = _variate(variates[1], "s1", torch.float32, B, S, dev)
            s2 = _variate(variates[2], "s2", torch.float32, B, S, dev)
        slots = torch.from_numpy(idx.astype(np.int32)).to(dev)
        out = {"cloud": torch.empty((B, 3, N), dtype=torch.float32, device=dev)}
        if split:
            out["eval_cloud"] = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
        faces = torch.empty((B, S), dtype=torch.int32, device=dev) if return_faces else None
        ptr = lambda t: None if t is None else t.data_ptr()                                           # noqa: E731
        check(L.dpf_mesh_sample(*store.abi_args()[:5], store.cdf.data_ptr(), store.flags.data_ptr(), ptr(store.orig_c),
                                ptr(store.orig_s), B, S, slots.data_ptr(), u.data_ptr(), s1.data_ptr(), s2.data_ptr(), int(split), mask,
                                float(shift[0]), float(shift[1]), float(shift[2]), float(scale), out["cloud"].data_ptr(),
                                ptr(out.get("eval_cloud")), ptr(faces), current_stream()), "mesh_sample")
        if store.orig_c is not None:
            out["orig_c"] = store.orig_c.index_select(0, slots.long())
        if store.orig_s is not None:
            out["orig_s"] = store.orig_s.index_select(0, slots.long())
        if faces is not None:
            out["faces"] = faces
        if transform is not None:
            transform.tail(out)
    return out
