"""Device-side construction of training batches: clouds sampled from triangle meshes by HIP kernels (sampling.py)."""
from .sampling import MeshStore, CloudTransform, sample_clouds, host_variates   # noqa: F401
