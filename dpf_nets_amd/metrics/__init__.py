from .point_mesh import point_mesh_distance, surface_accuracy   # noqa: F401
from .point_mesh import mesh_point_distance, surface_completeness, surface_chamfer   # noqa: F401
from .fps import farthest_point_sample   # noqa: F401
from .knn import knn_points, knn_gather, neighbour_spacing   # noqa: F401
from .normals import normals_from_index, estimate_normals, surface_variation, normal_consistency   # noqa: F401
from .sliced import sliced_directions, sliced_tables, sliced_wasserstein, pairwise_SWD   # noqa: F401
from .align import RigidTransform, rigid_fit, icp, apply_transform, icp_plane, PlaneICPInfo   # noqa: F401
from .dcd import density_aware_chamfer, density_aware_chamfer_raw, pairwise_DCD   # noqa: F401
