from .point_mesh import point_mesh_distance, surface_accuracy   # noqa: F401
