"""Host-side launchers for the HIP kernels behind the C ABI (include/vtaco_hip.h), one module per kernel family.

Thin and allocation-explicit: every function takes torch HIP tensors, hands raw
device pointers + the current stream to libvtaco_hip.so and returns torch
tensors.  No function here computes anything with torch ops.

This file only re-exports: callers write ``ops.name`` and look the name up at call time.  A switch that is assigned at run time
(``decode_train.GRID_SCATTER_SORTED``, ``unet3d._WGRAD_UP``) is read by its own module: assign it there, not to the copy here.
``resnet_train``, ``resnet_bneck``, ``planes``, ``voxel_encoder``, ``points`` and ``voxelize`` are submodules only: callers write ``ops.resnet_train.fwd``, ``ops.resnet_bneck.fwd``,
``ops.planes.sample_planes``, ``ops.voxel_encoder.encode_grid``, ``ops.points.point_sample``, ``ops.voxelize.surface``.
``ops.metrics`` is re-exported by the names of its ``__all__``; its closest-point launchers are reached as ``ops.metrics.closest_point_mesh``.
``icp`` is a submodule only as well: ``ops.icp.nn_points``, ``ops.icp.icp_fit``, ``ops.icp.icp``; so is ``mesh``: ``ops.mesh.components``,
``ops.mesh.component_table``, ``ops.mesh.component_stats``, ``ops.mesh.edge_stats``, ``ops.mesh.filter_components``, and for simplification and welding ``ops.mesh.cluster``, ``ops.mesh.weld``,
``ops.mesh.cluster_faces``, ``ops.mesh.cluster_place``.  ``winding`` is a submodule only too: ``ops.winding.build``, ``ops.winding.query``,
``ops.winding.fast``, ``ops.winding.query_scenes`` (the exact sum stays ``ops.winding_number``), and so is ``rays``: ``ops.rays.ray_mesh``,
``ops.rays.ray_tree_query``, ``ops.rays.camera_rays``, ``ops.rays.depth_from_hits``; and ``refine``: ``ops.refine.decode_jet``, ``ops.refine.refine_sample``,
``ops.refine.refine_face_grad``, ``ops.refine.refine_step``, ``ops.refine.refine``; and ``knn``: ``ops.knn.knn_points``, ``ops.knn.knn_slab_points``,
``ops.knn.normals``.
"""
from . import (_base, decode, decode_train, decode_wide, fusion, icp, knn, labels, mano, mc, mesh, metrics, mise, nets2d, planes, pointnet, points, rays, refine, resnet_bneck, resnet_train, touch,  # noqa: F401
               unet3d, voxel, voxel_encoder, voxelize, winding)
from ._base import *            # noqa: F401,F403
from ._base import _c, _lib, _ptr_array     # noqa: F401
from .decode import *           # noqa: F401,F403
from .decode import _cl_storage             # noqa: F401
from .decode_train import *     # noqa: F401,F403
from .decode_wide import *      # noqa: F401,F403
from .fusion import *           # noqa: F401,F403
from .labels import *           # noqa: F401,F403
from .mano import *             # noqa: F401,F403
from .mc import *               # noqa: F401,F403
from .mc import _mc_guess                   # noqa: F401
from .metrics import *          # noqa: F401,F403
from .mise import *             # noqa: F401,F403
from .nets2d import *           # noqa: F401,F403
from .pointnet import *         # noqa: F401,F403
from .touch import *            # noqa: F401,F403
from .unet3d import *           # noqa: F401,F403
from .voxel import *            # noqa: F401,F403
