"""Utilities beside the hot path that mirror the reference's src/utils (``voxels``: occupancy volumes from meshes and back; ``icp``:
rigid registration of point sets; ``pointcloud``: k nearest neighbours, normals and outlier removal of point clouds; ``io``: PLY point
clouds and OFF meshes)."""
