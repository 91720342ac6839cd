"""Utilities beside the hot path that mirror the reference's src/utils (``voxels``: occupancy volumes from meshes and back; ``icp``:
rigid registration of point sets)."""
