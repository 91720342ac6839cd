#!/usr/bin/env python3
"""Golden vectors for the visualise block's metrics (tests/golden/g21_metrics.npz) from the REAL reference functions
src/common.py: EarthMoverDistance (:45-51, cdist + scipy linear_sum_assignment) and chamfer_distance(..., use_kdtree=False)
(:54-91, the naive squared-distance Chamfer), on fixed seeded clouds:

    close      2048 x 2048: a 0.1-sigma Gaussian cloud, and the same plus 0.01-sigma noise
    far        2048 x 2048: a 0.1-sigma Gaussian cloud against a uniform cube [-0.5, 0.5]^3
    rect       2048 x 1500: two unrelated Gaussian clouds (the mesh side has fewer than 2048 vertices)
    mesh       the reference's metric block itself (generation.py:270-284) on g7's ``logits32`` marching-cubes vertices: rescaled
               by -nx/2 and 1.1/nx, shuffled with np.random.seed(MESH_SEED), the first 2048 kept, against a seeded 2048-point
               points_obj

Stored per case: ``<case>.a`` (points1 = points_obj), ``<case>.b`` (points2 = vertices), ``<case>.emd``, ``<case>.cd`` and
``<case>.cost`` (scipy's optimal total cost, d[assignment].sum()).  src/common.py imports pykdtree and pybullet at module level;
neither is installed and neither is used by the two functions, so both are stubbed.  The reference checkout is the first
argument (or VTACO_REFERENCE):

    python tests/golden/make_metric_goldens.py <reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
MESH_SEED = 2101


def load_reference_common(root):
    for name in ("pykdtree", "pykdtree.kdtree", "pybullet"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pykdtree.kdtree"].KDTree = None
    spec = importlib.util.spec_from_file_location("ref_common", os.path.join(root, "src", "common.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.RandomState(2100)
    g = (rng.randn(2048, 3) * 0.1).astype(np.float32)
    yield "close", g, (g + rng.randn(2048, 3) * 0.01).astype(np.float32)
    yield "far", (rng.randn(2048, 3) * 0.1).astype(np.float32), rng.uniform(-0.5, 0.5, (2048, 3)).astype(np.float32)
    yield "rect", (rng.randn(2048, 3) * 0.1).astype(np.float32), (rng.randn(1500, 3) * 0.12 + 0.02).astype(np.float32)
    # the metric block of generation.py:270-284 on a real marching-cubes vertex set
    z = np.load(os.path.join(HERE, "g7_mc.npz"))
    nx = z["logits32.vol"].shape[0]
    vertices = z["logits32.verts"].copy()
    vertices -= np.array([nx / 2, nx / 2, nx / 2], dtype=np.float32)
    vertices *= 1.1 / nx
    np.random.seed(MESH_SEED)
    np.random.shuffle(vertices)
    vertices = np.ascontiguousarray(vertices[:2048], dtype=np.float32)
    points_obj = (rng.randn(2048, 3) * 0.15).astype(np.float32)
    yield "mesh", points_obj, vertices


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VTACO_REFERENCE")
    if not root:
        sys.exit("usage: make_metric_goldens.py <reference checkout>  (or set VTACO_REFERENCE)")
    ref = load_reference_common(root)
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    out = {"cases": np.array(["close", "far", "rect", "mesh"]), "mesh_seed": np.int64(MESH_SEED)}
    for name, a, b in cases():
        emd = ref.EarthMoverDistance(a, b)
        cd = ref.chamfer_distance(torch.from_numpy(a)[None], torch.from_numpy(b)[None], use_kdtree=False)
        d = distance.cdist(a, b)
        cost = d[linear_sum_assignment(d)].sum()
        out.update({f"{name}.a": a, f"{name}.b": b, f"{name}.emd": np.float64(emd), f"{name}.cd": np.float32(cd.item()),
                    f"{name}.cost": np.float64(cost)})
        print(f"{name}: {len(a)} x {len(b)}  emd {emd:.9g}  cd {cd.item():.9g}")
    path = os.path.join(HERE, "g21_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g21_metrics.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
