#!/usr/bin/env python
"""Golden vectors of mesh subdivision (tests/golden/g31_subdivide.npz) from the REAL reference layer.

Build container only (needs /root/reference).  A harness around the unmodified reference file src/encoder/manopth/upsample_layer.py:
it is loaded through importlib with empty stand-ins for the modules its top imports (``manopth``, ``manopth.manolayer`` with a dummy
``ManoLayer``, ``open3d``), which only its ``__main__`` block uses.  ``UpSampleLayer.forward`` then runs on the CPU on the fixtures of
tests/mesh_subdivide_ref.py.  Arrays only are stored -- the inputs, new_verts, new_faces and the edge pairs of ``calculate_faces`` -- and
no reference code.

    tetra        the tetrahedron [[0,1,2],[0,2,3],[0,3,1],[1,3,2]]: edges [[0,1],[1,2],[0,2],[2,3],[0,3],[1,3]]
    batch2       two items of one shape and different faces: the tetrahedron above and tests/mesh_topo_ref.py's
    ball         the closed voxel-ball surface, 252 faces in a seeded shuffle
    strip        the open strip of 10 faces
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_subdivide_ref as R  # noqa: E402

REF_FILE = "/root/reference/src/encoder/manopth/upsample_layer.py"


def load_reference():
    for name in ("manopth", "manopth.manolayer", "open3d"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["manopth.manolayer"].ManoLayer = type("ManoLayer", (), {})
    spec = importlib.util.spec_from_file_location("reference_upsample_layer", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.UpSampleLayer


def run(layer, verts, faces):
    """verts [B,V,3] f32, faces [B,F,3] -> new_verts, new_faces, edge pairs [B,E,2]."""
    nv, nf = layer(torch.from_numpy(verts), torch.from_numpy(faces.astype(np.int64)))
    pairs = np.stack([layer.calculate_faces(tuple(tuple(int(i) for i in tri) for tri in fs), verts.shape[1])[0] for fs in faces])
    return nv.numpy(), nf.numpy(), pairs.astype(np.int32)


def main():
    layer = load_reference()()
    tv, tf = R.fixture("tetrahedron")
    tetra_faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], dtype=np.int32)
    rng = np.random.RandomState(31)
    cases = {
        "tetra": (tv[None], tetra_faces[None]),
        "batch2": (np.stack([tv, (tv + rng.randn(4, 3) * 0.1).astype(np.float32)]), np.stack([tetra_faces, tf])),
        "ball": tuple(a[None] for a in R.fixture("voxel_ball")),
        "strip": tuple(a[None] for a in R.fixture("strip10")),
    }
    out = {}
    for name, (v, f) in cases.items():
        v = np.ascontiguousarray(v, dtype=np.float32)
        nv, nf, pairs = run(layer, v, f)
        out[name + "_verts"], out[name + "_faces"] = v, f.astype(np.int32)
        out[name + "_new_verts"], out[name + "_new_faces"], out[name + "_pairs"] = nv, nf.astype(np.int32), pairs
        print(name, v.shape, f.shape, "->", nv.shape, nf.shape, pairs.shape)
    assert out["tetra_pairs"][0].tolist() == [[0, 1], [1, 2], [0, 2], [2, 3], [0, 3], [1, 3]]
    assert out["tetra_new_faces"][0, :4].tolist() == [[4, 5, 6], [0, 4, 6], [1, 5, 4], [2, 6, 5]]
    np.savez_compressed(os.path.join(HERE, "g31_subdivide.npz"), **out)


if __name__ == "__main__":
    main()
