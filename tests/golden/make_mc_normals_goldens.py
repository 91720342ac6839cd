#!/opt/conda/bin/python3.9
"""Marching-cubes normals and values from scikit-image 0.18.3 itself, for the volumes of g7_mc.npz (make_mc_goldens.py wrote them).
Runs only in the build container:  /opt/conda/bin/python3.9 tests/golden/make_mc_normals_goldens.py
Writes tests/golden/g30_mc_normals.npz: per case (the nine volumes at scikit-image's default level, the two explicit-level cases)
``<case>.normals`` f32 [V,3] and ``<case>.values`` f32 [V] as ``measure.marching_cubes(vol, level, gradient_direction='ascent')``
returns them, and ``<case>.unusable`` bool [V]: the vertices whose scikit-image normal is zero or not finite.  For the first N_CELLS
single-cell volumes of g7_mc.npz: ``cells.normals`` f32 [N,16,3], ``cells.values`` f32 [N,16], ``cells.unusable`` bool [N,16], padded
like ``cells.verts`` there.  The volumes themselves stay in g7_mc.npz.

Asserted here, so that a fixture that breaks it is never written: in every case at most 2 % of the vertices have a cancellation ratio
kappa > 2^12 in the restatement (tests/mc_normals_ref.py); such a volume would be replaced by another seed in make_mc_goldens.py."""
import os
import sys

import numpy as np
from skimage import measure

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import mc_normals_ref as R  # noqa: E402

N_CELLS = 2000                       # of the 4 000: they cover every case and sub-case, and the file stays well below 1 MiB
CASES = ["sphere16", "torus24", "noise12", "noise20", "noise_rect", "smoothnoise24", "plateau10", "tiny2", "checker8", "noise20@0.25",
         "sphere16@0.25"]

g7 = np.load(os.path.join(OUT, "g7_mc.npz"))
out = {}
for name in CASES:
    vol = g7[name + ".vol"]
    level = 0.25 if "@" in name else None
    verts, faces, normals, values = measure.marching_cubes(vol, level, gradient_direction="ascent")
    assert np.array_equal(faces.astype(np.int32), g7[name + ".faces"]) and normals.dtype == np.float32 and values.dtype == np.float32
    ref = R.mc(vol, level)
    assert np.array_equal(ref["faces"], g7[name + ".faces"]), name
    beyond = float((ref["kappa"] > R.KAPPA_MAX).mean())
    assert beyond <= 0.02, (name, beyond)
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    out[name + ".normals"] = normals
    out[name + ".values"] = values
    out[name + ".unusable"] = ~np.isfinite(length) | (length == 0)
    print(name, vol.shape, "V", len(verts), "kappa > 2^12: %.3f %%" % (100 * beyond), "unusable", int(out[name + ".unusable"].sum()),
          "centre %.2f %%" % (100 * ref["centre"].mean()))

cells = g7["cells.vols"][:N_CELLS]
c_normals = np.zeros((N_CELLS, 16, 3), np.float32)
c_values = np.zeros((N_CELLS, 16), np.float32)
c_unusable = np.zeros((N_CELLS, 16), bool)
cases_seen = set()
for i in range(N_CELLS):
    try:
        v, f, n, val = measure.marching_cubes(cells[i], 0.0, gradient_direction="ascent")
    except (RuntimeError, ValueError):
        continue
    assert len(v) == g7["cells.nv"][i]
    c_normals[i, :len(v)], c_values[i, :len(v)] = n, val
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    c_unusable[i, :len(v)] = ~np.isfinite(length) | (length == 0)
    corner = np.array([cells[i][R.CZ[k], R.CY[k], R.CX[k]] for k in range(8)], dtype=np.float64)
    index = sum(1 << k for k in range(8) if corner[k] > 0)
    cases_seen.add((int(R.tables()["CASES"][index][0]), len(f)))
assert {c for c, _ in cases_seen} == set(range(1, 15)), sorted(cases_seen)
out.update({"cells.normals": c_normals, "cells.values": c_values, "cells.unusable": c_unusable})
path = os.path.join(OUT, "g30_mc_normals.npz")
np.savez_compressed(path, **out)
print("g30_mc_normals.npz", os.path.getsize(path) // 1024, "KiB;", len(cases_seen), "(case, triangle count) pairs among the cells")
assert os.path.getsize(path) < (1 << 20)
