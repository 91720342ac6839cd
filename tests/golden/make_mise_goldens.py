#!/usr/bin/env python3
"""Golden vectors for multiresolution isosurface extraction (tests/golden/g22_mise.npz) from the REAL reference
``MultiGridExtractor`` (src/utils/mesh.py:7-84, with check_voxel_boundary from src/utils/voxels.py:222-257), which the reference
keeps but never calls.  Driven as Occupancy Networks drives it: level 0 queries every point, then per step
``increase_resolution`` -> ``query`` -> ``update``.

Fields (seeded, analytic): evaluated in float64 at the exact lattice coordinates box * (-0.5 + i / (n-1)) of the finest level and
rounded once to float32; a coarser level's point i is the finest point i * 2^(S-k).  Level 0.0 (the logit of 0.5); no value
equals it (asserted), so the reference's ``values < threshold`` and marching cubes' ``v - level > 0`` split the points alike.

    sphere   radius 0.3 about a seeded centre                                           r0 = 4, S = 3 (n = 33)
    needle   a sphere plus a 0.02-radius needle along x that the 8^3 level misses       r0 = 8, S = 2 (n = 33)
    noisy    a sphere plus seeded sinusoidal noise                                      r0 = 4, S = 3 (n = 33)

Stored per field ``f``: ``f.params`` (float64), ``f.r0_steps``, ``f.table`` (the field at every finest point, float32 [n,n,n]),
``f.q<k>`` (sorted lattice ids of level k that the reference queried, ids of the level-k lattice), ``f.values`` (float32 [n,n,n])
and ``f.known`` (u8 [n,n,n]).  src/utils/voxels.py imports trimesh, scikit-image and src.common at module level; none of them is used
by the two functions, so they are stubbed.  The reference checkout is the first argument (or VTACO_REFERENCE):

    python tests/golden/make_mise_goldens.py <reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
BOX = 1.1
LEVEL = 0.0


def load_reference_mesh(root):
    for name in ("trimesh", "skimage", "skimage.measure", "src", "src.common", "src.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.measure"].block_reduce = None
    sys.modules["src.common"].make_3d_grid = None

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    sys.modules["src.utils"].voxels = load("src.utils.voxels", ("src", "utils", "voxels.py"))
    return load("src.utils.mesh", ("src", "utils", "mesh.py"))


def field(kind, params, n):
    """float32 [n,n,n] of the field on the n^3 lattice (x-major)."""
    lin = BOX * (-0.5 + np.arange(n, dtype=np.float64) / (n - 1))
    x, y, z = np.meshgrid(lin, lin, lin, indexing="ij")
    cx, cy, cz, r = params[:4]
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
    f = r - d
    if kind == "needle":
        ny, nz, rad, length = params[4:8]
        along = (x >= cx) & (x <= cx + length)
        f = np.maximum(f, np.where(along, rad - np.sqrt((y - ny) ** 2 + (z - nz) ** 2), -1.0))
    elif kind == "noisy":
        for a, kx, ky, kz, ph in params[4:].reshape(-1, 5):
            f = f + a * np.sin(kx * x + ky * y + kz * z + ph)
    return f.astype(np.float32)


def cases():
    rng = np.random.RandomState(2200)
    c = rng.uniform(-0.05, 0.05, 3)
    yield "sphere", (4, 3), np.array([*c, 0.3])
    c = rng.uniform(-0.03, 0.03, 3)
    # the needle's axis sits between the lattice rows of the 8^3 level (spacing 0.1375) and is thinner than its finest spacing
    yield "needle", (8, 2), np.array([*c, 0.22, 0.0687 + 0.003, -0.0687 + 0.002, 0.02, 0.45])
    c = rng.uniform(-0.05, 0.05, 3)
    waves = np.concatenate([np.stack([rng.uniform(0.01, 0.04, 6), *rng.uniform(-25, 25, (3, 6)), rng.uniform(0, 6.28, 6)], 1).ravel()])
    yield "noisy", (4, 3), np.concatenate([[*c, 0.28], waves])


def run(MGE, r0, steps, table):
    """The reference driver (Occupancy Networks' generate_from_latent): queries per level and the final grids."""
    n = table.shape[0]
    ex = MGE(r0, LEVEL)
    queries = []
    for k in range(steps + 1):
        if k:
            ex.increase_resolution()
        pts = ex.query()
        s = (n - 1) // (r0 * 2 ** k)                 # level-k point i is the finest point s*i
        vals = table[pts[:, 0] * s, pts[:, 1] * s, pts[:, 2] * s].astype(np.float64)
        nk = r0 * 2 ** k + 1
        queries.append(np.sort((pts[:, 0] * nk + pts[:, 1]) * nk + pts[:, 2]).astype(np.int32))
        ex.update(pts, vals)
    return queries, ex.values.astype(np.float32), ex.value_known.astype(np.uint8)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VTACO_REFERENCE")
    if not root:
        raise SystemExit("usage: make_mise_goldens.py <reference checkout>")
    mesh = load_reference_mesh(root)
    out = {}
    for name, (r0, steps), params in cases():
        n = r0 * 2 ** steps + 1
        table = field(name, params, n)
        assert not np.any(table == LEVEL), name
        queries, values, known = run(mesh.MultiGridExtractor, r0, steps, table)
        out[f"{name}.params"] = params
        out[f"{name}.r0_steps"] = np.array([r0, steps], dtype=np.int32)
        out[f"{name}.table"] = table
        for k, q in enumerate(queries):
            out[f"{name}.q{k}"] = q
        out[f"{name}.values"] = values
        out[f"{name}.known"] = known
        print(name, "queries per level", [len(q) for q in queries], "known", int(known.sum()), "of", n ** 3)
    path = os.path.join(HERE, "g22_mise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
