"""A numpy float64 restatement of csrc/mesh_normals.hip, and the meshes its tests use.

    face_geometry(vertices, faces)            cross products, live mask, unit face normals, in the kernel's operation order
    corner_terms(vertices, faces, weight)     [F,3,3]: the term face f adds to its corner k ('area': the raw cross product; 'angle': the
                                              unit normal times atan2(|cross|, e1 . e2)); zero rows for degenerate faces
    normals(vertices, faces, weight)          (face_normals [F,3], vertex_normals [V,3]) float64: the kernel's rule, the per-vertex sums
                                              by its two-limb integer accumulation (exact to 2^-62 of the vertex's largest term component,
                                              independent of the order of the faces)
    vertex_normals_fsum(...)                  the same normals with every sum taken by math.fsum (correctly rounded): what the fixed-point
                                              sums are checked against on the CPU

The gate of the GPU tests: every component of a normal lies within 2 roundings of ``normals``' -- 2 * 2^-24 for float32 outputs,
2 * 2^-53 for float64 ones with weight='area' (every operation of the rule is then a correctly rounded IEEE operation on both sides;
with weight='angle' the two sides call different atan2 implementations, so float64 outputs are compared at float32's gate only)."""
import math

import numpy as np

WEIGHTS = ("area", "angle")


def face_geometry(vertices, faces):
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    p = [v[f[:, k]] for k in range(3)]
    u, w = p[1] - p[0], p[2] - p[0]
    with np.errstate(all="ignore"):
        cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        l2 = (cx * cx + cy * cy) + cz * cz
        live = (l2 > 0.0) & (l2 < np.inf)
        length = np.where(live, np.sqrt(np.where(live, l2, 1.0)), 0.0)
        cross = np.stack([cx, cy, cz], -1)
        unit = np.where(live[:, None], cross / np.where(live, length, 1.0)[:, None], 0.0)
    return p, cross, length, live, unit


def corner_terms(vertices, faces, weight="area"):
    assert weight in WEIGHTS
    p, cross, length, live, unit = face_geometry(vertices, faces)
    F = cross.shape[0]
    terms = np.zeros((F, 3, 3))
    for k in range(3):
        if weight == "area":
            t = cross
        else:
            e1, e2 = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
            dot = (e1[:, 0] * e2[:, 0] + e1[:, 1] * e2[:, 1]) + e1[:, 2] * e2[:, 2]
            t = np.arctan2(length, dot)[:, None] * unit
        terms[:, k] = np.where(live[:, None], t, 0.0)
    return terms, live, unit


def _normalise(s):
    l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    any_ = l2 > 0.0
    return np.where(any_[:, None], s / np.sqrt(np.where(any_, l2, 1.0))[:, None], 0.0)


def normals(vertices, faces, weight="area"):
    V = np.asarray(vertices).shape[0]
    f = np.asarray(faces).astype(np.int64)
    terms, live, unit = corner_terms(vertices, faces, weight)
    # pass 0: every vertex's largest |term component|
    big = np.zeros(V)
    for k in range(3):
        np.maximum.at(big, f[live, k], np.abs(terms[live, k]).max(-1))
    ex = np.frexp(big)[1] - 1                                    # big = m 2^ex, m in [1, 2)
    ex = np.where(big < 2.0 ** -1022, -1022, ex)                 # (zero and subnormal: the exponent field reads 1)
    # pass 1: two int64 limbs per component against that exponent
    hi, lo = np.zeros((V, 3), dtype=np.int64), np.zeros((V, 3), dtype=np.int64)
    for k in range(3):
        idx = f[live, k]
        s = np.ldexp(terms[live, k], (30 - ex[idx])[:, None])
        h = np.trunc(s)
        l = np.rint(np.ldexp(s - h, 31))
        np.add.at(hi, idx, h.astype(np.int64))
        np.add.at(lo, idx, l.astype(np.int64))
    sums = hi.astype(np.float64) + np.ldexp(lo.astype(np.float64), -31)      # left in the limbs' scale, as the kernel leaves them
    return unit, _normalise(sums)


def vertex_normals_fsum(vertices, faces, weight="area"):
    V = np.asarray(vertices).shape[0]
    f = np.asarray(faces).astype(np.int64)
    terms, live, _ = corner_terms(vertices, faces, weight)
    bucket = [[[], [], []] for _ in range(V)]
    for i in np.nonzero(live)[0].tolist():
        for k in range(3):
            for d in range(3):
                bucket[f[i, k]][d].append(float(terms[i, k, d]))
    s = np.array([[math.fsum(b[d]) for d in range(3)] for b in bucket]).reshape(V, 3)
    big = np.abs(s).max(-1)
    scale = np.where(big > 0, np.ldexp(1.0, -np.frexp(np.where(big > 0, big, 1.0))[1]), 1.0)   # a power of two: keeps the squares in range
    return _normalise(s * scale[:, None])


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)       # outward
    return v, f


def cube_degenerate_spare():
    """A unit cube, offset off the lattice, with a thirteenth face that is degenerate (two equal corners), a fourteenth whose three
    corners lie on one line, and a ninth vertex nothing references."""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32) * np.float32(0.7) + np.float32(0.1)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # outward quads
    f = []
    for a, b, c, d in q:
        f += [[a, b, c], [a, c, d]]
    v = np.concatenate([v, np.array([[5.0, 5.0, 5.0]], dtype=np.float32), (v[0:1] + v[1:2]) * np.float32(0.5)])   # 8: spare, 9: on edge 0-1
    f += [[3, 3, 5], [0, 9, 1]]
    return v, np.array(f, dtype=np.int32)


def torus(n_major=16, n_minor=8, R=1.0, r=0.3):
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    th, ph = 2 * np.pi * i / n_major, 2 * np.pi * j / n_minor
    v = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: (a % n_major) * n_minor + (b % n_minor)
    f = []
    for a in range(n_major):
        for b in range(n_minor):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v, np.array(f, dtype=np.int32)


def single_face():
    v = np.array([[0.25, -1.5, 3.0], [2.0, 0.125, -0.75], [-0.5, 1.0, 0.3]], dtype=np.float32)
    return v, np.array([[0, 1, 2]], dtype=np.int32)


def fan(n_faces=1000, seed=7):
    """n_faces triangles around vertex 0 (valence n_faces), the rim at seeded heights and radii: the terms at the hub differ in size."""
    rng = np.random.RandomState(seed)
    a = 2 * np.pi * np.arange(n_faces) / n_faces
    rad = 0.5 + rng.rand(n_faces)
    rim = np.stack([rad * np.cos(a), rad * np.sin(a), 0.3 * rng.randn(n_faces)], -1)
    v = np.concatenate([[[0.0, 0.0, 0.4]], rim]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % n_faces] for k in range(n_faces)], dtype=np.int32)
    return v, f


MESHES = {"tetrahedron": tetrahedron, "cube_degenerate_spare": cube_degenerate_spare, "torus16x8": torus, "single_face": single_face,
          "fan1000": fan}
