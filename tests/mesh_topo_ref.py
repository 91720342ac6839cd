"""A numpy restatement of csrc/mesh_topo.hip's results, and the meshes the tests use.

    topo(vertices, faces) -> dict         labels by union-find, the component table, counts, bbox, area / volume by math.fsum,
                                          the edge statistics from a dict of edges, euler / watertight / oriented
    filter_mesh(vertices, faces, t, keep) kept vertices, re-indexed faces, vertex_map
    face_terms(vertices, faces)           the per-face area and volume terms in the kernel's operation order (float64, unfused)
    term_bounds(vertices, faces)          M_f of the rounding gate: the face's own area; one sixth of the sum of |monomial| of the triple product
    fixed_point_sum(terms)                the kernel's two-limb integer accumulation, restated: what vt_mesh_component_stats returns
                                          for a component with these terms, whatever the order

The gate for area and volume: |got - ref| <= (n_faces_c + 16) 2^-52 sum_f M_f."""
import math
import os

import numpy as np


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def labels_of(n_vertices, faces):
    parent = list(range(n_vertices))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b, c in np.asarray(faces).tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(v) for v in range(n_vertices)], dtype=np.int32)


def face_terms(vertices, faces):
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = p1 - p0, p2 - p0
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    cx = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    cy = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    cz = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    vol = ((p0[:, 0] * cx + p0[:, 1] * cy) + p0[:, 2] * cz) / 6.0
    return area, vol


def term_bounds(vertices, faces):
    v = np.abs(np.asarray(vertices).astype(np.float64))
    f = np.asarray(faces).astype(np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    mono = (p0[:, 0] * (p1[:, 1] * p2[:, 2] + p1[:, 2] * p2[:, 1]) + p0[:, 1] * (p1[:, 2] * p2[:, 0] + p1[:, 0] * p2[:, 2])
            + p0[:, 2] * (p1[:, 0] * p2[:, 1] + p1[:, 1] * p2[:, 0]))
    return face_terms(vertices, faces)[0], mono / 6.0


def topo(vertices, faces):
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    V, F = vertices.shape[0], faces.shape[0]
    labels = labels_of(V, faces)
    referenced = np.zeros(V, dtype=bool)
    referenced[faces.reshape(-1)] = True
    roots = [r for r in range(V) if referenced[r] and labels[r] == r]
    rank = {r: i for i, r in enumerate(roots)}
    cov = np.array([rank[int(labels[v])] if referenced[v] else -1 for v in range(V)], dtype=np.int32)
    cof = cov[faces[:, 0]].astype(np.int32)
    C = len(roots)
    area_t, vol_t = face_terms(vertices, faces)
    n_faces = np.bincount(cof, minlength=C).astype(np.int32)
    n_vertices = np.bincount(cov[cov >= 0], minlength=C).astype(np.int32)
    area = np.array([math.fsum(area_t[cof == c].tolist()) for c in range(C)])
    volume = np.array([math.fsum(vol_t[cof == c].tolist()) for c in range(C)])
    bbox = np.stack([np.stack([vertices[cov == c].min(0), vertices[cov == c].max(0)]) for c in range(C)]).astype(vertices.dtype)
    edges = {}
    for a, b, c in faces.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                e = edges.setdefault((min(x, y), max(x, y)), [0, 0])
                e[0 if x < y else 1] += 1
    n_edges, n_boundary, n_nonmanifold, n_misoriented = (np.zeros(C, dtype=np.int32) for _ in range(4))
    for (lo, _), (fwd, bwd) in edges.items():
        c = cov[lo]
        n_edges[c] += 1
        n_boundary[c] += fwd + bwd == 1
        n_nonmanifold[c] += fwd + bwd >= 3
        n_misoriented[c] += fwd + bwd == 2 and fwd != 1
    watertight = (n_boundary == 0) & (n_nonmanifold == 0)
    return dict(labels=labels, n_components=C, comp_of_vertex=cov, comp_of_face=cof, n_faces=n_faces, n_vertices=n_vertices, bbox=bbox,
                area=area, volume=volume, n_edges=n_edges, n_boundary=n_boundary, n_nonmanifold=n_nonmanifold, n_misoriented=n_misoriented,
                euler=(n_vertices - n_edges + n_faces).astype(np.int32), watertight=watertight, oriented=watertight & (n_misoriented == 0))


def filter_mesh(vertices, faces, t, keep):
    keep = np.asarray(keep).astype(bool)
    cov, cof = t["comp_of_vertex"], t["comp_of_face"]
    kv = (cov >= 0) & keep[np.maximum(cov, 0)]
    kf = keep[cof]
    vmap = np.where(kv, np.cumsum(kv) - 1, -1).astype(np.int32)
    return np.asarray(vertices)[kv], vmap[np.asarray(faces)[kf]].astype(np.int32).reshape(-1, 3), vmap


def largest(t, by):
    size = {"faces": t["n_faces"], "area": t["area"], "volume": np.abs(t["volume"])}[by]
    keep = np.zeros(t["n_components"], dtype=bool)
    keep[int(np.argmax(size))] = True              # (numpy's argmax is the first maximum)
    return keep


def fixed_point_sum(terms):
    """The sum as csrc/mesh_topo.hip accumulates it: every term as two integer limbs against the exponent of the largest |term|."""
    terms = [float(x) for x in terms]
    big = max((abs(x) for x in terms), default=0.0)
    bits = np.float64(big).view(np.uint64)
    e = int((int(bits) >> 52) & 0x7ff)
    e = (1 if e == 0 else e) - 1023
    hi = lo = 0
    for x in terms:
        s = math.ldexp(x, 30 - e)
        h = math.trunc(s)
        hi += h
        lo += int(np.rint(math.ldexp(s - h, 31)))
    assert abs(hi) < 2 ** 63 and abs(lo) < 2 ** 63
    return math.ldexp(float(np.float64(hi)) + math.ldexp(float(np.float64(lo)), -31), e - 30)


def sum_gate(n_faces, bounds):
    return (n_faces + 16) * 2.0 ** -52 * math.fsum(bounds)


def log_line(line):
    """Print a RATIO / ROUNDS line; with VTACO_RATIO_LOG set, append it to that file (profiles/mesh_topo_f64_ratios.txt is made so)."""
    print(line)
    if os.environ.get("VTACO_RATIO_LOG"):
        with open(os.environ["VTACO_RATIO_LOG"], "a") as fh:
            fh.write(line + "\n")


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)       # outward
    return v, f


def torus(n_minor=8, n_major=16, R=1.0, r=0.3):
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    th, ph = 2 * np.pi * i / n_major, 2 * np.pi * j / n_minor
    v = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: (a % n_major) * n_minor + (b % n_minor)
    f = []
    for a in range(n_major):
        for b in range(n_minor):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v, np.array(f, dtype=np.int32)


def cube(offset=(0.0, 0.0, 0.0), size=1.0):
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32) * np.float32(size) + np.asarray(offset, dtype=np.float32)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # outward quads
    f = []
    for a, b, c, d in q:
        f += [[a, b, c], [a, c, d]]
    return v, np.array(f, dtype=np.int32)


def two_cubes_and_a_spare():
    (v0, f0), (v1, f1) = cube(), cube(offset=(3.0, 0.0, 0.0), size=0.5)
    spare = np.array([[9.0, 9.0, 9.0]], dtype=np.float32)
    return np.concatenate([v0, spare, v1]), np.concatenate([f0, f1 + 9]).astype(np.int32)        # the spare vertex is index 8


def disk(rim=12):
    a = 2 * np.pi * np.arange(rim) / rim
    v = np.concatenate([[[0, 0, 0]], np.stack([np.cos(a), np.sin(a), 0 * a], -1)]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % rim] for k in range(rim)], dtype=np.int32)
    return v, f


def fan_on_one_edge():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], dtype=np.int32)


def cube_one_face_flipped():
    v, f = cube()
    f = f.copy()
    f[0] = f[0][::-1]
    return v, f


def degenerate_face():
    v = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    return v, np.array([[0, 0, 1]], dtype=np.int32)


HAND_MESHES = (tetrahedron, torus, two_cubes_and_a_spare, disk, fan_on_one_edge, cube_one_face_flipped, degenerate_face)


def concatenated(seed=0):
    """The hand meshes as one mesh: each moved apart, the faces shuffled (components interleave in memory), one face twice."""
    rng = np.random.RandomState(seed)
    vs, fs, base = [], [], 0
    for k, make in enumerate(HAND_MESHES):
        v, f = make()
        vs.append(v + np.float32(5.0 * k))
        fs.append(f + base)
        base += v.shape[0]
    f = np.concatenate(fs)
    f = np.concatenate([f, f[:1]])                  # the tetrahedron's first face once more
    return np.concatenate(vs).astype(np.float32), f[rng.permutation(f.shape[0])].astype(np.int32)


def grid_strip(n_faces):
    """n_faces triangles of a two-row strip of unit squares (one component, open)."""
    n = n_faces // 2 + 2
    v = np.array([[k, r, 0.25 * k * r] for k in range(n) for r in (0, 1)], dtype=np.float32)
    f = []
    for k in range(n - 1):
        f += [[2 * k, 2 * k + 2, 2 * k + 1], [2 * k + 1, 2 * k + 2, 2 * k + 3]]
    return v, np.array(f[:n_faces], dtype=np.int32)


def permuted_strip(n_vertices=20000, seed=3):
    """A triangle strip over n_vertices vertices whose indices are a seeded permutation: one component of maximal diameter."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(n_vertices).astype(np.int32)
    k = np.arange(n_vertices)
    pos = np.stack([k // 2, k % 2, 0.001 * k], -1).astype(np.float32)
    v = np.empty_like(pos)
    v[perm] = pos
    f = np.stack([perm[:-2], perm[1:-1], perm[2:]], -1)
    f[1::2] = f[1::2, ::-1]
    return v, np.ascontiguousarray(f).astype(np.int32)


def triangles_and_spares(n_tri=2000, n_spare=100, seed=5):
    """n_tri disjoint triangles and n_spare unreferenced vertices scattered through the index range."""
    rng = np.random.RandomState(seed)
    V = 3 * n_tri + n_spare
    order = rng.permutation(V)
    used = order[:3 * n_tri].reshape(n_tri, 3)
    v = rng.rand(V, 3).astype(np.float32)
    return v, used.astype(np.int32)


def blob_volume(n=33):
    """Two spheres and a 3-voxel blob in an n^3 volume (float32, > 0 inside): marching cubes at level 0 gives three components."""
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    d1 = 7.3 - np.sqrt(((g - np.array([10, 10, 10], dtype=np.float32).reshape(3, 1, 1, 1)) ** 2).sum(0))
    d2 = 4.6 - np.sqrt(((g - np.array([23, 22, 21], dtype=np.float32).reshape(3, 1, 1, 1)) ** 2).sum(0))
    vol = np.maximum(d1, d2).astype(np.float32)
    vol[27:30, 5, 5] = 0.5
    return np.ascontiguousarray(vol)
