"""The definition of csrc/mesh_fill.hip's results in plain Python / numpy, and the meshes the tests use.

    boundary_loops(faces, n_vertices) -> dict   offsets, vertices, half_edges, n_boundary, n_irregular, n_loops: a dict of edges, then a
                                                sequential walk along succ
    fill_holes(vertices, faces, method, max_edges) -> dict   vertices, faces, n_loops, n_filled, n_new_faces, n_new_vertices, n_irregular
    centroid(coords)                            fixed_point_sum per axis / n in float64 (the caller rounds to the vertex dtype)

Half-edge h = 3 f + k runs from faces[f, k] (tail) to faces[f, (k+1) % 3] (head); tail == head contributes nothing.  An undirected edge
used by exactly one half-edge is a boundary edge.  A vertex is regular when exactly one boundary half-edge leaves it and exactly one enters
it; succ(h) is the boundary half-edge that leaves head(h) if that vertex is regular.  A loop is a cycle of succ, numbered by its smallest
half-edge and starting there; the other boundary half-edges are irregular and never filled."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_topo_ref as T  # noqa: E402

log_line = T.log_line


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def boundary_half_edges(faces, n_vertices):
    faces = np.asarray(faces).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= n_vertices):
        raise ValueError("a face index lies outside [0, V)")
    uses = {}
    for f, tri in enumerate(faces.tolist()):
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            if a != b:
                uses.setdefault((min(a, b), max(a, b)), []).append(3 * f + k)
    return sorted(hs[0] for hs in uses.values() if len(hs) == 1)


def boundary_loops(faces, n_vertices):
    faces = np.asarray(faces).reshape(-1, 3)
    flat = faces.reshape(-1)
    bhe = boundary_half_edges(faces, n_vertices)
    tail = {h: int(flat[h]) for h in bhe}
    head = {h: int(flat[h - 2 if h % 3 == 2 else h + 1]) for h in bhe}
    out, into = {}, {}
    for h in bhe:
        out.setdefault(tail[h], []).append(h)
        into.setdefault(head[h], []).append(h)
    succ = {}
    for h in bhe:
        v = head[h]
        succ[h] = out[v][0] if len(out.get(v, ())) == 1 and len(into[v]) == 1 else None
    seen, loops = set(), []
    for h0 in bhe:                                  # ascending: a cycle is met at its smallest half-edge first
        if h0 in seen:
            continue
        walk, h = [], h0
        while h is not None and h not in seen and not (walk and h == h0):
            walk.append(h)
            h = succ[h]
            if len(walk) > len(bhe):
                raise AssertionError("walk longer than the list")
        if h == h0 and walk:                         # came back to the start: a cycle (succ is injective, so it can close nowhere else)
            loops.append(walk)
            seen.update(walk)
    in_loops = sum(len(w) for w in loops)
    offsets = np.zeros(len(loops) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(w) for w in loops])
    half_edges = np.array([h for w in loops for h in w], dtype=np.int32)
    vertices = np.array([tail[h] for w in loops for h in w], dtype=np.int32)
    return dict(offsets=offsets, vertices=vertices, half_edges=half_edges, n_boundary=len(bhe), n_irregular=len(bhe) - in_loops,
                n_loops=len(loops))


def centroid(coords):
    coords = np.asarray(coords, dtype=np.float64)
    n = coords.shape[0]
    return np.array([T.fixed_point_sum(coords[:, a].tolist()) / np.float64(n) for a in range(3)], dtype=np.float64)


def fill_holes(vertices, faces, method="fan", max_edges=None):
    assert method in ("fan", "centroid")
    vertices = np.asarray(vertices)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int32)
    V = vertices.shape[0]
    loops = boundary_loops(faces, V)
    new_f, new_v, n_filled = [], [], 0
    for l in range(loops["n_loops"]):
        v = loops["vertices"][loops["offsets"][l]:loops["offsets"][l + 1]].tolist()
        n = len(v)
        if n < 3 or (max_edges is not None and n > max_edges):
            continue
        n_filled += 1
        if n == 3:
            new_f.append((v[0], v[2], v[1]))
        elif method == "fan":
            new_f += [(v[0], v[i + 1], v[i]) for i in range(1, n - 1)]
        else:
            c = V + len(new_v)
            new_v.append(centroid(vertices[v].astype(np.float64)).astype(vertices.dtype))
            new_f += [(c, v[(i + 1) % n], v[i]) for i in range(n)]
    out_v = np.concatenate([vertices, np.array(new_v, dtype=vertices.dtype).reshape(-1, 3)]) if new_v else vertices
    out_f = np.concatenate([faces, np.array(new_f, dtype=np.int32).reshape(-1, 3)]) if new_f else faces
    return dict(vertices=out_v, faces=out_f, n_loops=loops["n_loops"], n_filled=n_filled, n_new_faces=len(new_f), n_new_vertices=len(new_v),
                n_irregular=loops["n_irregular"], loops=loops)


# ---- independent counts (no code shared with the definition above) ---------------------------------------------------------------------
def directed_edge_counts(faces):
    """{(a, b): uses} over directed edges a -> b, a != b, by numpy's unique."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    d = d[d[:, 0] != d[:, 1]]
    keys, counts = np.unique(d[:, 0] << 32 | d[:, 1], return_counts=True)
    return {(int(k >> 32), int(k & 0xffffffff)): int(c) for k, c in zip(keys, counts)}


def closed_and_oriented(faces):
    """Every undirected edge is used exactly twice, once in each direction."""
    d = directed_edge_counts(faces)
    return all(c == 1 and d.get((b, a), 0) == 1 for (a, b), c in d.items())


def euler_number(faces):
    """V - E + F over the referenced vertices and the undirected edges, by numpy's unique."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    d = np.sort(d[d[:, 0] != d[:, 1]], axis=1)
    return int(np.unique(f).size - np.unique(d[:, 0] << 32 | d[:, 1]).size + f.shape[0])


def signed_volume(vertices, faces):
    import math
    return math.fsum(T.face_terms(vertices, faces)[1].tolist())


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def open_tetrahedron():
    v, f = T.tetrahedron()
    return v, np.ascontiguousarray(f[:3])


def open_cube():
    """The unit cube without its x = 1 side (faces 2, 3)."""
    v, f = T.cube()
    return v, np.ascontiguousarray(np.delete(f, [2, 3], axis=0))


CONE_SIZES = (3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def open_cone(n, height=1.5):
    """An apex above an n-gon rim in z = 0, n faces, outward (the missing base looks down)."""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.25, -0.125, height]], np.stack([np.cos(a), np.sin(a), 0 * a], -1)]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32)
    return v, f


def cone_volume(v):
    """The pyramid over the rim polygon (vertices 1 ..) with apex vertex 0: polygon area (shoelace, fsum) * height / 3, float64."""
    import math
    p = v[1:].astype(np.float64)
    q = np.roll(p, -1, axis=0)
    area = 0.5 * math.fsum((p[:, 0] * q[:, 1]).tolist() + (-(p[:, 1] * q[:, 0])).tolist())
    return area * float(v[0, 2]) / 3.0


def open_cylinder(n=16, height=2.0):
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(a), np.sin(a)], -1)
    v = np.concatenate([np.concatenate([ring, np.zeros((n, 1))], 1), np.concatenate([ring, np.full((n, 1), height)], 1)]).astype(np.float32)
    f = []
    for k in range(n):
        k1 = (k + 1) % n
        f += [[k, k1, n + k1], [k, n + k1, n + k]]
    return v, np.array(f, dtype=np.int32)


def _torus_face(a, b, t, n_minor=8):
    return 2 * (a * n_minor + b) + t


def torus_with_holes():
    """torus(8, 16) without four scattered faces and one 2 x 2 patch of quads: loops of 3 and one of 8."""
    v, f = T.torus(8, 16)
    gone = [_torus_face(1, 1, 0), _torus_face(5, 6, 1), _torus_face(9, 2, 0), _torus_face(14, 5, 1)]
    gone += [_torus_face(a, b, t) for a in (11, 12) for b in (3, 4) for t in (0, 1)]
    return v, np.ascontiguousarray(np.delete(f, gone, axis=0))


def torus_with_bowtie():
    """The same torus; of the scattered holes two now touch in one vertex only (the two triangles (3,3,t=1) and (4,4,t=0) share
    vertex idx(4,4) and no edge): six irregular edges there, the other holes stay loops."""
    v, f = T.torus(8, 16)
    gone = [_torus_face(3, 3, 1), _torus_face(4, 4, 0), _torus_face(9, 2, 0), _torus_face(14, 5, 1)]
    gone += [_torus_face(a, b, t) for a in (11, 12) for b in (6, 7) for t in (0, 1)]
    return v, np.ascontiguousarray(np.delete(f, gone, axis=0))


def flipped_next_to_hole():
    """cube_one_face_flipped without face 1, the flipped face's partner in its quad: the hole's rim meets the flipped face's edges."""
    v, f = T.cube_one_face_flipped()
    return v, np.ascontiguousarray(np.delete(f, [1], axis=0))


def open_tetrahedra(n=2000, seed=11):
    """n tetrahedra each without one face, vertex blocks and faces shuffled: n loops of 3."""
    rng = np.random.RandomState(seed)
    v0, f0 = T.tetrahedron()
    order = rng.permutation(n)
    v = np.concatenate([v0 * np.float32(0.5) + np.float32(2.0 * k) for k in range(n)]).astype(np.float32)
    f = np.concatenate([f0[np.delete(np.arange(4), order[k] % 4)] + 4 * k for k in range(n)])
    return v, np.ascontiguousarray(f[rng.permutation(f.shape[0])]).astype(np.int32)


def annulus(n_vertices=20000, seed=3):
    """permuted_strip closed into an annulus (the last two vertices joined to the first two), faces shuffled: two loops of
    n_vertices / 2 edges each, of opposite sense."""
    assert n_vertices % 2 == 0
    v, f = T.permuted_strip(n_vertices, seed=seed)
    # perm[k]: the vertex index at strip position k.  Row k of the strip is (perm[k], perm[k+1], perm[k+2]), reversed for odd k
    perm = np.empty(n_vertices, dtype=np.int64)
    perm[:-2] = np.where(np.arange(n_vertices - 2) % 2 == 0, f[:, 0], f[:, 2])
    last = f[-1] if (n_vertices - 3) % 2 == 0 else f[-1][::-1]
    perm[-2:] = last[1:]
    extra = []
    for k in (n_vertices - 2, n_vertices - 1):
        row = [perm[k], perm[(k + 1) % n_vertices], perm[(k + 2) % n_vertices]]
        extra.append(row if k % 2 == 0 else row[::-1])
    k = np.arange(n_vertices)
    ang = 2 * np.pi * (k // 2) / (n_vertices // 2)
    rad = 1.0 + 0.5 * (k % 2)
    pos = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0 * ang], -1).astype(np.float32)
    v = np.empty_like(pos)
    v[perm] = pos
    f = np.concatenate([f, np.array(extra, dtype=np.int32)])
    rng = np.random.RandomState(seed + 1)
    return v, np.ascontiguousarray(f[rng.permutation(f.shape[0])]).astype(np.int32)


def torus_f64():
    v, f = torus_with_holes()
    rng = np.random.RandomState(2)
    return v.astype(np.float64) + 1e-9 * rng.randn(*v.shape), f


def empty_mesh():
    v, _ = T.tetrahedron()
    return v, np.zeros((0, 3), dtype=np.int32)


# name -> (builder, expected loop lengths in loop order or None, expected n_irregular)
FIXTURES = {
    "open_tetrahedron": (open_tetrahedron, [3], 0),
    "open_cube": (open_cube, [4], 0),
    "open_cylinder": (open_cylinder, [16, 16], 0),
    "torus_with_holes": (torus_with_holes, None, 0),
    "torus_with_bowtie": (torus_with_bowtie, None, 6),
    "flipped_next_to_hole": (flipped_next_to_hole, None, None),
    "fan_on_one_edge": (T.fan_on_one_edge, None, None),
    "degenerate_face": (T.degenerate_face, [], 0),
    "open_tetrahedra": (open_tetrahedra, [3] * 2000, 0),
    "annulus": (annulus, [10000, 10000], 0),
    "closed_torus": (lambda: T.torus(8, 16), [], 0),
    "empty": (empty_mesh, [], 0),
    "torus_f64": (torus_f64, None, 0),
}
for _n in CONE_SIZES:
    FIXTURES[f"cone{_n}"] = ((lambda n=_n: open_cone(n)), [_n], 0)

_cache = {}


def fixture(name):
    """(vertices, faces) of the named fixture, built once."""
    if name not in _cache:
        _cache[name] = FIXTURES[name][0]()
    return _cache[name]


_ref_cache = {}


def reference(name, method, max_edges=None):
    """fill_holes of the named fixture, computed once and shared (callers do not modify it)."""
    key = (name, method, max_edges)
    if key not in _ref_cache:
        v, f = fixture(name)
        _ref_cache[key] = fill_holes(v, f, method, max_edges)
    return _ref_cache[key]


def sphere_volume(n=24, radius=13.5):
    """A sphere about the centre of an n^3 volume (float32, > 0 inside) whose radius is beyond the half side (n-1)/2 and below the half
    diagonal of a side: it leaves the volume through all six sides, through a disc each."""
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float32)
    c = np.float32((n - 1) / 2.0)
    return np.ascontiguousarray((np.float32(radius) - np.sqrt(((g - c) ** 2).sum(0))).astype(np.float32))
