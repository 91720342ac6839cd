"""The definition of csrc/mesh_subdivide.hip's results in numpy, and the meshes the tests use.

    edge_table(faces, n_vertices) -> dict          the undirected edges, their direction counts, their lowest half-edge
    marks(vertices, faces, table, max_edge, face_mask) -> bool [edges]
    subdivide(vertices, faces, scheme, max_edge, face_mask) -> (vertices, faces, info)
    subdivide_to_size(vertices, faces, max_edge, max_iter) -> (vertices, faces, rounds)
    backward(edge_verts, n_vertices, grad_out) -> (grad_verts, sum of |terms| float64 [V,3], terms per sum int [V])

Half-edge h = 3 f + k runs from faces[f, k] to faces[f, (k + 1) % 3].  One pipeline: mark a set of edges, give each marked edge one new
vertex, split each face by how many of its edges are marked.  An edge is marked by rule: every edge (``max_edge`` and ``face_mask``
None); squared length above max_edge^2, the length (dx dx + dy dy) + dz dz in float64 with d = x_hi - x_lo from the lower vertex index to
the higher; or the edges of the faces with face_mask != 0.  Marked edges are numbered in the order in which a walk over the half-edges
0, 1, 2, ... first meets them -- the order of a dict filled face by face -- and edge e's vertex is V + e.

Children of face (a, b, c) with x on ab, y on bc, z on ca, contiguous and in the faces' order:
    3 marks   (x, y, z) (a, x, z) (b, y, x) (c, z, y)
    0 marks   (a, b, c)
    1 mark    rotated so the marked edge is (p, q), r opposite, m its vertex: (p, m, r) (m, q, r)
    2 marks   rotated so the unmarked edge is (p, q), s on qr, t on rp: (r, t, s), then the quad p q s t cut along the shorter of its
              diagonals p-s and q-t: (p, q, s) (p, s, t) or (p, q, t) (q, s, t).  The squared lengths are float64, s and t the float64
              midpoints (x_q + x_r) * 0.5 and (x_r + x_p) * 0.5 of the INPUT positions under either scheme; on a tie, or when a length
              is NaN, the diagonal that leaves the lower of the vertex indices p and q is taken.
The diagonal is interior to the face: the result conforms whatever the neighbours do.

``'midpoint'``: the originals bit for bit, a new vertex (x_lo + x_hi) * 0.5 in the vertices' own type.  ``'loop'`` (every edge marked),
in float64 and rounded once: a new vertex on an edge with direction counts (1, 1) is 0.375 (x_lo + x_hi) + 0.125 (x_c + x_d), c and d the
opposite vertices of the lo -> hi and the hi -> lo face; on an edge with counts (1, 0) or (0, 1) the midpoint; any other edge is irregular:
the midpoint, counted in n_irregular.  An interior vertex of degree n becomes (1 - n b) x + b sum_j x_j, the sum from 0.0 over its
neighbours in ascending order, b = 3/16 for n = 3 and 3 / (8 n) otherwise (Warren); a boundary vertex with exactly two boundary neighbours
j < k becomes 0.75 x + 0.125 (x_j + x_k); a vertex at an irregular edge, with another boundary count or without neighbours keeps its bits.

A face with an index outside [0, V) or with a repeated index is refused (ValueError)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_smooth_ref as S  # noqa: E402
import mesh_topo_ref as T  # noqa: E402

SCHEMES = ("midpoint", "loop")
MT_CHUNK = 1024                                                     # csrc/mesh_common.h: elements per workgroup of a scan


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def edge_table(faces, n_vertices):
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = int(n_vertices)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("a face index lies outside [0, V)")
    if f.size and ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any():
        raise ValueError("a face has a repeated index")
    tail, head = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    keys, minh, inv = np.unique((np.minimum(tail, head) << 32) | np.maximum(tail, head), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    fwd = np.bincount(inv[tail < head], minlength=keys.shape[0])
    bwd = np.bincount(inv[tail > head], minlength=keys.shape[0])
    return dict(lo=keys >> 32, hi=keys & 0xffffffff, minh=minh, edge_of=inv, fwd=fwd, bwd=bwd, tail=tail, head=head, faces=f)


def marks(vertices, faces, table, max_edge=None, face_mask=None):
    n = table["lo"].shape[0]
    if max_edge is not None:
        x = np.asarray(vertices).astype(np.float64)
        d = x[table["hi"]] - x[table["lo"]]
        return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) > float(max_edge) * float(max_edge)
    if face_mask is not None:
        out = np.zeros(n, dtype=bool)
        out[table["edge_of"][np.repeat(np.asarray(face_mask).reshape(-1) != 0, 3)]] = True
        return out
    return np.ones(n, dtype=bool)


def _children(tri, m, x):
    """The children of one face: tri its three indices, m the new vertex on ab, bc, ca or -1, x the float64 input positions."""
    a, b, c = tri
    n = sum(v >= 0 for v in m)
    if n == 0:
        return [[a, b, c]]
    if n == 3:
        return [[m[0], m[1], m[2]], [a, m[0], m[2]], [b, m[1], m[0]], [c, m[2], m[1]]]
    if n == 1:
        k = [v >= 0 for v in m].index(True)
        p, q, r = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
        return [[p, m[k], r], [m[k], q, r]]
    k = [v >= 0 for v in m].index(False)
    p, q, r, s, t = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3], m[(k + 1) % 3], m[(k + 2) % 3]
    xs, xt = (x[q] + x[r]) * 0.5, (x[r] + x[p]) * 0.5
    dp, dq = xs - x[p], xt - x[q]
    lps = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]
    lqt = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]
    along_ps = lps < lqt or (not lqt < lps and p < q)
    return [[r, t, s]] + ([[p, q, s], [p, s, t]] if along_ps else [[p, q, t], [q, s, t]])


def _loop_even(x, adj, at_irregular):
    out, moved = x.copy(), np.zeros(x.shape[0], dtype=bool)
    off, nb, be, bv = adj["offsets"], adj["neighbors"], adj["boundary_edge"], adj["boundary_vertex"]
    for i in range(x.shape[0]):
        row = range(int(off[i]), int(off[i + 1]))
        if at_irregular[i] or len(row) == 0:
            continue
        if bv[i]:
            ends = [int(nb[k]) for k in row if be[k]]
            if len(ends) == 2:
                out[i] = 0.75 * x[i] + 0.125 * (x[ends[0]] + x[ends[1]])
                moved[i] = True
            continue
        s = np.zeros(3, dtype=np.float64)
        for k in row:
            s = s + x[nb[k]]
        n = float(len(row))
        beta = 0.1875 if len(row) == 3 else 3.0 / (8.0 * n)
        out[i] = (1.0 - n * beta) * x[i] + beta * s
        moved[i] = True
    return out, moved


def subdivide(vertices, faces, scheme="midpoint", max_edge=None, face_mask=None):
    """(vertices [V + n_marked, 3] in the input's dtype, faces int32 [F_out, 3], info): info holds edge_verts int32 [n_marked, 2],
    face_parent int32 [F_out], n_marked, n_irregular and marks_per_face int [F]."""
    if scheme not in SCHEMES or (scheme == "loop" and (max_edge is not None or face_mask is not None)):
        raise ValueError("scheme is 'midpoint' or 'loop', and 'loop' marks every edge")
    vertices = np.asarray(vertices)
    V = vertices.shape[0]
    t = edge_table(faces, V)
    f, F = t["faces"], t["faces"].shape[0]
    marked = marks(vertices, faces, t, max_edge, face_mask)
    order = np.argsort(np.where(marked, t["minh"], 3 * F + 1), kind="stable")[:int(marked.sum())]        # first-seen order
    eid = np.full(marked.shape[0], -1, dtype=np.int64)
    eid[order] = np.arange(order.shape[0])
    lo, hi = t["lo"][order], t["hi"][order]
    regular = (t["fwd"] <= 1) & (t["bwd"] <= 1)
    n_irregular = int((marked & ~regular).sum())
    x = vertices.astype(np.float64)
    new_of = np.where(eid >= 0, V + eid, -1)[t["edge_of"]].reshape(F, 3)
    out_faces, parent = [], []
    for i in range(F):
        kids = _children(f[i].tolist(), new_of[i].tolist(), x)
        out_faces += kids
        parent += [i] * len(kids)
    if scheme == "midpoint":
        new = (vertices[lo] + vertices[hi]) * vertices.dtype.type(0.5)
        out_verts = np.concatenate([vertices, new.astype(vertices.dtype)])
    else:
        opp = f[:, [2, 0, 1]].reshape(-1)                                                                  # opposite the half-edge
        c, d = np.zeros(marked.shape[0], dtype=np.int64), np.zeros(marked.shape[0], dtype=np.int64)
        up = t["tail"] < t["head"]
        c[t["edge_of"][up]] = opp[up]
        d[t["edge_of"][~up]] = opp[~up]
        interior = ((t["fwd"] == 1) & (t["bwd"] == 1))[order]
        c, d = c[order], d[order]
        new = (x[lo] + x[hi]) * 0.5
        new[interior] = (0.375 * (x[lo] + x[hi]) + 0.125 * (x[c] + x[d]))[interior]
        at_irregular = np.zeros(V, dtype=bool)
        at_irregular[t["lo"][marked & ~regular]] = True
        at_irregular[t["hi"][marked & ~regular]] = True
        even, moved = _loop_even(x, S.adjacency(faces, V), at_irregular)
        out_verts = np.concatenate([even, new]).astype(vertices.dtype)
        out_verts[:V][~moved] = vertices[~moved]                                                           # kept bit for bit
    info = dict(edge_verts=np.stack([lo, hi], -1).astype(np.int32).reshape(-1, 2), face_parent=np.array(parent, dtype=np.int32),
                n_marked=int(order.shape[0]), n_irregular=n_irregular, marks_per_face=(new_of >= 0).sum(1))
    return out_verts, np.array(out_faces, dtype=np.int32).reshape(-1, 3), info


def subdivide_to_size(vertices, faces, max_edge, max_iter=10):
    """Adaptive rounds until one marks nothing: (vertices, faces, rounds that split something).  RuntimeError naming the edges still
    above ``max_edge`` when ``max_iter`` rounds did not suffice."""
    v, f = np.asarray(vertices), np.asarray(faces)
    for it in range(max_iter + 1):
        n = int(marks(v, f, edge_table(f, v.shape[0]), max_edge=max_edge).sum())
        if n == 0:
            return v, f, it
        if it == max_iter:
            raise RuntimeError(f"{n} edges are still longer than {max_edge} after {max_iter} rounds")
        v, f, _ = subdivide(v, f, "midpoint", max_edge=max_edge)


def backward(edge_verts, n_vertices, grad_out):
    """g_v[i] = g[i] + 0.5 sum of g[V + e] over the edges e at i, every sum by math.fsum and rounded once to the gradient's dtype."""
    g = np.asarray(grad_out)
    V, ev = int(n_vertices), np.asarray(edge_verts).reshape(-1, 2)
    terms = [[[float(g[i, k])] for k in range(3)] for i in range(V)]
    for e, (a, b) in enumerate(ev.tolist()):
        for k in range(3):
            w = 0.5 * float(g[V + e, k])
            terms[a][k].append(w)
            terms[b][k].append(w)
    out = np.array([[math.fsum(c) for c in row] for row in terms], dtype=np.float64).reshape(V, 3)
    mag = np.array([[math.fsum(abs(w) for w in c) for c in row] for row in terms], dtype=np.float64).reshape(V, 3)
    return out.astype(g.dtype), mag, np.array([len(row[0]) for row in terms])


# ---- checks the tests share -----------------------------------------------------------------------------------------------------------
def total_area(vertices, faces):
    return math.fsum(T.face_terms(vertices, faces)[0].tolist())


def edge_lengths2(vertices, faces):
    t = edge_table(faces, np.asarray(vertices).shape[0])
    d = np.asarray(vertices).astype(np.float64)[t["hi"]] - np.asarray(vertices).astype(np.float64)[t["lo"]]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def triangle():
    return np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0.5]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def regular_grid(n=7):
    """n x n integer points in the plane z = 2, every cell cut along the same diagonal: every interior vertex has valence 6 and its
    neighbours are symmetric about it."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i, j, np.full_like(i, 2)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: a * n + b
    f = []
    for a in range(n - 1):
        for b in range(n - 1):
            f += [[idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)], [idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)]]
    return v, np.array(f, dtype=np.int32)


def odd_mesh():
    """An unreferenced vertex (0), a repeated face, an edge with four uses, three of them in one direction ({1, 2}), a cube with one
    face flipped (two edges used twice in one direction) and a vertex referenced once only."""
    rng = np.random.RandomState(7)
    cv, cf = T.cube_one_face_flipped()
    v = np.concatenate([rng.randn(7, 3).astype(np.float32), cv + np.float32(4.0)])
    f = np.concatenate([np.array([[1, 2, 3], [1, 2, 3], [2, 1, 4], [1, 2, 5], [3, 2, 6]], dtype=np.int32), cf + 7])
    return v, f.astype(np.int32)


def voxel_ball(n=7, radius=2.6, seed=11):
    """The boundary of the voxels of an n^3 lattice whose centres lie within ``radius`` of the middle: every boundary square as two
    triangles, corners welded, faces in a seeded shuffle.  Closed, with the valences 3 to 6 a marching-cubes mesh has."""
    g = np.arange(n) - (n - 1) / 2.0
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    inside = np.pad(np.sqrt(x * x + y * y + z * z) <= radius, 1)
    ids, verts, faces = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for i, j, k in np.argwhere(inside).tolist():
        for axis in range(3):
            for side in (0, 1):
                q = [i, j, k]
                q[axis] += 2 * side - 1
                if inside[tuple(q)]:
                    continue
                u, w = (axis + 1) % 3, (axis + 2) % 3
                corners = []
                for du, dw in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = [i, j, k]
                    p[axis] += side
                    p[u] += du
                    p[w] += dw
                    corners.append(vid(tuple(p)))
                if not side:
                    corners = corners[::-1]
                faces += [[corners[0], corners[1], corners[2]], [corners[0], corners[2], corners[3]]]
    f = np.array(faces, dtype=np.int32)
    return np.array(verts, dtype=np.float32), f[np.random.RandomState(seed).permutation(f.shape[0])]


def stretched_torus():
    """The torus stretched along z: with FOUR_CASES_MAX_EDGE faces with 0, 1, 2 and 3 edges that are too long all occur."""
    v, f = T.torus()
    return (v * np.array([1.0, 1.0, 3.0])).astype(np.float32), f


FOUR_CASES_MAX_EDGE = 0.5


def strip(n_faces=10):
    return T.grid_strip(n_faces)


def chunk_strip(three_f):
    """A strip whose half-edge count is ``three_f``: one below, at and one above a multiple of the scan chunk."""
    assert three_f % 3 == 0
    return T.grid_strip(three_f // 3)


FIXTURES = {
    "empty": S.empty_mesh,
    "triangle": triangle,
    "tetrahedron": T.tetrahedron,
    "fan300": S.fan,
    "odd": odd_mesh,
    "grid9": S.planar_grid,
    "regular7": regular_grid,
    "torus": T.torus,
    "stretched_torus": stretched_torus,
    "voxel_ball": voxel_ball,
    "strip10": strip,
    "chunk_below": lambda: chunk_strip(MT_CHUNK - 1),               # 3 F = 1023
    "chunk_at": lambda: chunk_strip(3 * MT_CHUNK),                  # 3 F = 3072, F = 1024
    "chunk_above": lambda: chunk_strip(2 * MT_CHUNK + 1),           # 3 F = 2049
}
INTEGER_GRIDS = ("grid9", "regular7", "voxel_ball")
CLOSED = ("tetrahedron", "torus", "stretched_torus", "voxel_ball")


def fixture(name):
    v, f = FIXTURES[name]()
    return np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)
