"""The definition of csrc/mesh_smooth.hip's results in numpy, and the meshes the tests use.

    adjacency(faces, n_vertices) -> dict   offsets int32 [V+1], neighbors int32 [nnz], boundary_edge uint8 [nnz], boundary_vertex uint8 [V]
    weights(vertices, adj, scheme) -> float64 [nnz]
    row_mean(x, adj, w, boundary) -> (m float64 [V,3], moves bool [V])
    smooth(vertices, adj, method, iterations, lam, mu, alpha, beta, weights, boundary) -> vertices in the input's dtype

The undirected edges {a, b}, a != b, each once however many faces use it, come from ``unique`` over 64-bit keys; an edge used by exactly
one face is a boundary edge.  Row i holds the other ends of vertex i's edges in ascending order (``lexsort``).  The row mean is
(sum_j w_ij x_j) / (sum_j w_ij): both sums start at 0.0 and take the row's entries in ascending neighbour order, per coordinate, in
float64, the product rounded before it is added -- here a loop over the k-th column of the rows, which is that order for every row at
once.  An entry takes part unless its weight is 0 or, under ``'loop'``, its vertex is a boundary vertex and its edge is not a boundary
edge.  A vertex moves unless it is pinned (``'pin'`` and a boundary vertex) or its weight sum is not above 0; one that does not move keeps
its bits through every pass.  Positions are float64 from the first pass to the last and are rounded once."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_topo_ref as T  # noqa: E402

log_line = T.log_line
METHODS = ("laplacian", "taubin", "humphrey")
WEIGHTS = ("uniform", "inverse_distance")
BOUNDARIES = ("pin", "free", "loop")


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def adjacency(faces, n_vertices):
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    V = int(n_vertices)
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("a face index lies outside [0, V)")
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    proper = a != b
    lo, hi = np.minimum(a, b)[proper], np.maximum(a, b)[proper]
    keys, uses = np.unique((lo << 32) | hi, return_counts=True)
    lo, hi = keys >> 32, keys & 0xffffffff
    row = np.concatenate([lo, hi])
    col = np.concatenate([hi, lo])
    be = np.concatenate([uses == 1, uses == 1])
    order = np.lexsort((col, row))
    row, col, be = row[order], col[order], be[order]
    offsets = np.zeros(V + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(np.bincount(row, minlength=V))
    bv = np.zeros(V, dtype=np.uint8)
    bv[row[be]] = 1
    return dict(offsets=offsets, neighbors=col.astype(np.int32), boundary_edge=be.astype(np.uint8), boundary_vertex=bv)


def _rows(adj):
    """(row of every entry, its position within the row, the largest degree)."""
    off = adj["offsets"].astype(np.int64)
    deg = np.diff(off)
    row = np.repeat(np.arange(deg.shape[0]), deg)
    return row, np.arange(off[-1]) - off[row], int(deg.max()) if deg.size else 0


def weights(vertices, adj, scheme="inverse_distance"):
    nb = adj["neighbors"]
    if scheme == "uniform":
        return np.ones(nb.shape[0], dtype=np.float64)
    x = np.asarray(vertices).astype(np.float64)
    row, _, _ = _rows(adj)
    d = x[nb] - x[row]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    w = np.zeros(nb.shape[0], dtype=np.float64)
    np.divide(1.0, dist, out=w, where=dist > 0)
    return w


def row_mean(x, adj, w, boundary):
    """(m, moves): m[i] is the row mean of x at vertex i where moves[i], and x[i] elsewhere."""
    V = x.shape[0]
    nb, bv = adj["neighbors"], adj["boundary_vertex"].astype(bool)
    row, pos, dmax = _rows(adj)
    take = w != 0.0
    if boundary == "loop":
        take &= ~bv[row] | adj["boundary_edge"].astype(bool)
    s, sw = np.zeros((V, 3), dtype=np.float64), np.zeros(V, dtype=np.float64)
    for k in range(dmax):                                         # the k-th entry of every row that has one: ascending neighbour order
        sel = (pos == k) & take
        r, j, wk = row[sel], nb[sel], w[sel]
        s[r] = s[r] + wk[:, None] * x[j]
        sw[r] = sw[r] + wk
    moves = sw > 0.0
    if boundary == "pin":
        moves &= ~bv
    m = x.copy()
    m[moves] = s[moves] / sw[moves][:, None]
    return m, moves


def smooth(vertices, adj, method="taubin", iterations=10, lam=0.5, mu=-0.53, alpha=0.1, beta=0.5, weights_scheme="uniform", boundary="pin"):
    vertices = np.asarray(vertices)
    if iterations == 0 or adj["neighbors"].shape[0] == 0:
        return vertices.copy()
    o = vertices.astype(np.float64)
    w = weights(vertices, adj, weights_scheme)
    x = o.copy()
    if method == "humphrey":
        for _ in range(iterations):
            q = x
            m, moves = row_mean(q, adj, w, boundary)
            x = m                                                   # (m is q where the vertex does not move)
            b = x - (alpha * o + (1.0 - alpha) * q)
            mb, _ = row_mean(b, adj, w, boundary)
            step = beta * b + (1.0 - beta) * mb
            x = np.where(moves[:, None], x - step, x)
    else:
        passes = 2 * iterations if method == "taubin" else iterations
        for k in range(passes):
            c = mu if method == "taubin" and k % 2 == 1 else lam
            m, moves = row_mean(x, adj, w, boundary)
            x = np.where(moves[:, None], x + c * (m - x), x)
    return x.astype(vertices.dtype)


# ---- independent constructions the CPU test compares with -------------------------------------------------------------------------------
def adjacency_by_sets(faces, n_vertices):
    """(list of sorted neighbour lists, set of boundary edges) by Python sets and a dict of use counts.  A use is a half-edge, as in
    mesh_fill_ref: the degenerate face (a, b, a) uses {a, b} twice, so that edge is no boundary edge."""
    nbrs = [set() for _ in range(n_vertices)]
    count = {}
    for tri in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                e = (min(a, b), max(a, b))
                count[e] = count.get(e, 0) + 1
                nbrs[a].add(b)
                nbrs[b].add(a)
    return [sorted(s) for s in nbrs], {e for e, n in count.items() if n == 1}


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def icosahedron():
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int32)
    return v, f


def planar_grid(n=9):
    """An n x n grid of integer points in the plane z = 2, every cell cut along alternating diagonals (so that every interior vertex's
    neighbours are symmetric about it: 4 or 8 of them)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i, j, np.full_like(i, 2)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: a * n + b
    f = []
    for a in range(n - 1):
        for b in range(n - 1):
            p, q, r, s = idx(a, b), idx(a + 1, b), idx(a + 1, b + 1), idx(a, b + 1)
            f += [[p, q, r], [p, r, s]] if (a + b) % 2 == 0 else [[p, q, s], [q, r, s]]
    return v, np.array(f, dtype=np.int32)


def fan(n=300):
    """A hub (vertex 0) with n spokes on a wavy circle: one row of n entries."""
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t) * (1 + 0.1 * np.sin(7 * t)), np.sin(t) * (1 + 0.1 * np.cos(5 * t)), 0.2 * np.sin(3 * t)], -1)
    v = np.concatenate([[[0.03, -0.02, 0.5]], rim]).astype(np.float32)
    f = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32)
    return v, f


def odd_mesh():
    """Unreferenced vertices (0, 7, 12), a duplicated face, an edge shared by three faces ({1, 2}), a face with a repeated index and
    two components (the second a tetrahedron)."""
    rng = np.random.RandomState(5)
    v = rng.randn(13, 3).astype(np.float32)
    f = np.array([[1, 2, 3], [1, 2, 3], [2, 1, 4], [1, 2, 5], [3, 2, 6], [6, 6, 3], [4, 4, 4],
                  [8, 10, 9], [8, 9, 11], [9, 10, 11], [8, 11, 10]], dtype=np.int32)
    return v, f


def coincident():
    """A tetrahedron-like mesh in which vertices 1 and 2 coincide, and vertex 5 whose every neighbour coincides with it."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 3, 3], [3, 3, 3], [3, 3, 3]], dtype=np.float32)
    f = np.array([[0, 1, 3], [1, 2, 3], [0, 2, 4], [2, 1, 4], [0, 3, 4], [5, 6, 7]], dtype=np.int32)
    return v, f


def empty_mesh():
    return np.array([[0.25, -1.5, 3.0]], dtype=np.float32), np.zeros((0, 3), dtype=np.int32)


def sphere_volume(radius, n=24):
    """tanh(4 (|x - c| - R)) on an n^3 lattice, float32: steep logits, as an occupancy field has them."""
    g = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return np.tanh(4.0 * (np.sqrt(x * x + y * y + z * z) - radius)).astype(np.float32)


CLOSED_RADIUS, CUT_RADIUS = 8.3, 14.0

FIXTURES = {
    "tetrahedron": T.tetrahedron,
    "empty": empty_mesh,
    "icosahedron": icosahedron,
    "grid9": planar_grid,
    "fan300": fan,
    "odd": odd_mesh,
    "coincident": coincident,
}


def fixture(name):
    v, f = FIXTURES[name]()
    return np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int32)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def radial_std(vertices, n=24):
    r = np.linalg.norm(np.asarray(vertices, dtype=np.float64) - (n - 1) / 2.0, axis=1)
    return float(r.std())
