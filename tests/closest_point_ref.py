"""vt_closest_point_mesh restated twice in float64 numpy ("closest_point.hip"), and the meshes the tests share.

by_regions  the kernel's algorithm in the kernel's operation order: a record per face (corner a, edges ab and ac, ab.ab, ab.ac, ac.ac,
            degenerate when ab x ac is exactly zero), the seven Voronoi regions of the closed triangle from d1 = ab.ap, d2 = ac.ap and the
            record's products, two divisions, q = (a + ab v) + ac w, d2 = (dx^2 + dy^2) + dz^2; a degenerate face is the nearest of its
            edges ab, ac, bc; the minimum over the faces is the first among equals.  Every product and sum is a separate rounding, so the
            device's outputs equal these bit for bit.
by_parts    an independent form: the projection onto the triangle's plane where it falls inside (edge functions against the normal),
            otherwise the nearest of the three segments; degenerate faces are their three segments.

Both return (d2 [N] f64, face [N] int32, closest [N,3] f64).
"""
import numpy as np


def _corners(verts, faces, dtype=np.float64):
    v = np.asarray(verts, dtype=np.float32).astype(dtype)
    f = np.asarray(faces).astype(np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def _dot(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def _segment(p, o, e, ew, ee):
    """cp_segment: nearest point of o + t e, t in [0, 1]; ew = e.(p - o), ee = e.e.  p [N,1,3], o / e [1,F,3]."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0.0, ew / ee, 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    q = o + e * t[..., None]
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], q


def _edges_nearest(p, a, ab, ac, d1, d2, d00, d11):
    """The degenerate face: the nearest of ab, ac, bc, the first among equals."""
    best, q = _segment(p, a, ab, d1, d00)
    dac, qac = _segment(p, a, ac, d2, d11)
    take = dac < best
    best, q = np.where(take, dac, best), np.where(take[..., None], qac, q)
    b, e = a + ab, ac - ab
    w = p - b
    dbc, qbc = _segment(p, b, e, _dot(e, w), _dot(e, e))
    take = dbc < best
    return np.where(take, dbc, best), np.where(take[..., None], qbc, q)


def pairs_by_regions(verts, faces, pts, dtype=np.float64):
    """(d2 [N,F], q [N,F,3]) of every (query, face) pair, the kernel's cp_face (``dtype``: the arithmetic's; the kernel's is float64)."""
    a, b, c = _corners(verts, faces, dtype)
    p = np.asarray(pts).astype(dtype)[:, None, :]
    ab, ac = (b - a)[None], (c - a)[None]
    a = a[None]
    d00, d01, d11 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    n = _cross(ab, ac)
    degenerate = (n[..., 0] == 0.0) & (n[..., 1] == 0.0) & (n[..., 2] == 0.0)
    ap = p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4, d5, d6 = d1 - d00, d2 - d01, d1 - d01, d2 - d11
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    nv, nw, den = vb, vc, (va + vb) + vc
    on_bc = np.zeros(d1.shape, dtype=bool)

    def override(cond, nv_new, nw_new, den_new, bc):
        nonlocal nv, nw, den, on_bc
        nv, nw, den = np.where(cond, nv_new, nv), np.where(cond, nw_new, nw), np.where(cond, den_new, den)
        on_bc = np.where(cond, bc, on_bc)
    override((va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0), zero, e43, e43 + e56, True)
    override((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), zero, d2, d2 - d6, False)
    override((d6 >= 0.0) & (d5 <= d6), zero, one, one, False)
    override((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), d1, zero, d1 - d3, False)
    override((d3 >= 0.0) & (d4 <= d3), one, zero, one, False)
    override((d1 <= 0.0) & (d2 <= 0.0), zero, zero, one, False)
    override(~(den > 0.0), zero, zero, one, False)
    w = nw / den
    v = np.where(on_bc, 1.0 - w, nv / den)
    q = (a + ab * v[..., None]) + ac * w[..., None]
    d = p - q
    dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    if degenerate.any():
        dd, qd = _edges_nearest(p, a, ab, ac, d1, d2, d00, d11)
        dist, q = np.where(degenerate, dd, dist), np.where(degenerate[..., None], qd, q)
    return dist, q


def pairs_by_parts(verts, faces, pts, dtype=np.float64):
    """(d2 [N,F], q [N,F,3]): plane projection where it falls inside the triangle, otherwise the nearest of the three segments."""
    a, b, c = _corners(verts, faces, dtype)
    p = np.asarray(pts).astype(dtype)[:, None, :]
    a, b, c = a[None], b[None], c[None]
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    best, q = None, None
    for o, e in ((a, b - a), (b, c - b), (c, a - c)):
        dist, qs = _segment(p, o, e, _dot(e, p - o), _dot(e, e))
        if best is None:
            best, q = dist, qs
        else:
            take = dist < best
            best, q = np.where(take, dist, best), np.where(take[..., None], qs, q)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = _dot(n, p - a) / nn
        foot = p - n * h[..., None]
        inside = (nn > 0.0)
        for o, e in ((a, b - a), (b, c - b), (c, a - c)):
            inside = inside & (_dot(_cross(e, foot - o), n) >= 0.0)
        dplane = _dot(n, p - a) * h
    best = np.where(inside, dplane, best)
    q = np.where(inside[..., None], foot, q)
    return best, q


def _reduce(pairs, verts, faces, pts, chunk, dtype=np.float64):
    pts = np.asarray(pts)
    faces = np.asarray(faces)
    N, F = pts.shape[0], faces.shape[0]
    d2 = np.full(N, np.inf)
    face = np.full(N, -1, dtype=np.int32)
    closest = np.full((N, 3), np.nan)
    rows = np.arange(N)
    for f0 in range(0, F, chunk):
        dist, q = pairs(verts, faces[f0:f0 + chunk], pts, dtype)
        j = np.argmin(dist, axis=1)                     # the first among equal minima
        d = dist[rows, j]
        take = d < d2                                   # strict: an earlier chunk keeps a tie
        d2[take], face[take], closest[take] = d[take], (f0 + j[take]).astype(np.int32), q[rows, j][take]
    return d2, face, closest


def by_regions(verts, faces, pts, chunk=2048, dtype=np.float64):
    return _reduce(pairs_by_regions, verts, faces, pts, chunk, dtype)


def by_parts(verts, faces, pts, chunk=2048, dtype=np.float64):
    return _reduce(pairs_by_parts, verts, faces, pts, chunk, dtype)


# ---- meshes and queries the tests share ------------------------------------------------------------------------------------------------
def torus(nu, nv, R=0.30, r=0.12, seed=None):
    """(verts f32 [nu*nv,3], faces i32 [2*nu*nv,3]) of a torus, rotated by a seeded rotation when ``seed`` is given."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u, v = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    faces = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    if seed is not None:
        q, _ = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
        verts = verts @ q.T
    return verts.astype(np.float32), faces.astype(np.int32)


def soup(F, seed):
    """F triangles over 3 + F // 2 random vertices in [-0.5, 0.5]^3 (faces share vertices: exact ties between neighbours occur)."""
    rng = np.random.RandomState(seed)
    V = 3 + F // 2
    verts = (rng.rand(V, 3) - 0.5).astype(np.float32)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    return verts, faces


def queries(N, seed, verts=None, faces=None):
    """N float32 queries in [-0.6, 0.6]^3; with a mesh, every fourth sits on a vertex and every fourth + 1 on an edge's midpoint (rounded to f32)."""
    rng = np.random.RandomState(seed)
    pts = (1.2 * rng.rand(N, 3) - 0.6).astype(np.float32)
    if verts is not None:
        f = np.asarray(faces)[rng.randint(len(faces), size=N)]
        on_v = verts[f[:, 0]]
        mid = (0.5 * (verts[f[:, 1]].astype(np.float64) + verts[f[:, 2]].astype(np.float64))).astype(np.float32)
        pts[0::4] = on_v[0::4]
        pts[1::4] = mid[1::4]
    return pts


CUBE_V = np.array([[x, y, z] for x in (-0.25, 0.25) for y in (-0.25, 0.25) for z in (-0.25, 0.25)], dtype=np.float32)
# outward-oriented: vertex index = 4 ix + 2 iy + iz
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                  dtype=np.int32)
