"""A numpy restatement of csrc/mesh_simplify.hip: simplification by vertex clustering with quadric-error placement (Lindstrom 2000) and
vertex welding, and the meshes the tests add to tests/mesh_topo_ref.py's.  This file is the definition; the kernels equal it bit for bit.

    cluster(vertices, faces, R) -> dict       the grid (lo, h), every vertex's cell, cluster_of_vertex, K, the representatives
    cluster_faces(faces, cov, V, unique)      the faces on cluster ids: degenerate ones dropped, of equal unordered triples the first kept
    quadrics(vertices, faces, c)              per cluster the 10 summed quadric values, the 3 summed centre-relative coordinates, the count
    place(...)                                the cluster's vertex: 'quadric' (eigen-solve about the mean, fallback to the mean) or 'mean'
    simplify(vertices, faces, resolution= | nfaces=, placement=) -> dict
    weld(vertices, faces, tol, unique_faces)  merge_vertices
    energy(q, x), energy_gate(q, x)           the quadric error of a position and the rounding gate of comparing two of them

Conventions: float64 on exactly widened inputs, one rounding per operation in the order written here, the lowest index among equals.
A face with an index outside [0, V) takes no part.  A vertex no valid face references belongs to no cluster (-1)."""
import math

import numpy as np

SWEEPS = 8                 # cyclic Jacobi sweeps over (0,1), (0,2), (1,2): a symmetric 3x3 settles in 4 to 6
EIG_REL = 1e-3             # eigenvalues <= EIG_REL * the largest are dropped (Lindstrom's threshold)
MAX_R = 1 << 20
MAX_K = 1 << 21            # three cluster ids fill 63 bits of a face key


def valid_faces(faces, V):
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def referenced(faces, V):
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ref = np.zeros(V, dtype=bool)
    ref[f[valid_faces(f, V)].reshape(-1)] = True
    return ref


# ---- 1. grid ---------------------------------------------------------------------------------------------------------------------------
def grid(vertices, faces, R):
    v = np.asarray(vertices).astype(np.float64)
    ref = referenced(faces, v.shape[0])
    if not np.isfinite(v[ref]).all():
        raise ValueError("a referenced vertex has a non-finite coordinate")
    lo, hi = v[ref].min(0), v[ref].max(0)
    d = hi - lo
    L = max(max(d[0], d[1]), d[2])
    return lo, L, L / R


def cells_of(v, lo, h, R):
    """min(R - 1, floor((x - lo) / h)) per axis; everything is cell 0 where the box has no extent."""
    if h == 0.0:
        return np.zeros(v.shape, dtype=np.int64)
    t = np.floor((v - lo) / h)
    return np.where(t >= R - 1, R - 1, np.where(t > 0, t, 0)).astype(np.int64)


def centre_of(cell, lo, h):
    return lo + (cell.astype(np.float64) + 0.5) * h


# ---- 2. clusters -----------------------------------------------------------------------------------------------------------------------
def clusters_of_keys(keys, member, solo=None):
    """cluster_of_vertex, K, representatives: the vertices ``member`` marks, grouped by equal rows of ``keys`` (``solo``: in a group of
    their own); the representative is the group's lowest index, the groups are numbered by ascending representative."""
    V = keys.shape[0]
    rep = np.full(V, -1, dtype=np.int64)
    groups = {}
    for v in np.nonzero(member)[0].tolist():
        if solo is not None and solo[v]:
            rep[v] = v
        else:
            rep[v] = groups.setdefault(tuple(keys[v].tolist()), v)
    reps = np.nonzero(rep == np.arange(V))[0]
    rank = np.full(V, -1, dtype=np.int64)
    rank[reps] = np.arange(reps.shape[0])
    cov = np.where(rep >= 0, rank[np.maximum(rep, 0)], -1).astype(np.int32)
    return cov, int(reps.shape[0]), reps.astype(np.int32)


def cluster(vertices, faces, R):
    if int(R) != R or not 1 <= R <= MAX_R:
        raise ValueError(f"resolution must be an integer in [1, {MAX_R}]")
    v = np.asarray(vertices).astype(np.float64)
    lo, L, h = grid(vertices, faces, int(R))
    cell = cells_of(v, lo, h, int(R))
    cov, K, rep = clusters_of_keys(cell, referenced(faces, v.shape[0]))
    return dict(lo=lo, L=L, h=h, cell=cell, cluster_of_vertex=cov, K=K, rep=rep, R=int(R))


# ---- 5. faces --------------------------------------------------------------------------------------------------------------------------
def cluster_faces(faces, cov, V, unique=True):
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ids = np.asarray(cov)[f[valid_faces(f, V)]].reshape(-1, 3)
    ids = ids[(ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])]
    if unique and ids.shape[0]:
        _, first = np.unique(np.sort(ids, axis=1), axis=0, return_index=True)          # (the first occurrence: the lowest face index)
        ids = ids[np.sort(first)]
    return ids.astype(np.int32).reshape(-1, 3)


# ---- 3. quadrics -----------------------------------------------------------------------------------------------------------------------
def exponent_of(big):
    e = (np.asarray(big, dtype=np.float64).view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7ff
    return np.where(e == 0, 1, e) - 1023


def fixed_sums(terms, owner, K, e):
    """Per owner the sum of its terms as csrc/mesh_topo.hip accumulates: two integer limbs against the exponent e[owner]."""
    s = np.ldexp(terms, (30 - e[owner]).astype(np.int32))
    h = np.trunc(s)
    l = np.rint(np.ldexp(s - h, 31))
    hi, lo = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    np.add.at(hi, owner, h.astype(np.int64))
    np.add.at(lo, owner, l.astype(np.int64))
    return np.ldexp(hi.astype(np.float64) + np.ldexp(lo.astype(np.float64), -31), (e - 30).astype(np.int32))


def quadric_terms(vertices, faces, c):
    """owner [N], terms [N,10]: one row per (face, distinct cluster among its corners) -- the upper triangle of [n,d][n,d]^T in the order
    nx nx, nx ny, nx nz, nx d, ny ny, ny nz, ny d, nz nz, nz d, d d; n = (b - a) x (c - a) unnormalised, d = -n.(p - centre) with p
    the face's first corner (a, b, c order) in that cluster."""
    v = np.asarray(vertices).astype(np.float64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    f = f[valid_faces(f, v.shape[0])]
    cov, lo, h, cell = c["cluster_of_vertex"], c["lo"], c["h"], c["cell"]
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = p1 - p0, p2 - p0
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    ids = cov[f].astype(np.int64)
    owners, rows = [], []
    for k in range(3):
        first = np.ones(f.shape[0], dtype=bool)
        for j in range(k):
            first &= ids[:, j] != ids[:, k]
        q = v[f[:, k]] - centre_of(cell[f[:, k]], lo, h)
        d = -((nx * q[:, 0] + ny * q[:, 1]) + nz * q[:, 2])
        t = np.stack([nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d], -1)
        owners.append(ids[first, k])
        rows.append(t[first])
    return np.concatenate(owners), np.concatenate(rows)


def quadrics(vertices, faces, c, with_faces=True):
    """q [K,10], s [K,3], n [K]: the fixed-point sums.  One exponent per cluster for the ten quadric values (the largest |term| of the
    cluster) and one for the three coordinate sums."""
    v = np.asarray(vertices).astype(np.float64)
    cov, K = c["cluster_of_vertex"], c["K"]
    member = np.nonzero(cov >= 0)[0]
    own_v = cov[member].astype(np.int64)
    rel = v[member] - centre_of(c["cell"][member], c["lo"], c["h"])
    big = np.zeros(K)
    np.maximum.at(big, own_v, np.abs(rel).max(1))
    e = exponent_of(big)
    s = np.stack([fixed_sums(rel[:, k], own_v, K, e) for k in range(3)], -1)
    n = np.bincount(own_v, minlength=K).astype(np.int64)
    q = np.zeros((K, 10))
    if with_faces:
        owner, terms = quadric_terms(vertices, faces, c)
        big = np.zeros(K)
        np.maximum.at(big, owner, np.abs(terms).max(1))
        e = exponent_of(big)
        q = np.stack([fixed_sums(terms[:, k], owner, K, e) for k in range(10)], -1)
    return q, s, n


# ---- 4. placement ----------------------------------------------------------------------------------------------------------------------
def jacobi(A):
    """Eigenvalues (the diagonal that is left) and eigenvectors (columns of v) of a symmetric 3x3, on Python floats."""
    a = [[float(A[i][j]) for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = v[k][p], v[k][q]
                v[k][p] = c * vp - s * vq
                v[k][q] = s * vp + c * vq
    return [a[0][0], a[1][1], a[2][2]], v


def solve(q, x0):
    """x = x0 + V pinv(Lambda) V^T (-b - A x0) over the eigenvalues above EIG_REL of the largest."""
    A = [[q[0], q[1], q[2]], [q[1], q[4], q[5]], [q[2], q[5], q[7]]]
    b = [q[3], q[6], q[8]]
    g = [(-b[i]) - ((A[i][0] * x0[0] + A[i][1] * x0[1]) + A[i][2] * x0[2]) for i in range(3)]
    lam, v = jacobi(A)
    bound = EIG_REL * max(max(lam[0], lam[1]), lam[2])
    coef = []
    for k in range(3):
        proj = (v[0][k] * g[0] + v[1][k] * g[1]) + v[2][k] * g[2]
        coef.append(proj / lam[k] if lam[k] > bound else 0.0)
    return [x0[i] + ((v[i][0] * coef[0] + v[i][1] * coef[1]) + v[i][2] * coef[2]) for i in range(3)]


SOLVE_SLACK = 2.0 ** -52 / EIG_REL
BOX_SLACK = 2.0 ** -51


def cell_bound(lo, L, h):
    """Per axis the largest |x| that still counts as inside the cell: h / 2 and what rounding can add to it.  In exact arithmetic a
    vertex on the box's upper face -- step 1 clamps it into the last cell -- lies exactly on that cell's face, |x| = h / 2; the computed
    centre carries up to two roundings at the box's scale (|lo| + L) and the solve inverts eigenvalues down to EIG_REL of the largest,
    so a computed x can exceed h / 2 by (2^-52 / EIG_REL) h / 2 + 2^-51 (|lo| + L) with the position still on the face."""
    half = h / 2.0
    return [half + (half * SOLVE_SLACK + (abs(float(lo[a])) + L) * BOX_SLACK) for a in range(3)]


def place(q, s, n, c, placement, dtype):
    """positions [K,3] in ``dtype``, the centre-relative x [K,3], x0 [K,3], and the number of fallbacks."""
    K, h = c["K"], float(c["h"])
    centre = centre_of(c["cell"][c["rep"]], c["lo"], c["h"]).reshape(K, 3)
    x0 = s / n[:, None].astype(np.float64)
    x = x0.copy()
    fallbacks = 0
    if placement == "quadric":
        bound = cell_bound(c["lo"], float(c["L"]), h)
        for k in range(K):
            xs = solve([float(t) for t in q[k]], [float(t) for t in x0[k]])
            if all(abs(xs[a]) <= bound[a] for a in range(3)):
                x[k] = xs
            else:
                fallbacks += 1
    elif placement != "mean":
        raise ValueError("placement must be 'quadric' or 'mean'")
    return (centre + x).astype(dtype), x, x0, fallbacks


def energy(q, x):
    """x^T A x + 2 b^T x + c of the summed quadric q [10] at the centre-relative x."""
    return float((q[0] * x[0] * x[0] + q[4] * x[1] * x[1] + q[7] * x[2] * x[2]) + 2.0 * (q[1] * x[0] * x[1] + q[2] * x[0] * x[2] + q[5] * x[1] * x[2])
                 + 2.0 * (q[3] * x[0] + q[6] * x[1] + q[8] * x[2]) + q[9])


def energy_gate(q, xa, xb):
    """The gate of E(xa) <= E(xb) + gate.  In exact arithmetic the solve can only lower E (it subtracts sum proj^2 / lambda over the kept
    eigenvalues).  M = the sum of |monomial| of E at both positions bounds what the evaluations round; the solve inverts eigenvalues
    down to EIG_REL of the largest, so its own rounding shows in E by up to 1 / EIG_REL ulps of M: gate = 2^-52 / EIG_REL * M."""
    q = np.abs(np.asarray(q, dtype=np.float64))
    m = 0.0
    for x in (np.abs(np.asarray(xa, dtype=np.float64)), np.abs(np.asarray(xb, dtype=np.float64))):
        m += energy(q, x)
    return 2.0 ** -52 / EIG_REL * m


# ---- 6. the whole thing ----------------------------------------------------------------------------------------------------------------
def simplify_at(vertices, faces, R, placement="quadric"):
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    c = cluster(vertices, faces, R)
    out_f = cluster_faces(faces, c["cluster_of_vertex"], vertices.shape[0])
    q, s, n = quadrics(vertices, faces, c, with_faces=placement == "quadric")
    pos, x, x0, fallbacks = place(q, s, n, c, placement, vertices.dtype)
    return dict(vertices=pos, faces=out_f, cluster_of_vertex=c["cluster_of_vertex"], K=c["K"], R=int(R), probes=0, fallbacks=fallbacks,
                q=q, x=x, x0=x0, h=c["h"], unchanged=False)


def count_at(vertices, faces, R):
    c = cluster(vertices, faces, R)
    return cluster_faces(faces, c["cluster_of_vertex"], np.asarray(vertices).shape[0]).shape[0]


def search(count, nfaces):
    """(R, probes): gallop from (1, 2) while count(hi) <= nfaces, then bisect on the same predicate; the answer is lo."""
    lo, hi, probes = 1, 2, 0
    while hi <= MAX_R:
        probes += 1
        if count(hi) > nfaces:
            break
        lo, hi = hi, 2 * hi
    hi = min(hi, MAX_R + 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        probes += 1
        if count(mid) <= nfaces:
            lo = mid
        else:
            hi = mid
    return lo, probes


def simplify(vertices, faces, resolution=None, nfaces=None, placement="quadric"):
    if (resolution is None) == (nfaces is None):
        raise ValueError("exactly one of nfaces / resolution")
    if resolution is not None:
        return simplify_at(vertices, faces, resolution, placement)
    if int(nfaces) != nfaces or nfaces < 1:
        raise ValueError("nfaces must be a positive integer")
    if np.asarray(faces).shape[0] <= nfaces:
        return dict(vertices=vertices, faces=faces, unchanged=True, R=None, probes=0, K=None, fallbacks=0)
    R, probes = search(lambda r: count_at(vertices, faces, r), int(nfaces))
    out = simplify_at(vertices, faces, R, placement)
    out["probes"] = probes
    return out


# ---- 7. welding ------------------------------------------------------------------------------------------------------------------------
def weld(vertices, faces, tol=0.0, unique_faces=False):
    """(vertices, faces, cluster_of_vertex): tol = 0 merges equal coordinates (-0.0 = +0.0; a vertex with a NaN merges with nothing),
    tol > 0 merges equal rint(x / tol) per axis."""
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    v = vertices.astype(np.float64)
    V = v.shape[0]
    if not tol >= 0.0 or not math.isfinite(tol):
        raise ValueError("tol must be finite and >= 0")
    ref = referenced(faces, V)
    solo = np.isnan(v).any(1)
    if tol == 0.0:
        keys = np.where(v == 0.0, 0.0, v).view(np.int64)
    else:
        r = np.rint(v / tol)
        if not (np.abs(r[ref & ~solo]) < 2.0 ** 63).all():
            raise ValueError("a key lies beyond the int64 range")
        keys = np.where(np.abs(r) < 2.0 ** 63, r, 0.0).astype(np.int64)
    cov, K, rep = clusters_of_keys(keys, ref, solo)
    return vertices[rep], cluster_faces(faces, cov, V, unique=unique_faces), cov


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def cube_grid(n=12):
    """The unit cube with n x n quads per side, outward: 6 n^2 + 2 vertices, 12 n^2 faces, float32."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:                      # (u x w = +axis: counter-clockwise seen from +axis; the low side looks the other way)
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return (np.array(verts, dtype=np.float64) / n).astype(np.float32), np.array(faces, dtype=np.int32)


def surface_distance_unit_cube(p):
    """The distance of points in or near the unit cube to its surface."""
    p = np.asarray(p).astype(np.float64)
    inside = np.minimum(p, 1.0 - p).min(1)
    outside = np.sqrt((np.maximum(np.maximum(-p, p - 1.0), 0.0) ** 2).sum(1))
    return np.where(inside >= 0, inside, outside)


def lattice_mesh(n=4):
    """An n x n x 1 sheet of unit squares with integer coordinates, lifted to z = n at one corner: with R = n every vertex sits on a
    cell boundary, those at x = n or y = n on the box's upper faces."""
    v = np.array([[i, j, n if (i, j) == (n, n) else 0] for i in range(n + 1) for j in range(n + 1)], dtype=np.float32)
    f = []
    for i in range(n):
        for j in range(n):
            a = i * (n + 1) + j
            f += [[a, a + n + 1, a + n + 2], [a, a + n + 2, a + 1]]
    return v, np.array(f, dtype=np.int32)


def doubled(v, f, seed=0):
    """The mesh concatenated with a copy of itself, the vertices and the faces shuffled."""
    rng = np.random.RandomState(seed)
    V = v.shape[0]
    vv, ff = np.concatenate([v, v]), np.concatenate([f, f + V])
    perm = rng.permutation(2 * V)
    out_v = np.empty_like(vv)
    out_v[perm] = vv
    return out_v, perm[ff][rng.permutation(ff.shape[0])].astype(np.int32)
