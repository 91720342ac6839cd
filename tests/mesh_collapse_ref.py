"""A numpy restatement of csrc/mesh_collapse.hip: mesh decimation by rounds of independent quadric edge collapses that keep a manifold a
manifold and land on the requested face count.  This file is the definition; the kernels equal it bit for bit.

    collapse(vertices, faces, nfaces, placement='optimal', max_rounds=None, hook=None) -> dict
        vertices, faces, vertex_map, rounds, stalled
    initial_quadrics(P, faces, c)     per vertex the 10 summed plane terms of its faces, about c (mesh_simplify_ref.fixed_sums)
    solve_rows(q, x0)                 mesh_simplify_ref.solve on rows: the same operations in the same order, elementwise
    energy_rows(q, x)                 x^T A x + 2 b.x + c0 on rows
    edge_hash(u, v, r)                the 20 hash bits of an edge's key in round r

One round, on the current face list (F faces over the original vertex indices), r = 1 + the rounds so far that collapsed something:
    1  tables      the undirected edges of the faces with three distinct corners: uses per direction, the lowest half-edge 3 f + k;
                   N(w) the neighbours of w; a vertex is pinned when it touches an edge not used exactly once in each direction
    2  candidates  {u, v}, u < v: neither end pinned; N(u) & N(v) is exactly {a, b}; not both {u,a,b} and {v,a,b} faces; the position
                   X = c + x and the cost E finite; no surviving face around u or v flips (n_new . n_old > 0; n_old = 0 does not vote)
    3  keys        (bits(float32(E)) >> 20) << 52 | h20 << 32 | lowest half-edge
    4  selection   m1[w] the smallest key of a candidate at w, m2[w] the smallest m1 over w and N(w); selected: key == m2[u] == m2[v]
    5  count       of the selected edges in ascending lowest half-edge only the first ceil((F - nfaces) / 2) are applied
    6  apply       P[u] = X, Q[u] = Q[u] + Q[v], v -> u in every face, the faces that had three distinct corners and lost that are
                   dropped, the rest keep their order
The loop ends at F <= nfaces, after max_rounds rounds, or in a round without a candidate (stalled).

Conventions: float64 on exactly widened inputs, one rounding per operation in the order written here, the lowest index among equals.
c is the centre of the referenced vertices' bounding box, 0.5 lo + 0.5 hi; quadrics and x are relative to it, P is absolute."""
import numpy as np

import mesh_simplify_ref as S

PLACEMENTS = ("optimal", "midpoint")
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
M32 = np.uint64(0xFFFFFFFF)


# ---- quadrics ------------------------------------------------------------------------------------------------------------------------
def face_normals_raw(p0, p1, p2):
    u, w = p1 - p0, p2 - p0
    return (u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0])


def initial_quadrics(P, faces, c):
    """Q [V,10]: per vertex the exact two-limb sum over its faces (once per corner) of the upper triangle of [n,d][n,d]^T in the order
    nx nx, nx ny, nx nz, nx d, ny ny, ny nz, ny d, nz nz, nz d, d d; n = (p1 - p0) x (p2 - p0) unnormalised, d = -n.(p0 - c)."""
    V = P.shape[0]
    f = faces
    nx, ny, nz = face_normals_raw(P[f[:, 0]], P[f[:, 1]], P[f[:, 2]])
    q = P[f[:, 0]] - c
    d = -((nx * q[:, 0] + ny * q[:, 1]) + nz * q[:, 2])
    t = np.stack([nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d], -1)
    owner = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    terms = np.concatenate([t, t, t])
    big = np.zeros(V)
    np.maximum.at(big, owner, np.abs(terms).max(1))
    e = S.exponent_of(big)
    return np.stack([S.fixed_sums(terms[:, k], owner, V, e) for k in range(10)], -1)


# ---- placement -----------------------------------------------------------------------------------------------------------------------
def solve_rows(q, x0):
    """mesh_simplify_ref.solve on every row of q [N,10], x0 [N,3]: the cyclic Jacobi with a rotation skipped where its pivot is 0."""
    n = q.shape[0]
    a = [[q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()], [q[:, 1].copy(), q[:, 4].copy(), q[:, 5].copy()],
         [q[:, 2].copy(), q[:, 5].copy(), q[:, 7].copy()]]
    b = [q[:, 3], q[:, 6], q[:, 8]]
    g = [(-b[i]) - ((a[i][0] * x0[:, 0] + a[i][1] * x0[:, 1]) + a[i][2] * x0[:, 2]) for i in range(3)]
    v = [[np.full(n, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(S.SWEEPS):
            for p, k, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                apq = a[p][k]
                skip = apq == 0.0
                theta = (a[k][k] - a[p][p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                keep = lambda old, new: np.where(skip, old, new)
                app, akk = keep(a[p][p], a[p][p] - t * apq), keep(a[k][k], a[k][k] + t * apq)
                arp, ark = a[r][p], a[r][k]
                nrp, nrk = keep(arp, c * arp - s * ark), keep(ark, s * arp + c * ark)
                a[p][p], a[k][k] = app, akk
                a[p][k] = a[k][p] = keep(apq, np.zeros(n))
                a[r][p] = a[p][r] = nrp
                a[r][k] = a[k][r] = nrk
                for i in range(3):
                    vp, vk = v[i][p], v[i][k]
                    v[i][p], v[i][k] = keep(vp, c * vp - s * vk), keep(vk, s * vp + c * vk)
        lam = [a[0][0], a[1][1], a[2][2]]
        bound = S.EIG_REL * np.fmax(np.fmax(lam[0], lam[1]), lam[2])
        coef = []
        for k in range(3):
            proj = (v[0][k] * g[0] + v[1][k] * g[1]) + v[2][k] * g[2]
            coef.append(np.where(lam[k] > bound, proj / lam[k], 0.0))
        return np.stack([x0[:, i] + ((v[i][0] * coef[0] + v[i][1] * coef[1]) + v[i][2] * coef[2]) for i in range(3)], -1)


def energy_rows(q, x):
    """((q0 x x + q4 y y + q7 z z) + 2 (q1 x y + q2 x z + q5 y z)) + 2 (q3 x + q6 y + q8 z) + q9, products and sums left to right."""
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(all="ignore"):
        s1 = (q[:, 0] * x0 * x0 + q[:, 4] * x1 * x1) + q[:, 7] * x2 * x2
        s2 = (q[:, 1] * x0 * x1 + q[:, 2] * x0 * x2) + q[:, 5] * x1 * x2
        s3 = (q[:, 3] * x0 + q[:, 6] * x1) + q[:, 8] * x2
        return ((s1 + 2.0 * s2) + 2.0 * s3) + q[:, 9]


def place_rows(q, pu, pv, placement):
    """(x [N,3], E [N]) of the merged quadric q for the ends at the centre-relative pu, pv; E before the clamp at 0."""
    with np.errstate(all="ignore"):
        x0 = (pu + pv) * 0.5
        e0 = energy_rows(q, x0)
        if placement == "midpoint":
            return x0, e0
        xs = solve_rows(q, x0)
        es = energy_rows(q, xs)
        back = ~np.isfinite(xs).all(1) | (es > e0)
        return np.where(back[:, None], x0, xs), np.where(back, e0, es)


# ---- keys ----------------------------------------------------------------------------------------------------------------------------
def edge_hash(u, v, r):
    """h20: uint32 arithmetic throughout."""
    u, v = np.asarray(u).astype(np.uint64), np.asarray(v).astype(np.uint64)
    h = ((u * np.uint64(0x9E3779B1)) & M32) ^ ((v * np.uint64(0x85EBCA77)) & M32) ^ ((np.uint64(r) * np.uint64(0xC2B2AE3D)) & M32)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & M32
    h ^= h >> np.uint64(12)
    return h >> np.uint64(12)


def edge_keys(E, u, v, r, low):
    with np.errstate(all="ignore"):
        bits = np.where(E > 0.0, E, 0.0).astype(np.float32).view(np.uint32).astype(np.uint64) >> np.uint64(20)
    return (bits << np.uint64(52)) | (edge_hash(u, v, r) << np.uint64(32)) | low.astype(np.uint64)


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def proper_faces(f):
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def edge_tables(f, V):
    """The undirected edges of the proper faces, ascending by (lo, hi): eu, ev, fwd, bwd, low (the lowest half-edge), and the
    codes lo V + hi for look-ups."""
    fid = np.nonzero(proper_faces(f))[0]
    a = np.concatenate([f[fid, k] for k in range(3)])
    b = np.concatenate([f[fid, (k + 1) % 3] for k in range(3)])
    h = np.concatenate([3 * fid + k for k in range(3)])
    code = np.minimum(a, b) * V + np.maximum(a, b)
    codes, inv = np.unique(code, return_inverse=True)
    inv = inv.reshape(-1)
    E = codes.shape[0]
    fwd = np.bincount(inv[a < b], minlength=E)
    bwd = np.bincount(inv[a > b], minlength=E)
    low = np.full(E, np.iinfo(np.int64).max)
    np.minimum.at(low, inv, h)
    return codes // V, codes % V, fwd, bwd, low, codes


def rows_of(src, dst, V):
    """CSR rows: dst sorted by (src, dst), and the offsets [V+1]."""
    order = np.lexsort((dst, src))
    return np.searchsorted(src[order], np.arange(V + 1)), dst[order]


def expand(off, rows):
    """For the row ids `rows`: (which, entry) -- entry runs over every element of each row, which is the position in `rows`."""
    n = off[rows + 1] - off[rows]
    which = np.repeat(np.arange(rows.shape[0]), n)
    start = np.repeat(off[rows], n)
    within = np.arange(which.shape[0]) - np.repeat(np.cumsum(n) - n, n)
    return which, start + within


def member(table, want):
    """Whether each of ``want`` is in the ascending ``table``."""
    if table.shape[0] == 0:
        return np.zeros(want.shape[0], dtype=bool)
    return table[np.minimum(np.searchsorted(table, want), table.shape[0] - 1)] == want


def is_face(fcodes, codes, V, a, b, c):
    """Whether the unordered triples {a, b, c} are proper faces of the list fcodes was made of."""
    s = np.sort(np.stack([a, b, c], -1), axis=1)
    pair = s[:, 0] * V + s[:, 1]
    eid = np.minimum(np.searchsorted(codes, pair), codes.shape[0] - 1)
    return (codes[eid] == pair) & member(fcodes, eid * V + s[:, 2])


# ---- one round -----------------------------------------------------------------------------------------------------------------------
def select(P, Q, c, f, r, placement):
    """The selected edges of round r on the faces f in ascending lowest half-edge: dict(u, v, X, n_candidates, candidates [n,2])."""
    V = P.shape[0]
    eu, ev, fwd, bwd, low, codes = edge_tables(f, V)
    manifold = (fwd == 1) & (bwd == 1)
    pinned = np.zeros(V, dtype=bool)
    pinned[eu[~manifold]] = True
    pinned[ev[~manifold]] = True
    noff, nbr = rows_of(np.concatenate([eu, ev]), np.concatenate([ev, eu]), V)
    dcodes = np.sort(np.concatenate([eu * V + ev, ev * V + eu]))
    pid = np.nonzero(proper_faces(f))[0]
    foff, vface = rows_of(np.concatenate([f[pid, k] for k in range(3)]), np.concatenate([pid, pid, pid]), V)
    ps = np.sort(f[pid], axis=1)
    fcodes = np.sort(np.searchsorted(codes, ps[:, 0] * V + ps[:, 1]) * V + ps[:, 2])

    e = np.nonzero(~pinned[eu] & ~pinned[ev])[0]
    # N(u) & N(v): the neighbours x of u with (v, x) an edge, ascending
    which, at = expand(noff, eu[e])
    x = nbr[at]
    want = ev[e][which] * V + x
    hit = member(dcodes, want)
    common = np.bincount(which[hit], minlength=e.shape[0])
    two = common == 2
    first = np.full(e.shape[0], np.iinfo(np.int64).max)
    last = np.full(e.shape[0], -1, dtype=np.int64)
    np.minimum.at(first, which[hit], x[hit])
    np.maximum.at(last, which[hit], x[hit])
    e, a, b = e[two], first[two], last[two]
    if e.shape[0]:
        tetra = is_face(fcodes, codes, V, eu[e], a, b) & is_face(fcodes, codes, V, ev[e], a, b)
        e = e[~tetra]
    u, v = eu[e], ev[e]
    q = Q[u] + Q[v]
    x, E = place_rows(q, P[u] - c, P[v] - c, placement)
    with np.errstate(all="ignore"):
        X = c + x
    ok = np.isfinite(X).all(1) & np.isfinite(E)
    # flips: every proper face around u or v that does not hold both
    flips = np.zeros(e.shape[0], dtype=bool)
    for w in (u, v):
        which, at = expand(foff, w)
        g = f[vface[at]]
        dies = ((g == u[which][:, None]).any(1)) & ((g == v[which][:, None]).any(1))
        which, g = which[~dies], g[~dies]
        old = [P[g[:, k]] for k in range(3)]
        new = [np.where((g[:, k] == w[which])[:, None], X[which], old[k]) for k in range(3)]
        with np.errstate(all="ignore"):
            ox, oy, oz = face_normals_raw(*old)
            nx, ny, nz = face_normals_raw(*new)
            dot = (nx * ox + ny * oy) + nz * oz
        votes = (ox != 0.0) | (oy != 0.0) | (oz != 0.0)
        np.logical_or.at(flips, which, votes & ~(dot > 0.0))
    cand = ok & ~flips
    e, u, v, X, E = e[cand], u[cand], v[cand], X[cand], E[cand]
    key = edge_keys(E, u, v, r, low[e])
    m1 = np.full(V, NO_KEY, dtype=np.uint64)
    np.minimum.at(m1, u, key)
    np.minimum.at(m1, v, key)
    m2 = m1.copy()
    np.minimum.at(m2, eu, m1[ev])
    np.minimum.at(m2, ev, m1[eu])
    sel = (key == m2[u]) & (key == m2[v])
    order = np.argsort(low[e][sel], kind="stable")
    return dict(u=u[sel][order], v=v[sel][order], X=X[sel][order], n_candidates=int(e.shape[0]), candidates=np.stack([u, v], -1))


def collapse(vertices, faces, nfaces, placement="optimal", max_rounds=None, hook=None):
    """dict(vertices, faces, vertex_map, rounds, stalled).  ``hook(faces, u, v)`` is called every round with the current faces and all
    the selected edges, before the count cuts them."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement must be one of {PLACEMENTS}")
    if int(nfaces) != nfaces or nfaces < 1:
        raise ValueError("nfaces must be a positive integer")
    if max_rounds is not None and (int(max_rounds) != max_rounds or max_rounds < 1):
        raise ValueError("max_rounds must be None or a positive integer")
    vertices = np.asarray(vertices)
    V = vertices.shape[0]
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    if not S.valid_faces(f, V).all():
        raise ValueError("a face index lies outside [0, V)")
    P = vertices.astype(np.float64).copy()
    ref0 = S.referenced(f, V)
    if not np.isfinite(P[ref0]).all():
        raise ValueError("a referenced vertex has a non-finite coordinate")
    lo, hi = P[ref0].min(0), P[ref0].max(0)
    c = 0.5 * lo + 0.5 * hi
    Q = initial_quadrics(P, f, c)
    moved = np.arange(V)
    rounds, stalled = 0, False
    while f.shape[0] > nfaces and (max_rounds is None or rounds < max_rounds):
        s = select(P, Q, c, f, rounds + 1, placement)
        if s["n_candidates"] == 0:
            stalled = True
            break
        if hook is not None:
            hook(f, s["u"], s["v"])
        quota = (f.shape[0] - int(nfaces) + 1) // 2
        u, v, X = s["u"][:quota], s["v"][:quota], s["X"][:quota]
        P[u] = X
        Q[u] = Q[u] + Q[v]
        moved[v] = u
        proper = proper_faces(f)
        f = moved[f]
        f = f[~(proper & ~proper_faces(f))]
        rounds += 1
    ref = S.referenced(f, V)
    rank = np.where(ref, np.cumsum(ref) - 1, -1)
    root = np.arange(V)
    while (moved[root] != root).any():
        root = moved[root]
    vmap = np.where(ref0, rank[root], -1).astype(np.int32)
    return dict(vertices=P[ref].astype(vertices.dtype), faces=rank[f].astype(np.int32).reshape(-1, 3), vertex_map=vmap, rounds=rounds,
                stalled=stalled)


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)     # outward
    return v, f


def quad_patch(n=12, dtype=np.float32):
    """An open n x n patch of quads over [0, 1]^2 with a bump: the boundary vertices come first in index order only by row."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = i / n, j / n
    v = np.stack([x, y, 0.2 * np.sin(3.0 * x) * np.cos(2.0 * y)], -1).reshape(-1, 3).astype(dtype)
    f = []
    for a in range(n):
        for b in range(n):
            k = a * (n + 1) + b
            f += [[k, k + n + 1, k + n + 2], [k, k + n + 2, k + 1]]
    return v, np.array(f, dtype=np.int32)


def together(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def sliver_torus():
    """The 8 x 16 torus with the third corner of its first face moved exactly onto the middle of the other two (their coordinates
    cut to multiples of 2^-10 first, so that the midpoint and both cross products are exact): a closed manifold with one face of
    three distinct corners and n = (0, 0, 0).  Returns (v, f, the face's corners)."""
    import mesh_topo_ref as T
    v, f = T.torus(8, 16)
    v = v.copy()
    a, b, c = (int(x) for x in f[0])
    v[[a, b]] = np.rint(v[[a, b]] * 1024.0) / 1024.0
    v[c] = (v[a] + v[b]) * np.float32(0.5)
    return v, f, (a, b, c)


def fin_mesh():
    """A 6 x 6 patch with a third face standing on one of its interior edges."""
    v, f = quad_patch(6)
    k = 3 * 7 + 3
    tip = (0.5 * (v[k] + v[k + 8]) + np.array([0, 0, 0.3], dtype=np.float32)).astype(np.float32)
    return np.concatenate([v, tip[None]]), np.concatenate([f, [[k, k + 8, v.shape[0]]]]).astype(np.int32), (k, k + 8)
