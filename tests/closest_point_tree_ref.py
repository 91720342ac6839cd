"""vt_closest_tree_build / vt_closest_tree_query restated in float64 numpy ("closest_point_tree.hip"): csrc/closest_point_tree.hip's
operations in that file's order, on the tree of tests/winding_fast_ref.py and the face arithmetic of tests/closest_point_ref.py.

  boxes     per occupied cell lo[3], hi[3]: a leaf's is the min / max over the exactly converted corners of the faces in its list, an inner
            cell's the min / max over its occupied children; a face with an index outside [0, V) is in no box and is never evaluated
  slack     delta = (S S) 2^-40, S = ((m_x + m_y) + m_z) + 4 side, m_a = max(|p_a - lo_a|, |p_a - (lo_a + side)|) over the tree's frame
  bound     e_a = max(lo_a - p_a, 0, p_a - hi_a), lb = (e_x^2 + e_y^2) + e_z^2; a cell and everything under it is skipped when
            lb - delta > best (false for a NaN: such a query skips nothing)
  leaf      cp_face (closest_point_ref.pairs_by_regions) over the list in list order; a face is taken on
            d2 < best or (d2 == best and face < best_face)
  seed      the leaf reached by descending towards the query's own cell (the build's binning, clamped into the frame; where the wanted
            child is empty the occupied child whose number is nearest, the lower of two) is evaluated first; the walk passes over it
  order     the children of a cell are visited as k ^ o, o the octant of the query about the cell's centre lo_a + (i_a + 0.5) (side / 2^level)
  walk      winding_fast_ref.query's: the state is (level, k-cell), "next" is cell + 1 climbing while cell % 8 == 0, "descend" (level + 1, 8 cell)

``query`` returns (d2 [N] f64, face [N] int32, closest [N,3] f64, stats [N,2] int32: boxes tested, faces tested).  The defaults of ``seed``
and ``order`` are the kernel's default walk.
"""
import numpy as np

import closest_point_ref as R
import winding_fast_ref as W

SLACK = 2.0 ** -40


def valid_faces(verts, faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < len(verts))).all(axis=1)


def build(verts, faces, depth=None):
    """winding_fast_ref's tree with ``boxes`` (per level float64 [count, 6]) and ``valid`` (bool [F]) added."""
    t = W.build(verts, faces, depth)
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    L = t.depth
    t.valid = valid_faces(v, f)
    t.boxes = [np.concatenate([np.full((int((t.pyramid[l] >= 0).sum()), 3), np.inf), np.full((int((t.pyramid[l] >= 0).sum()), 3), -np.inf)], axis=1)
               for l in range(L + 1)]
    ok = np.nonzero(t.valid)[0]
    tri = v[f[ok]]                                                     # [n, 3, 3]: the corners of the faces that are read
    rk = t.pyramid[L][t.codes[ok]]
    for a in range(3):
        np.minimum.at(t.boxes[L][:, a], rk, tri[:, :, a].min(axis=1))
        np.maximum.at(t.boxes[L][:, 3 + a], rk, tri[:, :, a].max(axis=1))
    for l in range(L - 1, -1, -1):
        cells = np.nonzero(t.pyramid[l + 1] >= 0)[0]
        parent = t.pyramid[l][cells >> 3]
        child = t.boxes[l + 1][t.pyramid[l + 1][cells]]
        for a in range(3):
            np.minimum.at(t.boxes[l][:, a], parent, child[:, a])
            np.maximum.at(t.boxes[l][:, 3 + a], parent, child[:, 3 + a])
    return t


def slack(t, q):
    u, v = np.abs(q - t.lo), np.abs(q - (t.lo + t.side))
    m = np.where(u > v, u, v)
    S = ((m[:, 0] + m[:, 1]) + m[:, 2]) + 4.0 * t.side
    return (S * S) * SLACK


def lower_bound(box, q):
    x = box[:, 0:3] - q
    x = np.where(x > 0.0, x, 0.0)
    y = q - box[:, 3:6]
    e = np.where(y > x, y, x)
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def _gather(m):
    r = np.zeros_like(m)
    for k in range(W.MAX_DEPTH):
        r |= ((m >> (3 * k)) & 1) << k
    return r


def pairs(verts, faces, pts, valid):
    """(d2 [N,F], q [N,F,3]) of every pair by cp_face; the columns of faces that are not read stay NaN."""
    N, F = len(pts), len(valid)
    D, Q = np.full((N, F), np.nan), np.full((N, F, 3), np.nan)
    ok = np.nonzero(valid)[0]
    with np.errstate(all="ignore"):
        for f0 in range(0, len(ok), 512):
            sel = ok[f0:f0 + 512]
            D[:, sel], Q[:, sel] = R.pairs_by_regions(verts, np.asarray(faces)[sel], pts)
    return D, Q


def query(t, verts, faces, pts, seed=True, order=True):
    q = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    N, L = len(q), t.depth
    best, bface = np.full(N, np.inf), np.full(N, -1, dtype=np.int32)
    stats = np.zeros((N, 2), dtype=np.int32)
    D, Q = pairs(verts, faces, np.asarray(pts, dtype=np.float32).reshape(-1, 3), t.valid)
    with np.errstate(invalid="ignore"):
        delta = slack(t, q)

    def leaf(at, rk):
        nonlocal best, bface
        o, e = t.list_offsets[rk], t.list_offsets[rk + 1]
        stats[at, 1] += (e - o)
        j = 0
        while len(at):
            keep = o + j < e
            at, o, e = at[keep], o[keep], e[keep]
            if len(at) == 0:
                break
            f = t.lists[o + j]
            d = D[at, f]
            with np.errstate(invalid="ignore"):
                take = t.valid[f] & ((d < best[at]) | ((d == best[at]) & (f < bface[at])))
            best[at[take]], bface[at[take]] = d[take], f[take]
            j += 1

    seed_rk = np.full(N, -1, dtype=np.int64)
    if seed and N:
        n = 2 ** L
        with np.errstate(invalid="ignore"):
            g = np.floor((q - t.lo) / t.side * n)
            g = np.where(g > 0.0, g, 0.0)
            g = np.where(g < n - 1, g, float(n - 1)).astype(np.int64)
        code = W.morton(g[:, 0], g[:, 1], g[:, 2], L)
        c = np.zeros(N, dtype=np.int64)
        for l in range(L):
            want = (code >> (3 * (L - 1 - l))) & 7
            ch = t.pyramid[l + 1][(8 * c)[:, None] + np.arange(8)[None]]
            gap = np.where(ch >= 0, np.abs(np.arange(8)[None] - want[:, None]), 16)
            c = 8 * c + np.argmin(gap, axis=1)                         # the first among equals: the lower number
        seed_rk = t.pyramid[L][c].astype(np.int64)
        leaf(np.arange(N), seed_rk)

    level, cell, flip = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    live = np.ones(N, dtype=bool)
    while live.any():
        descend = np.zeros(N, dtype=bool)
        actual = cell ^ flip
        for l in np.unique(level[live]):
            at = np.nonzero(live & (level == l))[0]
            rk = t.pyramid[l][actual[at]]
            at, rk = at[rk >= 0], rk[rk >= 0]
            if len(at) == 0:
                continue
            stats[at, 0] += 1
            with np.errstate(invalid="ignore"):
                skip = lower_bound(t.boxes[l][rk], q[at]) - delta[at] > best[at]
            at, rk = at[~skip], rk[~skip]
            if l < L:
                descend[at] = True
            else:
                mine = rk == seed_rk[at]
                leaf(at[~mine], rk[~mine])
        o = np.zeros(N, dtype=np.int64)
        if order:
            h = t.side * (1.0 / 2.0 ** level)
            for a in range(3):
                centre = t.lo[a] + (_gather(actual >> a).astype(np.float64) + 0.5) * h
                with np.errstate(invalid="ignore"):
                    o |= np.where(q[:, a] >= centre, 1 << a, 0)
        level = np.where(descend, level + 1, level)
        flip = np.where(descend, flip * 8 + o, flip)
        cell = np.where(descend, cell * 8, cell + np.where(live, 1, 0))
        while True:
            up = live & ~descend & (level > 0) & (cell % 8 == 0)
            if not up.any():
                break
            cell = np.where(up, cell // 8, cell)
            flip = np.where(up, flip // 8, flip)
            level = np.where(up, level - 1, level)
        live = live & (descend | (level > 0))
    closest = np.full((N, 3), np.nan)
    hit = bface >= 0
    closest[hit] = Q[np.nonzero(hit)[0], bface[hit]]
    return best, bface, closest, stats


def tree(verts, faces, pts, depth=None, seed=True, order=True):
    """``query(build(verts, faces, depth), ...)``."""
    return query(build(verts, faces, depth), verts, faces, pts, seed, order)


def brute(verts, faces, pts):
    """closest_point_ref.by_regions over the faces that are read, numbered as in the full mesh: what vt_closest_point_mesh computes when it
    skips a face with an index outside [0, V)."""
    valid = valid_faces(verts, faces)
    if valid.all():
        return R.by_regions(verts, faces, pts)
    ok = np.nonzero(valid)[0]
    d2, face, closest = R.by_regions(verts, np.asarray(faces)[ok], pts)
    return d2, np.where(face >= 0, ok[np.maximum(face, 0)], -1).astype(np.int32), closest


# ---- the inputs the CPU and the GPU tests share ------------------------------------------------------------------------------------------
GRID_F = (1, 8, 9, 65, 1000)
GRID_N = (1, 63, 65, 778)
GRID_DEPTH = (1, 2, 3, None)


def grid_mesh(F):
    """The soup of ``F`` faces, or the torus for ``F == 'torus'``."""
    return R.torus(24, 12) if F == "torus" else R.soup(F, 100 + F)


def grid_queries(F, N, verts, faces):
    return R.queries(N, 1000 * (576 if F == "torus" else F) + N, verts, faces)


def mirrored_pair(swap):
    """Two triangles that mirror each other in the plane x = 0 (equal d2, bit for bit, for a query on that plane), far enough apart to
    land in different leaves, among the faces of a soup; one triangle of the soup is repeated at two indices.  ``swap`` exchanges the
    two mirrored faces' indices.  Returns (verts, faces, pts, (i, j)): the mirrored faces' indices, i < j."""
    sv, sf = R.soup(40, 11)
    sv = (sv * np.float32(0.25) + np.array([0.0, 0.0, 2.0], dtype=np.float32)).astype(np.float32)   # the soup sits away from the pair
    tri = np.array([[0.5, -0.25, 0.0], [0.75, 0.25, 0.0], [0.5, 0.0, 0.25]], dtype=np.float32)
    mir = tri * np.array([-1.0, 1.0, 1.0], dtype=np.float32)
    verts = np.concatenate([sv, tri, mir]).astype(np.float32)
    V0 = len(sv)
    left, right = np.array([V0, V0 + 1, V0 + 2], dtype=np.int32), np.array([V0 + 3, V0 + 4, V0 + 5], dtype=np.int32)
    if swap:
        left, right = right, left
    faces = np.concatenate([sf[:7], left[None], sf[7:30], sf[3:4], right[None], sf[30:]]).astype(np.int32)   # soup face 3 again at index 31
    pts = np.array([[0.0, 0.0, 0.0], [0.0, 0.125, 0.5], [0.0, -1.0, 0.25], [0.0, 0.0, -3.0]], dtype=np.float32)
    return verts, faces, pts, (7, 32)


def one_leaf():
    """30 faces whose centroids are all exactly the origin: one leaf holds every face at any depth."""
    base = np.array([[1.0, 0.0, 0.0], [-0.5, 0.75, 0.0], [-0.5, -0.75, 0.0]], dtype=np.float32)
    spin = np.array([[0.0, 0.0, 1.0], [0.0, 0.75, -0.5], [0.0, -0.75, -0.5]], dtype=np.float32)
    verts = np.concatenate([base, base * np.float32(0.5), base * np.float32(-0.25), spin, spin * np.float32(-0.5)]).astype(np.float32)
    faces = np.tile(np.arange(15, dtype=np.int32).reshape(5, 3), (6, 1))
    return verts, faces


def degenerate(kind, mixed):
    """tests/test_closest_point_gpu.py's degenerate faces: repeated indices or collinear corners, alone or among 300 soup faces."""
    if kind == "repeated":
        verts = np.array([[0, 0, 0], [0.25, 0.5, 0], [0.75, 0, 0.5]], dtype=np.float32)
        bad = [[0, 0, 1], [1, 2, 2], [2, 2, 2]]
    else:
        verts = np.array([[0, 0, 0], [0.25, 0, 0], [0.75, 0, 0]], dtype=np.float32)
        bad = [[0, 1, 2], [2, 0, 1]]
    faces = np.array(bad, dtype=np.int32)
    if mixed:
        sv, sf = R.soup(300, 4)
        faces = np.concatenate([sf[:150] + 3, faces, sf[150:] + 3]).astype(np.int32)
        verts = np.concatenate([verts, sv + np.float32(0.25)])
    pts = np.concatenate([R.queries(61, 8), verts[:3], np.array([[0.5, 0, 0], [-1, 0, 0], [0.1, 0.5, 0]], dtype=np.float32)])
    return verts, faces, pts


def far_queries():
    """Queries 1e3 and 1e6 away from the frame, along an axis and along the diagonal, and two inside it."""
    return np.array([[1e3, 0, 0], [0, -1e3, 0], [1e3, 1e3, -1e3], [1e6, 0, 0], [0, 0, -1e6], [-1e6, 1e6, 1e6], [0.1, 0.2, -0.1], [0, 0, 0]],
                    dtype=np.float32)


def nan_queries(verts, faces):
    pts = R.queries(9, 77, verts, faces)
    pts[1, 0], pts[4, 1], pts[6, 2], pts[7] = np.nan, np.nan, np.nan, np.nan
    return pts


def bad_index_mesh():
    """A 65-face soup with two faces whose indices lie outside [0, V) (one below, one beyond), and the mesh without them."""
    verts, faces = R.soup(65, 165)
    faces = faces.copy()
    faces[9, 1], faces[40, 2] = -1, len(verts)
    return verts, faces
