"""vt_ray_mesh / vt_ray_tree_query / vt_camera_rays / vt_depth_from_hits restated in float64 numpy ("ray_mesh.hip"):
csrc/ray_face.h's and csrc/ray_mesh.hip's operations in those files' order, on the tree of tests/winding_fast_ref.py with the boxes of
tests/closest_point_tree_ref.py.

  ray       o + s d, float64, d not normalised.  kz = the axis of the largest |d_a| (the lowest among equals), kx, ky the next two
            cyclically, swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Invalid (it misses everything): a
            direction that is all zero, a direction or an origin that is not finite
  face      A = a - o, Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz] (B, C alike); U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;
            a miss when one is < 0 and another > 0; det = (U + V) + W, a miss when 0; s = ((U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz])) / det;
            a hit when t_min <= s <= t_max
  brute     the smallest s over the faces that are read, the lowest face among equals; weights U / det, V / det, W / det
  walk      closest_point_tree_ref.query's: (level, k-cell), children visited as k ^ o, o_a = (d_a < 0), for the whole ray
  skip      E = S 2^-40, S = (m_x + m_y) + m_z, m_a = max(|o_a - lo_a|, |o_a - (lo_a + side)|) over the tree's frame;
            x0_a = (lo_a - o_a) - E, x1_a = (hi_a - o_a) + E; d_a == 0: skipped when x0_a > 0 or x1_a < 0; otherwise (near_a, far_a) =
            (x0_a, x1_a) (1 / d_a), exchanged when d_a < 0; enter = t_min, exit = min(t_max, best), enter = near_a where near_a > enter,
            exit = far_a where far_a < exit; skipped when enter > exit (every comparison false for a NaN)
  leaf      the rule over the list in list order; a face is taken on s < best or (s == best and face < best_face)

``tree_query`` returns (s [N] f64, face [N] int32, bary [N,3] f64, stats [N,2] int32: boxes tested, faces tested).
"""
import math

import numpy as np

import closest_point_ref as R
import closest_point_tree_ref as C

SLACK = 2.0 ** -40


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
class Rays:
    pass


def setup(origins, dirs):
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    if len(o) == 1 and len(d) != 1:
        o = np.repeat(o, len(d), axis=0)
    r = Rays()
    r.o, r.d = o, d
    ad = np.abs(d)
    with np.errstate(invalid="ignore"):
        r.ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (ad > 0.0).any(axis=1)
        kz = np.zeros(len(d), dtype=np.int64)
        m = ad[:, 0].copy()
        for a in (1, 2):
            up = ad[:, a] > m
            kz, m = np.where(up, a, kz), np.where(up, ad[:, a], m)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    n = np.arange(len(d))
    dz = d[n, kz]
    with np.errstate(invalid="ignore"):
        swap = dz < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    r.kx, r.ky, r.kz = kx, ky, kz
    with np.errstate(all="ignore"):
        r.Sx, r.Sy, r.Sz = d[n, kx] / dz, d[n, ky] / dz, 1.0 / dz
    r.ox, r.oy, r.oz = o[n, kx], o[n, ky], o[n, kz]
    return r


def corners(verts, faces):
    """(a, b, c) float64 [F,3] and valid bool [F]; the corners of a face that is not read are zero."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    valid = C.valid_faces(v, f)
    g = np.where(valid[:, None], f, 0)
    tri = v[g] * valid[:, None, None]
    return tri[:, 0], tri[:, 1], tri[:, 2], valid


def _rule(r, sel, pa, pb, pc, t_min, t_max):
    """rf_face for the rays ``sel`` against corners picked per ray: pa = (a[kx], a[ky], a[kz]) and so on, arrays [len(sel), ...]."""
    ex = (slice(None),) + (None,) * (pa[0].ndim - 1)
    ox, oy, oz, Sx, Sy, Sz = (q[sel][ex] for q in (r.ox, r.oy, r.oz, r.Sx, r.Sy, r.Sz))

    def shear(p):
        z = p[2] - oz
        return (p[0] - ox) - Sx * z, (p[1] - oy) - Sy * z, z
    with np.errstate(all="ignore"):
        Ax, Ay, Az = shear(pa)
        Bx, By, Bz = shear(pb)
        Cx, Cy, Cz = shear(pc)
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        mixed = ((U < 0.0) | (V < 0.0) | (W < 0.0)) & ((U > 0.0) | (V > 0.0) | (W > 0.0))
        det = (U + V) + W
        s = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det
        hit = ~mixed & ~(det == 0.0) & (s >= t_min) & (s <= t_max) & r.ok[sel][ex]
    return np.where(hit, s, np.inf), U, V, W, det


def pairs(r, a, b, c, valid, t_min=0.0, t_max=np.inf, chunk=1024):
    """s [N,F] of every (ray, face) pair by rf_face, +inf for a miss and for a face that is not read."""
    N = len(r.d)
    S = np.full((N, len(a)), np.inf)
    for n0 in range(0, N, chunk):
        sel = np.arange(n0, min(N, n0 + chunk))
        pick = lambda p: (p.T[r.kx[sel]], p.T[r.ky[sel]], p.T[r.kz[sel]])
        S[sel] = np.where(valid[None, :], _rule(r, sel, pick(a), pick(b), pick(c), t_min, t_max)[0], np.inf)
    return S


def _weights(r, face, a, b, c, t_min, t_max):
    """The weights of the winning faces: the rule once more on (ray, face[ray])."""
    bary = np.full((len(face), 3), np.nan)
    sel = np.nonzero(face >= 0)[0]
    if len(sel):
        f = face[sel]
        pick = lambda p: (p[f, r.kx[sel]], p[f, r.ky[sel]], p[f, r.kz[sel]])
        _, U, V, W, det = _rule(r, sel, pick(a), pick(b), pick(c), t_min, t_max)
        with np.errstate(all="ignore"):
            bary[sel] = np.stack([U / det, V / det, W / det], axis=1)
    return bary


def brute(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf):
    """(s [N] f64, face [N] int32, bary [N,3] f64): vt_ray_mesh."""
    r = setup(origins, dirs)
    a, b, c, valid = corners(verts, faces)
    S = pairs(r, a, b, c, valid, t_min, t_max)
    face = np.argmin(S, axis=1).astype(np.int32)                         # the first among equals: the lowest face
    s = S[np.arange(len(S)), face]
    face = np.where(np.isinf(s), -1, face).astype(np.int32)
    return s, face, _weights(r, face, a, b, c, t_min, t_max)


def slack(t, o):
    u, v = np.abs(o - t.lo), np.abs(o - (t.lo + t.side))
    m = np.where(u > v, u, v)
    return ((m[:, 0] + m[:, 1]) + m[:, 2]) * SLACK


def tree_query(t, verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, order=True):
    """vt_ray_tree_query over ``t`` = closest_point_tree_ref.build(verts, faces, depth)."""
    r = setup(origins, dirs)
    o, d = r.o, r.d
    N, L = len(d), t.depth
    a, b, c, valid = corners(verts, faces)
    S = pairs(r, a, b, c, valid, t_min, t_max)
    best, bface = np.full(N, np.inf), np.full(N, -1, dtype=np.int32)
    stats = np.zeros((N, 2), dtype=np.int32)
    with np.errstate(all="ignore"):
        E = slack(t, o)
        inv = 1.0 / d
        neg = d < 0.0
    oct_ = np.zeros(N, dtype=np.int64)
    if order:
        for ax in range(3):
            oct_ |= np.where(neg[:, ax], 1 << ax, 0)

    def leaf(at, rk):
        lo_, hi_ = t.list_offsets[rk], t.list_offsets[rk + 1]
        stats[at, 1] += (hi_ - lo_)
        j = 0
        while len(at):
            keep = lo_ + j < hi_
            at, lo_, hi_ = at[keep], lo_[keep], hi_[keep]
            if len(at) == 0:
                break
            f = t.lists[lo_ + j]
            s = S[at, f]
            take = (s < best[at]) | ((s == best[at]) & (f < bface[at]))
            best[at[take]], bface[at[take]] = s[take], f[take]
            j += 1

    def skipped(box, at):
        enter = np.full(len(at), float(t_min))
        exit_ = np.where(best[at] < t_max, best[at], float(t_max))
        skip = np.zeros(len(at), dtype=bool)
        with np.errstate(all="ignore"):
            for ax in range(3):
                x0, x1 = (box[:, ax] - o[at, ax]) - E[at], (box[:, 3 + ax] - o[at, ax]) + E[at]
                zero = d[at, ax] == 0.0
                skip |= zero & ((x0 > 0.0) | (x1 < 0.0))
                u, v = x0 * inv[at, ax], x1 * inv[at, ax]
                near, far = np.where(neg[at, ax], v, u), np.where(neg[at, ax], u, v)
                enter = np.where(~zero & (near > enter), near, enter)
                exit_ = np.where(~zero & (far < exit_), far, exit_)
            skip |= enter > exit_
        return skip

    level, cell, flip = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    live = r.ok.copy()
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
            skip = skipped(t.boxes[l][rk], at)
            at, rk = at[~skip], rk[~skip]
            if l < L:
                descend[at] = True
            else:
                leaf(at, rk)
        level = np.where(descend, level + 1, level)
        flip = np.where(descend, flip * 8 + oct_, flip)
        cell = np.where(descend, cell * 8, cell + np.where(live, 1, 0))
        while True:
            up = live & ~descend & (level > 0) & (cell % 8 == 0)
            if not up.any():
                break
            cell = np.where(up, cell // 8, cell)
            flip = np.where(up, flip // 8, flip)
            level = np.where(up, level - 1, level)
        live = live & (descend | (level > 0))
    return best, bface, _weights(r, bface, a, b, c, t_min, t_max), stats


def tree(verts, faces, origins, dirs, depth=None, **kw):
    return tree_query(C.build(verts, faces, depth), verts, faces, origins, dirs, **kw)


def moller_trumbore(verts, faces, origins, dirs):
    """The independent check: float64 Moller-Trumbore, two-sided, s >= 0 -> (s [N], face [N], smallest weight of the hit [N])."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64)
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    a, e1, e2 = v[f[:, 0]][None], (v[f[:, 1]] - v[f[:, 0]])[None], (v[f[:, 2]] - v[f[:, 0]])[None]
    with np.errstate(all="ignore"):
        pv = np.cross(d[:, None, :], e2)
        det = (e1 * pv).sum(-1)
        tv = o[:, None, :] - a
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        w = (d[:, None, :] * qv).sum(-1) / det
        s = (e2 * qv).sum(-1) / det
        hit = (det != 0.0) & (u >= 0.0) & (w >= 0.0) & (u + w <= 1.0) & (s >= 0.0)
    s = np.where(hit, s, np.inf)
    face = np.argmin(s, axis=1)
    n = np.arange(len(s))
    smin = np.minimum(np.minimum(u[n, face], w[n, face]), 1.0 - u[n, face] - w[n, face])
    return s[n, face], np.where(np.isinf(s[n, face]), -1, face).astype(np.int32), smin


# ---- the camera -----------------------------------------------------------------------------------------------------------------------------
def camera_rays(pose, width, height, fov=60.0):
    """(origins [n,3], dirs [n, H*W, 3]): vt_camera_rays from the records [n,16] {M 3x3, t, centroid, scale}."""
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 16)
    f = height / (2.0 * math.tan(fov * 3.14159265358979323846 / 180.0 / 2.0))
    pix = np.arange(width * height)
    u, v = (pix % width).astype(np.float64), (pix // width).astype(np.float64)
    c1, c2 = (-(u - width / 2.0)) / f, (-(v - height / 2.0)) / f
    origins = (pose[:, 9:12] - pose[:, 12:15]) / pose[:, 15:16]
    m = pose[:, :9].reshape(-1, 3, 3)
    dirs = ((m[:, None, :, 0] + m[:, None, :, 1] * c1[None, :, None]) + m[:, None, :, 2] * c2[None, :, None]) / pose[:, None, 15:16]
    return origins, dirs


def depth_from_hits(s, origin=None, near=0.0):
    z = np.asarray(s, dtype=np.float64)
    if origin is not None:
        g = np.broadcast_to(np.asarray(origin, dtype=np.float64).reshape(-1), z.shape)
        z = np.where(z < g, z, g)
    z = np.where(z < near, near, z)
    with np.errstate(over="ignore"):
        return z.astype(np.float32)


def render(verts, faces, pose, width, height, fov=60.0):
    """(s [n, H*W], face [n, H*W], origins, dirs) by the brute-force restatement."""
    origins, dirs = camera_rays(pose, width, height, fov)
    n = len(origins)
    s, face = np.zeros((n, width * height)), np.zeros((n, width * height), dtype=np.int32)
    for i in range(n):
        s[i], face[i], _ = brute(verts, faces, origins[i:i + 1], dirs[i])
    return s, face, origins, dirs


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
GRID_F = C.GRID_F
GRID_DEPTH = C.GRID_DEPTH
N_RAYS = 300                                                            # crosses a 256-lane block
grid_mesh = C.grid_mesh


def grid_rays(F, verts, faces, n=N_RAYS):
    """n rays in float64: a quarter aimed at points of the mesh from inside the frame, a quarter aimed at them from far outside, a quarter
    random (mostly misses), a quarter starting far outside and pointing anywhere; some along an axis, with directions of any length."""
    rng = np.random.RandomState(7000 + (576 if F == "torus" else F))
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    w = rng.dirichlet([1.0, 1.0, 1.0], size=n)
    tri = v[f[rng.randint(len(f), size=n)]]
    target = (w[:, :, None] * tri).sum(1)
    o = 1.2 * rng.rand(n, 3) - 0.6
    far = (rng.rand(n, 3) - 0.5) * np.array([20.0, 2000.0, 2.0])
    kind = np.arange(n) % 4
    o = np.where((kind % 2 == 1)[:, None], far, o)
    d = np.where((kind < 2)[:, None], target - o, rng.randn(n, 3))
    d = d * np.exp(rng.uniform(-3.0, 3.0, size=(n, 1)))
    axis = np.arange(n) % 25 == 24                                       # along an axis: two zero components
    d[axis] = np.eye(3)[rng.randint(3, size=int(axis.sum()))] * rng.choice([-1.0, 2.0], size=(int(axis.sum()), 1))
    return o, d


def box12():
    """A closed box of 12 triangles (closest_point_ref's cube, scaled unevenly)."""
    return (R.CUBE_V * np.array([1.0, 1.5, 0.75], dtype=np.float32)).astype(np.float32), R.CUBE_F.copy()


def edges_of(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def leak_rays(verts, faces, inside):
    """From every point of ``inside`` (points inside the closed mesh): rays at every vertex, at every edge midpoint, 2 000 seeded random
    directions and the three axes both ways.  Whatever the roundings of the directions, a ray that starts inside a closed mesh hits it."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    e = edges_of(faces)
    mid = 0.5 * (v[e[:, 0]] + v[e[:, 1]])
    targets = np.concatenate([v, mid])
    rng = np.random.RandomState(4242)
    O, D = [], []
    for p in np.asarray(inside, dtype=np.float64).reshape(-1, 3):
        rnd = rng.randn(2000, 3)
        dd = np.concatenate([targets - p, rnd, np.eye(3), -np.eye(3)])
        O.append(np.repeat(p[None], len(dd), axis=0))
        D.append(dd)
    return np.concatenate(O), np.concatenate(D)


def axis_leak_rays(verts, faces):
    """Axis-parallel rays exactly through every vertex and every exactly representable edge midpoint of a closed mesh (two of the ray's
    coordinates ARE the target's: the sheared corner is the corner, exact arithmetic), started 4 units off.  They must hit: the line meets
    the closed surface at that very point."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    e = edges_of(faces)
    mid = 0.5 * (v[e[:, 0]] + v[e[:, 1]])
    exact = ((2.0 * mid - v[e[:, 0]] == v[e[:, 1]]) & (2.0 * mid - v[e[:, 1]] == v[e[:, 0]])).all(axis=1)   # the midpoint is ON the edge
    targets = np.concatenate([v, mid[exact]])
    O, D = [], []
    for ax in range(3):
        for sign in (1.0, -1.0):
            o = targets.copy()
            o[:, ax] = -sign * 4.0
            d = np.zeros_like(o)
            d[:, ax] = sign
            O.append(o)
            D.append(d)
    return np.concatenate(O), np.concatenate(D)


def torus_inside():
    """Three points on the centre circle of ``grid_mesh('torus')``'s tube (R = 0.30)."""
    ang = np.array([0.1, 2.0, 4.5])
    return np.stack([0.30 * np.cos(ang), 0.30 * np.sin(ang), np.zeros(3)], axis=1)


def tie_pair(swap):
    """Two triangles in the plane z = 0.25 sharing the edge x = 0, y in [-0.5, 0.5], their centroids far apart in x (different leaves at
    depth >= 1), among other faces; the ray down the z axis from (0, 0.125, 1) meets the shared edge: both faces give s = 0.75 exactly
    (every coordinate a small dyadic number).  ``swap`` exchanges the two faces' indices.  Returns (verts, faces, origin, dir, (i, j))."""
    sv, sf = R.soup(40, 11)
    sv = (sv * np.float32(0.25) + np.array([0.0, 0.0, -2.0], dtype=np.float32)).astype(np.float32)
    pair = np.array([[0.0, -0.5, 0.25], [0.0, 0.5, 0.25], [-1.0, 0.0, 0.25], [1.0, 0.0, 0.25]], dtype=np.float32)
    verts = np.concatenate([sv, pair]).astype(np.float32)
    V0 = len(sv)
    left, right = np.array([V0, V0 + 1, V0 + 2], dtype=np.int32), np.array([V0 + 1, V0, V0 + 3], dtype=np.int32)
    if swap:
        left, right = right, left
    faces = np.concatenate([sf[:7], left[None], sf[7:30], right[None], sf[30:]]).astype(np.int32)
    return verts, faces, np.array([[0.0, 0.125, 1.0]]), np.array([[0.0, 0.0, -1.0]]), (7, 31)


def bad_rays(verts, faces):
    """Rays that must miss with (+inf, -1): zero direction, NaN / inf in origin or direction, far outside pointing away; and two good rays."""
    o, d = grid_rays(8, verts, faces, 12)
    d[0] = 0.0
    d[1, 1] = np.nan
    d[2, 0] = np.inf
    o[3, 2] = np.nan
    o[4, 0] = -np.inf
    o[5], d[5] = [1e6, 1e6, 1e6], [1.0, 1.0, 1.0]
    o[6], d[6] = [0.0, -1e9, 0.0], [0.0, -1.0, 0.0]
    o[7], d[7] = [np.nan] * 3, [np.nan] * 3
    return o, d


def sensor_poses(n, seed, radius=1.0):
    """n seeded sensor poses (cam_pos, cam_rot [n,3]) round the origin at about ``radius``."""
    rng = np.random.RandomState(seed)
    pos = rng.randn(n, 3)
    pos = radius * pos / np.linalg.norm(pos, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, size=(n, 1))
    return pos, rng.uniform(-np.pi, np.pi, size=(n, 3))


def segment_case():
    """The unit square z = 0 (two faces) and a nearer one at z = 0.5, a ray down the z axis from (0.25, 0.125, 1): hits at s = 0.5 and 1.
    Returns (verts, faces, o, d, [(t_min, t_max, want_s, want_face)])."""
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, 0.5], [1, -1, 0.5], [1, 1, 0.5], [-1, 1, 0.5]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)
    o, d = np.array([[0.25, 0.125, 1.0]]), np.array([[0.0, 0.0, -1.0]])
    cases = [(0.0, np.inf, 0.5, 2),            # the nearer face
             (0.5, np.inf, 0.5, 2),            # a hit exactly at t_min is taken
             (0.5 + 2.0 ** -40, np.inf, 1.0, 0),
             (-3.0, -0.25, np.inf, -1),        # nothing behind the origin
             (0.0, 0.25, np.inf, -1),          # faces beyond t_max do not turn a miss into a hit
             (0.75, 1.0, 1.0, 0)]              # a hit exactly at t_max is taken; the nearer face is before t_min
    return verts, faces, o, d, cases


def behind_case():
    """A face behind the origin (s = -1) is not taken at the default t_min = 0."""
    verts, faces, o, d, _ = segment_case()
    return verts, faces, np.array([[0.25, 0.125, -1.0]]), d


def named_inputs():
    """(name, verts, faces, origins, dirs, depth) of every input the GPU test runs with the default segment [0, inf)."""
    for F in GRID_F + ("torus",):
        verts, faces = grid_mesh(F)
        o, d = grid_rays(F, verts, faces)
        for depth in GRID_DEPTH:
            yield f"grid-{F}-{depth}", verts, faces, o, d, depth
    verts, faces = grid_mesh("torus")
    yield ("leak-torus",) + (verts, faces) + leak_rays(verts, faces, torus_inside()) + (None,)
    yield ("axis-torus",) + (verts, faces) + axis_leak_rays(verts, faces) + (None,)
    verts, faces = box12()
    inside = np.array([[0.0, 0.0, 0.0], [0.125, -0.25, 0.0625], [-0.2, 0.3, 0.1]])
    yield ("leak-box",) + (verts, faces) + leak_rays(verts, faces, inside) + (1,)
    yield ("axis-box",) + (verts, faces) + axis_leak_rays(verts, faces) + (2,)
    for swap in (False, True):
        verts, faces, o, d, _ = tie_pair(swap)
        yield f"tie-{swap}", verts, faces, o, d, 2
    verts, faces = grid_mesh(8)
    yield ("bad-rays", verts, faces) + bad_rays(verts, faces) + (2,)
    for kind in ("repeated", "collinear"):
        for mixed in (False, True):
            verts, faces, pts = C.degenerate(kind, mixed)
            o, d = grid_rays(9, verts, faces, 64)
            o[:len(pts)] = pts[:len(o)]                                # starts on the degenerate faces' corners and lines too
            yield f"degenerate-{kind}-{mixed}", verts, faces, o, d, None
    verts, faces = C.one_leaf()
    yield ("one-leaf", verts, faces) + grid_rays(65, verts, faces, 70) + (3,)
    verts, faces = grid_mesh(65)
    yield ("sparse-deep", verts, faces) + grid_rays(65, verts, faces, 65) + (7,)
    verts, faces = C.bad_index_mesh()
    yield ("bad-index", verts, faces) + grid_rays(65, *grid_mesh(65), 130) + (None,)
