"""The voxelisers of vtaco_amd/csrc/voxelize.hip restated in float64 numpy ("voxelize.hip"), and the meshes the tests share.

Grid units: g = ((v - loc) / scale + 0.5) * res per component, in that order, float64 from the float32 vertices.  Voxel (i, j, k) is the
closed box [i, i+1] x [j, j+1] x [k, k+1] with centre (i+.5, j+.5, k+.5).

surface   a voxel is set when its box overlaps a triangle by the 13-axis separating-axis test (equality = overlap); only the voxels of
          the triangle's bounding box, clipped to the grid, are tested.
interior  parity of the crossings of the +z ray from each voxel centre, per triangle: every column centre of the projected bounding box is
          tested against three edge functions, each evaluated on the edge's canonical direction (lower vertex index first) and negated
          when the triangle walks it the other way; an exact 0 is decided as if the centre sat at (+eps, +eps^2).  Inside columns flip
          the voxels k < clamp(ceil(z - .5), 0, res).
ray       surface | interior.

Every function also reports its smallest decisive margin in grid units, so that a test can state how far its cases are from a tie.
"""
import numpy as np


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def torus(nu, nv, R=0.30, r=0.12):
    """(vertices float64 [nu*nv, 3], faces int64 [2*nu*nv, 3]): vertex (i, j) has index i*nv + j."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    u, v = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    faces = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)
    return verts, faces.astype(np.int64)


def rotate(verts, seed):
    """float32 vertices after the rotation Q of qr(RandomState(seed).randn(3, 3)) (first column negated when det < 0)."""
    q, _ = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return (verts @ q.T).astype(np.float32)


def solid_torus(nu, nv, seed):
    v, f = torus(nu, nv)
    return rotate(v, seed), f


def shell(seed=4):
    """A hollow shell: torus(24, 12, .30, .14) and, inside it, torus(24, 12, .30, .07) with reversed faces."""
    vo, fo = torus(24, 12, 0.30, 0.14)
    vi, fi = torus(24, 12, 0.30, 0.07)
    return rotate(np.concatenate([vo, vi]), seed), np.concatenate([fo, fi[:, ::-1] + len(vo)])


def box(lo=4.5, hi=11.5, res=16):
    """The axis-aligned box with corners at grid coordinates ``lo`` / ``hi`` (loc 0, scale 1): 12 triangles, outward, the diagonals of the
    z faces through column centres.  float32-exact for the defaults."""
    a, b = lo / res - 0.5, hi / res - 0.5
    v = np.array([[x, y, z] for x in (a, b) for y in (a, b) for z in (a, b)], dtype=np.float32)          # index 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]           # -x +x -y +y -z +z
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
    return v, f


# the committed cases: name -> (mesh builder, resolution); tests/test_voxelize_ref_cpu.py pins their counts and margins
CASES = {
    "torus16x8": (lambda: solid_torus(16, 8, 1), 16),
    "torus24x12": (lambda: solid_torus(24, 12, 2), 33),
    "torus12x6": (lambda: solid_torus(12, 6, 3), 24),
    "shell": (lambda: shell(4), 44),
}


def default_frame(verts):
    """(loc float64 [3], scale float): the bounds' centre and max extent / 0.9, float64 from the float32 vertices."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return (lo + hi) / 2, float((hi - lo).max() / 0.9)


def to_grid(verts, loc, scale, res):
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    return ((v - np.asarray(loc, dtype=np.float64)) / float(scale) + 0.5) * res


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def surface(verts, faces, res, loc=(0, 0, 0), scale=1.0):
    """(occ bool [res]^3, margin): margin = the smallest |slack| over the tested voxels, where a voxel's slack is the minimum over the 13
    axes of (box radius + triangle radius - centre distance) / |axis| (axes of zero length are skipped)."""
    g = to_grid(verts, loc, scale, res)
    occ = np.zeros((res,) * 3, dtype=bool)
    margin = np.inf
    unit = np.eye(3)
    for f in np.asarray(faces):
        t = g[f]                                                       # [3 vertices, 3]
        lo = np.maximum(np.ceil(t.min(0)).astype(np.int64) - 1, 0)
        hi = np.minimum(np.floor(t.max(0)).astype(np.int64), res - 1)
        if (lo > hi).any():
            continue
        ii, jj, kk = np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij")
        c = np.stack([ii, jj, kk], -1).reshape(-1, 3) + 0.5
        p = t[None, :, :] - c[:, None, :]                              # [cells, 3 vertices, 3]
        e = [t[1] - t[0], t[2] - t[1], t[0] - t[2]]
        axes = [unit[0], unit[1], unit[2], np.cross(e[0], e[1])] + [np.cross(e[a], unit[b]) for a in range(3) for b in range(3)]
        slack = np.full(len(c), np.inf)
        sep = np.zeros(len(c), dtype=bool)
        for ax in axes:
            d = p[:, :, 0] * ax[0] + p[:, :, 1] * ax[1] + p[:, :, 2] * ax[2]
            r = 0.5 * (abs(ax[0]) + abs(ax[1]) + abs(ax[2]))
            s = np.minimum(r - d.min(1), d.max(1) + r)                 # < 0: this axis separates
            sep |= s < 0
            n = np.sqrt(ax @ ax)
            if n > 0:
                slack = np.minimum(slack, s / n)
        if len(c):
            margin = min(margin, float(np.abs(slack).min()))
        hit = ~sep
        occ[ii.reshape(-1)[hit], jj.reshape(-1)[hit], kk.reshape(-1)[hit]] = True
    return occ, margin


# ---- interior -----------------------------------------------------------------------------------------------------------------------
def _edge(ia, ib, xy, cx, cy):
    """(value, sign) of the edge function of the edge the triangle walks ia -> ib at the centres: evaluated on the canonical direction
    (lower vertex index first) and negated when the walk is the other way; sign in {-1, +1} after the tie rule."""
    flip = ia > ib
    a, b = (xy[ib], xy[ia]) if flip else (xy[ia], xy[ib])
    val = (b[0] - a[0]) * (cy - a[1]) - (b[1] - a[1]) * (cx - a[0])
    tie = -(b[1] - a[1]) if (b[1] - a[1]) != 0 else (b[0] - a[0])
    sgn = np.where(val != 0, np.sign(val), np.sign(tie))
    return (-val, -sgn) if flip else (val, sgn)


def interior(verts, faces, res, loc=(0, 0, 0), scale=1.0):
    """(occ bool [res]^3, edge margin, crossing margin).  edge margin: over the tested centres, the distance to the edge line that decides
    the centre (inside: the nearest of the three; outside: the farthest of those on whose wrong side it lies).  crossing margin: the
    distance of z - .5 from an integer at the inside centres."""
    g = to_grid(verts, loc, scale, res)
    xy, z = g[:, :2], g[:, 2]
    occ = np.zeros((res,) * 3, dtype=bool)
    m_edge = m_cross = np.inf
    ks = np.arange(res)
    for f in np.asarray(faces):
        i0, i1, i2 = (int(x) for x in f)
        p0, p1, p2 = xy[i0], xy[i1], xy[i2]
        A = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])
        if A == 0:
            continue
        t = xy[[i0, i1, i2]]
        lo = np.maximum(np.ceil(t.min(0) - 0.5).astype(np.int64), 0)
        hi = np.minimum(np.floor(t.max(0) - 0.5).astype(np.int64), res - 1)
        if (lo > hi).any():
            continue
        ii, jj = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        cx, cy = ii + 0.5, jj + 0.5
        e0, s0 = _edge(i1, i2, xy, cx, cy)
        e1, s1 = _edge(i2, i0, xy, cx, cy)
        e2, s2 = _edge(i0, i1, xy, cx, cy)
        sa = 1.0 if A > 0 else -1.0
        inside = (s0 == sa) & (s1 == sa) & (s2 == sa)
        dist = np.stack([np.abs(e0) / np.hypot(*(p2 - p1)), np.abs(e1) / np.hypot(*(p0 - p2)), np.abs(e2) / np.hypot(*(p1 - p0))])
        wrong = np.stack([s0 != sa, s1 != sa, s2 != sa])
        decisive = np.where(inside, dist.min(0), np.where(wrong, dist, -np.inf).max(0))
        m_edge = min(m_edge, float(decisive.min()))
        if not inside.any():
            continue
        zc = (e0[inside] * z[i0] + e1[inside] * z[i1] + e2[inside] * z[i2]) / A
        m_cross = min(m_cross, float(np.abs((zc - 0.5) - np.round(zc - 0.5)).min()))
        n = np.clip(np.ceil(zc - 0.5), 0, res).astype(np.int64)
        occ[ii[inside], jj[inside]] ^= ks[None, :] < n[:, None]
    return occ, m_edge, m_cross


def ray(verts, faces, res, loc=(0, 0, 0), scale=1.0):
    return surface(verts, faces, res, loc, scale)[0] | interior(verts, faces, res, loc, scale)[0]


def pack_bits(occ):
    """bool [res]^3 -> uint32 [res, res, ceil(res / 32)]: bit k % 32 of word k // 32 (the layout of vt_voxelize_interior)."""
    res = occ.shape[0]
    words = (res + 31) // 32
    padded = np.zeros((res, res, words * 32), dtype=np.uint64)
    padded[:, :, :res] = occ
    return (padded.reshape(res, res, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def centres(res, loc, scale):
    """World coordinates float64 [res^3, 3] of the voxel centres, C order [x][y][z]."""
    c = (np.arange(res) + 0.5) / res - 0.5
    grid = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    return grid * float(scale) + np.asarray(loc, dtype=np.float64)


def winding_number(verts, faces, pts, chunk=8192):
    """float64 generalized winding number (Van Oosterom-Strackee solid angles), the independent check of ``interior``; torch on the CPU
    only for its threads."""
    import torch
    tri = torch.from_numpy(np.asarray(verts, dtype=np.float32).astype(np.float64)[np.asarray(faces)])       # [F, 3, 3]
    pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64))
    out = torch.empty(len(pts), dtype=torch.float64)
    for s in range(0, len(pts), chunk):
        q = pts[s:s + chunk, None, :]
        a, b, c = tri[None, :, 0] - q, tri[None, :, 1] - q, tri[None, :, 2] - q
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.linalg.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = (2.0 * torch.atan2(num, den)).sum(-1) / (4.0 * np.pi)
    return out.numpy()
