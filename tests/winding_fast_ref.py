"""The fast winding number (Barill et al. 2018) as numpy: csrc/winding_fast.hip's operations in that file's order.

Every number is float64 on the exactly converted float32 inputs; every product and sum below is one rounding (the library is built with
-ffp-contract=off), sums run left to right as written, and the only library call of a far term is one sqrt.

  frame     lo = the vertices' minimum corner, side = their largest extent (1 when that is 0), n = 2^depth cells per axis
  binning   a face lives in the leaf of its centroid ((a + b) + c) / 3: per axis clamp((int)floor((c - lo) / side * n), 0, n - 1);
            Morton code: bit 3k of a cell number is bit k of ix, bit 3k+1 of iy, bit 3k+2 of iz, so the children of cell m are 8m .. 8m+7
  pyramid   per level l an int32 [8^l]: the rank of an occupied cell among the occupied cells of its level in Morton order, else -1
  lists     the faces of every occupied leaf, ascending by face index; offsets [leaves + 1]
  record    36 float64 per occupied cell: p (3), r, N0 (3), M1[j][i] (9, at 7 + 3j + i), M2[jk][i] (18, at 16 + 3 pair + i with the pairs
            00 01 02 11 12 22), the total area A, the face count
  leaf      over its list in ascending order: A = sum a_t, S = sum a_t c_t, C = sum c_t; p = S / A (A > 0) or C / count; then about p the
            moments and r = sqrt(max |v - p|^2) over the faces' vertices
  inner     over its occupied children in Morton order: A = sum A_c, p = (sum A_c p_c) / A (A > 0) or (sum n_c p_c) / n; with d = p_c - p
            N0 += N0_c;  M1[j][i] += M1_c[j][i] + d_j N0_c[i];
            M2[jk][i] += ((M2_c[jk][i] + d_j M1_c[k][i]) + d_k M1_c[j][i]) + (d_j d_k) N0_c[i];  r = max(|d| + r_c)
  query     depth first, children in Morton order, the walk's state (level, cell); a cell with |q - p|^2 > beta^2 r^2 adds its expansion to
            `far`, a leaf that is not accepted adds 2 atan2(num, den) of each of its faces, in list order, to `near`;
            w = (far + near) / (4 pi)
"""
import numpy as np

MAX_DEPTH = 7
REC = 36
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
PAIR_OF = {(j, k): n for n, (j, k) in enumerate(PAIRS)}
PAIR_OF.update({(k, j): n for n, (j, k) in enumerate(PAIRS)})
FOUR_PI = 4.0 * 3.14159265358979323846


def default_depth(F):
    L = 1
    while L < MAX_DEPTH and 8 ** L * 8 < F:
        L += 1
    return L


def morton(ix, iy, iz, depth):
    code = np.zeros_like(ix)
    for k in range(depth):
        code |= ((ix >> k) & 1) << (3 * k) | ((iy >> k) & 1) << (3 * k + 1) | ((iz >> k) & 1) << (3 * k + 2)
    return code


def corners(verts, faces):
    """float64 [F, 3, 3] corners with the exact kernel's index clamp."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.clip(np.asarray(faces, dtype=np.int64), 0, len(v) - 1)
    return v[f]


def face_terms(tri):
    """(area vector [F,3], area [F], centroid [F,3]) of corners [F,3,3]."""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e1, e2 = b - a, c - a
    nv = np.stack([0.5 * (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]),
                   0.5 * (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]),
                   0.5 * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])], 1)
    area = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
    cen = ((a + b) + c) / 3.0
    return nv, area, cen


def face_moments(tri, nv, cen, p):
    """One face's (N0 [3], M1 [3][3], M2 [6][3]) about p, as the leaf pass adds them."""
    d = cen - p
    m1 = np.empty((3, 3))
    for j in range(3):
        for i in range(3):
            m1[j, i] = d[j] * nv[i]
    mids = (0.5 * (tri[0] + tri[1]) - p, 0.5 * (tri[1] + tri[2]) - p, 0.5 * (tri[2] + tri[0]) - p)
    m2 = np.empty((6, 3))
    for n, (j, k) in enumerate(PAIRS):
        cjk = ((mids[0][j] * mids[0][k] + mids[1][j] * mids[1][k]) + mids[2][j] * mids[2][k]) / 3.0
        for i in range(3):
            m2[n, i] = cjk * nv[i]
    return nv, m1, m2


def leaf_record(tri, nv, area, cen, idx):
    """The record of a leaf whose ascending face list is idx."""
    A = 0.0
    S = np.zeros(3)
    C = np.zeros(3)
    for t in idx:
        A = A + area[t]
        S = S + area[t] * cen[t]
        C = C + cen[t]
    p = S / A if A > 0.0 else C / float(len(idx))
    rec = np.zeros(REC)
    rec[0:3] = p
    r2 = 0.0
    n0 = np.zeros(3)
    m1 = np.zeros((3, 3))
    m2 = np.zeros((6, 3))
    for t in idx:
        f0, f1, f2 = face_moments(tri[t], nv[t], cen[t], p)
        n0 = n0 + f0
        m1 = m1 + f1
        m2 = m2 + f2
        for k in range(3):
            d = tri[t, k] - p
            r2 = max(r2, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    rec[3] = np.sqrt(r2)
    rec[4:7] = n0
    rec[7:16] = m1.reshape(9)
    rec[16:34] = m2.reshape(18)
    rec[34] = A
    rec[35] = float(len(idx))
    return rec


def translate(child, p):
    """A child's (N0, M1, M2, |d| + r) about the parent's p."""
    d = child[0:3] - p
    n0 = child[4:7]
    c1 = child[7:16].reshape(3, 3)
    c2 = child[16:34].reshape(6, 3)
    m1 = np.empty((3, 3))
    for j in range(3):
        for i in range(3):
            m1[j, i] = c1[j, i] + d[j] * n0[i]
    m2 = np.empty((6, 3))
    for n, (j, k) in enumerate(PAIRS):
        for i in range(3):
            m2[n, i] = ((c2[n, i] + d[j] * c1[k, i]) + d[k] * c1[j, i]) + (d[j] * d[k]) * n0[i]
    reach = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + child[3]
    return n0, m1, m2, reach


def inner_record(children):
    A = 0.0
    cnt = 0.0
    S = np.zeros(3)
    C = np.zeros(3)
    for c in children:
        A = A + c[34]
        cnt = cnt + c[35]
        S = S + c[34] * c[0:3]
        C = C + c[35] * c[0:3]
    p = S / A if A > 0.0 else C / cnt
    rec = np.zeros(REC)
    rec[0:3] = p
    n0 = np.zeros(3)
    m1 = np.zeros((3, 3))
    m2 = np.zeros((6, 3))
    r = 0.0
    for c in children:
        t0, t1, t2, reach = translate(c, p)
        n0 = n0 + t0
        m1 = m1 + t1
        m2 = m2 + t2
        r = max(r, reach)
    rec[3] = r
    rec[4:7] = n0
    rec[7:16] = m1.reshape(9)
    rec[16:34] = m2.reshape(18)
    rec[34] = A
    rec[35] = cnt
    return rec


class Tree:
    pass


def build(verts, faces, depth=None):
    tri = corners(verts, faces) if len(faces) else np.zeros((0, 3, 3))
    F = len(tri)
    L = default_depth(F) if depth is None else int(depth)
    assert 1 <= L <= MAX_DEPTH
    t = Tree()
    t.depth, t.n_faces, t.tri = L, F, tri
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t.lo = v.min(0) if len(v) else np.zeros(3)
    ext = (v.max(0) - t.lo).max() if len(v) else 0.0
    t.side = ext if ext > 0.0 else 1.0
    t.pyramid = [np.full(8 ** l, -1, dtype=np.int32) for l in range(L + 1)]
    t.records = [np.zeros((0, REC)) for _ in range(L + 1)]
    t.list_offsets = np.zeros(1, dtype=np.int32)
    t.lists = np.zeros(0, dtype=np.int32)
    t.codes = np.zeros(0, dtype=np.int64)
    if F == 0:
        return t
    nv, area, cen = face_terms(tri)
    n = 2 ** L
    cell = np.floor((cen - t.lo) / t.side * n)
    cell = np.clip(cell, 0, n - 1).astype(np.int64)
    t.codes = morton(cell[:, 0], cell[:, 1], cell[:, 2], L)
    occ = np.unique(t.codes)
    for l in range(L, -1, -1):
        t.pyramid[l][occ] = np.arange(len(occ), dtype=np.int32)
        occ = np.unique(occ >> 3)
    order = np.argsort(t.codes, kind="stable")                      # ascending face index inside every leaf
    t.lists = order.astype(np.int32)
    counts = np.bincount(t.pyramid[L][t.codes], minlength=int(t.pyramid[L].max()) + 1)
    t.list_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    leaves = [leaf_record(tri, nv, area, cen, t.lists[t.list_offsets[k]:t.list_offsets[k + 1]]) for k in range(len(counts))]
    t.records[L] = np.array(leaves)
    for l in range(L - 1, -1, -1):
        recs = []
        for m in np.nonzero(t.pyramid[l] >= 0)[0]:
            kids = t.pyramid[l + 1][8 * m:8 * m + 8]
            recs.append(inner_record([t.records[l + 1][k] for k in kids if k >= 0]))
        t.records[l] = np.array(recs)
    return t


def expansion(rec, q, order):
    """The cell expansions [n] of records [n, 36] at queries q [n, 3], in units of solid angle (w = sum / 4 pi)."""
    rx, ry, rz = rec[:, 0] - q[:, 0], rec[:, 1] - q[:, 1], rec[:, 2] - q[:, 2]
    rho = (rx, ry, rz)
    r2 = (rx * rx + ry * ry) + rz * rz
    r1 = np.sqrt(r2)
    r3 = r2 * r1
    out = ((rx * rec[:, 4] + ry * rec[:, 5]) + rz * rec[:, 6]) / r3
    if order >= 1:
        r5 = r3 * r2
        M1 = lambda j, i: rec[:, 7 + 3 * j + i]
        tr = (M1(0, 0) + M1(1, 1)) + M1(2, 2)
        q1 = 0.0
        for j in range(3):
            q1 = q1 + rho[j] * ((rx * M1(j, 0) + ry * M1(j, 1)) + rz * M1(j, 2))
        out = out + (tr / r3 - 3.0 * q1 / r5)
    if order >= 2:
        r7 = r5 * r2
        M2 = lambda j, k, i: rec[:, 16 + 3 * PAIR_OF[(j, k)] + i]
        sA = 0.0
        for k in range(3):
            sA = sA + rho[k] * ((M2(0, k, 0) + M2(1, k, 1)) + M2(2, k, 2))
        sB = 0.0
        sC = 0.0
        for i in range(3):
            sB = sB + rho[i] * ((M2(0, 0, i) + M2(1, 1, i)) + M2(2, 2, i))
            diag = ((rx * rx) * M2(0, 0, i) + (ry * ry) * M2(1, 1, i)) + (rz * rz) * M2(2, 2, i)
            off = ((rx * ry) * M2(0, 1, i) + (rx * rz) * M2(0, 2, i)) + (ry * rz) * M2(1, 2, i)
            sC = sC + rho[i] * (diag + 2.0 * off)
        out = out + 0.5 * (15.0 * sC / r7 - 3.0 * (2.0 * sA + sB) / r5)
    return out


def solid_angle(tri, q):
    """2 atan2(num, den) of corners [n,3,3] seen from q [n,3]: winding_kernel's expression."""
    a, b, c = tri[:, 0] - q, tri[:, 1] - q, tri[:, 2] - q
    dot = lambda u, v: u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    num = a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]) + \
        a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
    den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
    return 2.0 * np.arctan2(num, den)


def query(t, pts, accuracy=2.0, order=2):
    """(w float64 [N], stats int32 [N, 2], far [N], near [N], sum of |near terms| [N]): every query walks its own path; the walks
    advance together."""
    q = np.asarray(pts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    N = len(q)
    far, near, near_abs = np.zeros(N), np.zeros(N), np.zeros(N)
    stats = np.zeros((N, 2), dtype=np.int32)
    if t.n_faces == 0 or N == 0:
        return np.zeros(N), stats, far, near, near_abs
    beta2 = float(accuracy) * float(accuracy)
    L = t.depth
    level = np.zeros(N, dtype=np.int64)
    cell = np.zeros(N, dtype=np.int64)
    live = np.ones(N, dtype=bool)
    while live.any():
        descend = np.zeros(N, dtype=bool)
        for l in np.unique(level[live]):
            at = np.nonzero(live & (level == l))[0]
            rk = t.pyramid[l][cell[at]]
            at, rk = at[rk >= 0], rk[rk >= 0]
            if len(at) == 0:
                continue
            rec = t.records[l][rk]
            d = rec[:, 0:3] - q[at]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            ok = d2 > beta2 * (rec[:, 3] * rec[:, 3])
            if ok.any():
                far[at[ok]] = far[at[ok]] + expansion(rec[ok], q[at[ok]], order)
                stats[at[ok], 0] += 1
            if l < L:
                descend[at[~ok]] = True
            else:
                at, rk = at[~ok], rk[~ok]
                o, e = t.list_offsets[rk], t.list_offsets[rk + 1]
                stats[at, 1] += (e - o)
                j = 0
                while len(at):
                    keep = o + j < e
                    at, o, e = at[keep], o[keep], e[keep]
                    if len(at) == 0:
                        break
                    term = solid_angle(t.tri[t.lists[o + j]], q[at])
                    near[at] = near[at] + term
                    near_abs[at] += np.abs(term)
                    j += 1
        level = np.where(descend, level + 1, level)
        cell = np.where(descend, cell * 8, cell + np.where(live, 1, 0))
        while True:
            up = live & ~descend & (level > 0) & (cell % 8 == 0)
            if not up.any():
                break
            cell = np.where(up, cell // 8, cell)
            level = np.where(up, level - 1, level)
        live = live & (descend | (level > 0))
    return (far + near) / FOUR_PI, stats, far, near, near_abs


def fast(verts, faces, pts, depth=None, accuracy=2.0, order=2):
    return query(build(verts, faces, depth), pts, accuracy, order)[0]
