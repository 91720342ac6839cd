"""csrc/knn.hip restated in float64 numpy ("knn.hip"): the definition of the k nearest neighbours, the walk of the point tree
that finds them, the normals and the outlier rule, this file's operations in the kernels' order, and the inputs the CPU and the GPU
tests share.

brute(src, dst, k, T)                  d2 = (dx dx + dy dy) + dz dz, d = q - p, of every pair; per query the k smallest in the order
                                       (d2, index) by np.lexsort((index, d2)); entries that are not below +inf are (+inf, -1)
tree(ref_tree, src, k, T, seed, order) point_tree_ref.query's lock-step walk with a list per query: a target is taken when
                                       d < worst or (d == worst and m < worst_m), worst the list's last entry; a cell is skipped exactly
                                       when lb > worst.  Returns d2, idx and stats (boxes tested, points tested)
covariance(pts, idx), normals(pts, idx, view)   vt_knn_normals' operations in its order
outlier_mask(points, k, std_ratio)     the statistic, the threshold and the mask of utils.pointcloud.statistical_outlier_mask
"""
import functools

import numpy as np

import icp_ref as R
import point_tree_ref as P

MAX_K = 32
SWEEPS = 8
U = 2.0 ** -53


def slab_points(N, M, B=1):
    """vt_knn_points_slab_points."""
    qtiles = (N + 255) // 256 * B
    chunks = (M + 255) // 256
    want = max(1, 2048 // qtiles)
    return 256 * max(2, (chunks + want - 1) // want)


def _moved(src, T):
    q = np.ascontiguousarray(src, dtype=np.float64)
    return q if T is None else R._move(np.asarray(T, dtype=np.float64), q)


def brute(src, dst, k, T=None):
    q, dst = _moved(src, T), np.ascontiguousarray(dst, dtype=np.float64)
    N, M = len(q), len(dst)
    out_d, out_i = np.full((N, k), np.inf), np.full((N, k), -1, dtype=np.int32)
    kk = min(k, M)
    rows = max(1, (1 << 23) // M)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, N, rows):
            qc = q[r0:r0 + rows]
            dx, dy, dz = (qc[:, a, None] - dst[None, :, a] for a in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 < np.inf, d2, np.inf)                   # a NaN or an infinite d2 is never taken
            thr = np.partition(d2, kk - 1, axis=1)[:, kk - 1]        # only what can be among the k smallest is sorted
            row, col = np.nonzero(d2 <= thr[:, None])
            val = d2[row, col]
            at = np.lexsort((col, val, row))                         # per query (row) by (d2, index)
            row, col, val = row[at], col[at], val[at]
            slot = np.arange(len(row)) - np.searchsorted(row, row)   # the place inside the query's sorted candidates
            sel = (slot < kk) & (val < np.inf)
            out_d[r0 + row[sel], slot[sel]] = val[sel]
            out_i[r0 + row[sel], slot[sel]] = col[sel]
    return out_d, out_i


def tree(ref_tree, src, k, T=None, seed=True, order=True):
    q = _moved(src, T)
    N, L = q.shape[0], ref_tree["depth"]
    lo, side = ref_tree["lo"], ref_tree["side"]
    pyr = np.concatenate(ref_tree["pyramids"]).astype(np.int64)
    boxes = np.concatenate(ref_tree["boxes"])
    base = np.concatenate([[0], np.cumsum(ref_tree["counts"])]).astype(np.int64)
    loff, lists, points = ref_tree["offsets"].astype(np.int64), ref_tree["lists"], ref_tree["points"]
    best = np.full((N, k), np.inf)
    bidx = np.full((N, k), -1, dtype=np.int32)
    stats = np.zeros((N, 2), dtype=np.int32)

    def leaf(ids, rk):
        o, e = loff[rk], loff[rk + 1]
        stats[ids, 1] += (e - o).astype(np.int32)
        for j in range(int((e - o).max()) if len(ids) else 0):
            m = o + j < e
            i, t = ids[m], (o + j)[m]
            d = q[i] - points[t]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            li = lists[t]
            upd = (d2 < best[i, k - 1]) | ((d2 == best[i, k - 1]) & (li < bidx[i, k - 1]))
            ii = i[upd]
            ld = np.concatenate([best[ii], d2[upd][:, None]], axis=1)
            lm = np.concatenate([bidx[ii], li[upd][:, None]], axis=1)
            at = np.lexsort((lm, ld), axis=1)[:, :k]                 # the entry goes in front of the first it is smaller than; the last drops out
            best[ii] = np.take_along_axis(ld, at, axis=1)
            bidx[ii] = np.take_along_axis(lm, at, axis=1)

    with np.errstate(invalid="ignore", over="ignore"):
        seed_rk = np.full(N, -1, dtype=np.int64)
        if seed:
            seed_rk = pyr[(8 ** L - 1) // 7 + P.cell_codes(q, lo, side, L)]
            sel = np.nonzero(seed_rk >= 0)[0]
            leaf(sel, seed_rk[sel])
        level = np.zeros(N, dtype=np.int64)
        cell = np.zeros(N, dtype=np.int64)
        flip = np.zeros(N, dtype=np.int64)
        live = np.ones(N, dtype=bool)
        while live.any():
            ids = np.nonzero(live)[0]
            lv, actual = level[ids], cell[ids] ^ flip[ids]
            rk = pyr[(8 ** lv - 1) // 7 + actual]
            occ = rk >= 0
            b = boxes[np.where(occ, base[lv] + rk, 0)]
            qq = q[ids]
            e = np.where(qq < b[:, :3], b[:, :3] - qq, np.where(qq > b[:, 3:], qq - b[:, 3:], 0.0))
            lb = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            stats[ids[occ], 0] += 1
            go = occ & ~(lb > best[ids, k - 1])
            descend = go & (lv < L)
            at_leaf = go & (lv == L) & (rk != seed_rk[ids])
            leaf(ids[at_leaf], rk[at_leaf])
            o = np.zeros(len(ids), dtype=np.int64)
            if order:
                h = side * (1.0 / (1 << lv).astype(np.float64))
                for a in range(3):
                    centre = lo[a] + (P._gather(actual >> a).astype(np.float64) + 0.5) * h
                    o |= (qq[:, a] >= centre).astype(np.int64) << a
            d_ids = ids[descend]
            level[d_ids] += 1
            cell[d_ids] *= 8
            flip[d_ids] = flip[d_ids] * 8 + o[descend]
            n_ids = ids[~descend]
            cell[n_ids] += 1
            while True:
                up = n_ids[(level[n_ids] > 0) & ((cell[n_ids] & 7) == 0)]
                if not len(up):
                    break
                cell[up] >>= 3
                flip[up] >>= 3
                level[up] -= 1
            live[n_ids[level[n_ids] == 0]] = False
    return best, bidx, stats


# ---- normals ---------------------------------------------------------------------------------------------------------------------------
def covariance(pts, idx):
    """(C [N,3,3], count [N]): differences from the first valid neighbour, their mean, the six sums in ascending slot order, / count."""
    pts, idx = np.ascontiguousarray(pts, dtype=np.float64), np.asarray(idx).astype(np.int64)
    N, k = idx.shape
    M = len(pts)
    valid = (idx >= 0) & (idx < M)
    count = valid.sum(1)
    safe = np.where(valid, idx, 0)
    first = safe[np.arange(N), valid.argmax(1)]
    r = pts[first]
    s = np.zeros((N, 3))
    for j in range(k):
        s = np.where(valid[:, j, None], s + (pts[safe[:, j]] - r), s)
    cnt = np.maximum(count, 1).astype(np.float64)[:, None]
    mbar = s / cnt
    c = np.zeros((N, 6))
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j in range(k):
        f = (pts[safe[:, j]] - r) - mbar
        prod = np.stack([f[:, a] * f[:, b] for a, b in pairs], axis=1)
        c = np.where(valid[:, j, None], c + prod, c)
    c = c / cnt
    C = np.empty((N, 3, 3))
    for n, (a, b) in enumerate(pairs):
        C[:, a, b] = c[:, n]
        C[:, b, a] = c[:, n]
    return C, count


def _rotate(A, V, p, q, r):
    app, aqq, apq, arp, arq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy(), A[:, r, p].copy(), A[:, r, q].copy()
    act = apq != 0.0
    with np.errstate(all="ignore"):
        zeta = (aqq - app) / (2.0 * apq)
        t = 1.0 / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
        t = np.where(zeta < 0.0, -t, t)
        c = 1.0 / np.sqrt(1.0 + t * t)
        s = c * t
        new = {(p, p): app - t * apq, (q, q): aqq + t * apq, (p, q): np.zeros_like(apq), (r, p): c * arp - s * arq, (r, q): s * arp + c * arq}
        vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
        nvp, nvq = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    for (a, b), val in new.items():
        A[:, a, b] = np.where(act, val, A[:, a, b])
        A[:, b, a] = A[:, a, b]
    V[:, :, p] = np.where(act[:, None], nvp, vp)
    V[:, :, q] = np.where(act[:, None], nvq, vq)


def normals(pts, idx, view=None):
    """(normal [N,3], eig [N,3]); view None, [3] or [N,3]."""
    pts, idx = np.ascontiguousarray(pts, dtype=np.float64), np.asarray(idx).astype(np.int64)
    C, count = covariance(pts, idx)
    N, M = len(idx), len(pts)
    ok = (count >= 3) & (C != 0.0).any((1, 2))
    A = C.copy()
    V = np.tile(np.identity(3), (N, 1, 1))                           # V[:, :, j]: column j
    for _ in range(SWEEPS):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1)
    for a, b in ((0, 1), (1, 2), (0, 1)):
        sw = lam[:, a] > lam[:, b]
        lam[sw, a], lam[sw, b] = lam[sw, b], lam[sw, a]
        V[sw, :, a], V[sw, :, b] = V[sw, :, b], V[sw, :, a]
    v0 = V[:, :, 0]
    with np.errstate(all="ignore"):
        n = v0 / np.sqrt((v0[:, 0] * v0[:, 0] + v0[:, 1] * v0[:, 1]) + v0[:, 2] * v0[:, 2])[:, None]
    m_q = idx[:, 0]
    q_ok = (m_q >= 0) & (m_q < M)
    if view is not None:
        w = np.broadcast_to(np.asarray(view, dtype=np.float64), (N, 3))
        pq = pts[np.where(q_ok, m_q, 0)]
        by_view = (n[:, 0] * (w[:, 0] - pq[:, 0]) + n[:, 1] * (w[:, 1] - pq[:, 1])) + n[:, 2] * (w[:, 2] - pq[:, 2]) < 0.0
    big = n[:, 0].copy()
    for a in (1, 2):
        big = np.where(np.abs(n[:, a]) > np.abs(big), n[:, a], big)
    flip = big < 0.0
    if view is not None:
        flip = np.where(q_ok, by_view, flip)
    n = np.where(flip[:, None], -n, n)
    return np.where(ok[:, None], n, 0.0), np.where(ok[:, None], lam, 0.0)


def normal_gates(C, n, lam0, k):
    """(residual, Rayleigh error, length error) / their gates for one normal and the restatement's covariance C [3,3]."""
    frob = float(np.sqrt((C * C).sum()))
    gate = 8.0 * (k + 8) * U * frob
    cn = C @ n
    ray = float(n @ cn)
    return float(np.linalg.norm(cn - ray * n)) / gate, abs(ray - lam0) / gate, abs(float(np.sqrt(n @ n)) - 1.0) / (4.0 * U)


# ---- the outlier rule ----------------------------------------------------------------------------------------------------------------------
def outlier_mask(points, k=20, std_ratio=2.0):
    """(mask, statistic [N], threshold): the mean distance to the k nearest (self included), kept when <= mean + std_ratio std (N - 1)."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    N = len(points)
    d2, _ = brute(points, points, min(k, N))
    stat = np.sqrt(d2).mean(1)
    mean = stat.mean()
    std = np.sqrt(((stat - mean) ** 2).sum() / max(N - 1, 1))
    thr = mean + std_ratio * std
    return stat <= thr, stat, thr


# ---- the inputs the CPU and the GPU tests share ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def k1_case():
    """(src [2,257,3], dst [2,300,3], T [2,4,4])."""
    rng = np.random.default_rng(158)
    return rng.random((2, 257, 3)) - 0.5, rng.random((2, 300, 3)) - 0.5, np.stack([P.pose_of(11), P.pose_of(12)])


@functools.lru_cache(maxsize=None)
def short_cases():
    """[(src, dst, k)]: M 5 with k 8, M 8 with k 8, M 33 with k 32."""
    rng = np.random.default_rng(175)
    src = rng.random((65, 3)) - 0.5
    return [(src, rng.random((M, 3)) - 0.5, k) for M, k in ((5, 8), (8, 8), (33, 32))]


@functools.lru_cache(maxsize=None)
def tie_case():
    """(queries [91,3], targets [128,3]): a 4 x 4 x 4 integer lattice stored twice; its points and the 27 cell centres."""
    g = np.arange(4, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    centres = lat[(lat < 3.0).all(1)] + 0.5
    return np.concatenate([lat, centres]), np.concatenate([lat, lat])


@functools.lru_cache(maxsize=None)
def edge_case(N):
    """(src [N,3], dst [2 slab + 1, 3]): targets along a jittered line in index order, so the neighbours of a point with index near a
    multiple of the slab lie on both sides of the slab's edge; the first queries sit on targets slab, slab - 1, 2 slab and 256."""
    slab = slab_points(N, 1025)
    M = 2 * slab + 1
    rng = np.random.default_rng(1025)
    dst = np.stack([np.arange(M) / 64.0, 0.001 * rng.standard_normal(M), 0.001 * rng.standard_normal(M)], axis=1)
    src = dst[rng.integers(0, M, size=N)] + 0.002 * rng.standard_normal((N, 3))
    at = [slab, slab - 1, 2 * slab, 256][:N]
    src[:len(at)] = dst[at] + 1e-4
    return src, dst


@functools.lru_cache(maxsize=None)
def one_cell_case():
    """(src [3,3], dst [41,3]): 40 copies of one point and one far outlier."""
    p = np.array([0.3, -0.2, 0.1])
    dst = np.concatenate([np.tile(p, (40, 1)), [[5.0, 5.0, 5.0]]])
    return np.array([p, p + 0.25, [4.0, 4.0, 4.0]]), dst


@functools.lru_cache(maxsize=None)
def batch_case():
    """(src [3,64,3] with a NaN row in every problem, dst [3,100,3]): three problems with three target sets."""
    rng = np.random.default_rng(3)
    src, dst = rng.random((3, 64, 3)) - 0.5, (rng.random((3, 100, 3)) - 0.5) * np.array([1.0, 2.0, 0.5])[:, None, None]
    src[0, 5] = np.nan
    src[1, 6, 1] = np.nan
    src[2, 7, 2] = np.inf
    return src, dst


@functools.lru_cache(maxsize=None)
def pruning_cloud():
    return np.random.default_rng(20000).random((20000, 3)) - 0.5


@functools.lru_cache(maxsize=None)
def pruning_tree():
    return P.build(pruning_cloud())


@functools.lru_cache(maxsize=None)
def pruning_ref(k):
    """tree(...) of the 20 000-point self-query: computed once per process."""
    return tree(pruning_tree(), pruning_cloud(), k)


@functools.lru_cache(maxsize=None)
def normal_clouds():
    """{'plane': z = 0.002 noise over the unit square, 'sphere': the unit sphere}, 2 048 points each, default_rng(7)."""
    rng = np.random.default_rng(7)
    xy = rng.random((2048, 2))
    plane = np.concatenate([xy, 0.002 * rng.standard_normal((2048, 1))], axis=1)
    v = rng.standard_normal((2048, 3))
    return {"plane": plane, "sphere": v / np.linalg.norm(v, axis=1, keepdims=True)}


GAPS = {8: 0.0129, 16: 0.094, 32: 0.196}    # (lambda_1 - lambda_0) / lambda_2 at least, over both clouds (measured: 0.01296, 0.0941, 0.1962)


@functools.lru_cache(maxsize=None)
def outlier_cloud():
    """(points [2068,3], planted [20]): the plane cloud and 20 points at distance >= 0.5 from it."""
    rng = np.random.default_rng(20)
    plane = normal_clouds()["plane"]
    far = np.stack([rng.random(20), rng.random(20), np.where(rng.random(20) < 0.5, -1.0, 1.0) * (0.5 + rng.random(20))], axis=1)
    at = np.sort(rng.choice(len(plane) + 20, size=20, replace=False))
    pts = np.empty((len(plane) + 20, 3))
    keep = np.ones(len(pts), dtype=bool)
    keep[at] = False
    pts[keep], pts[at] = plane, far
    return pts, at
