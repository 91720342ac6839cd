"""csrc/point_tree.hip restated in float64 numpy ("point_tree.hip"): the octree over a point set and the nearest-neighbour
walk, this file's operations in the kernel's order, and the inputs the CPU and the GPU tests share.

default_depth(M)   the smallest L in 1..7 with 8^L * 8 >= M
build(dst, depth)  frame (lo = the minimum corner, side = the largest extent or 1), the Morton cell of every point, one dense int32 pyramid
                   per level (rank among the occupied cells, or -1), the list offsets, the lists (ascending index inside a leaf), the
                   points in list order and one tight box lo[3], hi[3] per occupied cell (+0.0 added: a zero is stored as +0.0)
query(...)         every query walks the tree as one lane of the kernel does: the state is (level, cell), "next" is cell + 1 climbing
                   while cell % 8 == 0, "descend" is (level + 1, 8 cell).  e_a = lo_a - q_a if q_a < lo_a, q_a - hi_a if q_a > hi_a,
                   else 0; lb = (e_x e_x + e_y e_y) + e_z e_z; a cell is skipped exactly when lb > best.  A leaf's points are taken in
                   list order on d2 < best or (d2 == best and index < best index).  seed: the query's own clamped leaf, when occupied,
                   is evaluated first and passed over by the walk; order: children are visited as k ^ o, o the octant of the query
                   about the cell's centre.  All queries advance in lock step (numpy over the live ones); no query reads another's state.
Returns (d2 f64 [N], idx i32 [N], stats i32 [N,2]: boxes tested, points tested).
"""
import numpy as np

import icp_ref as R

MAX_DEPTH = 7
SIZES = (1, 63, 64, 65, 257, 1025)                      # tests/test_icp_gpu.py's
WALKS = {"plain": (False, False), "seed": (True, False), "order": (False, True), "seed+order": (True, True)}


def default_depth(M):
    L = 1
    while L < MAX_DEPTH and 8 ** L * 8 < M:
        L += 1
    return L


def _spread(x):
    r = np.zeros_like(x)
    for k in range(MAX_DEPTH):
        r |= ((x >> k) & 1) << (3 * k)
    return r


def _gather(m):
    r = np.zeros_like(m)
    for k in range(MAX_DEPTH):
        r |= ((m >> (3 * k)) & 1) << k
    return r


def cell_codes(p, lo, side, L):
    """The Morton number of the leaf of every point: per axis clamp((int)floor((p - lo) / side * n), 0, n - 1); a NaN becomes 0."""
    n = 1 << L
    code = np.zeros(len(p), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            g = np.floor((p[:, a] - lo[a]) / side * float(n))
            g = np.where(g > 0.0, g, 0.0)
            g = np.where(g < float(n - 1), g, float(n - 1))
            code |= _spread(g.astype(np.int64)) << a
    return code


def build(dst, depth=None):
    dst = np.ascontiguousarray(dst, dtype=np.float64)
    M = dst.shape[0]
    L = default_depth(M) if depth is None else int(depth)
    lo = dst.min(0) + 0.0
    ext = 0.0
    for a in range(3):
        e = float(dst[:, a].max() - lo[a])
        ext = e if e > ext else ext
    side = ext if ext > 0.0 else 1.0
    codes = cell_codes(dst, lo, side, L)
    cnt = np.bincount(codes, minlength=8 ** L)
    pyramids = [None] * (L + 1)
    occ = cnt > 0
    for l in range(L, -1, -1):
        if l < L:
            occ = (pyramids[l + 1].reshape(-1, 8) >= 0).any(1)
        rank = np.cumsum(occ) - occ
        pyramids[l] = np.where(occ, rank, -1).astype(np.int32)
    doff = np.cumsum(cnt) - cnt
    leaves = int((cnt > 0).sum())
    offsets = np.concatenate([doff[cnt > 0], [M]]).astype(np.int32)
    lists = np.argsort(codes, kind="stable").astype(np.int32)
    points = np.ascontiguousarray(dst[lists])
    boxes = [None] * (L + 1)
    boxes[L] = np.concatenate([np.minimum.reduceat(points, offsets[:-1]), np.maximum.reduceat(points, offsets[:-1])], axis=1) + 0.0
    for l in range(L - 1, -1, -1):
        child = pyramids[l + 1].reshape(-1, 8)                           # per cell its children's ranks; an empty child adds +-inf
        cb = np.concatenate([boxes[l + 1], [[np.inf] * 3 + [-np.inf] * 3]])[child]
        full = np.concatenate([cb[:, :, :3].min(1), cb[:, :, 3:].max(1)], axis=1)
        boxes[l] = np.ascontiguousarray(full[pyramids[l] >= 0])
    assert len(offsets) == leaves + 1
    return {"depth": L, "M": M, "lo": lo, "side": side, "pyramids": pyramids, "offsets": offsets, "lists": lists, "points": points,
            "boxes": boxes, "counts": [len(b) for b in boxes]}


def query(tree, src, T=None, seed=True, order=True):
    q = np.ascontiguousarray(src, dtype=np.float64)
    if T is not None:
        q = R._move(np.asarray(T, dtype=np.float64), q)
    N, L = q.shape[0], tree["depth"]
    lo, side = tree["lo"], tree["side"]
    pyr = np.concatenate(tree["pyramids"]).astype(np.int64)
    boxes = np.concatenate(tree["boxes"])
    base = np.concatenate([[0], np.cumsum(tree["counts"])]).astype(np.int64)
    loff, lists, points = tree["offsets"].astype(np.int64), tree["lists"], tree["points"]
    best = np.full(N, np.inf)
    bidx = np.full(N, -1, dtype=np.int32)
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
            upd = (d2 < best[i]) | ((d2 == best[i]) & (li < bidx[i]))
            best[i[upd]] = d2[upd]
            bidx[i[upd]] = li[upd]

    with np.errstate(invalid="ignore", over="ignore"):
        seed_rk = np.full(N, -1, dtype=np.int64)
        if seed:
            seed_rk = pyr[(8 ** L - 1) // 7 + cell_codes(q, lo, side, L)]
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
            go = occ & ~(lb > best[ids])
            descend = go & (lv < L)
            at_leaf = go & (lv == L) & (rk != seed_rk[ids])
            leaf(ids[at_leaf], rk[at_leaf])
            o = np.zeros(len(ids), dtype=np.int64)
            if order:
                h = side * (1.0 / (1 << lv).astype(np.float64))
                for a in range(3):
                    centre = lo[a] + (_gather(actual >> a).astype(np.float64) + 0.5) * h
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


def brute(src, dst, T=None):
    """icp_ref.kernel_order.nn, with vt_nn_points' answer for a query no target is strictly below +inf of (a NaN or an infinite
    coordinate: every d2 is NaN or +inf, the strict < never fires): (+inf, -1)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d2, idx = R.kernel_order.nn(src, dst, T)
    none = ~(d2 < np.inf)
    return np.where(none, np.inf, d2), np.where(none, -1, idx).astype(np.int32)


# ---- the inputs the CPU and the GPU tests share ----------------------------------------------------------------------------------------
def clouds():
    """tests/test_icp_gpu.py's seeded clouds: one per size and role."""
    rng = np.random.default_rng(28)
    return {(role, n): rng.random((n, 3)) - 0.5 for role in ("src", "dst") for n in SIZES + (2, 255, 256, 600)}


def pose_of(seed, angle=0.3, shift=0.1):
    rng = np.random.default_rng(seed)
    T = np.identity(4)
    T[:3, :3] = R.rodrigues(rng.standard_normal(3), angle)
    T[:3, 3] = shift * rng.standard_normal(3)
    return T


def lattice(n=9):
    g = (np.arange(n) / float(n - 1)) - 0.5
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def special_cases():
    """name -> (src, dst, depth or None): the degenerate target sets and the queries of the issue."""
    rng = np.random.default_rng(2810)
    c = clouds()
    src = c[("src", 257)]
    out = {}
    out["sparse_deep"] = (src, c[("dst", 65)], 7)
    out["single"] = (src, c[("dst", 1)], None)
    out["all_equal"] = (src, np.tile(np.array([[0.25, -0.125, 0.5]]), (257, 1)), None)
    t = rng.random(300) - 0.5
    out["collinear"] = (src, np.stack([t, 0.5 * t + 0.1, -0.25 * t], axis=1), 3)
    uv = rng.random((300, 2)) - 0.5
    out["coplanar"] = (src, np.stack([uv[:, 0], uv[:, 1], np.full(300, 0.125)], axis=1), 3)
    faces = rng.integers(0, 9, size=(400, 3)) / 8.0 - 0.5             # every coordinate on a cell face of the depth-3 frame
    faces[0], faces[1] = -0.5, 0.5
    out["cell_faces"] = (np.concatenate([src, faces[:64]]), faces, 3)
    dst = c[("dst", 600)]
    out["duplicates"] = (src, np.concatenate([dst[::-1], dst, dst[:100]]), None)
    lat = lattice(9)
    twice = np.concatenate([lat, lat])
    centres = lat[(lat < 0.5).all(1)] + 1.0 / 16.0
    out["lattice_twice"] = (np.concatenate([lat, centres]), twice, None)
    out["far_outside"] = (np.concatenate([src * 0.05 + np.array([3.0, 0.0, 0.0]), src * 100.0, src - 7.0]), c[("dst", 1025)], None)
    out["on_targets"] = (c[("dst", 1025)][::3].copy(), c[("dst", 1025)], None)
    bad = src[:64].copy()
    bad[0, 0] = np.nan
    bad[1] = np.nan
    bad[2, 1] = np.inf
    bad[3, 2] = -np.inf
    bad[4] = (np.inf, -np.inf, np.inf)
    bad[5] = (np.nan, np.inf, 0.0)
    out["nonfinite_queries"] = (bad, c[("dst", 257)], None)
    return out


def batch_of_three():
    """(src [3,257,3], dst [3,600,3], T [3,4,4]): three clouds with three frames and three occupancies."""
    c = clouds()
    src = np.stack([c[("src", 257)], c[("dst", 257)], 2.0 * c[("src", 257)][::-1]])
    dst = np.stack([c[("dst", 600)], c[("src", 600)], c[("dst", 600)] * np.array([1.0, 0.5, 0.25])])
    return src, dst, np.stack([pose_of(1), pose_of(2), pose_of(3)])


def chamfer_clouds():
    """float32 [2,300,3] and [2,257,3]."""
    rng = np.random.default_rng(94)
    return (rng.random((2, 300, 3)) - 0.5).astype(np.float32), (rng.random((2, 257, 3)) - 0.4).astype(np.float32)


def chamfer_clouds_2048():
    rng = np.random.default_rng(2048)
    return (rng.random((2, 2048, 3)) - 0.5).astype(np.float32), (rng.random((2, 2048, 3)) - 0.5).astype(np.float32)


def pruning_case(M):
    """Uniform targets in [-0.5, 0.5)^3, 257 queries inside and 257 near (3, 0, 0)."""
    rng = np.random.default_rng(1000 + M)
    dst = rng.random((M, 3)) - 0.5
    inside = rng.random((257, 3)) - 0.5
    far = 0.1 * (rng.random((257, 3)) - 0.5) + np.array([3.0, 0.0, 0.0])
    return inside, far, dst
