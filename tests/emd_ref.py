"""csrc/metrics.hip's vt_emd_auction restated in numpy float32, the float64 certificate of an auction's result, and the inputs the
CPU and the GPU tests share.

auction_f32(a, b, eps_final, max_rounds, absolute_eps=False)
    The kernel's rule, operation for operation in f32: the problem padded with zero-cost dummies to n = max(N, M); cost
    sqrt((dx dx + dy dy) + dz dz); Jacobi rounds in which every unassigned person bids (price + gap) + eps for its best column (the
    smallest on ties; gap = second best value - best, 0 when n == 1) and the highest (bid, person) takes the column; prices shifted to
    a minimum of 0 and everybody unassigned at the start of a phase; epsilon from crange / 5 divided by 5 per phase down to
    eps_final * 2^floor(log2(crange)) (crange the f32 diagonal of the clouds' common bounding box; eps_final itself when it is 0).
    ``absolute_eps`` ends at eps_final itself whatever the scale: the rule before the scale rule, kept to keep its defect on record.
    Returns Auction(assign, prices, rounds, phases, eps_last), DID_NOT_FINISH after max_rounds rounds, or NON_FINITE.
    numpy's square root is correctly rounded and the kernel's is good to 1 ulp, so near-ties may resolve differently on the device:
    the two are compared through ``certificate`` and their round counts, never bit for bit.
certificate(a, b, assign, prices, emd, eps_last)
    The gate, in float64, independent of how the assignment was found (see there).
random / lattice / identical / coincident / offset
    The seeded case builders; each asserts on its inputs alone that the case is what its name says.
"""
import collections
import os

import numpy as np

Auction = collections.namedtuple("Auction", ["assign", "prices", "rounds", "phases", "eps_last"])
Certificate = collections.namedtuple("Certificate", ["opt", "bound", "excess", "R"])
DID_NOT_FINISH = "did not finish"
NON_FINITE = "non-finite"
EPS_FINAL = 1e-6              # ops.EMD_EPS_FINAL
THETA = np.float32(5.0)       # EMD_THETA
SCIPY_MAX = 1100              # the largest padded problem whose optimum scipy computes here; above it the dual bound stands in
CHUNK_BYTES = 64 << 20        # the largest float64 matrix alive at once in the certificate of a problem above SCIPY_MAX
F32 = np.float32
INF = F32(np.inf)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def cost_f32(a, b):
    """The padded n x n cost matrix as the kernel's scan evaluates it: f32 differences, (dx dx + dy dy) + dz dz, square root;
    dummy rows and dummy columns cost 0."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    N, M = len(a), len(b)
    n = max(N, M)
    c = np.zeros((n, n), dtype=F32)
    d = a[:, None, :] - b[None, :, :]
    c[:N, :M] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return c


def crange_f32(a, b):
    """The kernel's cost range: the f32 diagonal of the two clouds' common bounding box (x, y, z summed in that order)."""
    both = np.concatenate([np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)])
    ext = both.max(axis=0) - both.min(axis=0)
    diag2 = F32(0)
    for k in range(3):
        diag2 = F32(diag2 + ext[k] * ext[k])
    return F32(np.sqrt(diag2))


def eps_end_f32(crange, eps_final=EPS_FINAL, absolute_eps=False):
    """The last epsilon: eps_final * 2^floor(log2(crange)), exact in f32 (eps_final for crange == 0, or under the earlier absolute rule)."""
    if absolute_eps or not crange > 0:
        return F32(eps_final)
    return F32(np.ldexp(F32(eps_final), int(np.frexp(crange)[1]) - 1))


def auction_f32(a, b, eps_final=EPS_FINAL, max_rounds=500_000, absolute_eps=False):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return NON_FINITE
    with np.errstate(over="ignore"):
        crange = crange_f32(a, b)
    if not np.isfinite(crange):
        return NON_FINITE
    c = cost_f32(a, b)
    n = len(c)
    eps_end = eps_end_f32(crange, eps_final, absolute_eps)
    eps = max(F32(crange / THETA), eps_end)
    price = np.zeros(n, dtype=F32)
    rounds = phases = 0
    while True:
        price -= price.min()
        owner = np.full(n, -1, dtype=np.int64)
        asg = np.full(n, -1, dtype=np.int64)
        while True:
            un = np.flatnonzero(asg < 0)
            if len(un) == 0:
                break
            if rounds >= max_rounds:
                return DID_NOT_FINISH
            rounds += 1
            v = c[un] + price[None, :]                               # f32: one rounded sum per (bidder, column)
            rows = np.arange(len(un))
            i1 = v.argmin(axis=1)                                    # the smallest column among equal bests
            b1 = v[rows, i1]
            v[rows, i1] = INF
            b2 = v.min(axis=1)                                       # equal bests: the second best equals the best
            gap = np.where(b2 < INF, b2 - b1, F32(0)).astype(F32)
            bid = (price[i1] + gap) + eps
            assert bid.dtype == F32
            order = np.lexsort((un, bid))                            # ascending (bid, person): the last write per column is its highest
            win_p = np.full(n, -1, dtype=np.int64)
            win_b = np.zeros(n, dtype=F32)
            win_p[i1[order]] = un[order]
            win_b[i1[order]] = bid[order]
            js = np.flatnonzero(win_p >= 0)
            old = owner[js]
            asg[old[old >= 0]] = -1
            owner[js] = win_p[js]
            asg[win_p[js]] = js
            price[js] = win_b[js]
        phases += 1
        if eps <= eps_end:
            break
        eps = max(F32(eps / THETA), eps_end)
    return Auction(asg, price, rounds, phases, float(eps))


# ---- the certificate -----------------------------------------------------------------------------------------------------------
def cost_rows_f64(a, b, r0, r1):
    """Rows r0:r1 of the padded float64 cost matrix, as cdist evaluates it."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N, M = len(a), len(b)
    n = max(N, M)
    c = np.zeros((r1 - r0, n))
    top = min(r1, N)
    if top > r0:
        d = a[r0:top, None, :] - b[None, :, :]
        c[:top - r0, :M] = np.sqrt((d * d).sum(-1))
    return c


def emd_f64(a, b, assign):
    """The assignment's cost over its real pairs in float64 / N: what the kernel reports as emd."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N, M = len(a), len(b)
    j = np.asarray(assign)[:N]
    keep = j < M
    return float(np.sqrt(((a[keep] - b[j[keep]]) ** 2).sum(-1)).sum() / N)


def scipy_opt(a, b):
    """The optimum of the N x M problem (the padded one's too): the sum of the matched float64 distances."""
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    d = distance.cdist(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return float(d[linear_sum_assignment(d)].sum())


def certificate(a, b, assign, prices, emd, eps_last, use_scipy=None):
    """Asserts, in float64 and in this order, that (assign, prices, emd) is an eps_last-optimal answer to the padded problem:
      1. assign is a permutation of range(n), n = max(N, M);
      2. emd is the float64 cdist cost of the real pairs / N, to 1e-12 max(1, emd);
      3. eps-complementary slackness: c[i, assign[i]] + p[assign[i]] <= min_j (c[i, j] + p[j]) + eps_last + R for every i, c the
         float64 padded cost matrix, p the prices;
      4. optimality, which follows from 3: N emd <= opt + n (eps_last + R) and N emd >= opt (1 - 1e-9) (opt the total cost: scipy's
         for n <= SCIPY_MAX; above it the dual bound sum_i min_j (c[i, j] + p[j]) - sum_j p[j] <= opt, evaluated in row chunks).
    R = 8 * 2^-24 * (crange + max p) is the rounding allowance: the auction compares two f32 values, each one rounded sum of a price
    and a cost that carries at most three roundings (two in the sum of squares, one in the root): 4 u (crange + pmax) per value,
    u = 2^-24, crange the diagonal of the clouds' common bounding box (no cost is larger).  At unit scale (crange + pmax about 2.5)
    R is about 1.2e-6, so eps_last + R reproduces the 2 * eps of test_metrics_gpu.check_emd.
    Returns Certificate(opt, bound, excess, R): the optimum and "scipy" or "dual", the worst slackness excess / (eps_last + R)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N, M = len(a), len(b)
    n = max(N, M)
    assign = np.asarray(assign).astype(np.int64)
    p = np.asarray(prices).astype(np.float64)
    emd, eps_last = float(emd), float(eps_last)
    assert assign.shape == (n,) and p.shape == (n,)
    assert np.array_equal(np.sort(assign), np.arange(n)), "assign is not a permutation"
    assert np.isfinite(p).all() and eps_last > 0
    both = np.concatenate([a, b])
    crange = float(np.linalg.norm(both.max(axis=0) - both.min(axis=0)))
    R = 8.0 * 2.0 ** -24 * (crange + float(p.max()))
    tol = eps_last + R
    use_scipy = n <= SCIPY_MAX if use_scipy is None else use_scipy
    rows = max(1, CHUNK_BYTES // (8 * n) // 2)                       # the cost rows and the values: two matrices per chunk
    total, dual, excess = 0.0, -float(p.sum()), -np.inf
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        c = cost_rows_f64(a, b, r0, r1)
        mine = c[np.arange(r1 - r0), assign[r0:r1]]
        total += float(mine.sum())                                   # dummy rows and dummy columns add 0
        value = c + p[None, :]
        best = value.min(axis=1)
        dual += float(best.sum())
        excess = max(excess, float((mine + p[assign[r0:r1]] - best).max()))
    assert abs(emd - total / N) <= 1e-12 * max(1.0, emd), ("emd is not the assignment's float64 cost", emd, total / N)
    assert excess <= tol, ("eps-complementary slackness", excess, tol, excess / tol)
    opt, bound = (scipy_opt(a, b), "scipy") if use_scipy else (dual, "dual")
    assert N * emd <= opt + n * tol, ("optimality: above the optimum", N * emd, opt, n * tol)
    assert N * emd >= opt - 1e-9 * max(1.0, opt), ("optimality: below the optimum", N * emd, opt)
    return Certificate(opt / N, bound, excess / tol, R)


def record(tag, line):
    """One line of profiles/emd_f64_ratios.txt: printed, and appended to the file VTACO_RATIO_LOG names."""
    line = f"RATIO emd {tag}: {line}"
    print(line)
    if os.environ.get("VTACO_RATIO_LOG"):
        with open(os.environ["VTACO_RATIO_LOG"], "a") as fh:
            fh.write(line + "\n")


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _rng(name, n, m):
    return np.random.RandomState([{"random": 11, "lattice": 12, "identical": 13, "coincident": 14, "offset": 15}[name], n, m])


def _distinct(p):
    return len(np.unique(p, axis=0)) == len(p)


def random(n, m):
    """Two Gaussian clouds (sigma 0.2, the second 0.05 off the first): no two points equal."""
    rng = _rng("random", n, m)
    a = (rng.randn(n, 3) * 0.2).astype(F32)
    b = (rng.randn(m, 3) * 0.2 + 0.05).astype(F32)
    assert _distinct(np.concatenate([a, b]))
    return a, b


def lattice(n, m):
    """Gaussian points rounded to eighths, each side drawn from max(1, size // 2) such points so that every point of a side of two or
    more has a twin (in shuffled order); one point against one point is the same point.  Exact ties: at least a quarter of the points
    duplicate another, and every row of the float64 cost matrix with two or more entries has a repeated entry."""
    rng = _rng("lattice", n, m)

    def side(k):
        base = np.round(rng.randn(max(1, k // 2), 3) * 0.2 * 8) / 8
        return base[rng.permutation(k) % len(base)].astype(F32)
    a, b = side(n), side(m)
    if n == 1 and m == 1:
        b = a.copy()
    both = np.concatenate([a, b])
    assert np.array_equal(both * 8, np.round(both * 8))
    _, inverse, counts = np.unique(both, axis=0, return_inverse=True, return_counts=True)
    assert (counts[inverse.ravel()] > 1).sum() * 4 >= len(both)
    if m >= 2:
        c = np.sort(cost_rows_f64(a, b, 0, n)[:, :m], axis=1)
        assert ((np.diff(c, axis=1) == 0).any(axis=1)).all()
    return a, b


def identical(n):
    """b is a: the optimum is the identity at cost 0, and every person has a column at cost exactly 0."""
    a, _ = random(n, 1)
    return a, a.copy()


def coincident(n):
    """Every point of both clouds is one point: cost range 0, every value ties, one phase."""
    p = (_rng("coincident", n, n).randn(1, 3) * 0.2).astype(F32)
    a = np.repeat(p, n, axis=0)
    assert crange_f32(a, a) == 0
    return a, a.copy()


def offset(n):
    """Clouds of extent 0.3 at an offset of 100 on every axis: coordinates whose f32 spacing (7.6e-6) is far coarser than the
    epsilon, while the cost range stays below 1."""
    rng = _rng("offset", n, n)
    a = (rng.uniform(0, 0.3, (n, 3)) + 100).astype(F32)
    b = (rng.uniform(0, 0.3, (n, 3)) + 100).astype(F32)
    both = np.concatenate([a, b])
    assert both.min() >= 100 and both.max() <= 100.3001 and crange_f32(a, b) < 1
    return a, b


BUILDERS = {"random": random, "lattice": lattice, "identical": identical, "coincident": coincident, "offset": offset}


def case(name, n, m=None):
    return BUILDERS[name](n, m) if name in ("random", "lattice") else BUILDERS[name](n)
