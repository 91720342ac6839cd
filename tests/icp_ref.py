"""src/utils/icp.py of the reference restated twice in float64 numpy ("icp.hip"), the fixture's cases and the derived bound.

reference_order  the reference's arithmetic with a brute-force neighbour search in place of its kd-tree: np.mean, np.dot, np.linalg.svd,
                 np.linalg.det, the loop of icp.py:102-121 on homogeneous 4 x N points.  ``trace`` records per iteration the indices, the
                 neighbour margin (second-nearest minus nearest distance, the smallest over the points) and | |prev - mean| - tolerance |.
kernel_order     csrc/icp.hip's operations in its order: d2 = (dx dx + dy dy) + dz dz and the first among equal minima; chunks of 256
                 points summed by the tree s[t] = s[t] + s[t + h] (h = 128 ... 1, +0.0 past the end), the chunk sums added in chunk
                 order; the one-sided Jacobi SVD in scalar float64 operations, one rounding each (no np.dot); T p per row as
                 ((T0 x + T1 y) + T2 z) + T3.  The device's outputs equal these bit for bit.

Both expose fit(a, b) -> T, nn(src, dst) -> (d2, idx) and icp(A, B, init_pose, max_iterations, tolerance) -> (T, distances, i, idx).
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_icp.npz")

CHUNK = 256
SWEEPS = 10


# ---- the reference's order ---------------------------------------------------------------------------------------------------------------
class reference_order:
    @staticmethod
    def fit(A, B):
        A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        ca, cb = np.mean(A, axis=0), np.mean(B, axis=0)
        H = np.dot((A - ca).T, B - cb)
        U, S, Vt = np.linalg.svd(H)
        R = np.dot(Vt.T, U.T)
        if np.linalg.det(R) < 0:
            Vt[2, :] *= -1
            R = np.dot(Vt.T, U.T)
        t = cb.T - np.dot(R, ca.T)
        T = np.identity(4)
        T[:3, :3] = R
        T[:3, 3] = t
        return T

    @staticmethod
    def nn(src, dst, want_margin=False):
        src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
        d2 = ((src[:, None, :] - dst[None, :, :]) ** 2).sum(-1)
        idx = d2.argmin(1)
        near = d2[np.arange(len(src)), idx]
        if not want_margin:
            return near, idx
        if dst.shape[0] > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            margin = float((np.sqrt(two[:, 1]) - np.sqrt(two[:, 0])).min())
        else:
            margin = float("inf")
        return near, idx, margin

    @staticmethod
    def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001, trace=None):
        A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        src = np.ones((4, A.shape[0]))
        src[:3, :] = A.T
        if init_pose is not None:
            src = np.dot(init_pose, src)
        prev_error = 0
        for i in range(max_iterations):
            d2, idx, margin = reference_order.nn(src[:3, :].T, B, want_margin=True)
            distances = np.sqrt(d2)
            T = reference_order.fit(src[:3, :].T, B[idx])
            src = np.dot(T, src)
            mean_error = np.mean(distances)
            if trace is not None:
                trace.append((idx.copy(), margin, abs(abs(prev_error - mean_error) - tolerance)))
            if np.abs(prev_error - mean_error) < tolerance:
                break
            prev_error = mean_error
        return reference_order.fit(A, src[:3, :].T), distances, i, idx


# ---- the kernel's order ------------------------------------------------------------------------------------------------------------------
def _move(T, p):
    """T p per row: ((T0 x + T1 y) + T2 z) + T3."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def _two_stage_sum(v):
    """Column sums of v [N,K]: per chunk of 256 rows the tree, then the chunk sums in chunk order from +0.0."""
    N, K = v.shape
    chunks = (N + CHUNK - 1) // CHUNK
    s = np.zeros((chunks * CHUNK, K))
    s[:N] = v
    s = s.reshape(chunks, CHUNK, K)
    h = CHUNK // 2
    while h >= 1:
        s = s[:, :h] + s[:, h:2 * h]
        h //= 2
    acc = np.zeros(K)
    for c in range(chunks):
        acc = acc + s[c, 0]
    return acc


def _dot3(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def _rotation(H):
    """kabsch_rotation of icp.hip on Python floats (IEEE double, one rounding per operation)."""
    g = [[float(H[i][j]) for i in range(3)] for j in range(3)]          # columns
    v = [[1.0 if i == j else 0.0 for i in range(3)] for j in range(3)]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = _dot3(g[p], g[p]), _dot3(g[q], g[q]), _dot3(g[p], g[q])
            if gamma == 0.0:
                continue
            zeta = (beta - alpha) / (2.0 * gamma)
            zz = zeta * zeta
            t = 1.0 / (abs(zeta) + (math.sqrt(1.0 + zz) if zz != math.inf else math.inf))
            if zeta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for i in range(3):
                gp, gq, vp, vq = g[p][i], g[q][i], v[p][i], v[q][i]
                g[p][i], g[q][i] = c * gp - s * gq, s * gp + c * gq
                v[p][i], v[q][i] = c * vp - s * vq, s * vp + c * vq
    n2 = [_dot3(g[j], g[j]) for j in range(3)]
    for x, y in ((0, 1), (1, 2), (0, 1)):
        if n2[x] < n2[y]:
            n2[x], n2[y] = n2[y], n2[x]
            g[x], g[y] = g[y], g[x]
            v[x], v[y] = v[y], v[x]
    if not n2[0] > 0.0:
        return np.identity(3)
    u = [None, None, None]
    s0 = math.sqrt(n2[0])
    u[0] = [g[0][i] / s0 for i in range(3)]
    w = list(g[1])
    for _ in range(2):
        d = _dot3(u[0], w)
        w = [w[i] - u[0][i] * d for i in range(3)]
    wn2 = _dot3(w, w)
    if not wn2 > 0.0:
        k = 0
        if abs(u[0][1]) < abs(u[0][k]):
            k = 1
        if abs(u[0][2]) < abs(u[0][k]):
            k = 2
        w = [(1.0 if i == k else 0.0) - u[0][i] * u[0][k] for i in range(3)]
        wn2 = _dot3(w, w)
    wn = math.sqrt(wn2)
    u[1] = [w[i] / wn for i in range(3)]
    u[2] = [u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2], u[0][0] * u[1][1] - u[0][1] * u[1][0]]
    if _dot3(u[2], g[2]) < 0.0:
        u[2] = [-x for x in u[2]]
    R = np.zeros((3, 3))
    for _ in range(2):
        for r in range(3):
            for c in range(3):
                R[r, c] = (v[0][r] * u[0][c] + v[1][r] * u[1][c]) + v[2][r] * u[2][c]
        m = [[float(R[r, c]) for c in range(3)] for r in range(3)]
        det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) \
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0])
        if not det < 0.0:
            break
        v[2] = [-x for x in v[2]]
    return R


class kernel_order:
    @staticmethod
    def nn(src, dst, T=None):
        src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
        if T is not None:
            src = _move(np.asarray(T, dtype=np.float64), src)
        d = src[:, None, :] - dst[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx = d2.argmin(1)                                  # the first among equal minima
        return d2[np.arange(len(src)), idx], idx.astype(np.int32)

    @staticmethod
    def fit(a, b, idx=None, d2=None):
        """T; with d2 also the two-stage sum of sqrt(d2) / N."""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if idx is not None:
            b = b[idx]
        N = a.shape[0]
        cols = [a, b] if d2 is None else [a, b, np.sqrt(d2)[:, None]]
        sums = _two_stage_sum(np.concatenate(cols, axis=1))
        mean = sums[:6] / float(N)
        aa, bb = a - mean[:3], b - mean[3:6]
        H = _two_stage_sum(np.stack([aa[:, j] * bb[:, k] for j in range(3) for k in range(3)], axis=1)).reshape(3, 3)
        R = _rotation(H)
        T = np.identity(4)
        T[:3, :3] = R
        for r in range(3):
            T[r, 3] = mean[3 + r] - ((R[r, 0] * mean[0] + R[r, 1] * mean[1]) + R[r, 2] * mean[2])
        return T if d2 is None else (T, sums[6] / float(N))

    @staticmethod
    def icp(A, B, init_pose=None, max_iterations=20, tolerance=0.001):
        A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        work = A.copy() if init_pose is None else _move(np.asarray(init_pose, dtype=np.float64), A)
        prev_error = 0.0
        for i in range(max_iterations):
            d2, idx = kernel_order.nn(work, B)
            T, mean_error = kernel_order.fit(work, B, idx, d2)
            work = _move(T, work)
            if abs(prev_error - mean_error) < tolerance:
                break
            prev_error = mean_error
        return kernel_order.fit(A, work), np.sqrt(d2), i, idx


# ---- the fixture's cases (tests/golden/g28_icp.npz) ---------------------------------------------------------------------------------------
#        name     seed N     angle tr    noise  tolerance max_iterations
CASES = (("small", 1, 67, 0.15, 0.05, 0.002, 1e-3, 20),
         ("mid", 2, 300, 0.3, 0.1, 0.002, 1e-5, 20),
         ("tile", 3, 1025, 0.25, 0.08, 0.001, 1e-6, 30),
         ("cap", 4, 257, 0.5, 0.2, 0.0, 1e-9, 5))
LOOP_CASES = ("small", "mid", "tile", "cap", "pose")        # "pose": "mid" with init_pose
BATCH_CASES = ("batch0", "batch1", "batch2")
MIN_MARGIN = 1e-9                                           # every fixture case, every iteration: margin and tolerance gap at least this


def rodrigues(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_case(seed, N, angle, tr, noise):
    """(A, B) of the issue's recipe: draws in the order A, axis, translation, noise, permutation."""
    rng = np.random.default_rng(seed)
    A = rng.random((N, 3)) - 0.5
    R = rodrigues(rng.standard_normal(3), angle)
    B = (A @ R.T + tr * rng.standard_normal(3) + noise * rng.standard_normal((N, 3)))[rng.permutation(N)]
    return A, B


# ---- the derived bound --------------------------------------------------------------------------------------------------------------------
def fit_bound(a, b):
    """One fit's rotation error with identical correspondences: 2 |dH|_F / (sigma_2 + s sigma_3), s = sign det H,
    |dH|_F <= N 2^-53 sum |a_i - abar| |b_i - bbar|.  From the fixture's points alone."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    aa, bb = a - a.mean(0), b - b.mean(0)
    H = aa.T @ bb
    sig = np.linalg.svd(H, compute_uv=False)
    s = 1.0 if np.linalg.det(H) >= 0 else -1.0
    dH = a.shape[0] * 2.0 ** -53 * float((np.linalg.norm(aa, axis=1) * np.linalg.norm(bb, axis=1)).sum())
    return 2.0 * dH / (sig[1] + s * sig[2])


def loop_gates(A, B, idx_last, executed):
    """(gate on T, gate on the distances) of a loop that executed ``executed`` iterations: the fit bound of the final correspondences
    times (executed + 1) times 8, and that times (1 + max |p|) over both clouds."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    gate = fit_bound(A, B[idx_last]) * (executed + 1) * 8.0
    reach = max(float(np.linalg.norm(A, axis=1).max()), float(np.linalg.norm(B, axis=1).max()))
    return gate, gate * (1.0 + reach)


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
def ratio(tag, err, gate):
    line = f"RATIO {tag}: {err / gate:.3e} (gate {gate:.3e})"
    print(line)
    if os.environ.get("VTACO_RATIO_LOG"):
        with open(os.environ["VTACO_RATIO_LOG"], "a") as fh:
            fh.write(line + "\n")
    return err / gate


def case_of(z, name):
    pose = z[name + ".init_pose"] if name + ".init_pose" in z.files else None
    return z[name + ".A"], z[name + ".B"], pose, int(z[name + ".max_iterations"]), float(z[name + ".tolerance"])


def check_loop_against_fixture(z, name, tag, T, distances, i, idx):
    """The comparisons every candidate (numpy forms here, the device in tests/test_icp_gpu.py) goes through."""
    A, B = z[name + ".A"], z[name + ".B"]
    want_i, want_idx = int(z[name + ".i"]), z[name + ".idx"][-1].astype(np.int64)
    assert int(i) == want_i, (name, int(i), want_i)
    assert np.array_equal(np.asarray(idx).astype(np.int64), want_idx), name
    gate_T, gate_d = loop_gates(A, B, want_idx, want_i + 1)
    r_T = ratio(f"{tag} {name} T", float(np.abs(np.asarray(T) - z[name + ".T"]).max()), gate_T)
    r_d = ratio(f"{tag} {name} distances", float(np.abs(np.asarray(distances) - z[name + ".distances"]).max()), gate_d)
    assert r_T <= 1.0 and r_d <= 1.0, (name, r_T, r_d)
