"""Seeded inputs of the decoder training-path tests (CPU only): weight sets, the mixed point sets and a float32 numpy restatement
of the kernels' point normalisation, with which tests/test_decode_train_ref_cpu.py checks that the point sets hold what they claim."""
import numpy as np
import torch

from conftest import load_golden
from decode_train_ref import divisor

TOTALS = [(1, 1), (1, 31), (3, 11), (1, 1023), (5, 205), (3, 427), (1, 2303)]
RS = (2, 3, 5, 8)
F32 = np.float32


# ---- the kernels' normalisation in float32 (decode_common.h grid_coord, voxel.hip voxel_coord) --------------------------------
def norm32(v, padding=0.1):
    q = np.asarray(v, F32) / F32(divisor(padding)) + F32(0.5)
    q = np.where(q >= F32(1), F32(0.999), q).astype(F32)
    return np.where(q < F32(0), F32(0), q).astype(F32)


def raw_norm32(v, padding=0.1):
    return (np.asarray(v, F32) / F32(divisor(padding)) + F32(0.5)).astype(F32)


def grid_coord32(v, R, padding=0.1):
    g = F32(2) * norm32(v, padding) - F32(1)
    f = (((g + F32(1)) / F32(2)) * F32(R - 1)).astype(F32)
    return np.minimum(np.maximum(f, F32(0)), F32(R - 1)).astype(F32)


def voxel_bin32(v, reso, padding=0.1):
    return (norm32(v, padding) * F32(reso)).astype(F32).astype(np.int64)          # truncating cast of a non-negative value


# ---- weights -------------------------------------------------------------------------------------------------------------------
def weight_sets():
    """{"g1": the golden decoder's state dict, "half": a seeded one whose pre-activations are negative about half of the time}."""
    _, g1 = load_golden("g1_decode.npz")
    gen = torch.Generator().manual_seed(1234)
    half = {}
    for k, v in g1.items():
        if k.endswith(".weight"):
            gain = 0.45 if (".fc_1." in k or k.startswith("fc_c.")) else 1.0          # keeps the residual stream from growing block by block
            half[k] = torch.randn(v.shape, generator=gen) * (gain / float(v.shape[1]) ** 0.5)
        else:
            half[k] = 0.05 * torch.randn(v.shape, generator=gen)
    return {"g1": g1, "half": half}


# ---- points ------------------------------------------------------------------------------------------------------------------
def node_values(R, padding=0.1):
    """Per grid node k, a float32 coordinate whose float32 grid coordinate is exactly k (searched among the neighbours of the
    real-valued preimage); nodes without one are left out."""
    out = []
    d = divisor(padding)
    for k in range(R):
        v0 = F32((k / (R - 1) - 0.5) * d)
        cand = [v0]
        lo = hi = v0
        for _ in range(64):
            lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(1))
            cand += [lo, hi]
        hit = [v for v in cand if -0.5 * d <= float(v) < 0.5 * d and float(grid_coord32(v, R, padding)) == float(k)]
        if hit:
            out.append(hit[0])
    return np.array(out, F32)


def cluster_cell(R):
    return (min(2, R - 2), min(4, R - 2), min(1, R - 2))


def special_points(R, seed, padding=0.1):
    """The point families of the issue as a dict of float32 arrays [n,3]."""
    rng = np.random.RandomState(seed)
    d = divisor(padding)
    fam = {}
    cell = np.array(cluster_cell(R), np.float64)
    fam["cluster"] = (((cell + 0.1 + 0.8 * rng.rand(200, 3)) / (R - 1) - 0.5) * d).astype(F32)
    fam["dup"] = np.repeat(((rng.rand(8, 3) - 0.5) * 1.24).astype(F32), 8, axis=0)
    nv = node_values(R, padding)
    fam["node"] = nv[rng.randint(0, len(nv), size=(40, 3))]
    beyond = ((rng.rand(36, 3) - 0.5) * 1.0).astype(F32)
    for j in range(36):                                            # one axis pushed out, low and high sides in turn, by up to 0.2
        sign = -1.0 if (j // 3) % 2 == 0 else 1.0
        beyond[j, j % 3] = F32(sign * (0.5 * d + 1e-3 + 0.2 * rng.rand()))
    fam["beyond"] = beyond
    half = F32(0.5) * F32(d)
    edge = ((rng.rand(6, 3) - 0.5) * 1.0).astype(F32)
    for j in range(6):
        edge[j, j % 3] = half if j < 3 else -half
    edge = np.concatenate([edge, np.array([[half, half, half], [-half, -half, -half], [half, -half, half]], F32)])
    fam["edge"] = edge
    return fam


FAMILIES = ("cluster", "dup", "node", "beyond", "edge", "uniform")


def make_points(B, N, R, seed=0, padding=0.1):
    """float32 [B,N,3]: with B * N >= 600 every family whole (the cluster and the duplicates inside scene 0 when N allows) and
    uniform points over +-0.62 for the rest, shuffled within each scene; smaller totals take the families in turn."""
    rng = np.random.RandomState(1000 * R + 7 * B + N + seed)
    fam = special_points(R, seed + R, padding)
    total = B * N
    if total >= 600:
        rest = np.concatenate([fam[k] for k in FAMILIES[1:-1]])
        scenes = [[] for _ in range(B)]
        scenes[0].append(fam["cluster"])
        scenes[0 if N >= len(fam["cluster"]) + len(rest) else 1].append(rest)          # a family is never split between scenes
        pts = np.empty((B, N, 3), F32)
        for b in range(B):
            have = np.concatenate(scenes[b]) if scenes[b] else np.empty((0, 3), F32)
            uni = ((rng.rand(N - len(have), 3) - 0.5) * 1.24).astype(F32)
            pts[b] = np.concatenate([have, uni])[rng.permutation(N)]
        return torch.from_numpy(pts)
    rows = []
    for i in range(total):
        k = FAMILIES[i % len(FAMILIES)]
        rows.append(((rng.rand(3) - 0.5) * 1.24).astype(F32) if k == "uniform" else fam[k][(i // len(FAMILIES)) % len(fam[k])])
    return torch.from_numpy(np.stack(rows).reshape(B, N, 3))


def make_inputs(B, N, R, C=32, seed=0):
    """Everything a case needs besides the weights: pts, grid [B,C,R,R,R], c_img, grad_out (every 7th row 0), grad_out2."""
    g = torch.Generator().manual_seed(100003 * R + 101 * B + N + seed)
    pts = make_points(B, N, R, seed)
    grid = torch.randn(B, C, R, R, R, generator=g)
    c_img = torch.randn(B, N, C, generator=g)
    go = torch.randn(B, N, generator=g)
    go.view(-1)[::7] = 0.0
    go2 = torch.randn(B, N, generator=g)
    go2.view(-1)[3::11] = 0.0
    return {"pts": pts, "grid": grid, "c_img": c_img, "grad_out": go, "grad_out2": go2}


def lattice_points(nx, box=1.1):
    """The query lattice as the kernels generate it (decode_common.h lattice_point): box * linspace(-0.5, 0.5, nx)[i] per axis with one
    rounding per element (a fused multiply-add), axis 0 slowest.  float32 [nx^3, 3]."""
    step = F32(1.0) / F32(nx - 1)
    half = nx // 2
    lin = np.empty(nx, F32)
    for i in range(nx):
        v = float(step) * i - 0.5 if i < half else -float(step) * (nx - i - 1) + 0.5          # exact in float64: one rounding below
        lin[i] = F32(box) * F32(v)
    gx, gy, gz = np.meshgrid(lin, lin, lin, indexing="ij")
    return np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], 1)
