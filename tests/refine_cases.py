"""Seeded meshes and weights of the refinement tests (CPU only): small enough to run in seconds, shaped so that the kernels can go wrong.

  tetra     a tetrahedron, F = 4
  fan       200 faces around one vertex: every face collides on that vertex' accumulator
  mc        marching cubes (the oracle's) of a small seeded smooth field: a few hundred faces, F not a multiple of 64
  degen     a patch with one zero-area face (two equal corners) and one vertex no face uses

All lie inside the unit box scaled to +-0.4, so no face point is clamped."""
import numpy as np
import torch


def _tetra():
    v = np.array([[0.3, 0.3, 0.3], [-0.3, -0.3, 0.3], [-0.3, 0.3, -0.3], [0.3, -0.3, -0.3]], np.float32) * 0.8
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def _fan(n=200, seed=5):
    rng = np.random.RandomState(seed)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rim = np.stack([0.35 * np.cos(ang), 0.35 * np.sin(ang), 0.05 * rng.randn(n)], 1)
    v = np.concatenate([[[0.01, -0.02, 0.2]], rim]).astype(np.float32)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1).astype(np.int32)
    return v, f


def _mc(n=12, seed=11):
    from oracle import mc
    rng = np.random.RandomState(seed)
    lin = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(lin, lin, lin, indexing="ij")
    vol = (0.55 - np.sqrt(x * x + 1.3 * y * y + 0.8 * z * z) + 0.08 * np.sin(3 * x + rng.rand()) * np.cos(2 * y + rng.rand())).astype(np.float32)
    out = mc.marching_cubes(vol, 0.0)
    v, f = np.asarray(out[0], np.float32), np.asarray(out[1], np.int32)
    v = ((v / (n - 1)) - 0.5) * 0.8
    return v.astype(np.float32), f


def _degen(seed=3):
    rng = np.random.RandomState(seed)
    v = (rng.rand(9, 3).astype(np.float32) - 0.5) * 0.7
    v[4] = v[3]                                                    # face (2, 3, 4) has two equal corners: zero area
    f = np.array([[0, 1, 2], [2, 3, 4], [2, 4, 5], [5, 6, 0], [6, 7, 1], [0, 2, 5]], np.int32)      # vertex 8 is used by no face
    return v, f


def meshes():
    out = {}
    for name, (v, f) in (("tetra", _tetra()), ("fan", _fan()), ("mc", _mc()), ("degen", _degen())):
        out[name] = (torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(f)))
    return out


def eps_for(F, seed=0):
    """float32 [F,3] Dirichlet(1/2,1/2,1/2) weights from a seeded generator of the test's own."""
    return torch.from_numpy(np.random.RandomState(1000 + seed).dirichlet((0.5, 0.5, 0.5), size=F).astype(np.float32))
