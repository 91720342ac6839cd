"""GPU: vt_closest_point_mesh / _scenes through ``ops.metrics`` against tests/closest_point_ref.py's by_regions, the float64 numpy restatement
of the kernel in the kernel's operation order.

d2, face and closest are compared for EQUAL BITS, no element left out: the kernel's arithmetic is separate IEEE float64 products, sums and
two divisions (the tree is built without contraction), which numpy rounds the same way.  tests/test_closest_point_ref_cpu.py ties
by_regions to an independent form."""
import ctypes

import numpy as np
import pytest
import torch

import closest_point_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(verts, faces, pts, want_point=True):
    from vtaco_amd import ops
    out = ops.metrics.closest_point_mesh(torch.from_numpy(np.asarray(verts)).to(DEV), torch.from_numpy(np.asarray(faces)).to(DEV),
                                         torch.from_numpy(np.asarray(pts)).to(DEV), want_point=want_point)
    return out.d2.cpu().numpy(), out.face.cpu().numpy(), None if out.closest is None else out.closest.cpu().numpy()


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def _check(verts, faces, pts):
    d2, face, q = _run(verts, faces, pts)
    w_d2, w_face, w_q = R.by_regions(verts, faces, pts)
    assert np.isfinite(d2).all() and np.isfinite(q).all()
    assert np.array_equal(face, w_face)
    assert _same_bits(d2, w_d2), float(np.abs(d2 - w_d2).max())
    assert _same_bits(q, w_q), float(np.abs(q - w_q).max())
    return d2, face, q


@pytest.fixture(scope="module")
def meshes():
    """One soup per face count of the grid (shared vertices: ties between neighbouring faces), and the queries of every N."""
    return {F: R.soup(F, 100 + F) for F in (1, 63, 64, 65, 600, 1000)}


@pytest.mark.parametrize("N", [1, 63, 65, 778])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 1000])
def test_grid_of_sizes_equals_the_restatement(meshes, F, N):
    verts, faces = meshes[F]
    _check(verts, faces, R.queries(N, 1000 * F + N, verts, faces))


def test_faces_across_slabs_and_chunks(meshes):
    """600 faces: two slabs of two 256-record chunks (the second slab's last chunk partly filled); 1000 of the grid above: two full slabs."""
    from vtaco_amd import ops
    assert ops.metrics.closest_point_slab_faces(600, 65) == 512 and ops.metrics.closest_point_slab_faces(1000, 778) == 512
    verts, faces = meshes[600]
    pts = R.queries(65, 9, verts, faces)
    _, face, _ = _check(verts, faces, pts)
    assert (face < 512).any() and (face >= 512).any()                      # winners in both slabs


def test_voronoi_regions_of_one_triangle():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.25, 2],
                    [1, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]], dtype=np.float32)        # a, b, c, ab, ac, bc, inside; on a vertex, an edge, inside
    d2, face, q = _check(verts, faces, pts)
    assert np.array_equal(d2, np.array([2.25, 1.25, 1.25, 1, 1, 0.5, 4, 0, 0, 0]))
    assert (face == 0).all()
    assert np.array_equal(q[7:], pts[7:].astype(np.float64))


def test_equal_minima_give_the_lowest_face():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0], [0.5, 0, 1]], dtype=np.float32)
    pts = np.array([[0.5, 0, 0.25], [0.25, 0, 0], [0, 0, 0], [0.5, 0.0, -2]], dtype=np.float32)       # nearest the edge the faces share
    for faces in ([[0, 1, 2], [1, 0, 3], [0, 1, 4]], [[1, 0, 3], [0, 1, 4], [0, 1, 2]]):
        faces = np.array(faces, dtype=np.int32)
        d2, face, _ = _check(verts, faces, pts)
        assert np.array_equal(d2[[1, 2, 3]], [0, 0, 4]) and (face[[1, 2, 3]] == 0).all()
    # the same face 700 times, across a slab boundary: face 0 wins every query
    many = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (700, 1))
    _, face, _ = _check(verts, many, pts)
    assert (face == 0).all()


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("kind", ["repeated", "collinear"])
def test_degenerate_faces(kind, mixed):
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
    _check(verts, faces, pts)


def test_two_runs_give_equal_bits(meshes):
    verts, faces = meshes[1000]
    pts = R.queries(778, 5, verts, faces)
    first, second = _run(verts, faces, pts), _run(verts, faces, pts)
    for a, b in zip(first, second):
        assert _same_bits(a, b)
    d2, face, q = _run(verts, faces, pts, want_point=False)
    assert q is None and _same_bits(d2, first[0]) and _same_bits(face, first[1])
    i64 = _run(verts, faces.astype(np.int64), pts)
    assert _same_bits(i64[0], first[0]) and _same_bits(i64[2], first[2])


def test_scenes_equal_their_single_calls(meshes):
    from vtaco_amd import ops
    cases = [meshes[65], R.torus(24, 12, seed=2), meshes[600]]             # V / F = 35 / 65, 288 / 576, 303 / 600
    N = 130
    pts = np.stack([R.queries(N, 20 + b, *cases[b]) for b in range(3)])
    dev = [(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)) for v, f in cases]
    out = ops.metrics.closest_point_mesh_scenes(dev, torch.from_numpy(pts).to(DEV))
    assert tuple(out.d2.shape) == (3, N) and tuple(out.closest.shape) == (3, N, 3)
    for b in range(3):
        d2, face, q = _run(*cases[b], pts[b])
        assert _same_bits(out.d2[b].cpu().numpy(), d2) and _same_bits(out.face[b].cpu().numpy(), face) and _same_bits(out.closest[b].cpu().numpy(), q)
    w = R.by_regions(*cases[1], pts[1])
    assert _same_bits(out.d2[1].cpu().numpy(), w[0]) and np.array_equal(out.face[1].cpu().numpy(), w[1])


def test_bad_arguments():
    from vtaco_amd import _lib, ops
    from vtaco_amd._lib import VtError
    lib = _lib.load()
    verts = torch.zeros((3, 3), device=DEV)
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    pts = torch.zeros((4, 3), device=DEV)
    d2 = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    face = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros((4096,), dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(V, F, ws_bytes=ws.numel() * 4):
        return lib.vt_closest_point_mesh(P(verts), V, P(faces), F, P(pts), 4, P(d2), P(face), None, P(ws), ws_bytes, None)
    assert lib.vt_closest_point_mesh_workspace_bytes(0, 4) == 0 and 0 < lib.vt_closest_point_mesh_workspace_bytes(1, 4) <= ws.numel() * 4
    assert call(3, 0) == -1 and call(0, 1) == -1                            # VT_ERR_INVALID: no faces, no vertices
    assert call(3, 1, 16) == -3                                            # VT_ERR_WORKSPACE
    assert lib.vt_closest_point_mesh_scenes(None, 1, 1, P(pts), 4, P(d2), P(face), None, P(ws), ws.numel() * 4, None) == -1
    torch.cuda.synchronize()
    assert (d2 == 7.0).all() and (face == 7).all()                         # nothing was launched
    assert call(3, 1) == 0
    torch.cuda.synchronize()
    assert (d2 == 0.0).all() and (face == 0).all() and int(ws[0]) == 0
    for what, (v, f) in {"no faces": (verts, faces[:0]), "no vertices": (verts[:0], faces)}.items():
        with pytest.raises(VtError):
            ops.metrics.closest_point_mesh(v, f, pts)
    for bad in ([[0, 1, 3]], [[0, -1, 2]], [[0, 1, 2], [2 ** 31 - 1, 0, 1]]):                    # found by the prepare pass, never read
        with pytest.raises(VtError, match="face index"):
            ops.metrics.closest_point_mesh(verts, torch.tensor(bad, dtype=torch.int32, device=DEV), pts)
        with pytest.raises(VtError, match="face index"):
            ops.metrics.closest_point_mesh_scenes([(verts, faces), (verts, torch.tensor(bad, dtype=torch.int32, device=DEV))], torch.zeros((2, 4, 3), device=DEV))
    with pytest.raises(VtError):
        ops.metrics.closest_point_mesh(verts.cpu(), faces.cpu(), pts.cpu())
    with pytest.raises(VtError):
        ops.metrics.closest_point_mesh(verts.double(), faces, pts)
