"""CPU: the two float64 restatements of vt_closest_point_mesh (tests/closest_point_ref.py) agree.

by_regions (the kernel's algorithm, in its operation order) and by_parts (plane projection or the nearest of three segments) must give the
same per-query minimum d2 within 64 float64 roundings of the squared scene extent, 64 * 2^-53 * L^2: each form does fewer than 32 rounded
operations on quantities bounded by L^2.  No case is left out: on-vertex and mid-edge queries, shared edges and degenerate faces included."""
import numpy as np
import pytest

import closest_point_ref as R


def _extent2(verts, pts):
    both = np.concatenate([np.asarray(verts, dtype=np.float64), np.asarray(pts, dtype=np.float64)])
    return float(np.sum((both.max(0) - both.min(0)) ** 2))


CASES = {
    "torus": lambda: R.torus(24, 12, seed=3),
    "soup": lambda: R.soup(500, 7),
    "cube": lambda: (R.CUBE_V, R.CUBE_F),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_forms_agree(name):
    verts, faces = CASES[name]()
    pts = R.queries(200, 11, verts, faces)
    bound = 64 * 2.0 ** -53 * _extent2(verts, pts)
    d_r, q_r = R.pairs_by_regions(verts, faces, pts)
    d_p, _ = R.pairs_by_parts(verts, faces, pts)
    assert np.isfinite(d_r).all() and np.isfinite(d_p).all() and np.isfinite(q_r).all()
    worst_pair = float(np.abs(d_r - d_p).max())
    m_r, f_r, c_r = R.by_regions(verts, faces, pts)
    m_p, _, _ = R.by_parts(verts, faces, pts)
    worst = float(np.abs(m_r - m_p).max())
    print(f"{name}: {d_r.size} pairs, worst pair {worst_pair / bound:.4f} of the bound, worst minimum {worst / bound:.4f}")
    assert worst <= bound and worst_pair <= bound
    # the reported face and point belong to the minimum
    assert np.array_equal(m_r, d_r[np.arange(len(pts)), f_r])
    assert np.array_equal(m_r, d_r.min(axis=1)) and np.array_equal(f_r, d_r.argmin(axis=1).astype(np.int32))
    diff = pts.astype(np.float64) - c_r
    assert np.array_equal((diff[:, 0] ** 2 + diff[:, 1] ** 2) + diff[:, 2] ** 2, m_r)


def test_chunking_keeps_the_first_of_equal_minima():
    verts, faces = R.soup(300, 5)
    pts = R.queries(64, 2, verts, faces)                 # on-vertex queries: every face round that vertex ties at 0
    whole = R.by_regions(verts, faces, pts, chunk=4096)
    cut = R.by_regions(verts, faces, pts, chunk=37)
    for a, b in zip(whole, cut):
        assert np.array_equal(a, b)
    assert (whole[0][0::4] == 0).all()


def test_voronoi_regions_of_one_triangle():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.25, 2],
                    [1, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]], dtype=np.float32)
    want_q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0],
                       [1, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]], dtype=np.float64)
    want_d = np.array([2.25, 1.25, 1.25, 1, 1, 0.5, 4, 0, 0, 0])
    for form in (R.by_regions, R.by_parts):
        d2, face, q = form(verts, faces, pts)
        assert np.array_equal(d2, want_d) and np.array_equal(q, want_q) and (face == 0).all()


@pytest.mark.parametrize("face", [[0, 0, 1], [0, 1, 1], [2, 2, 2], [0, 1, 2]])
def test_degenerate_faces_are_their_edges(face):
    verts = np.array([[0, 0, 0], [0.25, 0, 0], [0.75, 0, 0]], dtype=np.float32)      # collinear: (0,1,2) has an exactly zero normal
    faces = np.array([face], dtype=np.int32)
    pts = np.array([[-1, 0, 0], [0.1, 0.5, 0], [0.5, 0, 1], [2, 0, 0], [0.25, 0, 0]], dtype=np.float32)
    lo, hi = float(verts[face, 0].min()), float(verts[face, 0].max())
    want_q = np.zeros((5, 3))
    want_q[:, 0] = np.clip(pts[:, 0].astype(np.float64), lo, hi)
    want_d = ((pts.astype(np.float64) - want_q) ** 2).sum(1)
    for form in (R.by_regions, R.by_parts):
        d2, f, q = form(verts, faces, pts)
        assert np.isfinite(d2).all() and np.isfinite(q).all()
        assert np.allclose(d2, want_d, rtol=0, atol=8 * 2.0 ** -53 * 9) and np.allclose(q, want_q, rtol=0, atol=2.0 ** -50)


def test_cube_is_closed_and_outward():
    v = R.CUBE_V.astype(np.float64)
    a, b, c = v[R.CUBE_F[:, 0]], v[R.CUBE_F[:, 1]], v[R.CUBE_F[:, 2]]
    n = np.cross(b - a, c - a)
    assert (np.einsum("ij,ij->i", n, (a + b + c) / 3) > 0).all()             # every normal points away from the centre
    assert np.isclose(np.einsum("ij,ij->i", a, n).sum() / 6, 0.125)           # volume of the 0.5 cube
