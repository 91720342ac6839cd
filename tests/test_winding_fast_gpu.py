"""GPU: the fast winding number of csrc/winding_fast.hip (``ops.winding``) against its numpy restatement tests/winding_fast_ref.py and
against the exact sum.  The tree (pyramids, lists, every record) is equal to the restatement's byte for byte and the traversal's
``stats`` exactly; ``w`` differs only by the device's atan2.  RATIO lines (error / gate) are appended to the file VTACO_RATIO_LOG names.

The gate of ``w``: the far terms are bit-equal by construction, so the difference is that of the near sums.  The ROCm installation
carries no accuracy table for its device maths library, so the device's float64 atan2 is ASSUMED good to 2 ulp (glibc's, which numpy
calls, to 1 ulp): per near term 3 ulp of |term|, plus the two running sums' roundings, 2 n u sum |terms|, plus the final add and
divide on both sides."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import closest_point_ref as C  # noqa: E402
import mesh_topo_ref as T  # noqa: E402
import voxelize_ref as VR  # noqa: E402
import winding_fast_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53
ATAN2_ULP = 2.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def named_torus():
    v, f = VR.torus(64, 32, 0.30, 0.12)
    pts = ((np.random.RandomState(0).rand(400, 3) - 0.5) * (1, 1, 0.4)).astype(np.float32)
    return v.astype(np.float32), f.astype(np.int32), pts


def mesh_of(F):
    if F == 12:
        return C.CUBE_V, C.CUBE_F
    if F == 4096:
        return named_torus()[:2]
    return C.soup(F, F)


def tree_bytes(t):
    """Everything a device tree holds, as host arrays."""
    L = t.depth
    return ([t.pyramid(l).cpu().numpy() for l in range(L + 1)], [t.records(l).cpu().numpy() for l in range(L + 1)],
            t.list_offsets.cpu().numpy(), t.lists.cpu().numpy())


def assert_tree_equals(t, ref):
    pyr, rec, loff, lists = tree_bytes(t)
    assert t.counts == [len(r) for r in ref.records]
    for l in range(ref.depth + 1):
        assert np.array_equal(pyr[l], ref.pyramid[l]), l
        assert rec[l].tobytes() == np.ascontiguousarray(ref.records[l]).tobytes(), (l, np.argwhere(rec[l] != ref.records[l])[:4])
    assert np.array_equal(loff, ref.list_offsets) and np.array_equal(lists, ref.lists)
    frame = t.frame.cpu().numpy()
    assert np.array_equal(frame[:3], ref.lo) and frame[3] == ref.side


def gate_of(ref_out):
    w, stats, far, near, near_abs = ref_out
    n = stats[:, 1].astype(np.float64)
    return ((ATAN2_ULP + 1) * 2 * U * near_abs + 2 * n * U * near_abs + 4 * U * (np.abs(far) + np.abs(near))) / W.FOUR_PI


CASES = [(1, 1, 1), (12, 63, 2), (63, 64, 1), (64, 65, 3), (65, 500, 2), (257, 64, 4), (257, 500, 1), (4096, 500, 3), (4096, 65, 4)]


@pytest.mark.parametrize("F,N,depth", CASES)
def test_tree_stats_and_w_against_the_restatement(F, N, depth):
    from vtaco_amd import ops
    v, f = mesh_of(F)
    pts = C.queries(N, 7 + F, v, f)
    ref = W.build(v, f, depth)
    tv, tf, tp = _t(v), _t(f), _t(pts)
    tree = ops.winding.build(tv, tf, depth)
    assert tree.depth == depth and tree.n_faces == F
    assert_tree_equals(tree, ref)
    worst = 0.0
    for order, accuracy in ((2, 2.0), (0, 1.0), (1, 4.0), (2, 1.0), (0, 2.0), (1, 2.0), (2, 4.0), (0, 4.0), (1, 1.0)):
        want = W.query(ref, pts, accuracy, order)
        w64, st = ops.winding.query(tree, tp, accuracy=accuracy, order=order, dtype=torch.float64, stats=True)
        assert np.array_equal(st.cpu().numpy(), want[1]), (order, accuracy)
        err, gate = np.abs(w64.cpu().numpy() - want[0]), gate_of(want)
        assert np.all(err <= gate), (order, accuracy, float((err / np.maximum(gate, 1e-300)).max()))
        worst = max(worst, float((err[gate > 0] / gate[gate > 0]).max()) if (gate > 0).any() else 0.0)
        w32 = ops.winding.query(tree, tp, accuracy=accuracy, order=order)
        assert w32.dtype == torch.float32 and torch.equal(w32, w64.float())                 # that value rounded once
    T.log_line(f"RATIO gpu winding_fast F {F} N {N} depth {depth}: |w - restatement| at most {worst:.3e} of the gate "
               f"(atan2 assumed {ATAN2_ULP:g} ulp)")


def test_a_minimum_of_minus_zero_stays_minus_zero_in_the_frame():
    """The face tree stores the vertices' minimum as it is (the point tree stores a zero as +0.0): ``np.array_equal`` cannot see that."""
    from vtaco_amd import ops
    v, f = C.CUBE_V.copy(), C.CUBE_F
    v[:, 0] += np.float32(0.25)
    v[v[:, 0] == 0, 0] = np.float32(-0.0)                           # x is -0.0 or 0.5: no +0.0 for the minimum to tie with
    ref = W.build(v, f, 2)
    assert np.signbit(ref.lo[0]) and ref.lo[0] == 0.0
    tree = ops.winding.build(_t(v), _t(f), 2)
    assert tree.frame.cpu().numpy().tobytes() == np.append(ref.lo, ref.side).astype(np.float64).tobytes()
    assert_tree_equals(tree, ref)


def test_default_depth_and_fast():
    from vtaco_amd import ops
    assert [ops.winding.default_depth(F) for F in (0, 1, 64, 65, 512, 513, 4096, 4097, 976125, 10 ** 8)] == \
        [W.default_depth(F) for F in (0, 1, 64, 65, 512, 513, 4096, 4097, 976125, 10 ** 8)] == [1, 1, 1, 2, 2, 3, 3, 4, 6, 7]
    v, f = C.soup(257, 257)
    pts = C.queries(64, 3)
    got = ops.winding.fast(_t(v), _t(f), _t(pts), dtype=torch.float64)
    assert np.abs(got.cpu().numpy() - W.fast(v, f, pts)).max() <= 1e-12


def sphere(n=9):
    """The closed sphere of test_tactile_gpu.py's winding test: a subdivided cube surface projected on radius 0.4."""
    g = np.linspace(-1, 1, n)
    verts, faces, index = [], [], {}

    def vid(p):
        key = tuple(np.round(p, 9))
        if key not in index:
            index[key] = len(verts)
            verts.append(np.array(p) / np.linalg.norm(p) * 0.4)
        return index[key]

    for axis in range(3):
        for sign in (-1.0, 1.0):
            for i in range(n - 1):
                for j in range(n - 1):
                    def pt(a, b):
                        q = [0.0, 0.0, 0.0]
                        q[axis] = sign
                        q[(axis + 1) % 3], q[(axis + 2) % 3] = g[a], g[b]
                        return q
                    quad = [vid(pt(i, j)), vid(pt(i + 1, j)), vid(pt(i + 1, j + 1)), vid(pt(i, j + 1))]
                    if sign < 0:
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)


def test_accuracy_1e30_equals_the_exact_kernel():
    from vtaco_amd import ops
    v, f = sphere()
    pts = ((np.random.RandomState(0).rand(3001, 3) - 0.5) * 1.2).astype(np.float32)
    tv, tf, tp = _t(v), _t(f), _t(pts)
    exact = ops.winding_number(tv, tf, tp).cpu().numpy()
    got, st = ops.winding.query(ops.winding.build(tv, tf), tp, accuracy=1e30, stats=True)
    got = got.cpu().numpy()
    assert np.abs(got - exact).max() <= 1e-6
    assert np.array_equal(st.cpu().numpy(), np.repeat([[0, len(f)]], len(pts), 0))
    r = np.linalg.norm(pts, axis=1)
    assert np.allclose(got[r < 0.39], 1, atol=1e-6) and np.allclose(got[r > 0.41], 0, atol=1e-6) and (r < 0.39).sum() > 100


def test_accuracy_2_on_the_named_torus():
    from vtaco_amd import ops
    v, f, pts = named_torus()
    truth = VR.winding_number(v, f, pts)
    tv, tf, tp = _t(v), _t(f), _t(pts)
    for depth in (3, 4):
        got, st = ops.winding.fast(tv, tf, tp, depth=depth, dtype=torch.float64, stats=True)
        err = np.abs(got.cpu().numpy() - truth).max()
        st = st.cpu().numpy().astype(np.float64).mean(0)
        T.log_line(f"RATIO gpu torus 4096 faces depth {depth}: max |fast - exact| {err:.3e} ({err / 1e-2:.3f} of the cap), "
                   f"mean cells {st[0]:.1f}, mean faces {st[1]:.1f}")
        assert err <= 1e-2
        assert np.array_equal(got.cpu().numpy() > 0.5, truth > 0.5)


def test_voxelize_interior_fast_winding_equals_parity_and_winding():
    from vtaco_amd.utils import voxels
    v, f, _ = named_torus()
    res = 32
    cen = VR.centres(res, (0, 0, 0), 1.0)
    # the mesh is inscribed in the torus: within the two sagittas (0.42 (1 - cos(pi/64)) + 0.12 (1 - cos(pi/32)) < 1.1e-3) of its surface
    ring = np.sqrt(cen[:, 0] ** 2 + cen[:, 1] ** 2) - 0.30
    analytic = np.abs(np.sqrt(ring ** 2 + cen[:, 2] ** 2) - 0.12)
    close = np.nonzero(analytic < 1e-3 + 1.2e-3)[0]
    dist = np.sqrt(C.by_regions(v, f, cen[close].astype(np.float32))[0])
    # No lattice of 32^3 centres keeps 1e-3 from a surface of this area (a shell that thin holds about 90 of them for a generic pose);
    # this one has 32 centres at 5.6e-4 and 7.9e-4.  Where the distance does not vouch for the label, the float64 exact sum does: it
    # must sit within 1e-6 of 0 or 1 there, ten thousand times the approximation's cap away from the threshold.
    near = close[dist <= 1e-3]
    assert len(near) <= 64
    truth = VR.winding_number(v, f, cen[near].astype(np.float32))
    assert np.all(np.minimum(np.abs(truth), np.abs(truth - 1)) <= 1e-6)
    mesh = (_t(v), _t(f))
    fast = voxels.voxelize_interior(mesh, res, rule='fast_winding')
    assert fast.dtype == torch.bool and tuple(fast.shape) == (res,) * 3 and int(fast.sum()) > 1000
    assert torch.equal(fast, voxels.voxelize_interior(mesh, res, rule='parity'))
    assert torch.equal(fast, voxels.voxelize_interior(mesh, res, rule='winding'))
    with pytest.raises(ValueError):
        voxels.voxelize_interior(mesh, res, rule='fastest')


def test_eval_winding_keyword():
    from vtaco_amd.eval import penetration_depth, penetration_depth_scenes, signed_distance
    v, f, pts = named_torus()
    tv, tf, tp = _t(v), _t(f), _t(pts)
    far = np.abs(VR.winding_number(v, f, pts) - 0.5) > 1e-2
    assert far.all()
    assert torch.equal(signed_distance(tp, tv, tf), signed_distance(tp, tv, tf, winding='exact'))
    assert torch.equal(signed_distance(tp, tv, tf, winding='fast'), signed_distance(tp, tv, tf))
    assert penetration_depth(tp, tv, tf, 2.0, winding='fast') == penetration_depth(tp, tv, tf, 2.0) > 0
    both = penetration_depth_scenes(torch.stack([tp, tp]), [(tv, tf), (_t(C.CUBE_V), _t(C.CUBE_F))], [2.0, 3.0], winding='fast')
    assert np.array_equal(both, penetration_depth_scenes(torch.stack([tp, tp]), [(tv, tf), (_t(C.CUBE_V), _t(C.CUBE_F))], [2.0, 3.0]))
    with pytest.raises(ValueError):
        signed_distance(tp, tv, tf, winding='libigl')


def test_run_to_run_and_batch_behaviour(monkeypatch):
    from vtaco_amd import ops
    monkeypatch.delenv("VTACO_WINDING_WALK", raising=False)
    v, f, pts = named_torus()
    tv, tf, tp = _t(v), _t(f), _t(pts)
    a, b = ops.winding.build(tv, tf, 4), ops.winding.build(tv, tf, 4)
    pa, pb = tree_bytes(a), tree_bytes(b)                                                   # (the padding between the parts is not written)
    assert all(x.tobytes() == y.tobytes() for l in range(2) for x, y in zip(pa[l], pb[l])) and a.counts == b.counts
    assert np.array_equal(pa[2], pb[2]) and np.array_equal(pa[3], pb[3]) and torch.equal(a.frame, b.frame)
    wa, sa = ops.winding.query(a, tp, dtype=torch.float64, stats=True)
    wb, sb = ops.winding.query(b, tp, dtype=torch.float64, stats=True)
    assert torch.equal(wa, wb) and torch.equal(sa, sb)
    monkeypatch.setenv("VTACO_WINDING_WALK", "skip")                                       # the walk past empty children: equal bits
    wq, sq = ops.winding.query(a, tp, dtype=torch.float64, stats=True)
    monkeypatch.delenv("VTACO_WINDING_WALK")
    assert torch.equal(wq, wa) and torch.equal(sq, sa)
    # neither N nor the position in the batch matters
    perm = torch.from_numpy(np.random.RandomState(1).permutation(len(pts))).to(DEV)
    wp, sp = ops.winding.query(a, tp[perm], dtype=torch.float64, stats=True)
    assert torch.equal(wp, wa[perm]) and torch.equal(sp, sa[perm])
    for n in (1, 63, 65):
        assert torch.equal(ops.winding.query(a, tp[100:100 + n], dtype=torch.float64), wa[100:100 + n])
    assert torch.equal(ops.winding.query(a, tp.reshape(20, 20, 3), dtype=torch.float64), wa.reshape(20, 20))
    cube = ops.winding.build(_t(C.CUBE_V), _t(C.CUBE_F))
    ws, ss = ops.winding.query_scenes([a, cube], torch.stack([tp, tp]), dtype=torch.float64, stats=True)
    wc, sc = ops.winding.query(cube, tp, dtype=torch.float64, stats=True)
    assert torch.equal(ws[0], wa) and torch.equal(ws[1], wc) and torch.equal(ss[0], sa) and torch.equal(ss[1], sc)
    assert ops.winding.query_scenes([a, cube], torch.stack([tp, tp])).dtype == torch.float32


def test_bad_arguments_and_empty_inputs():
    import ctypes
    from vtaco_amd import _lib, ops
    from vtaco_amd._lib import VtError
    lib = _lib.load()
    v, f, pts = named_torus()
    tv, tf, tp = _t(v), _t(f), _t(pts)
    empty = ops.winding.build(tv, torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert empty.n_faces == 0 and empty.counts == [0, 0]
    w, st = ops.winding.query(empty, tp, stats=True)
    assert torch.equal(w, torch.zeros(len(pts), device=DEV)) and int(st.abs().sum()) == 0
    assert torch.equal(ops.winding.query(empty, tp, dtype=torch.float64), torch.zeros(len(pts), dtype=torch.float64, device=DEV))
    tree = ops.winding.build(tv, tf)
    none, st = ops.winding.query(tree, torch.zeros((0, 3), device=DEV), stats=True)
    assert tuple(none.shape) == (0,) and tuple(st.shape) == (0, 2)
    for depth in (0, 8):
        assert lib.vt_winding_tree_workspace_bytes(len(v), len(f), depth) == 0
        with pytest.raises(VtError, match=r"code -2"):
            ops.winding.build(tv, tf, depth)
    bad = tv.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(VtError, match=r"code -1.*not finite"):
        ops.winding.build(bad, tf)
    bad[17, 1] = float("inf")
    with pytest.raises(VtError, match=r"code -1.*not finite"):
        ops.winding.build(bad, tf)
    # the C ABI itself: every check on the host, before any launch
    vp, fp = ctypes.c_void_p(tv.data_ptr()), ctypes.c_void_p(tf.contiguous().data_ptr())
    nbytes = lib.vt_winding_tree_workspace_bytes(len(v), len(f), 3)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    wp = ctypes.c_void_p(ws.data_ptr())
    assert lib.vt_winding_tree_count(vp, len(v), fp, len(f), 3, None, nbytes, None) == -1              # null workspace
    assert lib.vt_winding_tree_count(vp, len(v), fp, len(f), 3, wp, nbytes - 256, None) == -3          # short workspace
    assert lib.vt_winding_tree_count(None, len(v), fp, len(f), 3, wp, nbytes, None) == -1
    assert lib.vt_winding_tree_count(vp, len(v), fp, -1, 3, wp, nbytes, None) == -1
    assert lib.vt_winding_tree_count(vp, len(v), fp, len(f), 8, wp, nbytes, None) == -2
    assert lib.vt_winding_tree_count(vp, len(v), fp, 0x20000000, 3, wp, nbytes, None) == -2            # beyond MT_MAX_F
    state = (ctypes.c_int32 * 16)(*([0, 1, 8, 60, 300] + [0] * 11))
    out = torch.empty(4, device=DEV)
    op, pp = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(tp.data_ptr())
    assert lib.vt_winding_tree_build(vp, len(v), fp, len(f), 3, state, wp, nbytes, None, 1 << 30, None) == -1     # null tree
    assert lib.vt_winding_tree_build(vp, len(v), fp, len(f), 3, state, wp, nbytes, wp, 256, None) == -3           # short tree
    assert lib.vt_winding_tree_query(None, 0, len(f), 3, state, pp, 4, 2.0, 2, op, 0, None, None) == -1
    assert lib.vt_winding_tree_query(wp, 256, len(f), 3, state, pp, 4, 2.0, 2, op, 0, None, None) == -3
    assert lib.vt_winding_tree_query(wp, 1 << 30, len(f), 3, state, pp, 4, 2.0, 3, op, 0, None, None) == -1       # order 3
    assert lib.vt_winding_tree_query(wp, 1 << 30, len(f), 0, state, pp, 4, 2.0, 2, op, 0, None, None) == -2
    assert lib.vt_winding_tree_query(wp, 1 << 30, len(f), 3, state, pp, 0, 2.0, 2, None, 0, None, None) == 0       # N == 0
    torch.cuda.synchronize()


def test_vtaco_winding_knob(monkeypatch):
    """VTACO_WINDING unset / 'exact': ``_t2d_samples``' targets are the single vt_winding_number_scenes launch's, bit for bit; 'fast':
    the same labels at the 0.5 threshold, from trees cached per mesh object.  The meshes are the trainer goldens' cube and
    tetrahedron (tests/synth_dataset.py writes point files only, no mesh) and a torus."""
    from conftest import GOLDEN
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.training import Trainer
    z12 = np.load(os.path.join(GOLDEN, "g12_t2d.npz"))
    z13 = np.load(os.path.join(GOLDEN, "g13_trainer_t2d.npz"))
    tv, tf = C.torus(24, 12)
    vf = {"cube": {"v": z13["cube_v"], "f": z13["cube_f"]}, "tet": {"v": z13["tet_v"], "f": z13["tet_f"]}, "torus": {"v": tv, "f": tf}}
    trainer = Trainer.__new__(Trainer)
    trainer.device, trainer.num_sample, trainer.pretrained_t2d, trainer.depth_origin = DEV, 640, True, z12["depth_origin"]
    g = torch.Generator().manual_seed(2)
    d = torch.randn(3, 300, 3, generator=g)
    tile = lambda a: np.concatenate([a, a[:1]])
    batch = {"inputs": 0.3 * d / d.norm(dim=-1, keepdim=True), "points": (torch.rand(3, 900, 3, generator=g) - 0.5) * 1.1,
             "points.name": ["cube", "tet", "torus"], "points.cam_pos": torch.from_numpy(tile(z13["cam_pos"])),
             "points.cam_rot": torch.from_numpy(tile(z13["cam_rot"])), "inputs.pc_ply": torch.from_numpy(tile(z13["pc_ply"])),
             "inputs.img": torch.rand(3, 5, 3, 8, 6, generator=g),
             "inputs.depth": torch.from_numpy(np.stack([z12["depths"], np.roll(z12["depths"], 7, axis=0), z12["depths"]])),
             "inputs.touch_success": torch.from_numpy(tile(z13["touch"]))}

    def samples(mode):
        if mode is None:
            monkeypatch.delenv("VTACO_WINDING", raising=False)
        else:
            monkeypatch.setenv("VTACO_WINDING", mode)
        np.random.seed(0)
        return trainer._t2d_samples(batch, vf, False)

    unset, exact, fast = samples(None), samples("exact"), samples("fast")
    direct = ops.winding_number_scenes([trainer._device_mesh(vf, n) for n in batch["points.name"]], unset["p_sample"])
    assert torch.equal(unset["p_sample"], exact["p_sample"]) and torch.equal(unset["p_sample"], fast["p_sample"])
    assert torch.equal(unset["occ"], direct) and torch.equal(exact["occ"], direct)
    assert fast["occ"].dtype == direct.dtype and fast["occ"].shape == direct.shape
    assert torch.equal(fast["occ"] > 0.5, direct > 0.5)
    assert float((fast["occ"] - direct).abs().max()) <= 1e-2
    trees = dict(trainer._tree_cache)
    samples("fast")
    assert all(trainer._tree_cache[k][2] is trees[k][2] for k in trees) and sorted(trees) == ["cube", "tet", "torus"]
    vf["tet"] = {"v": z13["tet_v"].copy(), "f": z13["tet_f"]}                                 # a replaced mesh object: a new tree
    samples("fast")
    assert trainer._tree_cache["tet"][2] is not trees["tet"][2] and trainer._tree_cache["cube"][2] is trees["cube"][2]
    monkeypatch.setenv("VTACO_WINDING", "libigl")
    with pytest.raises(VtError, match="VTACO_WINDING"):
        trainer._t2d_samples(batch, vf, False)
