"""GPU: csrc/mc_normals.hip (vt_mc_emit_normals through ops.mc.marching_cubes_normals) against the float64 restatement of scikit-image's
rule (tests/mc_normals_ref.py) on every volume of the fixtures.  Normals: |got - ref64| <= (n + 6) 2^-24 kappa per component (vertices
with kappa > 2^12: finite only, at most 2 % of a volume's); values: equal bits; rows in vt_mc_emit's numbering; two runs give equal bits;
the count / emit outputs are what they are without the extra call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mc_normals_ref as R  # noqa: E402
from test_mc_normals_ref_cpu import CASES, check_normals, fixtures, restated  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(vol, level=None, rescale=None):
    from vtaco_amd import ops
    return ops.mc.marching_cubes_normals(torch.from_numpy(np.ascontiguousarray(vol)).to(DEV), level=level, rescale=rescale)


@pytest.mark.parametrize("name", CASES)
def test_volume(name):
    from vtaco_amd import ops
    g7, g30 = fixtures()
    vol = g7[name + ".vol"]
    level = 0.25 if "@" in name else None
    ref = restated(name)
    tv = torch.from_numpy(vol).to(DEV)
    plain_v, plain_f, plain_level = ops.marching_cubes(tv, level=level)
    plain_v, plain_f = plain_v.clone(), plain_f.clone()
    verts, faces, normals, values, lvl = _run(vol, level)
    # the extra call changes nothing of count / emit, and the rows follow vt_mc_emit's numbering: faces and vertices are scikit-image's
    assert torch.equal(verts, plain_v) and torch.equal(faces, plain_f) and lvl == plain_level
    assert np.array_equal(faces.cpu().numpy(), g7[name + ".faces"]) and verts.cpu().numpy().tobytes() == g7[name + ".verts"].tobytes()
    assert normals.dtype == torch.float32 and tuple(normals.shape) == (len(ref["verts"]), 3) and tuple(values.shape) == (len(ref["verts"]),)
    got = normals.cpu().numpy()
    check_normals("gpu " + name, got, ref)
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) <= 4 * 2.0 ** -24) | (length == 0))
    assert np.array_equal(length == 0, np.all(ref["normals"] == 0, axis=1))
    assert values.cpu().numpy().tobytes() == ref["values"].tobytes()
    # scikit-image itself, where its normal is usable: the kernel and scikit-image each lie within the bound of the restatement
    usable = (ref["kappa"] <= R.KAPPA_MAX) & ~g30[name + ".unusable"]
    gate = 2 * R.bound(ref["n"], ref["kappa"])[usable, None]
    assert np.all(np.abs(got[usable].astype(np.float64) - g30[name + ".normals"][usable]) <= gate)
    # a second run: equal bits
    again = _run(vol, level)
    assert torch.equal(again[2], normals) and torch.equal(again[3], values) and torch.equal(again[0], verts) and torch.equal(again[1], faces)


def test_non_cubic_and_tiny_shapes_are_in_the_fixtures():
    g7, _ = fixtures()
    assert tuple(g7["noise_rect.vol"].shape) == (9, 14, 7) and tuple(g7["tiny2.vol"].shape) == (2, 2, 2)
    assert len(set(g7["noise_rect.vol"].shape)) == 3


def test_rescale_leaves_normals():
    g7, _ = fixtures()
    vol = g7["noise_rect.vol"]
    a, b = _run(vol), _run(vol, rescale=(4.5, 1.1 / 9))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[1], b[1])
    assert torch.equal(b[0], (a[0] - 4.5) * float(np.float32(1.1 / 9)))


def test_more_than_one_workgroup_and_capacity():
    """smoothnoise24 has 12 167 cells (48 chunks of 256); a capacity below the vertex count drops the rows beyond it and nothing else."""
    from vtaco_amd import ops
    g7, _ = fixtures()
    tv = torch.from_numpy(g7["smoothnoise24.vol"]).to(DEV)
    verts, faces, normals, values, _ = ops.mc.marching_cubes_normals(tv)
    ws = ops.mc.mc_count(tv)
    ops.mc.mc_emit(tv, ws, capacity=(verts.shape[0], faces.shape[0]))
    full_n, full_v = ops.mc.mc_emit_normals(tv, ws, verts.shape[0] + 7)
    assert torch.equal(full_n[:verts.shape[0]], normals) and torch.equal(full_v[:verts.shape[0]], values)
    part_n, part_v = ops.mc.mc_emit_normals(tv, ws, 1000)
    assert torch.equal(part_n, normals[:1000]) and torch.equal(part_v, values[:1000])


def test_single_cells():
    """The first 600 single-cell fixtures: every Lewiner case, centre vertices and exact ties with the level included."""
    g7, _ = fixtures()
    seen, worst = set(), 0.0
    for i in range(600):
        if int(g7["cells.nv"][i]) == 0:
            continue
        vol = g7["cells.vols"][i]
        ref = R.mc(vol, 0.0)
        verts, faces, normals, values, _ = _run(vol, 0.0)
        assert np.array_equal(faces.cpu().numpy(), ref["faces"]), i
        got = normals.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), i
        usable = ref["kappa"] <= R.KAPPA_MAX
        err = np.abs(got[usable] - ref["normals"][usable]) / R.bound(ref["n"][usable], ref["kappa"][usable])[:, None]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        assert worst <= 1.0, (i, worst)
        assert values.cpu().numpy().tobytes() == ref["values"].tobytes(), i
        corner = [float(vol[R.CZ[k], R.CY[k], R.CX[k]]) for k in range(8)]
        seen.add(int(R.tables()["CASES"][sum(1 << k for k in range(8) if corner[k] > 0)][0]))
    print(f"RATIO gpu cells: {worst:.3f} of the bound")
    assert seen == set(range(1, 15))


def test_refused_inputs():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    with pytest.raises(VtError):
        ops.mc.marching_cubes_normals(torch.zeros(4, 4, device=DEV))
    with pytest.raises(RuntimeError):
        ops.mc.marching_cubes_normals(torch.ones(4, 4, 4, device=DEV), level=5.0)       # no surface, as marching_cubes answers
