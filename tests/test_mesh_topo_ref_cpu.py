"""CPU: the numpy restatement of csrc/mesh_topo.hip (tests/mesh_topo_ref.py) on meshes whose answers are known by hand, the kernel's
fixed-point accumulation restated against math.fsum, and the generator's new arguments without a device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_topo_ref as R  # noqa: E402


def test_tetrahedron():
    v, f = R.tetrahedron()
    t = R.topo(v, f)
    assert t["n_components"] == 1 and t["labels"].tolist() == [0, 0, 0, 0]
    assert (int(t["n_vertices"][0]), int(t["n_edges"][0]), int(t["n_faces"][0]), int(t["euler"][0])) == (4, 6, 4, 2)
    assert bool(t["watertight"][0]) and bool(t["oriented"][0])
    det = np.linalg.det(np.stack([v[1] - v[0], v[2] - v[0], v[3] - v[0]]).astype(np.float64))
    assert t["volume"][0] == pytest.approx(det / 6.0, rel=1e-15) and t["volume"][0] > 0
    assert t["area"][0] == pytest.approx(1.5 + math.sqrt(3.0) / 2.0, rel=1e-15)
    assert t["bbox"].tolist() == [[[0, 0, 0], [1, 1, 1]]]


def test_torus_has_euler_number_zero():
    v, f = R.torus(8, 16)
    t = R.topo(v, f)
    assert t["n_components"] == 1 and int(t["euler"][0]) == 0 and bool(t["oriented"][0])
    assert (int(t["n_vertices"][0]), int(t["n_edges"][0]), int(t["n_faces"][0])) == (128, 384, 256)


def test_two_cubes_and_a_spare_vertex():
    v, f = R.two_cubes_and_a_spare()
    t = R.topo(v, f)
    assert t["n_components"] == 2
    assert t["comp_of_vertex"].tolist() == [0] * 8 + [-1] + [1] * 8 and t["labels"][8] == 8
    assert t["comp_of_face"].tolist() == [0] * 12 + [1] * 12
    assert t["euler"].tolist() == [2, 2] and t["oriented"].tolist() == [True, True]
    assert t["volume"].tolist() == [1.0, 0.125] and t["area"].tolist() == [6.0, 1.5]
    vk, fk, vmap = R.filter_mesh(v, f, t, [0, 1])
    assert vk.shape == (8, 3) and fk.min() == 0 and fk.max() == 7 and vmap.tolist() == [-1] * 9 + list(range(8))
    assert np.array_equal(vk, v[9:])
    assert R.largest(t, "faces").tolist() == [True, False] and R.largest(t, "volume").tolist() == [True, False]


def test_open_disk():
    v, f = R.disk(12)
    t = R.topo(v, f)
    assert int(t["n_boundary"][0]) == 12 and int(t["euler"][0]) == 1 and not bool(t["watertight"][0])


def test_three_faces_on_one_edge():
    t = R.topo(*R.fan_on_one_edge())
    assert int(t["n_nonmanifold"][0]) == 1 and int(t["n_edges"][0]) == 7 and not bool(t["watertight"][0])


def test_cube_with_one_face_flipped():
    t = R.topo(*R.cube_one_face_flipped())
    assert int(t["n_misoriented"][0]) == 3 and bool(t["watertight"][0]) and not bool(t["oriented"][0])


def test_face_with_a_repeated_index():
    t = R.topo(*R.degenerate_face())
    assert int(t["n_edges"][0]) == 1 and int(t["n_faces"][0]) == 1 and int(t["n_boundary"][0]) == 0
    assert t["area"][0] == 0.0 and t["volume"][0] == 0.0


def test_builders_have_the_shape_the_gpu_tests_rely_on():
    v, f = R.permuted_strip(2000, seed=3)
    t = R.topo(v, f)
    assert t["n_components"] == 1 and f.shape == (1998, 3) and int(t["labels"].max()) == 0
    assert int(t["n_misoriented"][0]) == 0 and int(t["euler"][0]) == 1
    v, f = R.triangles_and_spares(50, 7)
    t = R.topo(v, f)
    assert t["n_components"] == 50 and int((t["comp_of_vertex"] < 0).sum()) == 7
    for n in (1, 63, 64, 65):
        assert R.grid_strip(n)[1].shape == (n, 3) and R.topo(*R.grid_strip(n))["n_components"] == 1
    v, f = R.concatenated()
    t = R.topo(v, f)
    assert t["n_components"] == 8 and int(t["n_nonmanifold"][0]) == 3          # the tetrahedron's doubled face: three edges with three faces


def test_fixed_point_sum_is_inside_the_gate_and_order_free():
    rng = np.random.RandomState(11)
    for scale, n in ((1.0, 1), (1e-30, 7), (1e12, 1000), (3.0, 5000)):
        terms = (rng.randn(n) * scale * 10.0 ** rng.uniform(-6, 0, n)).tolist()
        got, ref = R.fixed_point_sum(terms), math.fsum(terms)
        assert abs(got - ref) <= (n + 16) * 2.0 ** -52 * math.fsum(abs(x) for x in terms)
        assert abs(got - ref) <= 2.0 ** -52 * math.fsum(abs(x) for x in terms)       # in fact one rounding of the whole sum, about
        assert R.fixed_point_sum(terms[::-1]) == got
    assert R.fixed_point_sum([0.0, 0.0]) == 0.0 and R.fixed_point_sum([5e-324, 5e-324]) == 1e-323


def test_generator_arguments_without_a_device():
    import torch
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config as cfgmod
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    model = torch.nn.Linear(1, 1)
    gen = Generator3D(model)
    assert gen.components == "all" and gen.min_component_faces == 0 and not gen._filters_components()
    assert Generator3D.COMPONENTS == ("all", "largest", "largest_area", "largest_volume")
    with pytest.raises(VtError):
        Generator3D(model, components="biggest")
    with pytest.raises(VtError):
        Generator3D(model, min_component_faces=-1)
    cfg = {"data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}, "test": {"threshold": 0.5},
           "generation": {"resolution_0": 8, "upsampling_steps": 0}}
    gen = cfgmod.get_generator(model, cfg, None)
    assert (gen.components, gen.min_component_faces) == ("all", 0)
    cfg["generation"].update(components="largest_area", min_component_faces=12)
    gen = cfgmod.get_generator(model, cfg, None)
    assert (gen.components, gen.min_component_faces) == ("largest_area", 12) and gen._filters_components()
    with pytest.raises(VtError, match="sharded"):
        gen.generate_obj_mesh_sharded({"inputs": torch.zeros(1, 4, 3)})
    m = Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    assert gen._clean(Mesh(m.vertices, m.faces[:0])).faces.shape[0] == 0
    for name in ("components", "split", "keep_largest", "remove_small"):
        assert callable(getattr(m, name))
    with pytest.raises(VtError):
        m.components()                                  # a CPU mesh: there is no host path
    assert m == (m.vertices, m.faces) and len(m) == 2


def test_ops_mesh_is_a_submodule_only():
    from vtaco_amd import ops
    for name in ("components", "component_table", "component_stats", "edge_stats", "filter_components"):
        assert callable(getattr(ops.mesh, name)) and not hasattr(ops, name)
