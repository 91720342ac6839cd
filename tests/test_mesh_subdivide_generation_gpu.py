"""GPU: Generator3D.configure_subdivide on the shipped scene's model (tests/config2_case.py, as tests/test_refine_generation_gpu.py loads
it) at resolution0 = 8: a 32^3 lattice, a few thousand faces.  The default state changes nothing and calls nothing; 'midpoint' gives four
times the faces on the same vertices; the step stands after smooth and before simplify_nfaces; refinement_step moves the vertices of the
subdivided connectivity; with_normals gives geometric normals; the sharded route refuses; the config keys arrive."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import config2_case as c2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(device=DEV, resolution0=8, padding=0.1, decode_precision="f32")


@pytest.fixture(scope="module")
def shipped():
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    z = c2.fixture()
    enc, dec = c2.models(z)
    model = ConvolutionalOccupancyNetwork(dec, enc, device=DEV).eval()
    data = {"inputs": torch.from_numpy(z["cloud"]).float()}
    return model, data, Generator3D(model, **KW).generate_obj_mesh_wnf(data)


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_default_calls_nothing_and_midpoint_gives_four_times_the_faces(shipped, monkeypatch):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    model, data, plain = shipped
    V, F = plain.vertices.shape[0], plain.faces.shape[0]
    assert 500 <= F <= 20000
    with monkeypatch.context() as mp:                                   # the default state never reaches the new operations

        def boom(*a, **k):
            raise AssertionError("the default must launch nothing")
        for name in ("subdivide", "subdivide_count", "subdivide_midpoints"):
            mp.setattr(ops.mesh, name, boom)
        for graph in (True, False):
            for gen in (Generator3D(model, **KW), Generator3D(model, **KW).configure_subdivide(), Generator3D(model, **KW).configure_subdivide("loop", 0)):
                gen.scene_graph = graph
                mesh = gen.generate_obj_mesh_wnf(data)
                assert type(mesh) is Mesh and _same(mesh, plain)
        with pytest.raises(AssertionError, match="launch nothing"):
            Generator3D(model, **KW).configure_subdivide("midpoint").generate_obj_mesh_wnf(data)
    got = Generator3D(model, **KW).configure_subdivide("midpoint", 1).generate_obj_mesh_wnf(data)
    assert got.faces.shape[0] == 4 * F and torch.equal(got.vertices[:V], plain.vertices) and _same(got, plain.subdivide())
    two = Generator3D(model, **KW).configure_subdivide("midpoint", 2).generate_obj_mesh_wnf(data)
    assert two.faces.shape[0] == 16 * F and _same(two, plain.subdivide(2))
    loop = Generator3D(model, **KW).configure_subdivide("loop").generate_obj_mesh_wnf(data)
    assert _same(loop, plain.subdivide_loop()) and torch.equal(loop.faces, got.faces) and not torch.equal(loop.vertices[:V], plain.vertices)
    edge = 0.6 * float((plain.vertices[plain.faces[:, 0].long()] - plain.vertices[plain.faces[:, 1].long()]).norm(dim=1).max())
    sized = Generator3D(model, **KW).configure_subdivide("midpoint", max_edge=edge).generate_obj_mesh_wnf(data)
    assert _same(sized, plain.subdivide_to_size(edge)) and F < sized.faces.shape[0] < 16 * F
    # the order: smooth, subdivide, simplify
    want = plain.smooth("taubin").subdivide()
    assert not _same(want, plain.subdivide().smooth("taubin"))
    assert _same(Generator3D(model, smooth="taubin", **KW).configure_subdivide("midpoint").generate_obj_mesh_wnf(data), want)
    target = 2 * F
    got = Generator3D(model, simplify_nfaces=target, **KW).configure_subdivide("midpoint").generate_obj_mesh_wnf(data)
    assert _same(got, plain.subdivide().simplify(nfaces=target)) and 0 < got.faces.shape[0] <= target


def test_refinement_sees_the_subdivided_mesh_and_normals_are_geometric(shipped):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D, NormalMesh
    model, data, plain = shipped
    dense = plain.subdivide()
    gen = Generator3D(model, refinement_step=3, **KW).configure_subdivide("midpoint", 1)
    mesh = gen.generate_obj_mesh_wnf(data)
    assert torch.equal(mesh.faces, dense.faces) and mesh.vertices.shape == dense.vertices.shape
    moved = (mesh.vertices.double() - dense.vertices.double()).abs().max(1).values
    assert float(moved.max()) > 0 and float(moved[plain.vertices.shape[0]:].max()) > 0          # the new vertices are refined too
    assert torch.equal(mesh.vertices, gen.generate_obj_mesh_wnf(data).vertices)
    nm = Generator3D(model, with_normals=True, **KW).configure_subdivide("midpoint").generate_obj_mesh_wnf(data)
    assert isinstance(nm, NormalMesh) and nm.normals_source == "geometry" and nm.values is None and _same(nm, dense)
    assert torch.equal(nm.vertex_normals, ops.mesh.normals(nm.vertices, nm.faces, face=False).vertex_normals)


def test_sharded_route_refuses_and_config_keys_arrive(shipped):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D
    model, data, _ = shipped
    with pytest.raises(VtError, match="sharded"):
        Generator3D(model, **KW).configure_subdivide("loop").generate_obj_mesh_sharded(data)
    cfg = {"generation": {"resolution_0": 8, "upsampling_steps": 0, "subdivide": "midpoint", "subdivide_iterations": 2, "subdivide_max_edge": None},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.subdivide, gen.subdivide_iterations, gen.subdivide_max_edge) == ("midpoint", 2, None)
    cfg["generation"] = {"resolution_0": 8, "upsampling_steps": 0}
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.subdivide, gen.subdivide_iterations, gen.subdivide_max_edge) == (None, 1, None)
