"""GPU: Generator3D(with_normals=True) on the 32^3 lattice of the golden PointNet + decoder pair (the scene of
tests/test_mesh_clean_generation_gpu.py, far blob included): the routes return a NormalMesh whose normals and values are
ops.mc.marching_cubes_normals of the same logits, the default returns the plain Mesh it always returned, the component filter gathers
the normals, simplification recomputes them from the geometry, the sharded route refuses, an exported file reads back to the normals;
and eval.mesh_distances(..., normals=True)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX = 32


def _blob_generator(corner):
    from vtaco_amd.conv_onet.generation import Generator3D

    class BlobGenerator(Generator3D):
        def eval_lattice(self, c, nx, c_img_all=None, first=0, count=None, out=None):
            values = super().eval_lattice(c, nx, c_img_all=c_img_all, first=first, count=count, out=out)
            if first == 0 and count is None and corner is not None:
                v = values.view(nx, nx, nx)
                sl = tuple(slice(nx - 5, nx - 2) if hi else slice(2, 5) for hi in corner)
                v[sl] = values.max()
            return values
    return BlobGenerator


@pytest.fixture(scope="module")
def scene():
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    from vtaco_amd.encoder import encoder_dict
    a, sd_e = load_golden("g3_pointnet.npz")
    _, sd_d = load_golden("g1_decode.npz")
    dec = decoder_dict['simple_local'](dim=3, c_dim=32, hidden_size=32, with_contact=True)
    dec.load_state_dict(sd_d, strict=True)
    enc = encoder_dict['pointnet_local_pool'](c_dim=32, dim=3, hidden_dim=32, unet3d=False, unet3d_kwargs=None, grid_resolution=16,
                                              plane_type='grid')
    enc.load_state_dict(sd_e, strict=True)
    model = ConvolutionalOccupancyNetwork(dec, enc.to(DEV), device=DEV)
    p = torch.from_numpy(a["p"])[:1]
    plain = _blob_generator(None)(model, device=DEV, resolution0=NX // 4, padding=0.1)
    with torch.no_grad():
        vol = plain.eval_lattice(model.encode_inputs(p.to(DEV)), NX).view(NX, NX, NX)
    corners = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    mean = lambda cr: float(vol[tuple(slice(NX - 8, NX) if hi else slice(0, 8) for hi in cr)].mean())
    return model, p, _blob_generator(min(corners, key=mean))


KW = dict(device=DEV, resolution0=NX // 4, padding=0.1)


def _eager(gen, data):
    gen.scene_graph = False
    try:
        return gen.generate_obj_mesh_wnf(data)
    finally:
        del gen.scene_graph


def test_with_normals_is_marching_cubes_normals_of_the_logits(scene):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    model, p, Gen = scene
    on, off = Gen(model, with_normals=True, **KW), Gen(model, **KW)
    data = {"inputs": p}
    mesh, plain = _eager(on, data), _eager(off, data)
    assert type(plain) is Mesh and type(mesh) is NormalMesh and mesh.normals_source == "marching_cubes"
    assert torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces) and mesh.faces.shape[0] > 0
    v, f = mesh                                                   # still a (vertices, faces) pair
    assert v is mesh.vertices and f is mesh.faces
    with torch.no_grad():
        vol = on.eval_lattice(model.encode_inputs(p.to(DEV)), NX).view(NX, NX, NX)
    verts, faces, normals, values, _ = ops.mc.marching_cubes_normals(vol, rescale=(NX / 2, 1.1 / NX))
    assert torch.equal(verts, mesh.vertices) and torch.equal(faces, mesh.faces)
    assert torch.equal(normals, mesh.vertex_normals) and torch.equal(values, mesh.values)
    length = mesh.vertex_normals.double().norm(dim=1)
    assert ((length - 1).abs() < 1e-6).all() and (mesh.values > 0).all()
    # low-minus-high gradients point down the field, and so does the winding of gradient_direction='ascent': marching cubes' normals
    # and the normals of the geometry are two estimates of one direction
    geo = mesh.geometric_vertex_normals()
    assert float((geo * mesh.vertex_normals).sum(dim=1).mean()) > 0.9
    # the graphed scene: the extra launch goes behind the emit, outside the graph
    for _ in range(3):                                            # (a shape is captured when it comes back)
        g_on, g_off = on.generate_mesh_graphed(p), off.generate_mesh_graphed(p)
        assert type(g_off) is Mesh and torch.equal(g_off.vertices, plain.vertices) and torch.equal(g_off.faces, plain.faces)
        assert type(g_on) is NormalMesh and torch.equal(g_on.vertices, mesh.vertices) and torch.equal(g_on.faces, mesh.faces)
        assert torch.equal(g_on.vertex_normals, mesh.vertex_normals) and torch.equal(g_on.values, mesh.values)


def test_mise_route(scene):
    from vtaco_amd.conv_onet.generation import Mesh, NormalMesh
    model, p, Gen = scene
    kw = dict(device=DEV, resolution0=8, upsampling_steps=2, padding=0.1, extraction="mise")
    on, off = Gen(model, with_normals=True, **kw), Gen(model, **kw)
    mesh, plain = on.generate_obj_mesh_wnf({"inputs": p}), off.generate_obj_mesh_wnf({"inputs": p})
    assert type(plain) is Mesh and type(mesh) is NormalMesh and mesh.normals_source == "marching_cubes"
    assert torch.equal(mesh.vertices, plain.vertices) and torch.equal(mesh.faces, plain.faces) and mesh.faces.shape[0] > 0
    assert tuple(mesh.vertex_normals.shape) == tuple(mesh.vertices.shape) and torch.isfinite(mesh.vertex_normals).all()


def test_component_filter_gathers_and_simplification_recomputes(scene):
    from vtaco_amd.conv_onet.generation import NormalMesh
    model, p, Gen = scene
    data = {"inputs": p}
    full = _eager(Gen(model, with_normals=True, **KW), data)
    comps = full.components()
    assert comps.n_components >= 2
    biggest = int(torch.argmax(comps.n_faces))
    kept = comps.comp_of_vertex == biggest
    for route in ("eager", "graphed"):
        gen = Gen(model, with_normals=True, components="largest", **KW)
        got = _eager(gen, data) if route == "eager" else gen.generate_mesh_graphed(p)
        assert type(got) is NormalMesh and got.normals_source == "marching_cubes", route
        assert 0 < got.vertices.shape[0] < full.vertices.shape[0]
        assert torch.equal(got.vertices, full.vertices[kept]) and torch.equal(got.vertex_normals, full.vertex_normals[kept]), route
        assert torch.equal(got.values, full.values[kept]), route
    target = max(50, full.faces.shape[0] // 8)
    slim = _eager(Gen(model, with_normals=True, simplify_nfaces=target, **KW), data)
    bare = _eager(Gen(model, simplify_nfaces=target, **KW), data)
    assert type(slim) is NormalMesh and slim.normals_source == "geometry" and slim.values is None
    assert 0 < slim.faces.shape[0] <= target and torch.equal(slim.vertices, bare.vertices) and torch.equal(slim.faces, bare.faces)
    assert torch.equal(slim.vertex_normals, bare.vertex_normals(weight="area"))
    # nothing to simplify: marching cubes' normals stay
    roomy = _eager(Gen(model, with_normals=True, simplify_nfaces=10 ** 7, **KW), data)
    assert roomy.normals_source == "marching_cubes" and torch.equal(roomy.vertex_normals, full.vertex_normals)


def test_sharded_route_refuses_and_config_key(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    model, p, Gen = scene
    with pytest.raises(VtError, match="sharded"):
        Gen(model, with_normals=True, **KW).generate_obj_mesh_sharded({"inputs": p})
    cfg = {"generation": {"resolution_0": 8, "upsampling_steps": 0, "with_normals": True}, "test": {"threshold": 0.5},
           "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    assert config.get_generator(model, cfg, DEV).with_normals is True
    cfg["generation"].pop("with_normals")
    assert config.get_generator(model, cfg, DEV).with_normals is False


def test_exported_files_read_back(scene, tmp_path):
    model, p, Gen = scene
    mesh = _eager(Gen(model, with_normals=True, **KW), {"inputs": p})
    want = mesh.vertex_normals.cpu().numpy()
    mesh.export(str(tmp_path / "m.ply"))
    lines = open(tmp_path / "m.ply").read().split("\n")
    end = lines.index("end_header")
    assert [l.split()[2] for l in lines[:end] if l.startswith("property float")] == ["x", "y", "z", "nx", "ny", "nz"]
    rows = np.array([[float(x) for x in l.split()] for l in lines[end + 1:end + 1 + len(want)]], dtype=np.float32)
    assert rows[:, 3:].tobytes() == want.tobytes() and rows[:, :3].tobytes() == mesh.vertices.cpu().numpy().tobytes()
    mesh.export(str(tmp_path / "m.obj"))
    obj = open(tmp_path / "m.obj").read().split("\n")
    vn = np.array([[float(x) for x in l.split()[1:]] for l in obj if l.startswith("vn ")], dtype=np.float32)
    assert vn.tobytes() == want.tobytes()
    first_face = [l for l in obj if l.startswith("f ")][0].split()[1:]
    assert [c.split("//")[0] for c in first_face] == [c.split("//")[1] for c in first_face] == [str(int(i) + 1) for i in mesh.faces[0]]


# ---- eval.mesh_distances(..., normals=True) ---------------------------------------------------------------------------------------------
def _iso_mesh(kind, n=32):
    from vtaco_amd import ops
    g = torch.linspace(-0.5, 0.5, n, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    if kind == "sphere":
        vol = torch.sqrt(x * x + y * y + z * z) - 0.35
    else:
        vol = torch.maximum(torch.maximum(x.abs(), y.abs()), z.abs()) - 0.3
    verts, faces, _ = ops.marching_cubes(vol.contiguous(), 0.0, rescale=(n / 2, 1.0 / n))
    return verts.clone(), faces.clone()


def test_mesh_distances_normals():
    from vtaco_amd import eval as ev
    sphere, cube = _iso_mesh("sphere"), _iso_mesh("cube")
    inside_out = (sphere[0], sphere[1][:, [0, 2, 1]].contiguous())
    n = 2000

    def run(a, b, **kw):
        return ev.mesh_distances(a, b, n, generator=torch.Generator(device=DEV).manual_seed(5), **kw)
    plain, both = run(sphere, sphere), run(sphere, sphere, normals=True)
    assert sorted(plain) == ["accuracy", "chamfer_l1", "completeness", "f_score"]
    assert sorted(both) == sorted(list(plain) + ["normals_accuracy", "normals_completeness", "normals_consistency"])
    assert all(both[k] == plain[k] for k in plain)                   # the old keys: equal bits from the same generator state
    assert both["normals_accuracy"] > 0.99 and both["normals_completeness"] > 0.99 and both["normals_consistency"] > 0.99
    assert both["normals_consistency"] == 0.5 * (both["normals_accuracy"] + both["normals_completeness"])
    flipped = run(sphere, inside_out, normals=True)
    assert flipped["normals_consistency"] > 0.99                     # (the absolute dot product)
    other = run(sphere, cube, normals=True)
    assert other["normals_consistency"] < both["normals_consistency"] - 0.05
    tree = run(sphere, cube, normals=True, distance="tree")
    assert all(tree[k] == other[k] for k in ("accuracy", "completeness", "chamfer_l1", "f_score"))
    assert abs(tree["normals_consistency"] - other["normals_consistency"]) < 0.02      # (equidistant faces may be told apart differently)
    aligned = ev.mesh_distances_aligned(sphere, sphere, n, generator=torch.Generator(device=DEV).manual_seed(5), normals=True)
    assert aligned["normals_consistency"] > 0.99 and "transform" in aligned
    assert "normals_consistency" not in ev.mesh_distances_aligned(sphere, sphere, n, generator=torch.Generator(device=DEV).manual_seed(5))
