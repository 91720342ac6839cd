"""GPU: Generator3D(smooth=..., smooth_iterations=...) on the 32^3 lattice of the golden PointNet + decoder pair, with the cut and the
floater of tests/test_mesh_fill_generation_gpu.py written into the field (an open surface against the x = 0 side, so that there are
boundary vertices to pin, and a small closed piece for the component filter).  None changes nothing and calls nothing; a method is
filter -> fill_holes -> Mesh.smooth -> simplify, on the eager and the graphed route; with_normals gives the normals of the smoothed
geometry; the sharded route refuses; the config keys arrive."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX = 32
KW = dict(device=DEV, resolution0=NX // 4, padding=0.1)


def _cut_generator(corner):
    from vtaco_amd.conv_onet.generation import Generator3D

    class CutGenerator(Generator3D):
        def eval_lattice(self, c, nx, c_img_all=None, first=0, count=None, out=None):
            values = super().eval_lattice(c, nx, c_img_all=c_img_all, first=first, count=count, out=out)
            if first == 0 and count is None:
                v = values.view(nx, nx, nx)
                top = values.max()
                y, z = (slice(nx - 7, nx - 3) if hi else slice(3, 7) for hi in corner)
                v[0:3, y, z] = top                                 # against the x = 0 side: an open surface with one planar loop
                v[nx - 6:nx - 4, y.start:y.start + 2, z.start:z.start + 2] = top      # a closed floater inside the box, the smallest piece
            return values
    return CutGenerator


@pytest.fixture(scope="module")
def scene():
    from vtaco_amd.conv_onet.generation import Generator3D
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
    with torch.no_grad():
        vol = Generator3D(model, **KW).eval_lattice(model.encode_inputs(p.to(DEV)), NX).view(NX, NX, NX)
    corners = [(j, k) for j in (0, 1) for k in (0, 1)]
    mean = lambda cr: float(vol[(slice(None),) + tuple(slice(NX - 10, NX) if hi else slice(0, 10) for hi in cr)].mean())
    return model, p, _cut_generator(min(corners, key=mean))       # the (y, z) corner where the field is lowest along all of x


def _eager(gen, data):
    gen.scene_graph = False
    try:
        return gen.generate_obj_mesh_wnf(data)
    finally:
        del gen.scene_graph


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_none_calls_nothing_and_a_method_is_filter_fill_smooth_simplify(scene, monkeypatch):
    from vtaco_amd import ops
    model, p, Gen = scene
    data = {"inputs": p}
    bare, none = Gen(model, **KW), Gen(model, smooth=None, smooth_iterations=10, **KW)
    mesh = _eager(bare, data)
    assert int(mesh.boundary_vertices().sum()) >= 3 and mesh.components().n_components >= 3     # there is something to pin and to filter
    with monkeypatch.context() as mp:                                   # the default never reaches the new operations

        def boom(*a, **k):
            raise AssertionError("smooth=None must launch nothing")
        for name in ("vertex_adjacency", "smooth", "smooth_weights"):
            mp.setattr(ops.mesh, name, boom)
        assert _same(_eager(none, data), mesh) and _same(none.generate_mesh_graphed(p), mesh) and _same(bare.generate_mesh_graphed(p), mesh)
        with pytest.raises(AssertionError, match="launch nothing"):
            _eager(Gen(model, smooth="taubin", **KW), data)
    for method in ("laplacian", "taubin", "humphrey"):
        want = mesh.smooth(method)
        assert torch.equal(want.faces, mesh.faces) and not torch.equal(want.vertices, mesh.vertices)
        pinned = mesh.boundary_vertices()
        assert torch.equal(want.vertices[pinned], mesh.vertices[pinned])
        gen = Gen(model, smooth=method, **KW)
        assert _same(_eager(gen, data), want) and _same(gen.generate_mesh_graphed(p), want) and _same(gen.generate_mesh_graphed(p), want)
    assert _same(_eager(Gen(model, smooth="taubin", smooth_iterations=3, **KW), data), mesh.smooth("taubin", 3))
    assert _same(_eager(Gen(model, smooth="taubin", smooth_iterations=0, **KW), data), mesh)
    # the order: component filter, fill, smooth, simplify
    filled = mesh.fill_holes("fan")
    want = filled.smooth("taubin")
    assert filled.faces.shape[0] > mesh.faces.shape[0] and int(filled.boundary_vertices().sum()) == 0
    assert not _same(want, mesh.smooth("taubin").fill_holes("fan"))     # the other order pins the rim: a different mesh
    assert _same(_eager(Gen(model, fill_holes="fan", smooth="taubin", **KW), data), want)
    small = int(mesh.components().n_faces.min()) + 1
    kept = mesh.remove_small(min_faces=small).fill_holes("fan")
    target = kept.faces.shape[0] // 3
    want = kept.smooth("taubin").simplify(nfaces=target)
    got = _eager(Gen(model, min_component_faces=small, fill_holes="fan", smooth="taubin", simplify_nfaces=target, **KW), data)
    assert _same(got, want) and 0 < got.faces.shape[0] <= target
    assert not _same(want, kept.simplify(nfaces=target).smooth("taubin"))


def test_with_normals(scene):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import NormalMesh
    model, p, Gen = scene
    data = {"inputs": p}
    plain = _eager(Gen(model, with_normals=True, **KW), data)
    got = _eager(Gen(model, with_normals=True, smooth="taubin", **KW), data)
    assert isinstance(plain, NormalMesh) and plain.normals_source == "marching_cubes"
    assert isinstance(got, NormalMesh) and got.normals_source == "geometry" and got.values is None
    assert _same(got, plain.smooth("taubin")) and torch.equal(got.faces, plain.faces)
    assert torch.equal(got.vertex_normals, ops.mesh.normals(got.vertices, got.faces, face=False).vertex_normals)


def test_sharded_route_refuses_and_config_keys_arrive(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    model, p, Gen = scene
    with pytest.raises(VtError, match="sharded"):
        Gen(model, smooth="taubin", **KW).generate_obj_mesh_sharded({"inputs": p})
    for bad in ("nonsense", True, 0):
        with pytest.raises(VtError, match="smooth"):
            Gen(model, smooth=bad, **KW)
    cfg = {"generation": {"resolution_0": NX // 4, "upsampling_steps": 0, "smooth": "humphrey", "smooth_iterations": 6},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.smooth, gen.smooth_iterations) == ("humphrey", 6)
    del cfg["generation"]["smooth"], cfg["generation"]["smooth_iterations"]
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.smooth, gen.smooth_iterations) == (None, 10)
