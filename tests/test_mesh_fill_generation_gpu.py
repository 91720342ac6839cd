"""GPU: Generator3D(fill_holes=..., fill_holes_max_edges=...) on the 32^3 lattice of the golden PointNet + decoder pair
(tests/test_mesh_clean_generation_gpu.py's model).  That scene's own surface already leaves the box -- the default mesh has a loop of 154
edges, which the first test asserts before anything else -- and the field gets two blocks of lattice points at its maximum besides: one
against the x = 0 side of the lattice, which marching cubes cuts open there (a short loop, so that fill_holes_max_edges has two lengths to
tell apart), and a small floater inside the box for the component filter.  None changes nothing, 'fan' is filter -> Mesh.fill_holes -> simplify,
on the eager and the graphed route; with_normals keeps the marching-cubes normals under 'fan' and refuses 'centroid'; the sharded route
refuses; the config keys arrive."""
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


def test_none_is_the_parent_mesh_and_fan_is_filter_fill_simplify(scene):
    model, p, Gen = scene
    data = {"inputs": p}
    bare, none = Gen(model, **KW), Gen(model, fill_holes=None, fill_holes_max_edges=None, **KW)
    mesh = _eager(bare, data)
    loops = mesh.boundary_loops()
    assert loops.offsets.shape[0] - 1 >= 1 and loops.n_irregular == 0, loops        # the cut is there: nothing below passes vacuously
    assert mesh.components().n_components >= 3
    assert _same(_eager(none, data), mesh) and _same(none.generate_mesh_graphed(p), mesh) and _same(bare.generate_mesh_graphed(p), mesh)
    for method in ("fan", "centroid"):
        want = mesh.fill_holes(method)
        assert want.faces.shape[0] > mesh.faces.shape[0] and bool(want.components().watertight.all())
        gen = Gen(model, fill_holes=method, **KW)
        assert _same(_eager(gen, data), want) and _same(gen.generate_mesh_graphed(p), want) and _same(gen.generate_mesh_graphed(p), want)
    # a bound below the shortest loop fills nothing: the mesh as extracted; the shortest length itself fills the loops of that length only
    lens = (loops.offsets[1:] - loops.offsets[:-1]).tolist()
    n = min(lens)
    assert 3 < n < max(lens), lens
    assert _same(_eager(Gen(model, fill_holes="fan", fill_holes_max_edges=n - 1, **KW), data), mesh)
    short = _eager(Gen(model, fill_holes="fan", fill_holes_max_edges=n, **KW), data)
    assert _same(short, mesh.fill_holes("fan", max_edges=n)) and short.faces.shape[0] == mesh.faces.shape[0] + lens.count(n) * (n - 2)
    # the order: component filter, fill, simplify.  The floater is the smallest piece: the filter drops it, the cut piece stays and is closed
    small = int(mesh.components().n_faces.min()) + 1
    kept = mesh.remove_small(min_faces=small)
    want = kept.fill_holes("fan")
    assert kept.faces.shape[0] < mesh.faces.shape[0] and want.faces.shape[0] > kept.faces.shape[0]
    assert _same(_eager(Gen(model, min_component_faces=small, fill_holes="fan", **KW), data), want)
    target = want.faces.shape[0] // 3
    slim = want.simplify(nfaces=target)
    got = _eager(Gen(model, min_component_faces=small, fill_holes="fan", simplify_nfaces=target, **KW), data)
    assert _same(got, slim) and 0 < got.faces.shape[0] <= target


def test_with_normals(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import NormalMesh
    model, p, Gen = scene
    data = {"inputs": p}
    plain = _eager(Gen(model, with_normals=True, **KW), data)
    got = _eager(Gen(model, with_normals=True, fill_holes="fan", **KW), data)
    assert isinstance(got, NormalMesh) and got.normals_source == "marching_cubes"
    assert torch.equal(got.vertices, plain.vertices) and torch.equal(got.vertex_normals, plain.vertex_normals)
    assert torch.equal(got.values, plain.values) and got.faces.shape[0] > plain.faces.shape[0]
    assert torch.equal(got.faces, plain.fill_holes("fan").faces)
    with pytest.raises(VtError, match=r"'fan'.*with_vertex_normals\(\)"):
        Gen(model, with_normals=True, fill_holes="centroid", **KW)
    for bad in ("ear", True, 0):
        with pytest.raises(VtError, match="fill_holes"):
            Gen(model, fill_holes=bad, **KW)
    for bad in (2, 4.0, True):
        with pytest.raises(VtError, match="fill_holes_max_edges"):
            Gen(model, fill_holes="fan", fill_holes_max_edges=bad, **KW)


def test_sharded_route_refuses_and_config_keys_arrive(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    model, p, Gen = scene
    with pytest.raises(VtError, match="sharded"):
        Gen(model, fill_holes="fan", **KW).generate_obj_mesh_sharded({"inputs": p})
    cfg = {"generation": {"resolution_0": NX // 4, "upsampling_steps": 0, "fill_holes": "centroid", "fill_holes_max_edges": 64},
           "test": {"threshold": 0.5}, "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.fill_holes, gen.fill_holes_max_edges) == ("centroid", 64)
    del cfg["generation"]["fill_holes"], cfg["generation"]["fill_holes_max_edges"]
    gen = config.get_generator(model, cfg, DEV)
    assert (gen.fill_holes, gen.fill_holes_max_edges) == (None, None)
