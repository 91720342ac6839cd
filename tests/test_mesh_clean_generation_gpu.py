"""GPU: Generator3D(components=..., min_component_faces=...) on the 32^3 lattice of the golden PointNet + decoder pair
(tests/test_encoder_gpu.py's generator): the defaults change nothing, 'largest' is keep_largest of the unfiltered mesh on the eager and
the graphed route, reference_returns measures the returned mesh, the sharded route refuses.  The field gets a far blob -- a 3^3 block of
lattice points at the field's maximum, in the emptiest corner -- so that the mesh has at least two components."""
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
                v[sl] = values.max()                       # (the default level -- the mean of the extremes -- stays where it was)
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
    corner = min(corners, key=mean)                        # the corner where the field is lowest: far from the object
    return model, p, _blob_generator(corner)


def _eager(gen, data):
    gen.scene_graph = False
    try:
        return gen.generate_obj_mesh_wnf(data)
    finally:
        del gen.scene_graph


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_components_all_is_the_unfiltered_mesh_and_largest_is_keep_largest(scene):
    model, p, Gen = scene
    kw = dict(device=DEV, resolution0=NX // 4, padding=0.1)
    bare, every, biggest = Gen(model, **kw), Gen(model, components="all", **kw), Gen(model, components="largest", **kw)
    data = {"inputs": p}
    mesh_bare, mesh_all = _eager(bare, data), _eager(every, data)
    assert _same(mesh_bare, mesh_all) and mesh_all.faces.shape[0] > 0
    comps = mesh_all.components()
    assert comps.n_components >= 2, comps.report()        # the blob is there: nothing below passes vacuously
    want = mesh_all.keep_largest()
    assert 0 < want.faces.shape[0] < mesh_all.faces.shape[0]
    assert _same(_eager(biggest, data), want)
    # the graphed route: the filter runs behind the replay
    g_bare, g_all, g_big = bare.generate_mesh_graphed(p), every.generate_mesh_graphed(p), biggest.generate_mesh_graphed(p)
    assert _same(g_bare, mesh_bare) and _same(g_all, mesh_bare) and _same(g_big, want)
    assert _same(biggest.generate_mesh_graphed(p), want)
    for by, name in (("area", "largest_area"), ("volume", "largest_volume")):
        assert _same(_eager(Gen(model, components=name, **kw), data), mesh_all.keep_largest(by=by)), name
    # min_component_faces alone drops the components below it
    n_faces = comps.n_faces.cpu().tolist()
    bound = sorted(n_faces)[-1]
    kept = _eager(Gen(model, min_component_faces=bound, **kw), data)
    assert _same(kept, mesh_all.remove_small(min_faces=bound)) and kept.faces.shape[0] == sum(n for n in n_faces if n >= bound)


def test_reference_returns_measures_the_returned_mesh(scene):
    model, p, Gen = scene
    gen = Gen(model, device=DEV, resolution0=NX // 4, padding=0.1, components="largest", reference_returns=True)
    every = Gen(model, device=DEV, resolution0=NX // 4, padding=0.1)
    gen.scene_graph = every.scene_graph = False
    whole = every.generate_obj_mesh_wnf({"inputs": p})
    # the target: the unfiltered mesh's own vertices, slightly moved -- at least as many as the returned mesh has (chamfer_distance's
    # truncation rule), and near the returned ones, which keeps the EMD's auction short (the cloud itself took it 24 s)
    g = torch.Generator().manual_seed(3)
    target = (whole.vertices.cpu() + 0.003 * torch.randn(whole.vertices.shape, generator=g))[None]
    data = {"inputs": p, "points.points_obj": target}
    np.random.seed(7)
    mesh, emd, cd = gen.generate_obj_mesh_wnf(data)
    np.random.seed(7)
    emd2, cd2 = gen.reference_metrics(mesh, data)
    assert (emd, cd) == (emd2, cd2) and np.isfinite(emd) and np.isfinite(cd)
    assert 0 < mesh.faces.shape[0] < whole.faces.shape[0]
    np.random.seed(7)
    assert (emd, cd) != every.reference_metrics(whole, data)           # (the unfiltered mesh measures differently)


def test_sharded_route_refuses_a_component_filter(scene):
    from vtaco_amd._lib import VtError
    model, p, Gen = scene
    for kw in ({"components": "largest"}, {"min_component_faces": 10}):
        with pytest.raises(VtError, match="sharded"):
            Gen(model, device=DEV, resolution0=NX // 4, padding=0.1, **kw).generate_obj_mesh_sharded({"inputs": p})
    mesh = Gen(model, device=DEV, resolution0=NX // 4, padding=0.1).generate_obj_mesh_sharded({"inputs": p})
    assert mesh.faces.shape[0] > 0
