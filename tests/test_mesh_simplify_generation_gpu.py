"""GPU: Generator3D(simplify_nfaces=...) on the 32^3 lattice of the golden PointNet + decoder pair, with the far blob of
tests/test_mesh_clean_generation_gpu.py (two components at least): None changes nothing, N is Mesh.simplify(nfaces=N) of the
unsimplified result on the eager and the graphed route, the component filter runs first, reference_returns measures the simplified
mesh, the sharded route refuses, the config key arrives, a bad value raises."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX = 32
N = 500


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


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_none_is_the_mesh_as_before_and_n_is_mesh_simplify(scene):
    model, p, Gen = scene
    bare, none, small = Gen(model, **KW), Gen(model, simplify_nfaces=None, **KW), Gen(model, simplify_nfaces=N, **KW)
    data = {"inputs": p}
    whole = _eager(bare, data)
    assert whole.faces.shape[0] > 2 * N                      # there is something to simplify
    assert _same(_eager(none, data), whole) and _same(none.generate_mesh_graphed(p), whole)
    want, rep = whole.simplify_report(nfaces=N)
    assert N / 2 <= want.faces.shape[0] <= N and rep.probes >= 1 and want.vertices.shape[0] == rep.n_clusters
    got = _eager(small, data)
    assert got.faces.shape[0] <= N and _same(got, want)
    # the graphed route: the simplification runs behind the replay
    assert _same(small.generate_mesh_graphed(p), want) and _same(small.generate_mesh_graphed(p), want)
    # a target the mesh meets already returns it as it is
    assert _same(_eager(Gen(model, simplify_nfaces=whole.faces.shape[0], **KW), data), whole)


def test_the_component_filter_runs_first(scene):
    model, p, Gen = scene
    data = {"inputs": p}
    whole = _eager(Gen(model, **KW), data)
    assert whole.components().n_components >= 2
    biggest = whole.keep_largest()
    want = biggest.simplify(nfaces=N)
    got = _eager(Gen(model, components="largest", simplify_nfaces=N, **KW), data)
    assert _same(got, want) and got.faces.shape[0] <= N
    assert not _same(want, whole.simplify(nfaces=N))         # (the other order, or no filter, is another mesh)
    assert _same(Gen(model, components="largest", simplify_nfaces=N, **KW).generate_mesh_graphed(p), want)


def test_reference_returns_measures_the_simplified_mesh(scene):
    model, p, Gen = scene
    gen = Gen(model, simplify_nfaces=N, reference_returns=True, **KW)
    every = Gen(model, **KW)
    gen.scene_graph = every.scene_graph = False
    whole = every.generate_obj_mesh_wnf({"inputs": p})
    want = whole.simplify(nfaces=N)
    # the target: the simplified mesh's own vertices, slightly moved -- as many as the returned mesh has (chamfer_distance's truncation
    # rule), and near them, which keeps the EMD's auction short
    g = torch.Generator().manual_seed(3)
    target = (want.vertices.cpu() + 0.003 * torch.randn(want.vertices.shape, generator=g))[None]
    data = {"inputs": p, "points.points_obj": target}
    np.random.seed(7)
    mesh, emd, cd = gen.generate_obj_mesh_wnf(data)
    np.random.seed(7)
    assert (emd, cd) == gen.reference_metrics(mesh, data) and np.isfinite(emd) and np.isfinite(cd)
    assert mesh.faces.shape[0] <= N and _same(mesh, want)


def test_sharded_route_config_key_and_bad_values(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    model, p, Gen = scene
    with pytest.raises(VtError, match="Mesh.simplify"):
        Gen(model, simplify_nfaces=N, **KW).generate_obj_mesh_sharded({"inputs": p})
    cfg = {"generation": {"resolution_0": NX // 4, "upsampling_steps": 0, "simplify_nfaces": N}, "test": {"threshold": 0.5},
           "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, DEV)
    assert gen.simplify_nfaces == N
    mesh = gen.generate_obj_mesh_wnf({"inputs": p})
    assert 0 < mesh.faces.shape[0] <= N
    del cfg["generation"]["simplify_nfaces"]
    assert config.get_generator(model, cfg, DEV).simplify_nfaces is None
    for bad in (0, -1, 1.5, "500", True):
        with pytest.raises(VtError, match="simplify_nfaces"):
            Gen(model, simplify_nfaces=bad, **KW)
