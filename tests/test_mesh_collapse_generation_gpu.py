"""GPU: Generator3D.configure_simplify('collapse') on the 64^3 lattice of the golden PointNet + decoder pair: simplify_nfaces is met by
Mesh.decimate, the largest component stays closed with its Euler number, the default route is untouched bit for bit, the config key
arrives, a bad method raises and the sharded route refuses."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NX = 64
N = 2000
KW = dict(device=DEV, resolution0=NX // 4, padding=0.1)


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
    return model, torch.from_numpy(a["p"])[:1]


def _same(a, b):
    return torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_collapse_keeps_the_largest_component_closed_with_its_euler_number(scene):
    from vtaco_amd.conv_onet.generation import Generator3D
    model, p = scene
    data = {"inputs": p}
    # the cuts where the object reaches the box are capped first (planar loops: exact): the largest component is then closed
    FILL = dict(components="largest", fill_holes="fan", **KW)
    whole = Generator3D(model, **FILL).generate_obj_mesh_wnf(data)
    before = whole.components().report()
    assert whole.faces.shape[0] > 2 * N and before["n_components"] == 1, before
    assert before["watertight"] == [True] and before["n_boundary"] == [0] and before["n_nonmanifold"] == [0] and before["oriented"] == [True], before
    gen = Generator3D(model, simplify_nfaces=N, **FILL).configure_simplify("collapse")
    got = gen.generate_obj_mesh_wnf(data)
    after = got.components().report()
    print(f"collapse: {whole.faces.shape[0]} -> {got.faces.shape[0]} faces, euler {before['euler']} -> {after['euler']}, "
          f"boundary {before['n_boundary']} -> {after['n_boundary']}, watertight {before['watertight']} -> {after['watertight']}")
    assert 0 < got.faces.shape[0] <= N
    # closed stays closed, oriented, one piece, with its Euler number
    assert after["n_components"] == 1 and after["watertight"] == [True] and after["oriented"] == [True], after
    assert after["n_boundary"] == [0] and after["n_nonmanifold"] == [0] and after["euler"] == before["euler"], (before, after)
    want, rep = whole.decimate_report(N)
    assert _same(got, want) and not rep.stalled and got.faces.shape[0] in (N, N - 1)
    assert _same(gen.generate_mesh_graphed(p), want)            # the graphed route: the decimation runs behind the replay
    # clustering at the same count is another mesh
    assert not _same(Generator3D(model, simplify_nfaces=N, **FILL).generate_obj_mesh_wnf(data), want)


def test_the_default_is_clustering_bit_for_bit(scene):
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D
    model, p = scene
    data = {"inputs": p}
    bare = Generator3D(model, simplify_nfaces=N, **KW).generate_obj_mesh_wnf(data)
    named = Generator3D(model, simplify_nfaces=N, **KW).configure_simplify("cluster").generate_obj_mesh_wnf(data)
    want = Generator3D(model, **KW).generate_obj_mesh_wnf(data).simplify(nfaces=N)
    assert _same(bare, named) and _same(bare, want)
    cfg = {"generation": {"resolution_0": NX // 4, "upsampling_steps": 0, "simplify_nfaces": N}, "test": {"threshold": 0.5},
           "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    gen = config.get_generator(model, cfg, DEV)
    assert gen.simplify_method == "cluster" and "simplify_method" not in vars(gen) and _same(gen.generate_obj_mesh_wnf(data), bare)
    cfg["generation"]["simplify_method"] = "collapse"
    gen = config.get_generator(model, cfg, DEV)
    assert gen.simplify_method == "collapse"
    assert _same(gen.generate_obj_mesh_wnf(data), Generator3D(model, **KW).generate_obj_mesh_wnf(data).decimate(N))


def test_bad_method_raises_and_the_sharded_route_refuses(scene):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet import config
    from vtaco_amd.conv_onet.generation import Generator3D
    model, p = scene
    for bad in ("quadric", "Collapse", None, 0):
        with pytest.raises(VtError, match="method"):
            Generator3D(model, **KW).configure_simplify(bad)
    cfg = {"generation": {"resolution_0": NX // 4, "upsampling_steps": 0, "simplify_method": "edge"}, "test": {"threshold": 0.5},
           "data": {"input_type": "pointcloud", "padding": 0.1}, "model": {}}
    with pytest.raises(VtError, match="method"):
        config.get_generator(model, cfg, DEV)
    with pytest.raises(VtError, match="Mesh.decimate"):
        Generator3D(model, simplify_nfaces=N, **KW).configure_simplify("collapse").generate_obj_mesh_sharded({"inputs": p})
    with pytest.raises(VtError, match="Mesh.decimate"):
        Generator3D(model, **KW).configure_simplify("collapse").generate_obj_mesh_sharded({"inputs": p})
