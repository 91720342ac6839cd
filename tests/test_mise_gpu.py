"""GPU: multiresolution isosurface extraction (vtaco_amd/mise.py, csrc/mise.hip) and Generator3D(extraction="mise").

Against the reference's MultiGridExtractor (g22_mise.npz); on the shipped scene (BASELINE config 2) against the dense n^3
field decoded through the same point path; on the two tactile routes; and the configurations it refuses."""
import os

import numpy as np
import pytest
import torch

import config2_case as c2
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOX = 1.1


def lattice(n):
    from vtaco_amd.common import make_3d_grid
    return BOX * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def triangles(mesh):
    """The mesh's triangles as a set of byte strings of their three vertices' coordinates."""
    v, f = mesh[0], mesh[1]
    if f.shape[0] == 0:
        return set()
    tri = v[f.long()].reshape(-1, 9).contiguous().cpu().numpy()
    return set(map(bytes, tri))


def check_against_dense(values, known, prev, dense, level, what):
    """Known entries = the dense field bit for bit; the others = their nearest-coarse fill from the previous level.  The meshes: a
    marching-cubes vertex depends on the two values of its edge (on the cell's eight for a centre vertex), so every vertex of the
    MISE mesh whose values are all known is a vertex of the dense field's mesh, bit for bit.  Vertices on an edge with a filled end
    (the rim of the refined band, where a coarse cell was judged empty but its refined neighbour is not) are not, and the dense mesh's
    parts in cells the coarse levels judged empty are missing.  Returns (MISE vertices, those not in the dense mesh, dense vertices
    not in the MISE mesh)."""
    from vtaco_amd import ops
    n = values.shape[0]
    k = known.bool()
    assert torch.equal(bits(values[k]), bits(dense.reshape(n, n, n)[k])), what
    idx = torch.arange(n, device=values.device) // 2
    fill = prev[idx][:, idx][:, :, idx]
    assert torch.equal(bits(values[~k]), bits(fill[~k])), what
    vm = ops.marching_cubes(values, level)[0]                              # index space: the edge / cell of a vertex is exact
    vd = ops.marching_cubes(dense.reshape(n, n, n).contiguous(), level)[0]
    dset = set(map(bytes, vd.cpu().numpy()))
    mrows = vm.cpu().numpy()
    mset = set(map(bytes, mrows))
    extra = torch.tensor([i for i, r in enumerate(mrows) if bytes(r) not in dset], dtype=torch.long)
    if extra.numel():
        v = vm[extra.to(vm.device)].double()
        lo = torch.floor(v).long().clamp(0, n - 1)
        frac = (v != torch.floor(v)).sum(dim=1)
        all_known = torch.ones(v.shape[0], dtype=torch.bool, device=v.device)
        for d in range(8):                                                  # the cell's 8 corners (an edge's 2 are among them)
            off = torch.tensor([(d >> 2) & 1, (d >> 1) & 1, d & 1], device=v.device)
            c = (lo + off).clamp(max=n - 1)
            on = torch.where(frac[:, None] >= 2, torch.ones_like(off)[None].expand_as(c) > 0, (off[None] == 0) | (v != torch.floor(v)))
            corner_known = k[c[:, 0], c[:, 1], c[:, 2]]
            all_known &= ~on.all(dim=1) | corner_known
        assert not bool(all_known.any()), (what, int(all_known.sum()))
    missed = sum(1 for r in vd.cpu().numpy() if bytes(r) not in mset)
    return len(mrows), int(extra.numel()), missed


# -- 1: the reference's own extractor -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "needle", "noisy"))
def test_extract_reproduces_the_reference_multigrid_extractor(name):
    from vtaco_amd import mise, ops
    z = np.load(os.path.join(GOLDEN, "g22_mise.npz"))
    r0, steps = (int(v) for v in z[f"{name}.r0_steps"])
    table = torch.from_numpy(z[f"{name}.table"]).to(DEV)
    n = table.shape[0]
    seen = []

    def evaluate(ids, pts):
        nk = round(ids_level_n[0])
        s = (n - 1) // (nk - 1)
        i = ids.long()
        x, y, zz = i // (nk * nk), (i // nk) % nk, i % nk
        _, ref_pts = ops.mise_lattice(nk, BOX, DEV, want_ids=False)
        assert torch.equal(bits(pts), bits(ref_pts[i]))                   # the coordinates are the lattice's
        seen.append(torch.sort(ids)[0].cpu().numpy())
        ids_level_n[0] = 2 * nk - 1
        return table[x * s, y * s, zz * s]
    ids_level_n = [r0 + 1]
    values, known, per_level = mise.extract(evaluate, r0, steps, 0.0, BOX, DEV)
    assert per_level == [len(z[f"{name}.q{k}"]) for k in range(steps + 1)]
    for k, q in enumerate(seen):
        assert np.array_equal(q, z[f"{name}.q{k}"]), (name, k)
    assert np.array_equal(known.cpu().numpy(), z[f"{name}.known"])
    assert np.array_equal(values.cpu().numpy().view(np.uint32), z[f"{name}.values"].view(np.uint32))


def test_coarse_and_fine_lattice_points_coincide():
    from vtaco_amd import ops
    for nc in (5, 33, 129, 257):
        _, pc = ops.mise_lattice(nc, BOX, DEV, want_ids=False)
        _, pf = ops.mise_lattice(2 * nc - 1, BOX, DEV, want_ids=False)
        nf = 2 * nc - 1
        i = torch.arange(nc, device=DEV) * 2
        even = ((i[:, None, None] * nf + i[None, :, None]) * nf + i[None, None, :]).reshape(-1)
        assert torch.equal(bits(pc), bits(pf[even])), nc
    _, p = ops.mise_lattice(65, BOX, DEV, want_ids=False)
    assert torch.equal(bits(p), bits(lattice(65).to(DEV)))                  # and they are make_3d_grid's


# -- 2: the shipped scene ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    z = c2.fixture()
    enc, dec = c2.models(z)
    model = ConvolutionalOccupancyNetwork(dec, enc, device=DEV).eval()
    cloud = torch.from_numpy(z["cloud"]).float()
    return model, cloud


@pytest.mark.parametrize("precision", ("f32", "f16x3"))
@pytest.mark.parametrize("r0,steps", [(32, 2), (16, 4)])
def test_shipped_scene_known_entries_are_the_dense_field(scene, precision, r0, steps):
    from vtaco_amd import mise
    from vtaco_amd.conv_onet.generation import Generator3D
    model, cloud = scene
    gen = Generator3D(model, device=DEV, resolution0=r0, upsampling_steps=steps, extraction="mise", decode_precision=precision)
    n = mise.size(r0, steps)
    mesh = gen.generate_obj_mesh_wnf({"inputs": cloud})
    per_level = gen.mise_points_per_level
    with torch.no_grad():
        c = model.encode_inputs(cloud.to(DEV))
        evaluate = gen.mise_evaluator(c)
        values, known, again = mise.extract(evaluate, r0, steps, 0.0, BOX, DEV)
        prev, _, _ = mise.extract(evaluate, r0, steps - 1, 0.0, BOX, DEV)
        dense = evaluate(None, lattice(n).to(DEV))
        lat = gen.eval_lattice(c, n)
    assert again == per_level
    from vtaco_amd import ops
    own = ops.marching_cubes(values, 0.0, rescale=((n - 1) / 2, BOX / (n - 1)))
    assert torch.equal(mesh.vertices, own[0]) and torch.equal(mesh.faces, own[1])     # the generator's mesh is the extraction's
    if precision == "f32":
        assert torch.equal(bits(dense), bits(lat))                          # the point path is the lattice decode, bit for bit
    else:
        assert float((dense - lat).abs().max()) <= 1e-4                      # f16x3 contract; measured: DESIGN.md (MISE section)
    verts, extra, missed = check_against_dense(values, known, prev, dense, 0.0, (precision, r0, steps))
    assert verts > 10000 and extra < 0.1 * verts and missed < 0.2 * verts, (verts, extra, missed)
    print(f"MISE {precision} n={n}: {verts} vertices, {extra} not in the dense mesh, {missed} dense vertices missed")
    if n == 257:
        assert sum(per_level) < n ** 3 / 2


# -- 3: the tactile routes ----------------------------------------------------------------------------------------------------------
def _tactile_check(gen, data, r0, steps):
    from vtaco_amd import mise, ops
    mesh = gen.generate_obj_mesh_wnf(data)
    n = mise.size(r0, steps)
    c, setup = gen._tactile_encode(data)
    with torch.no_grad():
        evaluate = gen.mise_evaluator(c, setup)
        values, known, _ = mise.extract(evaluate, r0, steps, 0.0, BOX, DEV)
        prev, _, _ = mise.extract(evaluate, r0, steps - 1, 0.0, BOX, DEV)
        pts = lattice(n).to(DEV)[None]
        ids = ops.tactile_assign(setup['anchors'].to(DEV), setup['success'].to(DEV), setup['mode'], setup['radius'], pts=pts,
                                 count=setup['count'].to(DEV))
        dec = gen.model.decoder
        dense = ops.decode_fwd_ids(c['grid'], dec._blob(img=True, precision="f32"), ids, setup['feats'].to(DEV), pts=pts,
                                   padding=dec.padding, precision="f32").reshape(-1)
    assert int((ids != 255).sum()) > 0                                      # some points carry a finger's feature
    own = ops.marching_cubes(values, 0.0, rescale=((n - 1) / 2, BOX / (n - 1)))
    assert torch.equal(mesh.vertices, own[0]) and torch.equal(mesh.faces, own[1])
    return check_against_dense(values, known, prev, dense, 0.0, "tactile")


def test_vtaco_t2d_route(tmp_path):
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    from vtaco_amd.encoder import encoder_dict
    z = np.load(os.path.join(GOLDEN, "g12_t2d.npz"))
    torch.manual_seed(3)
    dec = decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32)
    enc = encoder_dict["pointnet_local_pool"](c_dim=32, dim=3, hidden_dim=32, grid_resolution=16, plane_type="grid", unet3d=False)
    for blk in list(dec.blocks) + list(enc.blocks):
        torch.nn.init.normal_(blk.fc_1.weight, 0, 0.1)
    img = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=2, start_filts=8)
    model = ConvolutionalOccupancyNetwork(dec, enc, None, img, None, device=DEV)
    g = torch.Generator().manual_seed(4)
    d = torch.randn(1, 3000, 3, generator=g)
    data = {"inputs": 0.3 * d / d.norm(dim=-1, keepdim=True), "inputs.img": torch.rand(1, 5, 3, 8, 4, generator=g),
            "inputs.depth": torch.from_numpy(z["depths"])[None], "inputs.touch_success": torch.from_numpy(z["touch"]),
            "inputs.pc_ply": torch.from_numpy(z["pc_ply"]), "points.cam_pos": torch.from_numpy(z["cam_pos"]),
            "points.cam_rot": torch.from_numpy(z["cam_rot"])}
    gen = Generator3D(model, device=DEV, resolution0=16, upsampling_steps=3, padding=0.1, with_img=True, encode_t2d=True,
                      decode_precision="f32", depth_origin=z["depth_origin"], extraction="mise")
    state = np.random.get_state()
    try:
        np.random.seed(int(z["seed"]))       # the contact clouds are drawn with numpy's generator: the same draw for every call
        verts, _, _ = _tactile_check(gen, _Reseed(data, int(z["seed"])), 16, 3)
    finally:
        np.random.set_state(state)
    assert verts > 100


class _Reseed(dict):
    """The scene's data; every read of the depth images reseeds numpy's generator, so that the route's contact-cloud draw (numpy)
    is the same in the generator's call and in the test's own."""
    def __init__(self, data, seed):
        super().__init__(data)
        self.seed = seed

    def get(self, key, default=None):
        if key == "inputs.depth":
            np.random.seed(self.seed)
        return super().get(key, default)


def test_vtacoh_route(tmp_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import synth_mano
    from synth_dataset import make_cfg, make_synthetic_dataset
    from test_hand_gpu import MANO_KW
    from vtaco_amd import data as vdata
    from vtaco_amd.common import fingertips_in_object_frame
    from vtaco_amd.config import get_dataset
    from vtaco_amd.conv_onet import config as cfgmod
    os.makedirs(tmp_path / "ds")
    make_synthetic_dataset(str(tmp_path / "ds"), seed=7)
    synth_mano.write_pkl(synth_mano.make_asset(0), str(tmp_path / "mano"))
    cfg = make_cfg(str(tmp_path / "ds"), points_subsample=64)
    cfg["model"] = {"decoder": "simple_local", "encoder": "pointnet_local_pool", "c_dim": 32, "with_img": True,
                    "decoder_kwargs": {"sample_mode": "bilinear", "hidden_size": 32},
                    "encoder_kwargs": {"hidden_dim": 32, "plane_type": "grid", "grid_resolution": 16, "unet3d": False},
                    "encoder_hand": "pointnet_local_pool",
                    "encoder_hand_kwargs": {"hidden_dim": 32, "plane_type": ["xz", "xy", "yz"], "plane_resolution": 32,
                                            "unet": False, "out_mano": True, "out_dim": 51,
                                            "manolayer_kwargs": dict(MANO_KW, mano_root=str(tmp_path / "mano"))},
                    "encoder_img": "UNet", "encoder_img_kwargs": {"num_classes": 1, "in_channels": 3, "depth": 2, "start_filts": 8}}
    cfg["test"] = {"threshold": 0.5}
    cfg["generation"] = {"resolution_0": 16, "upsampling_steps": 3, "extraction": "mise"}
    torch.manual_seed(1)
    model = cfgmod.get_model(cfg, device=DEV)
    for blk in list(model.decoder.blocks) + list(model.encoder.blocks):
        torch.nn.init.normal_(blk.fc_1.weight, 0, 0.1)
    gen = cfgmod.get_generator(model, cfg, DEV)
    assert gen.extraction == "mise"
    gen.decode_precision = "f32"
    batch = next(iter(torch.utils.data.DataLoader(get_dataset("test", cfg), batch_size=1, collate_fn=vdata.collate_remove_none)))
    batch["inputs.img"] = torch.nn.functional.interpolate(batch["inputs.img"].flatten(0, 1), size=(8, 4)).unflatten(0, (1, 5))
    batch["inputs.touch_success"] = torch.tensor([[True, False, True, True, True]])
    with torch.no_grad():
        joints = model.encode_hand_inputs(batch["inputs"].to(DEV))["mano_joints"].cpu().numpy()
    cloud = batch["inputs.pc_ply"][0].numpy()
    m = np.max(np.sqrt(np.sum((cloud - cloud.mean(0)) ** 2, axis=1)))
    tips0 = fingertips_in_object_frame(joints, np.zeros((1, 3)), batch["points.wrist"].numpy(), batch["inputs.pc_ply"].numpy())
    batch["points.mano"][0, :3] = torch.from_numpy(-tips0[0, 0] * 2 * m).float()       # the first fingertip at the lattice centre
    verts, _, _ = _tactile_check(gen, batch, 16, 3)
    assert verts > 100


# -- 4, 5, 6 ----------------------------------------------------------------------------------------------------------------------
def test_no_upsampling_is_the_dense_lattice_mesh(scene):
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.generation import Generator3D
    model, cloud = scene
    for precision in ("f32", "f16x3"):
        gen = Generator3D(model, device=DEV, resolution0=32, upsampling_steps=0, extraction="mise", decode_precision=precision)
        mesh = gen.generate_obj_mesh_wnf({"inputs": cloud})
        with torch.no_grad():
            c = model.encode_inputs(cloud.to(DEV))
            vals = gen.mise_evaluator(c)(None, lattice(33).to(DEV)).reshape(33, 33, 33)
            if precision == "f32":                                          # ... which is the lattice decode's field
                assert torch.equal(bits(vals.reshape(-1)), bits(gen.eval_lattice(c, 33)))
        ref = ops.marching_cubes(vals, 0.0, rescale=(16.0, BOX / 32))
        assert torch.equal(mesh.vertices, ref[0]) and torch.equal(mesh.faces, ref[1]), precision
        assert gen.mise_points_per_level == [33 ** 3]


def test_reference_returns_under_mise(scene):
    from vtaco_amd.conv_onet.generation import Generator3D
    model, cloud = scene
    gen = Generator3D(model, device=DEV, resolution0=16, upsampling_steps=2, extraction="mise", reference_returns=True)
    g = torch.Generator().manual_seed(9)
    mesh, emd, cd = gen.generate_obj_mesh_wnf({"inputs": cloud, "points.points_obj": 0.3 * torch.rand(1, 2048, 3, generator=g) - 0.15})
    assert mesh.faces.shape[0] > 0 and np.isfinite(emd) and np.isfinite(cd)


def test_refused_configurations(scene):
    from vtaco_amd import mise
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    model, cloud = scene
    with pytest.raises(VtError):
        Generator3D(model, device=DEV, extraction="sparse")
    att = ConvolutionalOccupancyNetwork(decoder_dict["attention_local"](dim=3, c_dim=32, hidden_size=32), model.encoder, device=DEV)
    with pytest.raises(VtError, match="attention"):
        Generator3D(att, device=DEV, extraction="mise")
    gen = Generator3D(model, device=DEV, resolution0=16, upsampling_steps=1, extraction="mise")
    with pytest.raises(VtError, match="c_img_all"):
        gen.generate_obj_mesh_wnf({"inputs": cloud}, c_img_all=torch.zeros(1, 32 ** 3, 32, device=DEV))
    with pytest.raises(VtError, match="dense extraction only"):
        gen.generate_obj_mesh_sharded({"inputs": cloud})
    with pytest.raises(VtError, match="dense extraction only"):
        gen.generate_mesh_graphed(cloud)
    with pytest.raises(VtError, match="513"):
        Generator3D(model, device=DEV, resolution0=64, upsampling_steps=4, extraction="mise").generate_obj_mesh_wnf({"inputs": cloud})
    with pytest.raises(VtError):
        mise.extract(lambda i, p: torch.zeros(3, device=DEV), 8, 1, 0.0, BOX, DEV)        # evaluate must return one logit per point
