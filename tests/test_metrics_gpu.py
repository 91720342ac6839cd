"""GPU: the visualise block's metrics on the device -- vt_chamfer_nn (nearest neighbours, bit for bit against numpy's f32
restatement) and vt_emd_auction (the optimal assignment of cdist + linear_sum_assignment) against the reference's own results
(g21) and scipy -- and Generator3D(reference_returns=True) running the reference's visualise block (train.py:243-256)."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy


def nn_numpy(a, b):
    """Squared distances (dx*dx + dy*dy) + dz*dz in float32, their minima over b for every point of a, the minima's multiplicity."""
    d = a[:, None, :] - b[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    m = d2.min(axis=1)
    return d2, m, (d2 == m[:, None]).sum(axis=1)


def check_nn(a, b, d_ab, i_ab, d_ba, i_ba):
    for x, y, d, i in ((a, b, d_ab, i_ab), (b, a, d_ba, i_ba)):
        d2, m, mult = nn_numpy(x, y)
        assert d2.dtype == np.float32
        assert np.array_equal(d.view(np.uint32), m.view(np.uint32))           # bit for bit
        unique = mult == 1
        assert np.array_equal(i[unique], d2.argmin(axis=1)[unique])
        assert np.all(d2[np.arange(len(x)), i] == m)                          # ties: an index that attains the minimum ...
        assert np.array_equal(i, d2.argmin(axis=1))                           # ... the smallest (argmin's first)


def test_chamfer_nn_bit_exact_on_g21_and_random_batches():
    from vtaco_amd import eval as veval, ops
    z, _ = load_golden("g21_metrics.npz")
    for case in z["cases"]:
        a, b = z[f"{case}.a"], z[f"{case}.b"]
        ta, tb = T(a)[None].to(DEV), T(b)[None].to(DEV)
        d_ab, i_ab, d_ba, i_ba = (t[0].cpu().numpy() for t in ops.chamfer_nn(ta, tb))
        check_nn(a, b, d_ab, i_ab, d_ba, i_ba)
        cd = float(veval.chamfer_distance_device(ta, tb)[0])
        assert abs(cd - float(z[f"{case}.cd"])) <= 1e-6 * abs(float(z[f"{case}.cd"])), case
        naive = float(veval.chamfer_distance_naive(ta, tb)[0])
        assert abs(cd - naive) <= 1e-6 * abs(naive), case
    rng = np.random.RandomState(5)
    for N, M in ((700, 1300), (1025, 3), (1, 257)):
        a = (rng.randn(3, N, 3) * 0.2).astype(np.float32)
        b = (rng.randn(3, M, 3) * 0.2).astype(np.float32)
        b[:, ::7] = np.round(b[:, ::7] * 8) / 8                               # repeated points: ties
        a[:, ::5] = np.round(a[:, ::5] * 8) / 8
        out = [t.cpu().numpy() for t in ops.chamfer_nn(T(a).to(DEV), T(b).to(DEV))]
        for k in range(3):
            check_nn(a[k], b[k], *(o[k] for o in out))


def test_chamfer_device_truncation_rule_and_ids():
    from vtaco_amd import eval as veval
    from vtaco_amd._lib import VtError
    rng = np.random.RandomState(6)
    p1 = T(rng.randn(2, 2048, 3).astype(np.float32)).to(DEV)
    p2 = T(rng.randn(2, 1500, 3).astype(np.float32)).to(DEV)
    cd, i12, i21 = veval.chamfer_distance_device(p1, p2, give_id=True)       # p1 cut to 1500 points, as the reference does
    ref = veval.chamfer_distance_naive(p1, p2)
    assert float((cd - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    assert i12.shape == (2, 1500) and i12.dtype == torch.int64 and i21.shape == (2, 1500)
    with pytest.raises(VtError):
        veval.chamfer_distance_device(p1[:, :1000], p2)                       # fewer points1 than points2: sizes differ


def check_emd(a, b, res, k, emd_scipy, eps):
    """The auction's result for problem k: a permutation of the padded problem, within the bars of scipy's optimum, and
    eps-complementary slackness of the returned prices checked in float64."""
    N, M = len(a), len(b)
    n = max(N, M)
    assign = res.assign[k].cpu().numpy().astype(np.int64)
    prices = res.prices[k].cpu().numpy().astype(np.float64)
    assert np.array_equal(np.sort(assign), np.arange(n))
    emd = float(res.emd[k])
    assert emd >= emd_scipy - 1e-9
    assert emd <= emd_scipy * (1 + 1e-4) + 1e-6, (emd, emd_scipy)
    cost = np.zeros((n, n))
    cost[:N, :M] = np.sqrt((((a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64)) ** 2)).sum(-1))
    value = cost + prices[None, :]
    assert np.all(value[np.arange(n), assign] <= value.min(axis=1) + 2 * eps)
    # the f64 cost the kernel reports is the assignment's, as cdist evaluates it
    rows = np.arange(N)
    keep = assign[:N] < M
    assert abs(emd - cost[rows[keep], assign[:N][keep]].sum() / N) <= 1e-12 * max(1.0, emd)


def test_emd_auction_g21_against_the_reference():
    from vtaco_amd import ops
    z, _ = load_golden("g21_metrics.npz")
    for case in z["cases"]:
        a, b = z[f"{case}.a"], z[f"{case}.b"]
        ta, tb = T(a)[None].to(DEV), T(b)[None].to(DEV)
        res = ops.emd_assignment(ta, tb)
        check_emd(a, b, res, 0, float(z[f"{case}.emd"]), ops.EMD_EPS_FINAL)
        assert abs(float(z[f"{case}.cost"]) / len(a) - float(z[f"{case}.emd"])) <= 1e-12
        again = ops.emd_assignment(ta, tb)
        assert torch.equal(again.assign, res.assign) and torch.equal(again.prices, res.prices)
        print(f"{case}: emd {float(res.emd[0]):.9g} (reference {float(z[f'{case}.emd']):.9g}), rounds {int(res.rounds[0])}, "
              f"bids {int(res.bids[0])}, phases {int(res.phases[0])}")


def test_emd_auction_batch_of_eight():
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial import distance
    from vtaco_amd import eval as veval, ops
    rng = np.random.RandomState(8)
    N, M = 1024, 900
    a = (rng.randn(8, N, 3) * 0.1).astype(np.float32)
    b = np.concatenate([(rng.randn(4, M, 3) * 0.1 + 0.01).astype(np.float32),
                        rng.uniform(-0.5, 0.5, (4, M, 3)).astype(np.float32)])
    ta, tb = T(a).to(DEV), T(b).to(DEV)
    res = ops.emd_assignment(ta, tb)
    for k in range(8):
        d = distance.cdist(a[k], b[k])
        check_emd(a[k], b[k], res, k, d[linear_sum_assignment(d)].sum() / len(d), ops.EMD_EPS_FINAL)
    again = ops.emd_assignment(ta, tb)
    assert torch.equal(again.assign, res.assign)
    # one problem of the batch alone gives the same assignment as inside the batch
    single = ops.emd_assignment(ta[5:6].contiguous(), tb[5:6].contiguous())
    assert torch.equal(single.assign[0], res.assign[5])
    emd, full = veval.earth_mover_distance_device(a[3], b[3], return_assignment=True)
    assert emd == float(res.emd[3]) and torch.equal(full.assign[0], res.assign[3])
    # persons fewer than objects: dummy persons pad the rows
    d = distance.cdist(b[6][:700], a[6])
    res2 = ops.emd_assignment(tb[6:7, :700].contiguous(), ta[6:7].contiguous())
    check_emd(b[6][:700], a[6], res2, 0, d[linear_sum_assignment(d)].sum() / len(d), ops.EMD_EPS_FINAL)


def test_emd_auction_limits_raise():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    rng = np.random.RandomState(9)
    big = T(rng.randn(1, ops.EMD_MAX_POINTS + 1, 3).astype(np.float32)).to(DEV)
    small = T(rng.randn(1, 64, 3).astype(np.float32)).to(DEV)
    with pytest.raises(VtError):
        ops.emd_assignment(big, small)
    with pytest.raises(VtError):
        ops.emd_assignment(small, big)
    # a round cap too small to finish: the kernel stops and reports, the host raises (no loop, no host fallback)
    with pytest.raises(VtError, match="did not finish"):
        ops.emd_assignment(small, T(rng.randn(1, 64, 3).astype(np.float32)).to(DEV), max_rounds=2)
    with pytest.raises(VtError):
        ops.emd_assignment(small.cpu(), small.cpu())
    # the largest size the kernel covers runs
    top = T((rng.randn(1, ops.EMD_MAX_POINTS, 3) * 0.1).astype(np.float32)).to(DEV)
    res = ops.emd_assignment(top, (top + 0.01 * torch.randn_like(top)).contiguous())
    assert np.array_equal(np.sort(res.assign[0].cpu().numpy()), np.arange(ops.EMD_MAX_POINTS))


# ---- the reference's visualise block ---------------------------------------------------------------------------------------
def host_metrics(mesh, points_obj, seed):
    """The reference's metric block (generation.py:274-284) on the host, from the generator's vertices."""
    from vtaco_amd import eval as veval
    vertices = mesh.vertices.cpu().numpy().astype(np.float32)
    np.random.seed(seed)
    np.random.shuffle(vertices)
    vertices = np.ascontiguousarray(vertices[:2048], dtype=np.float32)
    cd = veval.chamfer_distance_naive(points_obj, torch.FloatTensor(vertices[None])).item()
    emd = veval.earth_mover_distance(np.array(points_obj[0]), vertices)
    return emd, cd


def read_off(path):
    with open(path) as f:
        assert f.readline().strip() == "OFF"
        V, F, _ = map(int, f.readline().split())
        rows = [f.readline() for _ in range(V + F)]
    v = np.array([list(map(float, r.split())) for r in rows[:V]]).reshape(-1, 3)
    faces = np.array([list(map(int, r.split()))[1:] for r in rows[V:]], dtype=np.int64).reshape(-1, 3)
    return v, faces


def visualise(generator, data_vis_list, out_dir, it, seed):
    """train.py:243-256, restated (the reference's loop body), with numpy's generator seeded per scene."""
    emd_total, cd_total = [], []
    for data_vis in data_vis_list:
        mesh_hand = generator.generate_hand_mesh(data_vis['data']) if data_vis.get('hand', True) else None
        np.random.seed(seed)
        mesh_obj, emd, cd = generator.generate_obj_mesh_wnf(data_vis['data'])
        emd_total.append(emd)
        cd_total.append(cd)
        if mesh_hand is not None:
            mesh_hand.export(os.path.join(out_dir, 'vis', '{}_{}_hand.off'.format(it, data_vis['name'])))
        mesh_obj.export(os.path.join(out_dir, 'vis', '{}_{}_obj.off'.format(it, data_vis['name'])))
    print("Metrics EMD: {}".format(np.mean(emd_total)))
    print("Metrics CD: {}".format(np.mean(cd_total)))
    return mesh_hand, mesh_obj, emd_total, cd_total


def check_block(gen, data, name, tmp_path, hand, seed=1234):
    from vtaco_amd.conv_onet.generation import Mesh
    os.makedirs(tmp_path / "vis", exist_ok=True)
    mesh_hand, mesh_obj, emds, cds = visualise(gen, [{'data': data, 'name': name, 'hand': hand}], str(tmp_path), 100, seed)
    assert isinstance(mesh_obj, Mesh) and mesh_obj.vertices.shape[0] > 0
    assert isinstance(emds[0], float) and isinstance(cds[0], float)
    v, f = read_off(tmp_path / "vis" / f"100_{name}_obj.off")
    assert np.array_equal(v.astype(np.float32), mesh_obj.vertices.cpu().numpy()) and np.array_equal(f, mesh_obj.faces.cpu().numpy())
    if hand:
        v, f = read_off(tmp_path / "vis" / f"100_{name}_hand.off")
        assert np.array_equal(v, mesh_hand.vertices.cpu().numpy()) and np.array_equal(f, mesh_hand.faces.cpu().numpy())
    emd_host, cd_host = host_metrics(mesh_obj, data['points.points_obj'], seed)
    assert emds[0] >= emd_host - 1e-9 and emds[0] <= emd_host * (1 + 1e-4) + 1e-6, (emds[0], emd_host)
    assert abs(cds[0] - cd_host) <= 1e-6 * abs(cd_host), (cds[0], cd_host)
    return mesh_obj


def test_visualise_block_visual_route(tmp_path):
    """The visual branch (eager first call, captured scene graph on the second): the object half of the block -- this small model has
    no hand encoder -- runs as written with reference_returns=True; with the flag off the return is the bare Mesh."""
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    from vtaco_amd.encoder import encoder_dict
    a, sd_e = load_golden("g3_pointnet.npz")
    _, sd_d = load_golden("g1_decode.npz")
    dec = decoder_dict['simple_local'](dim=3, c_dim=32, hidden_size=32, with_contact=True)
    dec.load_state_dict(sd_d, strict=True)
    enc = encoder_dict['pointnet_local_pool'](c_dim=32, dim=3, hidden_dim=32, unet3d=False, grid_resolution=16, plane_type='grid')
    enc.load_state_dict(sd_e, strict=True)
    model = ConvolutionalOccupancyNetwork(dec, enc.to(DEV), device=DEV)
    points_obj = torch.from_numpy((np.random.RandomState(21).randn(1, 2048, 3) * 0.3).astype(np.float32))
    data = {"inputs": T(a["p"])[:1], "points.points_obj": points_obj}
    gen = Generator3D(model, device=DEV, resolution0=16, padding=0.1, reference_returns=True)
    first = check_block(gen, data, "visual", tmp_path, hand=False)
    second = check_block(gen, data, "visual", tmp_path, hand=False)
    assert torch.equal(first.vertices, second.vertices)
    plain = Generator3D(model, device=DEV, resolution0=16, padding=0.1).generate_obj_mesh_wnf(data)
    assert type(plain) is Mesh and torch.equal(plain.vertices, first.vertices)
    from vtaco_amd._lib import VtError
    with pytest.raises(VtError, match="points_obj"):
        gen.generate_obj_mesh_wnf({"inputs": data["inputs"]})


def test_visualise_block_tactile_route(tmp_path):
    """The VTacOH route (fingertips from the hand encoder, tactile features by finger id): the whole block, hand mesh included."""
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    model, data, depth_origin = build_tactile_scene(torch.device(DEV), variant="vtacoh")
    data = dict(data, **{"points.points_obj": torch.from_numpy((np.random.RandomState(22).randn(1, 2048, 3) * 0.3).astype(np.float32))})
    kw = dict(device=torch.device(DEV), resolution0=16, padding=0.1, with_img=True, depth_origin=depth_origin)
    gen = Generator3D(model, reference_returns=True, **kw)
    check_block(gen, data, "tactile", tmp_path, hand=True)
    assert type(Generator3D(model, **kw).generate_obj_mesh_wnf(data)) is Mesh
