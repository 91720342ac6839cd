"""GPU: the touch session -- vt_touch_merge against the real reference Inferencer's carried-over lattice (g23_touch.npz), and
``conv_onet.inferencing.Inferencer`` on the shipped scene (tests/config2_case.py) with the tactile modules the tactile tests build:
incremental decode against the whole-lattice decode from the merged ids, touch 0 against Generator3D, order, refusals, determinism."""
import os
import sys

import numpy as np
import pytest
import torch

import config2_case as c2
import touch_rule as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BOX = 1.1


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_mesh(a, b):
    return torch.equal(a.faces, b.faces) and torch.equal(bits(a.vertices.float()), bits(b.vertices.float())) and a.vertices.dtype == b.vertices.dtype


def gpu_merge(ids, setup, mode, radius, nx, row_base, capacity=1 << 16):
    from vtaco_amd import ops
    anchors, count, success = setup
    cid, cpts, n = ops.touch_merge(ids, torch.from_numpy(anchors).to(DEV), torch.from_numpy(success).to(DEV), mode, radius, nx, BOX,
                                   row_base, capacity, count=torch.from_numpy(count).to(DEV))
    n = int(n.item())
    return cid[:min(n, capacity)].clone(), cpts[:min(n, capacity)].clone(), n


# -- 1, 2: the merge kernel against the reference's lattice ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["h", "d"])
def test_touch_merge_reproduces_the_reference_lattice_and_lists_what_changed(route):
    from vtaco_amd import ops
    z = tr.fixture()
    nx = int(z["nx"])
    mode, radius = tr.ROUTES[route]
    _, lattice_pts = ops.mise_lattice(nx, BOX, DEV, want_ids=False)
    ids = torch.full((nx ** 3,), 255, dtype=torch.uint8, device=DEV)
    prev = np.full(nx ** 3, 255, dtype=np.uint8)
    for k, (anchors, count, success, _, _) in enumerate(tr.walk(z, route)):
        before = ids.clone()
        cid, cpts, n = gpu_merge(ids, (anchors, count, success), mode, radius, nx, 5 * k)
        ref = tr.expected(z, route, k)
        got = ids.cpu().numpy()
        assert np.array_equal(got, ref), (route, k, int((got != ref).sum()))
        changed = np.nonzero(ref != prev)[0]
        print(f"{route} touch {k}: {n} of {nx ** 3} points changed")
        assert n == changed.size and np.array_equal(cid.cpu().numpy(), changed)      # exactly the ascending set of changed points
        assert torch.equal(bits(cpts), bits(lattice_pts[cid.long()]))               # with the lattice's coordinates
        assert success.any() and n >= 1                                              # every touch with a successful finger changes a point
        if k == 0:                                                                   # the existing assignment on an empty lattice
            fresh = ops.tactile_assign(torch.from_numpy(anchors).to(DEV), torch.from_numpy(success).to(DEV), mode, radius,
                                       lattice=(nx, BOX, 0, nx ** 3), count=torch.from_numpy(count).to(DEV))
            assert torch.equal(fresh[0], ids)
        # a list longer than its capacity: the length is reported, the first entries are written, the lattice is merged all the same
        again = before.clone()
        cid2, _, n2 = gpu_merge(again, (anchors, count, success), mode, radius, nx, 5 * k, capacity=7)
        assert n2 == n and torch.equal(cid2, cid[:7]) and torch.equal(again, ids)
        prev = ref
    assert n < 0.01 * nx ** 3                                                        # the last touch is sparse: < 1 % of the lattice


def test_touch_merge_order_and_row_limit():
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    z = tr.fixture()
    nx = int(z["nx"])
    finals = []
    for order in ([0, 1, 2], [0, 2, 1]):
        ids = torch.full((nx ** 3,), 255, dtype=torch.uint8, device=DEV)
        steps = tr.walk(z, "h", order)
        for i, (anchors, count, success, ref, changed) in enumerate(steps):
            cid, _, n = gpu_merge(ids, (anchors, count, success), "nearest", 0.05, nx, 5 * i)
            assert np.array_equal(ids.cpu().numpy(), ref) and np.array_equal(cid.cpu().numpy(), changed)
        finals.append(ids.cpu().numpy())
    assert not np.array_equal(finals[0], finals[1])                                  # later touches overwrite: the order is part of the result
    anchors, count, success, _, _ = tr.walk(z, "h", [0])[0]
    ids = torch.full((nx ** 3,), 255, dtype=torch.uint8, device=DEV)
    gpu_merge(ids, (anchors, count, success), "nearest", 0.05, nx, 249)              # rows 249..253: the last that fit
    assert int(ids[ids != 255].max()) <= 253
    keep = ids.clone()
    with pytest.raises(VtError, match="254"):
        gpu_merge(ids, (anchors, count, success), "nearest", 0.05, nx, 250)
    assert torch.equal(ids, keep)                                                    # refused before any launch
    with pytest.raises(VtError):
        ops.touch_merge(ids[:100], torch.from_numpy(anchors).to(DEV), torch.from_numpy(success).to(DEV), "nearest", 0.05, nx, BOX, 0, 16)


# -- the session on a real model ----------------------------------------------------------------------------------------------------
def build_model(tmp, decoder="simple_local"):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import synth_mano
    from test_hand_gpu import MANO_KW
    from vtaco_amd.bench_util import randomise_fc1
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork, decoder_dict
    from vtaco_amd.encoder import encoder_dict
    z = c2.fixture()
    enc, dec = c2.models(z)
    if decoder != "simple_local":
        torch.manual_seed(0)
        dec = decoder_dict[decoder](dim=3, c_dim=32, hidden_size=32).eval()
        randomise_fc1(dec, 3)
    synth_mano.write_pkl(synth_mano.make_asset(0), str(tmp / "mano"))
    torch.manual_seed(21)
    img = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=2, start_filts=8)
    hand = encoder_dict["pointnet_local_pool"](dim=3, c_dim=32, padding=0.1, hidden_dim=32, plane_type=["xz", "xy", "yz"],
                                               plane_resolution=32, unet=False, out_mano=True, out_dim=51,
                                               manolayer_kwargs=dict(MANO_KW, mano_root=str(tmp / "mano")))
    model = ConvolutionalOccupancyNetwork(dec, enc, hand, img, None, device=DEV).eval()
    return model, torch.from_numpy(z["cloud"]).float().reshape(1, -1, 3)


def touch_data(model, cloud, route, success=None):
    """The fixture's touches as sample dictionaries for ``model`` on the shipped cloud.  VTacO: the fixture's depth images and sensor
    poses (so the id lattices are the reference's own).  VTacOH: the fingertips come from the model's hand encoder, so the wrist is
    placed with the first fingertip near the lattice centre and drifts 3 cm per touch (overlapping touches)."""
    from vtaco_amd.common import fingertips_in_object_frame
    z = tr.fixture()
    g = torch.Generator().manual_seed(31)
    out = []
    if route == "h":
        with torch.no_grad():
            joints = model.encode_hand_inputs(cloud.to(DEV))["mano_joints"].float().cpu().numpy()
        pc = z["pc_ply"]
        m = np.max(np.sqrt(np.sum((pc[0] - pc[0].mean(0)) ** 2, axis=1)))
        wrist = torch.from_numpy(z["h.wrist"][:1])
        tips0 = fingertips_in_object_frame(joints, np.zeros((1, 3)), wrist.numpy(), pc)
    for k in range(tr.touches(z)):
        d = tr.sample(z, route, k)
        d["inputs"] = cloud
        d["inputs.img"] = torch.rand(1, 5, 3, 8, 4, generator=g)
        if route == "h":
            d["points.wrist"] = wrist
            d["points.mano"] = torch.zeros(1, 51)
            d["points.mano"][0, :3] = torch.from_numpy((np.array([0.03 * k, 0.01 * k, 0.0]) - tips0[0, 0]) * 2 * m).float()
        if success is not None and k > 0:
            d["inputs.touch_success"] = torch.tensor([success], dtype=torch.bool)
        out.append(d)
    return z, out


def make(model, route, precision, incremental=True, **kw):
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.inferencing import Inferencer
    z = tr.fixture()
    gen = Generator3D(model, device=DEV, resolution0=kw.pop("resolution0", int(z["nx"]) // 4), padding=0.1, with_img=True,
                      encode_t2d=route == "d", decode_precision=precision, depth_origin=z["d.depth_origin"], **kw)
    return gen, Inferencer(model, None, gen, device=DEV, with_img=True, encode_t2d=route == "d", incremental=incremental)


def run(inf, touches, seed, hook=None):
    """The sequence through add_touch; per touch (ids, values, list, mesh_obj, mesh_hand), cloned.  numpy is seeded ONCE."""
    state = np.random.get_state()
    rec = []
    try:
        np.random.seed(seed)
        inf.reset()
        for k, d in enumerate(touches):
            before = None if inf.session is None else inf.session.values.clone()
            mo, mh = inf.add_touch(d)
            s = inf.session
            n = inf.changed_points[-1]
            item = {"ids": s.ids.clone(), "values": s.values.clone(), "n": n, "list": s.changed_ids[:max(n, 0)].clone(),
                    "obj": type(mo)(mo.vertices.clone(), mo.faces.clone()), "hand": mh, "before": before}
            if hook is not None:
                hook(k, s, item)
            rec.append(item)
    finally:
        np.random.set_state(state)
    return rec


@pytest.mark.parametrize("route", ["h", "d"])
def test_session_f32_is_the_whole_lattice_decode_bit_for_bit(route, tmp_path):
    model, cloud = build_model(tmp_path)
    z, touches = touch_data(model, cloud, route)
    nx, seed = int(z["nx"]), int(z["seed"])
    gen, inf = make(model, route, "f32")
    dec = model.decoder

    def hook(k, s, item):
        with torch.no_grad():
            ref = dec.decode_lattice_ids(s.c['grid'], nx, s.ids.view(1, -1), s.feats[:5 * (k + 1)], box=BOX, precision="f32").reshape(-1)
        assert torch.equal(bits(s.values), bits(ref)), (route, k)
        if route == "d":                                            # the fixture's sensors: the reference's own lattice
            assert np.array_equal(s.ids.cpu().numpy(), tr.expected(z, route, k))
    rec = run(inf, touches, seed, hook)
    assert [r["n"] for r in rec][0] == -1 and all(0 < r["n"] < 0.01 * nx ** 3 for r in rec[1:])     # the sparse path really ran
    # inference_step is reset() + add_touch per entry
    np_state = np.random.get_state()
    np.random.seed(seed)
    objs, hands = inf.inference_step([{"data": d, "name": "x", "touch_id": i} for i, d in enumerate(touches)])
    np.random.set_state(np_state)
    assert len(objs) == len(hands) == len(touches) and all(same_mesh(o, r["obj"]) for o, r in zip(objs, rec))
    _, whole = make(model, route, "f32", incremental=False)
    ref = run(whole, touches, seed)
    for k, (a, b) in enumerate(zip(rec, ref)):
        assert torch.equal(a["ids"], b["ids"]) and torch.equal(bits(a["values"]), bits(b["values"])), k
        assert same_mesh(a["obj"], b["obj"]) and same_mesh(a["hand"], b["hand"]), k
        assert a["obj"].faces.shape[0] > 0
    assert not torch.equal(rec[0]["values"], rec[-1]["values"])    # the later touches changed the field


@pytest.mark.parametrize("route", ["h", "d"])
def test_session_f16x3_lists_points_and_keeps_the_rest(route, tmp_path):
    from vtaco_amd import ops
    model, cloud = build_model(tmp_path)
    z, touches = touch_data(model, cloud, route)
    nx, seed = int(z["nx"]), int(z["seed"])
    gen, inf = make(model, route, "f16x3")
    assert gen.decode_precision == "f16x3"
    dec = model.decoder

    def hook(k, s, item):
        rows = s.feats[:5 * (k + 1)]
        with torch.no_grad():
            whole = dec.decode_lattice_ids(s.c['grid'], nx, s.ids.view(1, -1), rows, box=BOX, precision="f16x3").reshape(-1)
            err = float((s.values - whole).abs().max())
            print(f"{route} touch {k}: {item['n']} points decoded, max |session - whole-lattice decode| = {err:.3e}")
            assert err <= 1e-4                                      # the standing contract between the two f16x3 paths
            if k == 0:
                return
            idx = item["list"].long()
            pts = c2.lattice_points(idx.cpu(), nx, BOX).to(DEV)[None]
            own = ops.decode_fwd_ids(s.c['grid'], dec._blob(img=True, precision="f16x3"), s.ids[idx].view(1, -1), rows, pts=pts,
                                     padding=dec.padding, precision="f16x3").reshape(-1)
        assert torch.equal(bits(s.values[idx]), bits(own))          # listed entries: the point path's decode of those points
        rest = torch.ones(nx ** 3, dtype=torch.bool, device=DEV)
        rest[idx] = False
        assert torch.equal(bits(s.values[rest]), bits(item["before"][rest]))      # every other entry keeps the previous touch's bits
    rec = run(inf, touches, seed, hook)
    assert all(0 < r["n"] < 0.01 * nx ** 3 for r in rec[1:])
    # touch 0 is Generator3D's own scene
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        c, setup = gen._tactile_encode(touches[0])
        with torch.no_grad():
            lat = gen._eval_lattice_tactile(c, nx, setup)
        np.random.seed(seed)
        mesh = gen.generate_obj_mesh_wnf(touches[0])
        hand = gen.generate_hand_mesh(touches[0])
    finally:
        np.random.set_state(state)
    assert torch.equal(bits(rec[0]["values"]), bits(lat))
    assert same_mesh(rec[0]["obj"], mesh) and same_mesh(rec[0]["hand"], hand)


def test_failed_touches_reset_and_determinism(tmp_path):
    model, cloud = build_model(tmp_path)
    for route in ("h", "d"):
        z, touches = touch_data(model, cloud, route)
        seed = int(z["seed"])
        _, inf = make(model, route, "f16x3")
        a, b = run(inf, touches, seed), run(inf, touches, seed)     # (run() resets first)
        for k, (x, y) in enumerate(zip(a, b)):                      # two runs: bit-identical lattices, lists and meshes
            assert torch.equal(x["ids"], y["ids"]) and torch.equal(bits(x["values"]), bits(y["values"])), (route, k)
            assert x["n"] == y["n"] and torch.equal(x["list"], y["list"])
            assert same_mesh(x["obj"], y["obj"]) and same_mesh(x["hand"], y["hand"])
        # later touches that all fail: touch 0's lattice and mesh stay
        _, failing = touch_data(model, cloud, route, success=[False] * 5)
        f = run(inf, failing, seed)
        assert [r["n"] for r in f[1:]] == [0] * (len(f) - 1)
        for r in f[1:]:
            assert torch.equal(r["ids"], f[0]["ids"]) and torch.equal(bits(r["values"]), bits(f[0]["values"])) and same_mesh(r["obj"], f[0]["obj"])
        assert same_mesh(f[0]["obj"], a[0]["obj"])
        # reset() forgets everything: the next touch is a touch 0 again
        inf.reset()
        assert inf.session is None and inf.changed_points == []
        state = np.random.get_state()
        np.random.seed(seed)
        mo, _ = inf.add_touch(touches[0])
        np.random.set_state(state)
        assert inf.session.touches == 1 and same_mesh(mo, a[0]["obj"])


def test_refusals_and_the_attention_decoder(tmp_path):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.inferencing import Inferencer
    model, cloud = build_model(tmp_path)
    z, touches = touch_data(model, cloud, "d")
    seed = int(z["seed"])
    with pytest.raises(VtError, match="mise"):
        make(model, "d", "f32", extraction="mise", upsampling_steps=1)
    gen, inf = make(model, "d", "f32")
    with pytest.raises(VtError, match="sharded"):
        inf.inference_step([{"data": touches[0]}], group=object())
    with pytest.raises(VtError, match="one scene"):
        inf.add_touch(dict(touches[0], inputs=cloud.expand(2, -1, -1)))
    with pytest.raises(VtError, match="with_img"):
        Inferencer(model, None, gen, device=DEV, with_img=False).inference_step([{"data": touches[0]}])
    with pytest.raises(VtError, match="same route"):
        Inferencer(model, None, gen, device=DEV, with_img=True, encode_t2d=False).add_touch(touches[0])
    assert inf.session is None
    run(inf, touches[:1], seed)
    inf.session.touches = 50                                        # fifty touches fill the 254 rows
    keep = (inf.session.ids.clone(), inf.session.values.clone())
    with pytest.raises(VtError, match="50 touches"):
        inf.add_touch(touches[1])
    assert torch.equal(inf.session.ids, keep[0]) and torch.equal(inf.session.values, keep[1])
    # attention_local: the session decodes the whole lattice from the merged ids each touch
    amodel, _ = build_model(tmp_path, decoder="attention_local")
    agen, ainf = make(amodel, "d", "f32", resolution0=16, points_batch_size=2048)
    nx = 64

    def hook(k, s, item):
        with torch.no_grad():
            ref = agen._eval_lattice_fused(s.c, nx, s.ids.view(1, -1), s.feats[:5 * (k + 1)], 0, nx ** 3)
        assert torch.equal(bits(s.values), bits(ref)), k
        assert item["n"] == -1
    rec = run(ainf, touches, seed, hook)
    assert len(rec) == len(touches) and int((rec[-1]["ids"] != 255).sum()) > 0
    assert not torch.equal(rec[0]["values"], rec[-1]["values"])
