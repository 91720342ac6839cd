"""GPU: the PointConv baseline's modules -- ``PointNetPlusPlus`` (pointnet_plus_plus) and ``LocalPointDecoder`` (simple_local_point)
-- on the golden made from the real reference (tests/golden/g26_pointconv.npz), through autograd, through one Trainer step and
through the generator.

Tolerance of the module outputs: the one tests/test_pointconv_ref_cpu.py establishes -- the float64 restatement is the reference,
e32 = max |restatement in float32 - float64| per tensor what float32 costs there, and the result lies within MARGIN = 4 of it.
Gradients go through the project's gate, |got - ref64| <= 8 max(e32, 2^-24 bound) elementwise."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointconv_ref as R
from decode_train_ref import gate_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
SEED_EVAL, SEED_TRAIN = 2611, 2612          # tests/golden/make_pointconv_goldens.py


@functools.lru_cache(maxsize=None)
def _gold():
    return R.golden()


def _encoder(form=None):
    from vtaco_amd.encoder import encoder_dict
    return R.fill(encoder_dict["pointnet_plus_plus"](dim=3, c_dim=32, padding=0.1), R.SEED_ENC).to(DEV)


def _decoder(kw):
    from vtaco_amd.conv_onet.models import decoder_dict
    return R.fill(decoder_dict["simple_local_point"](dim=3, c_dim=32, hidden_size=32, padding=0.1, with_contact=False, **kw), R.SEED_DEC).to(DEV)


@functools.lru_cache(maxsize=None)
def _enc_ref(mode):
    gold = _gold()
    sd = {k: v.cpu() for k, v in _encoder().state_dict().items()}
    args = (sd, gold["cloud"], gold[f"enc.{mode}.starts"])
    f64, tr = R.encoder(*args, train=mode == "train", dtype=torch.float64)
    f32, _ = R.encoder(*args, train=mode == "train", dtype=torch.float32)
    return f64, f32, tr


@functools.lru_cache(maxsize=None)
def _dec_ref(tag):
    gold = _gold()
    kw = dict(R.MODES)[tag]
    sd = {k: v.cpu() for k, v in _decoder(kw).state_dict().items()}
    args = (sd, gold["queries"], gold["cloud"], gold["enc.eval.fea"], gold["occ"], kw["sample_mode"], kw.get("gaussian_val"))
    return R.decoder(*args, dtype=torch.float64), R.decoder(*args, dtype=torch.float32)


def _close(what, got, r64, r32, golden=None):
    e32 = float((r32.double() - r64).abs().max())
    err = float((got.detach().double().cpu().reshape(r64.shape) - r64).abs().max())
    extra = "" if golden is None else f", |got - golden| = {float((got.detach().cpu().double() - golden.double()).abs().max()):.3e}"
    print(f"CLOSE {what}: |got - f64| = {err:.3e}, e32 = {e32:.3e}{extra}")
    assert err <= R.MARGIN * e32, f"{what}: {err:.3e} > {R.MARGIN} x {e32:.3e}"


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"


class _form:
    """Run a block with every stage on one form of vtaco_amd.pointconv_host ('hip' or 'host')."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from vtaco_amd import pointconv_host as host
        self.host, self.saved = host, dict(host.FORM)
        host.FORM.update({s: self.name for s in host.STAGES})

    def __exit__(self, *exc):
        self.host.FORM.update(self.saved)
        return False


@pytest.mark.parametrize("form", ["hip", "host"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_encoder_reproduces_golden(mode, form):
    gold = _gold()
    enc = _encoder().train(mode == "train")
    f64, f32, _ = _enc_ref(mode)
    with _form(form):
        torch.manual_seed(SEED_EVAL if mode == "eval" else SEED_TRAIN)
        with torch.no_grad():
            xyz, fea = enc(gold["cloud"].to(DEV))
    assert torch.equal(xyz.cpu(), gold["cloud"]) and fea.shape == (2, 600, 32)
    _close(f"encoder features ({mode}, {form})", fea, f64, f32, gold[f"enc.{mode}.fea"])


def test_encoder_geometry_hip_equals_host_and_reference():
    """The index stages on the golden cloud: both forms give the float64 restatement's farthest points, ball rows and neighbours."""
    from vtaco_amd.encoder import pointnetpp
    gold = _gold()
    _, _, tr = _enc_ref("eval")
    fps1, ball1 = tr[0], tr[1]
    cloud = gold["cloud"].to(DEV)
    centres = R.index_points(gold["cloud"], fps1)
    for form in ("hip", "host"):
        with _form(form):
            assert torch.equal(pointnetpp.fps(cloud, 512, gold["enc.eval.starts"][0]).cpu(), fps1), form
            assert torch.equal(pointnetpp.ball_query(cloud, centres.to(DEV), 0.2, 32).cpu(), ball1), form
            idx, w = pointnetpp.three_nn(cloud, centres.to(DEV))
            ridx, rw, _ = R.three_nn(gold["cloud"], centres, torch.float64)
            assert torch.equal(idx.cpu().sort(dim=-1)[0], ridx.sort(dim=-1)[0]), form
            f = torch.randn(2, 512, 8, generator=torch.Generator().manual_seed(1))
            i32, w32, _ = R.three_nn(gold["cloud"], centres, torch.float32)
            _gate(f"three_nn interpolation ({form})", R.interpolate(f, idx.cpu(), w.cpu()), R.interpolate(f.double(), ridx, rw),
                  R.interpolate(f, i32, w32), R.interpolate(f.double(), ridx, rw, absolute=True))


@pytest.mark.parametrize("form", ["hip", "host"])
@pytest.mark.parametrize("tag", [t for t, _ in R.MODES])
def test_decoder_reproduces_golden_and_gradients(tag, form):
    """Logits against the golden's tolerance; the feature gradient and every parameter gradient of the L1 loss through autograd
    (the sampler's autograd function, then the MLP's) against float64 under the gate."""
    gold = _gold()
    dec = _decoder(dict(R.MODES)[tag])
    r64, r32 = _dec_ref(tag)
    q, cloud = gold["queries"].to(DEV), gold["cloud"].to(DEV)
    with _form(form):
        with torch.no_grad():
            logits = dec(q, (cloud, gold["enc.eval.fea"].to(DEV)))
        _close(f"logits ({tag}, {form})", logits, r64["logits"], r32["logits"], gold[f"dec.{tag}.logits"])
        fea = gold["enc.eval.fea"].to(DEV).requires_grad_(True)
        out = dec(q, (cloud, fea))
        torch.nn.functional.l1_loss(out, gold["occ"].to(DEV)).backward()
    _gate(f"train logits ({tag}, {form})", out, r64["logits"], r32["logits"], r64["bound.logits"])
    _gate(f"grad fea ({tag}, {form})", fea.grad, r64["grad_fea"], r32["grad_fea"], r64["bound.grad_fea"])
    for name, prm in dec.named_parameters():
        _gate(f"grad {name} ({tag}, {form})", prm.grad, r64["grads"][name], r32["grads"][name], r64["bound.grads"][name])


# ---- trainer and generator -----------------------------------------------------------------------------------------------------
def _cfg():
    return {"data": {"dim": 3, "padding": 0.1, "input_type": "pointcloud"},
            "model": {"encoder": "pointnet_plus_plus", "decoder": "simple_local_point", "c_dim": 32, "encoder_kwargs": {},
                      "decoder_kwargs": {"hidden_size": 32, "sample_mode": "gaussian", "gaussian_val": 0.1}},
            "test": {"threshold": 0.5}, "generation": {"resolution_0": 8, "upsampling_steps": 2}}


def _model():
    from vtaco_amd.conv_onet import config
    model = config.get_model(_cfg(), device=DEV)
    R.fill(model.encoder, R.SEED_ENC)
    R.fill(model.decoder, R.SEED_DEC)
    return model


@functools.lru_cache(maxsize=None)
def _scene():
    """One model of tests/synth_dataset.py: its 256 query points with occupancies, and as the input cloud its 200 surface points
    three times over with the loader's 0.005 noise (seeded) -- the encoder's first stage samples 512 points, so 600."""
    import tempfile
    from synth_dataset import make_synthetic_dataset
    with tempfile.TemporaryDirectory() as root:
        make_synthetic_dataset(root, seed=3)
        d = os.path.join(root, "ycb", "obj_a_0001")
        pts = np.load(os.path.join(d, "points.npz"))
        surf = np.load(os.path.join(d, "pointcloud.npz"))["points"]
        p, occ, obj = pts["points"].astype(np.float32), pts["occupancies"].astype(np.float32), pts["points_obj"].astype(np.float32)
    cloud = np.tile(surf, (3, 1)) + 0.005 * np.random.RandomState(4).randn(600, 3).astype(np.float32)
    return {"points": torch.from_numpy(p)[None], "points.occ": torch.from_numpy(occ)[None], "inputs": torch.from_numpy(cloud)[None],
            "points.points_obj": torch.from_numpy(obj)[None]}


def test_trainer_step_moves_parameters_and_matches_reference_loss():
    from vtaco_amd.conv_onet.training import Trainer
    data = _scene()
    model = _model()
    sd_enc = {k: v.detach().cpu().clone() for k, v in model.encoder.state_dict().items()}
    sd_dec = {k: v.detach().cpu().clone() for k, v in model.decoder.state_dict().items()}
    trainer = Trainer(model, torch.optim.SGD(model.parameters(), lr=1e-2), device=DEV)
    torch.manual_seed(77)
    starts = (torch.randint(0, 600, (1,)), torch.randint(0, 512, (1,)))          # what the encoder's two stages draw under this seed
    torch.manual_seed(77)
    with _form("hip"):
        loss = trainer.train_step(data)[0]
    ref = {}
    for dt in (torch.float64, torch.float32):
        fea, _ = R.encoder(sd_enc, data["inputs"], starts, train=True, dtype=dt)
        ref[dt] = R.decoder(sd_dec, data["points"], data["inputs"], fea, data["points.occ"], "gaussian", 0.1, dtype=dt)["logits"]
    l64 = float((ref[torch.float64] - data["points.occ"].double()).abs().mean())
    e32 = float((ref[torch.float32].double() - ref[torch.float64]).abs().max())
    # the L1 loss is a mean of |logit - occ|: it moves by at most the largest logit error
    print(f"CLOSE trainer loss: {loss:.8f} against {l64:.8f}, logits' e32 = {e32:.3e}")
    assert abs(loss - l64) <= R.MARGIN * e32
    moved = [k for k, v in list(model.encoder.state_dict().items()) + list(model.decoder.state_dict().items())
             if v.dtype.is_floating_point and not torch.equal(v.cpu(), {**sd_enc, **sd_dec}[k])]
    assert any(k.startswith("sa1.mlp_convs.0") for k in moved) and any(k.startswith("fc_out") for k in moved), moved
    with _form("hip"):
        out = trainer.eval_step({**data, "points_iou": data["points"], "points_iou.occ": data["points.occ"]})
    assert np.isfinite(out["loss"]) and 0.0 <= out["iou"] <= 1.0


@pytest.fixture
def hip_form():
    """The generator tests run the kernels whatever the default form is."""
    with _form("hip"):
        yield


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_generate_obj_mesh_wnf_is_the_mesh_of_eval_points(precision, hip_form):
    """resolution_0 8 (a 32^3 lattice): generate_obj_mesh_wnf returns the mesh extract_mesh gives on eval_points of the same lattice,
    and eval_lattice equals eval_points bit for bit, at the decoder's stated precision."""
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet import config
    data = _scene()
    model = _model().eval()
    model.decoder.precision = precision
    gen = config.get_generator(model, _cfg(), DEV)
    gen.decode_precision = precision
    nx = 32
    torch.manual_seed(5)
    mesh = gen.generate_obj_mesh_wnf(data)
    torch.manual_seed(5)
    with torch.no_grad():
        c = model.encode_inputs(data["inputs"].to(DEV))
    lattice = gen.eval_lattice(c, nx)
    pts = 1.1 * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (nx,) * 3)
    gen.points_batch_size = 10000                                                # several ragged chunks
    points = gen.eval_points(pts, c)
    assert torch.equal(lattice.cpu(), points), f"eval_lattice and eval_points differ by {float((lattice.cpu() - points).abs().max()):.3e}"
    want = gen.extract_mesh(points.to(DEV).reshape(nx, nx, nx))
    assert mesh.vertices.shape[0] > 0 and torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.faces, want.faces)
    part = gen.eval_lattice(c, nx, first=nx * nx + 3, count=2 * nx * nx + 7)
    assert torch.equal(part, lattice[nx * nx + 3:3 * nx * nx + 10])


def test_generator_reference_returns_and_mise(hip_form):
    from vtaco_amd import mise
    from vtaco_amd.common import make_3d_grid
    from vtaco_amd.conv_onet.generation import Generator3D
    data = _scene()
    model = _model().eval()
    gen = Generator3D(model, device=DEV, resolution0=8, upsampling_steps=2, reference_returns=True, padding=0.1)
    torch.manual_seed(5)
    np.random.seed(0)
    mesh, emd, cd = gen.generate_obj_mesh_wnf(data)
    assert mesh.vertices.shape[0] > 0 and np.isfinite(emd) and np.isfinite(cd)
    # MISE falls out of the point form of the sampler: every entry a level decoded is the point path's logit at that lattice point
    gm = Generator3D(model, device=DEV, resolution0=8, upsampling_steps=2, padding=0.1, extraction="mise", decode_precision="f32")
    torch.manual_seed(5)
    mm = gm.generate_obj_mesh_wnf(data)
    assert mm.vertices.shape[0] > 0 and len(gm.mise_points_per_level) == 3
    torch.manual_seed(5)
    with torch.no_grad():
        c = model.encode_inputs(data["inputs"].to(DEV))
    values, known, _ = mise.extract(gm.mise_evaluator(c), 8, 2, gm.mise_level(), 1.1, DEV)
    n = values.shape[0]
    model.decoder.precision = "f32"
    dense = gm.eval_points(1.1 * make_3d_grid((-0.5,) * 3, (0.5,) * 3, (n,) * 3), c).reshape(n, n, n)
    k = known.cpu().bool()
    assert 0 < int(k.sum()) < n ** 3 and torch.equal(values.cpu()[k], dense[k])


def test_refused_routes_raise(hip_form):
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.inferencing import Inferencer
    data = _scene()
    model = _model().eval()
    gen = Generator3D(model, device=DEV, resolution0=8, padding=0.1)
    with pytest.raises(VtError, match="CPU generator"):
        gen.generate_mesh_graphed(data["inputs"])
    with pytest.raises(VtError, match="start indices"):
        gen.generate_obj_mesh_sharded(data)
    with pytest.raises(VtError, match="tactile"):
        gen.generate_obj_mesh_tactile(data, None, None, None)
    with pytest.raises(VtError, match="tactile"):
        Generator3D(model, device=DEV, resolution0=8, padding=0.1, with_img=True).generate_obj_mesh_wnf(data)
    with pytest.raises(VtError, match="tactile"):
        gen.generate_obj_mesh_wnf(data, c_img_all=torch.zeros(1, 32 ** 3, 32))
    with pytest.raises(VtError, match="PointConv"):
        Inferencer(model, None, gen, device=DEV, with_img=True)
    with pytest.raises(VtError):
        model.decoder.forward_img(data["points"].to(DEV), None, None)
    with pytest.raises(VtError):
        model.decode_contact(data["points"].to(DEV), None)
    with pytest.raises(VtError, match="fewer"):
        model.encode_inputs(data["inputs"][:, :300].to(DEV))
