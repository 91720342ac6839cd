"""GPU: the tactile depth estimator's train-mode forward and backward on the HIP kernels (vt_tactile_unet_train_fwd / vt_tactile_unet_bwd,
csrc/unet2d_train.hip) through ``TactileUNet.forward`` / ``forward_scenes`` under autograd.  In every test of the HIP path F.conv2d,
F.conv_transpose2d, F.batch_norm, F.max_pool2d and the sigmoids raise, so a silent fall-back to the nn modules cannot pass.  The tests
set VTACO_TACTILE_UNET_TRAIN themselves: they do not depend on the default."""
import copy

import pytest
import torch
from torch.nn import functional as F
from conftest import load_golden
from tactile_unet_util import no_framework_ops, report as _report, seeded_unet as _net
from tactile_unet_train_util import CASES, IDS, reference, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def hip(monkeypatch):
    monkeypatch.setenv("VTACO_TACTILE_UNET_TRAIN", "hip")

    def run(net, x, scenes=1):
        with no_framework_ops():
            assert net.train_hip_supported(x, scenes)
            return net(x, scenes=scenes)
    return run


def _grads(net):
    return {n: p.grad.clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64_autograd(i, hip):
    """Output, every parameter's gradient and every running statistic after one L1 step against a .double() copy of the host module on
    the CPU called once per scene: err <= 8 e32 per tensor, err = ||t - t64|| / ||t64||, e32 the same for the f32 host module on the CPU
    (the factor of tests/test_resnet_gpu.py::_f64_gate, applied to the host module's error).  num_batches_tracked must be equal."""
    S, G, chw, depth, sf, seed = CASES[i]
    cpu, x, target, r64, e32 = reference(i)
    assert G * (chw[1] >> (depth - 1)) * (chw[2] >> (depth - 1)) >= 8
    net = copy.deepcopy(cpu).to(DEV).train()
    out = hip(net, x.to(DEV), S)
    with no_framework_ops():
        F.l1_loss(out, target.to(DEV)).backward()
    got = {"out": out.detach()}
    got.update({"grad:" + n: p.grad for n, p in net.named_parameters()})
    got.update({"buf:" + n: b for n, b in net.named_buffers()})
    assert set(got) == set(r64)
    rep, bad = {}, []
    for k, t64 in r64.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(t64) == 2 * S, k
            continue
        assert got[k].shape == t64.shape and torch.isfinite(got[k]).all(), k
        err = rel_err(got[k], t64)
        rep[k] = {"e32": e32[k], "err": err}
        if not err <= 8 * e32[k]:
            bad.append((k, err, e32[k]))
    unsat = float(((r64["out"] > 0.05) & (r64["out"] < 0.95)).double().mean())
    rep["unsaturated"] = unsat
    print(rep)
    _report("train_f64:" + IDS[i], rep)
    assert unsat >= 0.5, unsat
    assert not bad, bad


def test_g6_reference_golden_train_on_hip(hip):
    arrs, sd = load_golden("g6_tactile.npz")
    from vtaco_amd.encoder import encoder_dict
    net = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=3, start_filts=8)
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    y = hip(net, torch.from_numpy(arrs["x"]).to(DEV))
    assert y.requires_grad
    ref = torch.from_numpy(arrs["y_train"])
    rep = {"max_abs_err": float((y.detach().cpu() - ref).abs().max()), "output_max": float(ref.abs().max())}
    print(rep)
    _report("train_g6", rep)
    assert y.shape == ref.shape
    assert rep["max_abs_err"] <= 1e-4 * max(1.0, rep["output_max"]), rep


def test_bit_reproducible_and_scene_invariant(hip):
    base = _net(3, 32, 3, 1, 31).train().to(DEV)
    gen = torch.Generator().manual_seed(32)
    imgs = torch.rand(3, 5, 3, 16, 12, generator=gen).to(DEV)
    target = torch.rand(3, 5, 16 * 12, generator=gen).to(DEV)

    def scenes(net, im):
        with no_framework_ops():
            assert net.train_hip_supported(im.reshape(-1, *im.shape[2:]), im.shape[0])
            return net.forward_scenes(im)

    def step(lo, hi):
        net = copy.deepcopy(base)
        out = scenes(net, imgs)
        F.l1_loss(out[lo:hi], target[lo:hi]).backward()
        return net, out.detach(), _grads(net)
    # two identical steps: equal bits
    net_a, out_a, g_a = step(0, 3)
    _, out_b, g_b = step(0, 3)
    assert torch.equal(out_a, out_b)
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), n
    # three scenes in one call = three calls, bit for bit, running statistics included
    net_c = copy.deepcopy(base)
    for s in range(3):
        assert torch.equal(scenes(net_c, imgs[s:s + 1]).detach()[0], out_a[s]), s
    for (n, b), (_, c) in zip(net_a.named_buffers(), net_c.named_buffers()):
        assert torch.equal(b, c), n
        assert not torch.equal(b, dict(base.named_buffers())[n]), n
    # a loss over scene 0 alone: the one-scene call's gradients = the three-scene call's with the other scenes' dout zero
    net_d = copy.deepcopy(base)
    F.l1_loss(scenes(net_d, imgs[0:1]), target[0:1]).backward()
    _, _, g_e = step(0, 1)
    for n, g in _grads(net_d).items():
        assert torch.equal(g, g_e[n]), n
        assert float(g.abs().sum()) > 0 or n.endswith("bias"), n


def _trainer(seed_model):
    from vtaco_amd.conv_onet.training import Trainer
    model = copy.deepcopy(seed_model)
    return model, Trainer(model, torch.optim.Adam(model.parameters(), lr=1e-3), device=torch.device(DEV), train_tactile=True)


def test_trainer_step_on_hip_and_on_the_modules(monkeypatch):
    """Trainer(train_tactile=True).train_step on the model of test_trainer_train_tactile_step: the HIP path (framework operators raising
    inside the U-Net call) against VTACO_TACTILE_UNET_TRAIN=host; one ops.tactile_unet_train_fwd per step, not one per scene."""
    from vtaco_amd import ops
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    from vtaco_amd.encoder import encoder_dict
    torch.manual_seed(1)
    depth_net = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=2, start_filts=8)
    digits = encoder_dict["pointnet_local_pool"](dim=3, c_dim=16, padding=0.1, hidden_dim=32, plane_type=["xz", "xy", "yz"],
                                                 plane_resolution=32, unet=False, out_mano=True, out_dim=30)
    seed_model = ConvolutionalOccupancyNetwork(None, None, digits, depth_net, None, device=torch.device(DEV))
    g = torch.Generator().manual_seed(2)
    data = {"inputs": torch.randn(2, 300, 3, generator=g) * 0.2, "inputs.img": torch.rand(2, 5, 3, 16, 12, generator=g),
            "inputs.depth": 0.019 + 0.003 * torch.rand(2, 5, 16 * 12, generator=g), "points.cam_pos": torch.randn(2, 5, 3, generator=g) * 0.1,
            "points.cam_rot": torch.randn(2, 5, 3, generator=g)}
    calls = []
    real = ops.tactile_unet_train_fwd

    def counted(x, *a, **k):
        calls.append(x.shape[0])
        return real(x, *a, **k)
    monkeypatch.setattr(ops, "tactile_unet_train_fwd", counted)
    losses = {}
    for mode in ("hip", "host"):
        monkeypatch.setenv("VTACO_TACTILE_UNET_TRAIN", mode)
        model, trainer = _trainer(seed_model)
        model.train()
        if mode == "hip":
            unet = model.encoder_img
            inner = unet.forward

            def guarded(*a, _inner=inner, **k):
                with no_framework_ops():
                    return _inner(*a, **k)
            unet.forward = guarded
        losses[mode] = [trainer.train_step(data)[0] for _ in range(11)]
    print(losses)
    assert calls == [10] * 11, calls
    assert abs(losses["hip"][0] - losses["host"][0]) <= 1e-5, losses
    assert losses["hip"][-1] < losses["hip"][0] and losses["host"][-1] < losses["host"][0], losses


def test_dispatch_keeps_the_modules(monkeypatch):
    """x.requires_grad, train mode under no_grad, eval mode under autograd, the host knob, an uncovered shape and momentum=None all run
    the nn modules: ops.tactile_unet_train_fwd raises if it is reached (and IS reached by the covered call)."""
    from vtaco_amd import ops
    monkeypatch.setenv("VTACO_TACTILE_UNET_TRAIN", "hip")
    monkeypatch.setenv("VTACO_TACTILE_UNET", "host")

    def unreachable(*a, **k):
        raise AssertionError("the HIP train forward ran where the nn modules must")
    monkeypatch.setattr(ops, "tactile_unet_train_fwd", unreachable)
    base = _net(3, 8, 3, 1, 41).train().to(DEV)
    x = torch.rand(4, 3, 16, 12, generator=torch.Generator().manual_seed(42)).to(DEV)

    def modules(net, x, scenes=1):
        ref = copy.deepcopy(net)
        G = x.shape[0] // scenes
        want = torch.cat([ref.forward_modules(x[s * G:(s + 1) * G]) for s in range(scenes)])
        got = net(x, scenes=scenes)
        assert got.shape == want.shape and float((got - want).detach().abs().max()) <= 1e-5
        for (n, b), (_, c) in zip(net.named_buffers(), ref.named_buffers()):
            assert float((b.double() - c.double()).abs().max()) <= 1e-5, n
        return got
    assert base.train_hip_supported(x, 2)
    with pytest.raises(AssertionError, match="HIP train forward ran"):
        copy.deepcopy(base)(x, scenes=2)
    net = copy.deepcopy(base)
    xg = x.clone().requires_grad_(True)
    assert not net.train_hip_supported(xg, 2)
    modules(net, xg, 2).sum().backward()
    assert xg.grad is not None and float(xg.grad.abs().sum()) > 0
    with torch.no_grad():
        assert not net.train_hip_supported(x, 2)
        modules(net, x, 2)
    net.eval()
    assert not net.train_hip_supported(x, 2)
    assert modules(net, x, 2).requires_grad
    net.train()
    monkeypatch.setenv("VTACO_TACTILE_UNET_TRAIN", "host")
    assert not net.train_hip_supported(x, 2)
    modules(net, x, 2)
    monkeypatch.setenv("VTACO_TACTILE_UNET_TRAIN", "hip")
    assert net.train_hip_supported(x, 2)
    wide = _net(3, 24, 3, 1, 43).train().to(DEV)                        # start_filts no power of two: not covered
    assert not wide.train_hip_supported(x, 2)
    modules(wide, x, 2)
    assert not net.train_hip_supported(x, 3)                             # 4 images are not 3 scenes
    for blk in net.up_convs:
        blk.bn.momentum = None
    assert not net.train_hip_supported(x, 2)
    modules(net, x, 2)
