"""GPU: the tactile depth estimator's eval-mode forward on the HIP kernels (vt_tactile_unet_pack / vt_tactile_unet_fwd, csrc/unet2d.hip),
through ``TactileUNet.forward`` and through raw ``ops.tactile_unet_fwd``.  In every test of the HIP path F.conv2d, F.conv_transpose2d,
F.batch_norm, F.max_pool2d and the sigmoids raise, so a silent fall-back to the nn modules cannot pass.  The tests set
VTACO_TACTILE_UNET themselves: they do not depend on the default."""
import copy

import pytest
import torch
from conftest import load_golden
from tactile_unet_util import no_framework_ops, report as _report, seeded_unet as _net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def hip(monkeypatch):
    monkeypatch.setenv("VTACO_TACTILE_UNET", "hip")

    def run(net, x):
        with torch.no_grad(), no_framework_ops():
            assert net.hip_supported(x)
            return net(x)
    return run


def test_g6_reference_golden_eval_on_hip_and_train_on_the_modules(hip):
    arrs, sd = load_golden("g6_tactile.npz")
    from vtaco_amd.encoder import encoder_dict
    net = encoder_dict["UNet"](num_classes=1, in_channels=3, depth=3, start_filts=8)
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).eval()
    x = torch.from_numpy(arrs["x"]).to(DEV)
    y = hip(net, x).cpu()
    ref = torch.from_numpy(arrs["y_eval"])
    rep = {"eval": {"max_abs_err": float((y - ref).abs().max()), "output_max": float(ref.abs().max())}}
    print(rep)
    assert y.shape == ref.shape
    assert rep["eval"]["max_abs_err"] <= 1e-4 * max(1.0, rep["eval"]["output_max"]), rep
    net.train()
    with torch.no_grad():
        assert not net.hip_supported(x)
        yt = net(x).cpu()
    ref = torch.from_numpy(arrs["y_train"])
    rep["train"] = {"max_abs_err": float((yt - ref).abs().max()), "output_max": float(ref.abs().max())}
    print(rep)
    assert rep["train"]["max_abs_err"] <= 1e-4 * max(1.0, rep["train"]["output_max"]), rep
    _report("g6", rep)


# (shape, depth, start_filts, num_classes, seed): the smallest shapes at which each part of the kernels can go wrong
F64_CASES = [((1, 3, 4, 4), 3, 32, 1, 11),          # bottom level 1 x 1: every tap of a 3x3 is padding somewhere
             ((2, 3, 8, 12), 3, 32, 1, 12),         # non-square
             ((3, 3, 20, 28), 3, 32, 1, 13),        # H and W no multiple of the 2 x 16 patch
             ((2, 3, 64, 48), 3, 8, 1, 14),         # widths 8 / 16 / 32: below an MFMA tile
             ((1, 1, 16, 16), 1, 16, 1, 15),        # depth 1: no pool, no up path; in_channels 1
             ((1, 3, 32, 32), 5, 8, 1, 16),         # depth 5
             ((1, 4, 8, 8), 2, 32, 3, 17),          # in_channels 4, num_classes 3
             ((1, 3, 320, 240), 3, 32, 1, 18)]      # the shipped image


def _f64_gate(net_cpu, x, y_hip):
    """max |y_hip - y64| <= 8 * e32 (the rule of tests/test_resnet_gpu.py::_f64_gate): y64 from a .double() copy of the host module on
    the CPU, e32 the error of the same host module in f32 on the CPU against it -- measured on the host module, never on the kernel.
    At least half of the outputs must lie in (0.05, 0.95): a saturated sigmoid would shrink both errors and hide a fault."""
    with torch.no_grad():
        y64 = copy.deepcopy(net_cpu).double()(x.double())
        y32 = net_cpu.forward_modules(x)
    e32 = float((y32.double() - y64).abs().max())
    err = float((y_hip.double().cpu() - y64).abs().max())
    spread = float(((y32 > 0.05) & (y32 < 0.95)).float().mean())
    return {"e32": e32, "hip_err": err, "ratio": err / e32, "unsaturated": spread}


@pytest.mark.parametrize("shape,depth,sf,classes,seed", F64_CASES,
                         ids=[f"d{d}-sf{s}-{'x'.join(map(str, sh))}" for sh, d, s, _, _ in F64_CASES])
def test_against_float64(shape, depth, sf, classes, seed, hip):
    cpu = _net(depth, sf, shape[1], classes, seed)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed))
    net = copy.deepcopy(cpu).to(DEV)
    xd = x.to(DEV)
    y = hip(net, xd)
    assert y.shape == (shape[0], classes, shape[2], shape[3])
    rep = _f64_gate(cpu, x, y)
    # raw ops.tactile_unet_fwd with a blob and a workspace of its own: the same bits
    from vtaco_amd import _lib, ops
    n = _lib.load().vt_tactile_unet_workspace_bytes(depth, sf, shape[1], classes, shape[0], shape[2], shape[3])
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    with no_framework_ops():
        raw = ops.tactile_unet_fwd(xd, net, ops.tactile_unet_pack(net), ws=ws)
    print(rep)
    _report(f"f64:d{depth}:sf{sf}:{'x'.join(map(str, shape))}", rep)
    assert torch.equal(raw, y)
    assert torch.isfinite(y).all()
    assert rep["unsaturated"] >= 0.5, rep
    assert rep["hip_err"] <= 8 * rep["e32"], rep


def test_bit_reproducible_and_batch_invariant(hip):
    net = _net(seed=18).to(DEV)
    x5 = torch.rand(5, 3, 320, 240, generator=torch.Generator().manual_seed(5)).to(DEV)
    a, b = hip(net, x5), hip(net, x5)
    assert torch.equal(a, b)
    for i in range(5):
        assert torch.equal(hip(net, x5[i:i + 1].contiguous())[0], a[i]), i


def test_packed_weights_follow_load_state_dict_and_a_running_statistic(hip):
    net = _net(sf=8).to(DEV)
    x = torch.rand(2, 3, 16, 12, generator=torch.Generator().manual_seed(91)).to(DEV)
    y0 = hip(net, x)
    fresh = _net(sf=8, seed=17).to(DEV)
    net.load_state_dict(fresh.state_dict())
    y1 = hip(net, x)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, hip(fresh, x))
    with torch.no_grad():
        net.up_convs[1].bn.running_var.mul_(1.5)
    y2 = hip(net, x)
    assert not torch.equal(y2, y1)
    again = _net(sf=8, seed=17).to(DEV)
    again.load_state_dict(net.state_dict())
    assert torch.equal(y2, hip(again, x))
    with torch.no_grad():
        assert float((y2 - net.forward_modules(x)).abs().max()) <= 1e-5


def test_dispatch_falls_back_to_the_modules(monkeypatch):
    """hip_supported is False and the call IS the modules' (ops.tactile_unet_fwd raises if it is reached) for: autograd through the call,
    train mode, the host knob, H no multiple of 4 at depth 3 (where the modules' result is their error), CPU tensors.  The CPU result
    is compared with torch.equal (deterministic); on the device two calls of the framework's convolutions are held to f32 rounding."""
    from vtaco_amd import ops
    monkeypatch.setenv("VTACO_TACTILE_UNET", "hip")
    net = _net(sf=8).to(DEV)
    x = torch.rand(2, 3, 16, 12, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        assert net.hip_supported(x)

    def unreachable(*a, **k):
        raise AssertionError("the HIP forward ran where the nn modules must")
    monkeypatch.setattr(ops, "tactile_unet_fwd", unreachable)

    def close(a, b):
        return a.shape == b.shape and float((a - b).detach().abs().max()) <= 1e-6
    xg = x.clone().requires_grad_(True)
    assert not net.hip_supported(xg)
    assert close(net(xg), net.forward_modules(xg))
    net(xg).sum().backward()
    assert xg.grad is not None and float(xg.grad.abs().sum()) > 0
    with torch.no_grad():
        # H = 18 at depth 3: the modules cannot concatenate 8 up-sampled rows with 9 skipped ones (nor can the reference); the call must
        # reach them and fail as they do, not run a kernel on a shape it does not cover
        odd = torch.rand(1, 3, 18, 12, device=DEV)
        assert not net.hip_supported(odd)
        with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
            net.forward_modules(odd)
        with pytest.raises(RuntimeError, match="Sizes of tensors must match"):
            net(odd)
        cpu_net = _net(sf=8)
        assert not cpu_net.hip_supported(x.cpu())
        assert torch.equal(cpu_net(x.cpu()), cpu_net.forward_modules(x.cpu()))
        monkeypatch.setenv("VTACO_TACTILE_UNET", "host")
        assert not net.hip_supported(x)
        assert close(net(x), net.forward_modules(x))
        monkeypatch.setenv("VTACO_TACTILE_UNET", "hip")
        stats = copy.deepcopy(net.state_dict())
        net.train()
        assert not net.hip_supported(x)
        y_train = net(x)
        net.load_state_dict(stats)
        assert close(y_train, net.forward_modules(x))


def test_odd_sizes_run_on_the_kernels_at_depth_1(hip):
    """At depth 1 every size is covered: an odd one runs on the kernels and agrees with the modules."""
    d1 = _net(depth=1, sf=8).to(DEV)
    odd = torch.rand(1, 3, 9, 7, generator=torch.Generator().manual_seed(6)).to(DEV)
    y = hip(d1, odd)
    with torch.no_grad():
        assert float((y - d1.forward_modules(odd)).abs().max()) <= 1e-5


def test_batched_scenes_go_through_one_hip_call(hip):
    """encode_img_inputs at B > 1 in eval mode: all B x 5 images in one call, the per-scene results bit for bit."""
    from vtaco_amd.conv_onet.models import ConvolutionalOccupancyNetwork
    net = _net(sf=8)
    model = ConvolutionalOccupancyNetwork(None, None, None, net, None, device=DEV).eval()
    imgs = torch.rand(1, 5, 3, 16, 12, generator=torch.Generator().manual_seed(4)).to(DEV)
    two = torch.cat([imgs, imgs.flip(1)], dim=0)
    calls = []
    from vtaco_amd import ops
    real = ops.tactile_unet_fwd

    def counted(x, *a, **k):
        calls.append(x.shape[0])
        return real(x, *a, **k)
    ops.tactile_unet_fwd = counted
    try:
        with torch.no_grad(), no_framework_ops():
            both = model.encode_img_inputs(two)
            one = model.encode_img_inputs(imgs)
    finally:
        ops.tactile_unet_fwd = real
    assert calls == [10, 5]
    assert both.shape == (2, 5, 16 * 12)
    assert torch.equal(both[0:1], one) and torch.equal(both[1:2].flip(1), one)
