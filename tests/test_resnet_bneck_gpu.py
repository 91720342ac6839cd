"""GPU: the Bottleneck tactile ResNets' eval-mode forward on the HIP kernels (vt_resnet_bneck_pack / vt_resnet_bneck_fwd,
csrc/resnet2d_bneck.hip), through ``TactileResNet.forward`` and through raw ``ops.resnet_bneck.fwd``.  Every test sets
VTACO_TACTILE_BOTTLENECK=hip itself (it does not depend on the default), and in every test of the HIP path F.conv2d, F.batch_norm,
F.max_pool2d, F.adaptive_avg_pool2d and F.linear raise, so a silent fall-back to the nn modules cannot pass."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
_PATCHED = ("conv2d", "batch_norm", "max_pool2d", "adaptive_avg_pool2d", "linear")
BLOCKS = {"Resnet50": (3, 4, 6, 3), "Resnet101": (3, 4, 23, 3), "all-project": (1, 1, 1, 1)}


@pytest.fixture(autouse=True)
def _hip_knob(monkeypatch):
    monkeypatch.setenv("VTACO_TACTILE_BOTTLENECK", "hip")


class no_framework_ops:
    """``with no_framework_ops():`` -- the functional ops the nn modules of the ResNet go through raise."""

    def __enter__(self):
        self.saved = {n: getattr(F, n) for n in _PATCHED}

        def boom(*a, **k):
            raise AssertionError("a framework operator ran under the HIP tactile ResNet")
        for n in _PATCHED:
            setattr(F, n, boom)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(F, n, f)
        return False


def _report(name, rep):
    out = os.environ.get("VTACO_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "out")
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "resnet_bneck_gpu.json")
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur[name] = rep
        json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


def _net(name, classes=32, seed=90):
    sys.path.insert(0, GOLDEN)
    from make_resnet_bneck_goldens import bottleneck_fill
    from vtaco_amd import layers
    net = layers.TactileResNet(BLOCKS[name], num_classes=classes, block=layers._Bottleneck)
    bottleneck_fill(net, seed)
    return net.eval()


def _hip(net, x):
    with torch.no_grad(), no_framework_ops():
        assert net.hip_supported(x)
        return net(x)


def _module_tensors(net, x):
    """[layer1 .. layer4 outputs as channels-last [n, h, w, C], logits] of the nn modules."""
    out = []
    with torch.no_grad():
        y = net.maxpool(F.relu(net.bn1(net.conv1(x))))
        for stage in (net.layer1, net.layer2, net.layer3, net.layer4):
            y = stage(y)
            out.append(y.permute(0, 2, 3, 1).contiguous())
        out.append(net.fc(net.linear(torch.flatten(net.avgpool(y), 1))))
    return out


def _f64_gate(net_cpu, x, hip_tensors):
    """Per tensor (the four stage outputs, the logits): max |hip - t64| <= 8 * e32, t64 from a .double() copy of the host module on the
    CPU, e32 the max error of the same host module in f32 on the CPU against it: the gate and the argument of
    tests/test_resnet_gpu.py::_f64_gate, elementwise max abs on each tensor."""
    t64 = _module_tensors(copy.deepcopy(net_cpu).double(), x.double())
    t32 = _module_tensors(net_cpu, x)
    rep = {}
    for name, a64, a32, hip in zip(("layer1", "layer2", "layer3", "layer4", "logits"), t64, t32, hip_tensors):
        assert hip.shape == a64.shape, (name, hip.shape, a64.shape)
        e32 = float((a32.double() - a64).abs().max())
        err = float((hip.double().cpu() - a64).abs().max())
        rep[name] = {"e32": e32, "hip_err": err, "max": float(a64.abs().max()), "ratio": err / e32}
    return rep


def test_g29_reference_golden_eval_on_hip():
    z = np.load(os.path.join(GOLDEN, "g29_resnet_bneck.npz"))
    net = _net("Resnet50").to(DEV)
    y = _hip(net, T(z["x"]).to(DEV)).cpu()
    ref = T(z["y_eval"])
    rep = {"max_abs_err": float((y - ref).abs().max()), "output_max": float(ref.abs().max())}
    print(rep)
    _report("g29", rep)
    assert rep["max_abs_err"] <= 1e-4 * rep["output_max"], rep


F64_CASES = [("Resnet50", (1, 3, 33, 47), 9), ("Resnet50", (3, 3, 70, 50), 8), ("Resnet50", (2, 3, 64, 48), 91),
             ("all-project", (2, 3, 40, 40), 11), ("Resnet101", (1, 3, 33, 47), 9), ("Resnet50", (5, 3, 320, 240), 7)]


@pytest.mark.parametrize("name,shape,seed", F64_CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s, _ in F64_CASES])
def test_against_float64_per_stage_and_raw_path(name, shape, seed):
    from vtaco_amd import ops
    cpu = _net(name)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(seed))
    net = copy.deepcopy(cpu).to(DEV)
    xd = x.to(DEV)
    y = _hip(net, xd)
    # raw ops.resnet_bneck.fwd with a blob and a workspace of its own: the module path's bits, with and without the stage taps
    with no_framework_ops():
        blob = ops.resnet_bneck.pack(net)
        ws = torch.empty(4 * ops.resnet_bneck.workspace_floats(BLOCKS[name], *shape[:1], *shape[2:]), dtype=torch.uint8, device=DEV)
        raw = ops.resnet_bneck.fwd(xd, net, blob, ws=ws)
        tapped, stages = ops.resnet_bneck.fwd(xd, net, blob, ws=ws, stages=True)
    assert torch.equal(raw, y) and torch.equal(tapped, y)
    assert torch.isfinite(y).all()
    rep = _f64_gate(cpu, x, stages + [y])
    print(rep)
    _report(f"f64:{name}:{'x'.join(map(str, shape))}", rep)
    for tensor, r in rep.items():
        assert r["hip_err"] <= 8 * r["e32"], (tensor, r)


def test_bit_reproducible_and_batch_invariant():
    net = _net("Resnet50").to(DEV)
    x12 = torch.rand(12, 3, 96, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    x3 = x12[4:7].contiguous()
    a, b = _hip(net, x3), _hip(net, x3)
    assert torch.equal(a, b)
    assert torch.equal(_hip(net, x12)[4:7], a)
    for i in range(3):
        assert torch.equal(_hip(net, x3[i:i + 1].contiguous())[0], a[i]), i


def test_graph_capture_on_a_side_stream_and_two_encoders_on_two_streams():
    from vtaco_amd import ops
    net = _net("Resnet50").to(DEV)
    x = torch.rand(3, 3, 70, 50, generator=torch.Generator().manual_seed(8)).to(DEV)
    eager = _hip(net, x)
    side = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_keepalive() as keep:
        with torch.cuda.graph(graph, stream=side):
            with torch.no_grad(), no_framework_ops():
                out = net(x)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del keep
    # two encoders with different weights on two streams at once: the results they give alone
    other = _net("Resnet50", seed=17).to(DEV)
    alone_a, alone_b = eager, _hip(other, x)
    assert not torch.equal(alone_a, alone_b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    for _ in range(4):
        got = []
        for s, n in ((s1, net), (s2, other)):
            with torch.cuda.stream(s):
                got.append([_hip(n, x) for _ in range(3)])
        torch.cuda.synchronize()
        for ya, yb in zip(*got):
            assert torch.equal(ya, alone_a) and torch.equal(yb, alone_b)


def test_packed_weights_follow_load_state_dict_and_a_train_mode_forward():
    net = _net("Resnet50").to(DEV)
    x = torch.rand(2, 3, 64, 48, generator=torch.Generator().manual_seed(91)).to(DEV)
    y0 = _hip(net, x)
    fresh = _net("Resnet50", seed=17).to(DEV)
    net.load_state_dict(fresh.state_dict())
    y1 = _hip(net, x)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, _hip(fresh, x))
    net.train()
    with torch.no_grad():
        net(x)                                                             # moves every running statistic
    net.eval()
    y2 = _hip(net, x)
    assert not torch.equal(y2, y1)
    again = _net("Resnet50", seed=17).to(DEV)
    again.load_state_dict(net.state_dict())
    assert torch.equal(y2, _hip(again, x))


def test_generation_route_with_a_resnet50_image_encoder():
    """The VTacOH model with ``encoder_img`` swapped for a filled Resnet50: encode_img_inputs meets the f64 gate against the CPU modules,
    and 4 successive generate_obj_mesh_wnf calls -- eager, capturing, replays -- give a non-empty mesh with the SAME vertices and
    faces bit for bit."""
    from vtaco_amd.bench_util import build_tactile_scene
    from vtaco_amd.conv_onet.generation import Generator3D
    model, data, depth_origin = build_tactile_scene(torch.device(DEV), variant="vtacoh")
    cpu = _net("Resnet50")
    model.encoder_img = copy.deepcopy(cpu).to(DEV)
    model.eval()
    imgs = data["inputs.img"]
    with torch.no_grad(), no_framework_ops():
        c = model.encode_img_inputs(imgs.to(DEV))
    assert c.shape == (1, imgs.shape[1], 32)
    with torch.no_grad():
        c64 = copy.deepcopy(cpu).double()(imgs[0].double())
        c32 = cpu.forward_modules(imgs[0])
    e32 = float((c32.double() - c64).abs().max())
    err = float((c[0].double().cpu() - c64).abs().max())
    rep = {"e32": e32, "hip_err": err, "max": float(c64.abs().max()), "ratio": err / e32}
    print(rep)
    _report("generation:encode_img_inputs", rep)
    assert err <= 8 * e32, rep
    gen = Generator3D(model, device=torch.device(DEV), resolution0=16, padding=0.1, with_img=True, encode_t2d=False, depth_origin=depth_origin)
    got = []
    for _ in range(4):
        np.random.seed(11)
        m = gen.generate_obj_mesh_wnf(data)
        got.append((m.vertices.clone(), m.faces.clone()))
    assert got[0][0].shape[0] > 0 and got[0][1].shape[0] > 0
    for v, f in got[1:]:
        assert torch.equal(v, got[0][0]) and torch.equal(f, got[0][1])
