"""CPU: the Bottleneck tactile ResNets (Resnet50 / 101 / 152) -- the registry, the state_dict against the reference's (g29), the nn
modules against the reference's outputs, and the host side of the HIP path's C ABI (csrc/resnet2d_bneck.hip; no kernel runs here)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

R18, R50 = (2, 2, 2, 2), (3, 4, 6, 3)
T = torch.from_numpy


def _blocks(b):
    return (ctypes.c_int32 * 4)(*b)


def _fill(net, seed):
    sys.path.insert(0, GOLDEN)
    from make_resnet_bneck_goldens import bottleneck_fill
    bottleneck_fill(net, seed)
    return net


@pytest.fixture(scope="module")
def g29():
    return np.load(os.path.join(GOLDEN, "g29_resnet_bneck.npz"))


@pytest.fixture(scope="module")
def resnet50():
    from vtaco_amd.encoder import encoder_dict
    return _fill(encoder_dict["Resnet50"](num_classes=32), 90)


def test_registry_name_and_state_dict_equal_the_reference(g29, resnet50):
    from vtaco_amd.encoder import encoder_dict
    assert "Resnet50" in encoder_dict
    keys = [f"{k}:{tuple(v.shape)}" for k, v in resnet50.state_dict().items() if "num_batches_tracked" not in k]
    assert keys == [str(k) for k in g29["keys"]]
    # a reference-keyed state_dict loads (strict)
    sd = {}
    for entry in g29["keys"]:
        name, shape = str(entry).split(":")
        sd[name] = torch.zeros(eval(shape))
    for k, v in resnet50.state_dict().items():
        if "num_batches_tracked" in k:
            sd[k] = v.clone()
    fresh = encoder_dict["Resnet50"](num_classes=32)
    fresh.load_state_dict(sd)
    assert float(fresh.layer4[2].conv3.weight.detach().abs().max()) == 0.0


def test_g29_reference_outputs_on_the_modules(g29, resnet50):
    import copy
    net = copy.deepcopy(resnet50).eval()
    x = T(g29["x"])
    with torch.no_grad():
        y = net(x)
    ref = T(g29["y_eval"])
    assert float((y - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    net.train()
    with torch.no_grad():
        yt = net(x)
    ref = T(g29["y_train"])
    assert float((yt - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_forward_scenes_equals_the_per_scene_loop(g29, resnet50):
    """One pass over the S * F images with per-scene statistics IS the loop over the scenes, in exact arithmetic: checked in float64 to
    1e-9 (values, running statistics) in both modes.  In f32 the eval mode agrees to rounding (1e-5); the train mode at ONE 64x48 image
    per scene takes layer4's statistics from 4 values per channel, where the f32 loop itself is 1.7e-3 from its float64 copy, so there
    the f32 pass is held to 8 x that error of the loop's (the factor of tests/test_resnet_gpu.py::_f64_gate)."""
    import copy
    imgs = T(g29["x"]).unsqueeze(1)                                         # [2, 1, 3, 64, 48]
    for train in (False, True):
        a, b = copy.deepcopy(resnet50).double().train(train), copy.deepcopy(resnet50).double().train(train)
        with torch.no_grad():
            got64 = a.forward_scenes(imgs.double())
            ref64 = torch.stack([b(imgs[s].double()) for s in range(imgs.shape[0])])
        assert got64.shape == ref64.shape == (2, 1, 32)
        assert float((got64 - ref64).abs().max()) <= 1e-9 * float(ref64.abs().max()), train
        for (k, u), v in zip(a.state_dict().items(), b.state_dict().values()):
            assert float((u.double() - v.double()).abs().max()) <= 1e-9 * max(1.0, float(v.double().abs().max())), k
        a, b = copy.deepcopy(resnet50).train(train), copy.deepcopy(resnet50).train(train)
        with torch.no_grad():
            got = a.forward_scenes(imgs)
            ref = torch.stack([b(imgs[s]) for s in range(imgs.shape[0])])
        e_loop = float((ref.double() - ref64).abs().max())
        bound = 8 * e_loop if train else 1e-5 * float(ref64.abs().max())
        assert float((got.double() - ref64).abs().max()) <= bound, (train, e_loop)
    assert int(a.layer2[0].bn3.num_batches_tracked) == 2


def test_block_counts_and_the_stride_1_projection():
    from vtaco_amd import layers
    for ctor, counts in ((layers.Resnet50, (3, 4, 6, 3)), (layers.Resnet101, (3, 4, 23, 3)), (layers.Resnet152, (3, 8, 36, 3))):
        net = ctor(num_classes=8)
        assert tuple(len(s) for s in (net.layer1, net.layer2, net.layer3, net.layer4)) == counts
        assert all(type(blk).expansion == 4 for blk in net.layer1)
        proj = net.layer1[0].downsample
        assert proj is not None and proj[0].stride == (1, 1) and proj[0].weight.shape == (256, 64, 1, 1)
        assert net.layer1[1].downsample is None
        assert net.layer2[0].conv1.stride == (1, 1) and net.layer2[0].conv2.stride == (2, 2) and net.layer2[0].downsample[0].stride == (2, 2)
        assert net.linear.in_features == 2048 and net.fc.out_features == 8
        assert len(net._batchnorms()) == sum(1 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
        x = torch.rand(2, 3, 40, 24)
        assert not net.train_hip_supported(x) and not net.hip_supported(x)
    # the BasicBlock nets are what they were
    r18 = layers.Resnet18(8)
    assert r18.layer1[0].downsample is None and r18.linear.in_features == 512 and not hasattr(r18.layer1[0], "conv3")


def test_bneck_size_queries_answer_on_the_host(resnet50):
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    # the blob: the stem with kx padded to 8; every conv weight once; ONE bias per BatchNorm'd conv, the projection sharing conv3's;
    # linear.weight; linear.bias, fc.weight, fc.bias padded to multiples of 4
    floats = 0
    for k, v in resnet50.state_dict().items():
        if k == "conv1.weight":
            floats += 64 * 3 * 7 * 8
        elif k.endswith("conv1.weight") or k.endswith("conv2.weight") or k.endswith("conv3.weight") or k.endswith("downsample.0.weight"):
            floats += v.numel()
        elif k.endswith(".bias") and ("bn" in k) :
            floats += v.numel()
    pad4 = lambda n: (n + 3) // 4 * 4
    floats += 100 * 2048 + pad4(100) + pad4(32 * 100) + pad4(32)
    assert lib.vt_resnet_bneck_blob_bytes(_blocks(R50), 32) == 4 * floats
    assert lib.vt_resnet_bneck_blob_bytes(_blocks(R50), 0) == 0
    for blocks in (R50, (3, 4, 23, 3), (3, 8, 36, 3), (1, 1, 1, 1)):
        for n, H, W in ((5, 320, 240), (2, 64, 48), (1, 33, 47)):
            assert lib.vt_resnet_bneck_supported(_blocks(blocks), 32, n, H, W) == 1
            assert lib.vt_resnet_bneck_workspace_bytes(_blocks(blocks), 32, n, H, W) == 4 * ops.resnet_bneck.workspace_floats(blocks, n, H, W)
    assert ops.resnet_bneck.workspace_floats(R50, 5, 320, 240) == 4 * 5 * 80 * 60 * 256
    assert ops.resnet_bneck.workspace_floats(R50, 1, 1, 1) == 4 * 2048
    bad = [((3, 0, 6, 3), 32, 5, 320, 240), ((3, 4, _lib.VT_RESNET_MAX_BLOCKS + 1, 3), 32, 5, 320, 240), (R50, 32, 0, 320, 240),
           (R50, 0, 5, 320, 240), (R50, 32, 5, 0, 240), (R50, 32, 5, 320, 2049), (R50, 32, 1025, 32, 32)]
    for blocks, nc, n, H, W in bad:
        assert lib.vt_resnet_bneck_supported(_blocks(blocks), nc, n, H, W) == 0
        assert lib.vt_resnet_bneck_workspace_bytes(_blocks(blocks), nc, n, H, W) == 0
    # every buffer below 2^31 elements, the widest being four times the BasicBlock net's: n * 512 * 512 * 256
    assert lib.vt_resnet_bneck_supported(_blocks(R50), 32, 31, 2048, 2048) == 1
    assert lib.vt_resnet_bneck_supported(_blocks(R50), 32, 32, 2048, 2048) == 0
    # the BasicBlock queries answer what they did
    assert lib.vt_resnet_supported(_blocks(R18), 32, 127, 2048, 2048) == 1 and lib.vt_resnet_supported(_blocks(R18), 32, 128, 2048, 2048) == 0
    assert lib.vt_resnet_workspace_bytes(_blocks(R18), 32, 5, 320, 240) == 4 * 4 * 5 * 80 * 60 * 64
    assert ctypes.sizeof(_lib.ResnetParams) == 24 + 8 + 40 + 4 * 36 * (3 * 8 + 3 * 40) + 32


def test_dispatch_and_the_knob(resnet50, monkeypatch):
    import copy
    from vtaco_amd import ops
    net = copy.deepcopy(resnet50).eval()

    class Probe:
        is_cuda, dtype, requires_grad, shape = True, torch.float32, False, (2, 3, 40, 24)

        def dim(self):
            return 4
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)
    monkeypatch.setattr(ops.resnet_bneck, "supported", lambda *a: True)
    monkeypatch.setattr(ops, "resnet_supported", lambda *a: False)
    with torch.no_grad():
        monkeypatch.setenv("VTACO_TACTILE_BOTTLENECK", "hip")
        assert net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_RESNET", "host")                 # (the BasicBlock nets' knob does not reach this net)
        assert net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_BOTTLENECK", "host")
        assert not net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_BOTTLENECK", "hip")
        net.train()
        assert not net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_BOTTLENECK", "fast")
        with pytest.raises(ValueError):
            net.hip_supported(Probe())


def test_trains_through_the_modules(resnet50):
    import copy
    net = copy.deepcopy(resnet50).train()
    x = torch.rand(2, 3, 40, 24, generator=torch.Generator().manual_seed(1))
    before = net.layer3[0].bn3.running_mean.clone()
    net(x).square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    assert float(net.layer1[0].conv3.weight.grad.abs().max()) > 0
    assert not torch.equal(net.layer3[0].bn3.running_mean, before)
