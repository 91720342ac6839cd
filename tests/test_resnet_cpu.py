"""CPU: the host side of the tactile ResNet's HIP path (csrc/resnet2d.hip) -- the size queries of the C ABI, the BatchNorm fold
vt_resnet_pack computes, and the dispatch rules of ``TactileResNet.forward`` (no kernel runs here)."""
import ctypes
import os
import sys

import pytest
import torch
from torch.nn import functional as F

from conftest import GOLDEN

R18, R34 = (2, 2, 2, 2), (3, 4, 6, 3)


def _blocks(b):
    return (ctypes.c_int32 * 4)(*b)


def _fill(net, seed):
    sys.path.insert(0, GOLDEN)
    from make_resnet_goldens import deterministic_fill
    deterministic_fill(net, seed)
    return net


def test_resnet_size_queries_answer_on_the_host():
    from vtaco_amd import _lib, ops
    lib = _lib.load()
    for blocks in (R18, R34):
        for n, H, W in ((5, 320, 240), (2, 96, 64)):
            assert lib.vt_resnet_supported(_blocks(blocks), 32, n, H, W) == 1
            assert lib.vt_resnet_blob_bytes(_blocks(blocks), 32) > 0
            # four buffers of the largest stage's activations, sizes ceil(H / 4), ceil(H / 8), ... (320 x 240: 80 x 60 down to 10 x 8)
            assert lib.vt_resnet_workspace_bytes(_blocks(blocks), 32, n, H, W) == 4 * ops.resnet_workspace_floats(blocks, n, H, W)
    assert ops.resnet_workspace_floats(R18, 5, 320, 240) == 4 * 5 * 80 * 60 * 64
    assert ops.resnet_workspace_floats(R18, 1, 1, 1) == 4 * 512             # one pixel everywhere: the widest stage decides
    # the blob: every conv weight once, a bias per conv, linear and fc
    convs = 64 * 3 * 8 * 7 + 64                                            # the stem's kx padded to 8
    cin = 64
    for s, nb in enumerate(R18):
        c = 64 << s
        for b in range(nb):
            convs += c * cin * 9 + c + c * c * 9 + c + ((c * cin + c) if (s > 0 and b == 0) else 0)
            cin = c
    assert lib.vt_resnet_blob_bytes(_blocks(R18), 32) == 4 * (convs + 100 * 512 + 100 + 32 * 100 + 32)
    # refused: size 0
    bad = [(R18, 32, 0, 320, 240), (R18, 0, 5, 320, 240), ((2, 0, 2, 2), 32, 5, 320, 240), (R18, 32, 5, 0, 240), (R18, 32, 5, 320, 0),
           (R18, 32, -1, 320, 240), ((2, 2, 2, _lib.VT_RESNET_MAX_BLOCKS + 1), 32, 5, 320, 240)]
    for blocks, nc, n, H, W in bad:
        assert lib.vt_resnet_supported(_blocks(blocks), nc, n, H, W) == 0
        assert lib.vt_resnet_workspace_bytes(_blocks(blocks), nc, n, H, W) == 0
    assert lib.vt_resnet_blob_bytes(_blocks(R18), 0) == 0
    assert lib.vt_resnet_blob_bytes(_blocks((2, 0, 2, 2)), 32) == 0
    # the limits the header states, at the edge: H, W <= 2048, n_img <= 1024, every tensor below 2^31 elements
    assert lib.vt_resnet_supported(_blocks(R18), 32, 1, 2048, 64) == 1 and lib.vt_resnet_supported(_blocks(R18), 32, 1, 2049, 64) == 0
    assert lib.vt_resnet_supported(_blocks(R18), 32, 1, 64, 2048) == 1 and lib.vt_resnet_supported(_blocks(R18), 32, 1, 64, 2049) == 0
    assert lib.vt_resnet_supported(_blocks(R18), 32, 1024, 32, 32) == 1 and lib.vt_resnet_supported(_blocks(R18), 32, 1025, 32, 32) == 0
    assert lib.vt_resnet_supported(_blocks(R18), 32, 127, 2048, 2048) == 1                   # layer1's tensor: n * 512 * 512 * 64 < 2^31
    assert lib.vt_resnet_supported(_blocks(R18), 32, 128, 2048, 2048) == 0
    assert lib.vt_resnet_supported(_blocks((36, 36, 36, 36)), 32, 1, 64, 64) == 1


def test_batchnorm_fold_equals_bn_of_conv_in_float64():
    from vtaco_amd import ops
    from vtaco_amd.layers import Resnet18
    net = _fill(Resnet18(32), 90).double().eval()
    g = torch.Generator().manual_seed(3)
    blk = net.layer2[0]
    cases = [(net.conv1, net.bn1, torch.rand(2, 3, 37, 29, generator=g, dtype=torch.float64)),                 # the stem
             (blk.conv1, blk.bn1, torch.randn(2, 64, 13, 11, generator=g, dtype=torch.float64)),               # 3x3 stride 2
             (blk.downsample[0], blk.downsample[1], torch.randn(2, 64, 13, 11, generator=g, dtype=torch.float64))]   # 1x1 projection
    for conv, bn, x in cases:
        w, b = ops.resnet_fold_bn(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        assert w.dtype == torch.float64 and b.dtype == torch.float64
        with torch.no_grad():
            ref = bn(conv(x))
            got = F.conv2d(x, w, b, stride=conv.stride, padding=conv.padding)
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_dispatch_keeps_the_modules_off_the_device_in_train_mode_and_under_autograd(monkeypatch):
    from vtaco_amd import ops
    from vtaco_amd.layers import Resnet18
    net = _fill(Resnet18(8), 90)

    def boom(*a, **k):
        raise AssertionError("the HIP path was taken")
    monkeypatch.setattr(ops, "resnet_fwd", boom)
    monkeypatch.setattr(ops, "resnet_pack", boom)
    x = torch.rand(2, 3, 40, 24, generator=torch.Generator().manual_seed(1))
    net.eval()
    assert not net.hip_supported(x)                                        # a CPU tensor
    with torch.no_grad():
        assert torch.equal(net(x), net.forward_modules(x))
    assert torch.equal(net(x), net.forward_modules(x))                     # grad enabled
    assert net(x).requires_grad
    net.train()
    assert not net.hip_supported(x)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        a = net(x)
    net.load_state_dict(sd)
    with torch.no_grad():
        b = net.forward_modules(x)
    assert torch.equal(a, b)

    # a fake device tensor would need a GPU; the rules themselves: eval + no autograd is the only way in
    class Probe:
        is_cuda, dtype, requires_grad, shape = True, torch.float32, False, (2, 3, 40, 24)

        def dim(self):
            return 4
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)
    monkeypatch.setattr(ops, "resnet_supported", lambda *a: True)
    net.eval()
    assert not net.hip_supported(Probe())                                  # parameters require grad and grad is enabled
    with torch.no_grad():
        assert net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_RESNET", "host")
        assert not net.hip_supported(Probe())
        monkeypatch.setenv("VTACO_TACTILE_RESNET", "hip")
        net.train()
        assert not net.hip_supported(Probe())
    net.eval()
    net.requires_grad_(False)
    assert net.hip_supported(Probe())                                      # grad enabled but nothing requires it


def test_blob_stamp_follows_parameters_and_buffers():
    from vtaco_amd.layers import Resnet18
    net = _fill(Resnet18(8), 90)
    s0 = net._blob_stamp()
    assert net._blob_stamp() == s0
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    s1 = net._blob_stamp()
    assert s1 != s0
    with torch.no_grad():
        net.layer3[0].bn1.running_mean.add_(0.5)
    s2 = net._blob_stamp()
    assert s2 != s1
    net.train()
    with torch.no_grad():
        net(torch.rand(2, 3, 33, 20))                                      # a train-mode forward moves the running statistics
    assert net._blob_stamp() != s2
