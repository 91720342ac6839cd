"""CPU: the host side of the tactile ResNet's train path (csrc/resnet2d_train.hip) -- the two host-only queries of the C ABI, the
workspace size against a restatement of the buffer list, and the dispatch rules of ``TactileResNet.forward`` (no kernel runs here)."""
import ctypes

import torch

from resnet_train_util import CASES, seeded_resnet, workspace_floats

R18, R34 = (2, 2, 2, 2), (3, 4, 6, 3)
KNOB = "VTACO_TACTILE_RESNET_TRAIN"


def _blocks(b):
    return (ctypes.c_int32 * 4)(*b)


def test_train_queries_answer_on_the_host():
    from vtaco_amd import _lib
    lib = _lib.load()
    for blocks in (R18, R34):
        for n, S, H, W in ((5, 1, 320, 240), (40, 8, 320, 240), (10, 2, 40, 24), (4, 2, 37, 45)):
            assert lib.vt_resnet_train_supported(_blocks(blocks), 32, n, S, H, W) == 1
            assert lib.vt_resnet_train_workspace_bytes(_blocks(blocks), 32, n, S, H, W) == 4 * workspace_floats(blocks, n, S, H, W)
    for name, S, G, (H, W), _ in CASES:
        blocks = R18 if name == "Resnet18" else R34
        assert lib.vt_resnet_train_workspace_bytes(_blocks(blocks), 8, S * G, S, H, W) == 4 * workspace_floats(blocks, S * G, S, H, W)
    # refused: 0
    bad = [(R18, 32, 5, 0, 320, 240), (R18, 32, 5, 2, 320, 240), (R18, 32, 0, 1, 320, 240), (R18, 0, 5, 1, 320, 240), ((2, 0, 2, 2), 32, 5, 1, 320, 240),
           (R18, 32, 1, 1, 32, 32),                                     # layer4 is 1 x 1: one value per scene and channel
           (R18, 32, 2, 2, 32, 32), (R18, 32, 5, 1, 0, 240), ((2, 2, 2, _lib.VT_RESNET_MAX_BLOCKS + 1), 32, 5, 1, 320, 240)]
    for blocks, nc, n, S, H, W in bad:
        assert lib.vt_resnet_train_supported(_blocks(blocks), nc, n, S, H, W) == 0, (blocks, nc, n, S, H, W)
        assert lib.vt_resnet_train_workspace_bytes(_blocks(blocks), nc, n, S, H, W) == 0
    assert lib.vt_resnet_train_supported(_blocks(R18), 32, 2, 1, 32, 32) == 1          # two images: two values
    assert lib.vt_resnet_train_supported(_blocks(R18), 32, 1, 1, 33, 32) == 1          # layer4 is 2 x 1


def test_ops_resnet_train_is_a_submodule_only():
    from vtaco_amd import ops
    assert callable(ops.resnet_train.fwd) and callable(ops.resnet_train.bwd) and callable(ops.resnet_train.supported)
    for name in ("fwd", "bwd", "supported", "workspace", "Workspace"):
        assert not hasattr(ops, name)


def test_dispatch_rules_with_a_probe_tensor(monkeypatch):
    from vtaco_amd import ops
    net = seeded_resnet("Resnet18", 90)
    x = torch.rand(4, 3, 40, 24, generator=torch.Generator().manual_seed(1))
    monkeypatch.setenv(KNOB, "hip")
    assert not net.train_hip_supported(x, 2)                               # a CPU tensor

    def boom(*a, **k):
        raise AssertionError("the HIP path was taken")
    monkeypatch.setattr(ops.resnet_train, "fwd", boom)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    a = net(x, scenes=2)
    net.load_state_dict(sd)
    assert torch.equal(a, net.forward_modules(x, 2)) and a.requires_grad

    class Probe:
        is_cuda, dtype, requires_grad, shape, device = True, torch.float32, False, (4, 3, 40, 24), torch.device("cpu")

        def dim(self):
            return 4
    seen = []
    monkeypatch.setattr(torch, "is_tensor", lambda t: True)
    monkeypatch.setattr(ops.resnet_train, "supported", lambda net, n, S, H, W: seen.append((n, S, H, W)) or True)
    assert net.train_hip_supported(Probe(), 2) and seen[-1] == (4, 2, 40, 24)
    assert not net.train_hip_supported(Probe(), 3)                         # 4 images are not 3 scenes
    assert not net.train_hip_supported(Probe(), 0)
    monkeypatch.setenv(KNOB, "host")
    assert not net.train_hip_supported(Probe(), 2)
    monkeypatch.delenv(KNOB)
    from vtaco_amd import layers
    assert net.train_hip_supported(Probe(), 2) == (layers._TACTILE_RESNET_TRAIN_DEFAULT == "hip")
    monkeypatch.setenv(KNOB, "hip")
    with torch.no_grad():
        assert not net.train_hip_supported(Probe(), 2)
    net.eval()
    assert not net.train_hip_supported(Probe(), 2)
    net.train()
    grad = Probe()
    grad.requires_grad = True
    assert not net.train_hip_supported(grad, 2)
    half = Probe()
    half.dtype = torch.float16
    assert not net.train_hip_supported(half, 2)
    net.requires_grad_(False)
    assert not net.train_hip_supported(Probe(), 2)                         # nothing to train
    net.requires_grad_(True)
    net.layer2[0].downsample[1].momentum = None
    assert not net.train_hip_supported(Probe(), 2)
    net.layer2[0].downsample[1].momentum = 0.1
    net.layer3[1].bn2.track_running_stats = False
    assert not net.train_hip_supported(Probe(), 2)
    net.layer3[1].bn2.track_running_stats = True
    assert net.train_hip_supported(Probe(), 2)
    net.layer1[0] = torch.nn.Identity()                                    # not a BasicBlock
    assert not net.train_hip_supported(Probe(), 2)
    # the eval path's rules are untouched by the knob
    net = seeded_resnet("Resnet18", 90).eval()
    monkeypatch.setattr(ops, "resnet_supported", lambda *a: True)
    with torch.no_grad():
        assert net.hip_supported(Probe())
