"""GPU: the workspace caches of the 2-D nets (vtaco_amd/ops/nets2d.py): eight entries, the oldest out first; one buffer per stream for
the tactile nets; ``fresh`` plane U-Net workspaces are never stored; a train workspace comes back as the same object with its ``gen``;
the eval caches and the plane U-Net hand every workspace they return to a graph that is being prepared, the train cache none.
Only workspaces are made: nothing is launched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tactile_unet_util import seeded_unet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = 4, 4                             # depth 1 covers every size (test_odd_sizes_run_on_the_kernels_at_depth_1)


@pytest.fixture
def nets2d(monkeypatch):
    """ops.nets2d with empty caches (the entries other tests left come back afterwards) and every launch turned into a failure."""
    from vtaco_amd import ops
    caches = (ops.nets2d._plane_unet_ws, ops.nets2d._resnet_ws, ops.nets2d._tactile_unet_ws, ops.nets2d._tactile_unet_train_ws)
    saved = [dict(c.entries) for c in caches]
    for c in caches:
        c.entries.clear()

    def launched(*a, **k):
        raise AssertionError("a kernel entry point was reached")
    monkeypatch.setattr(ops.nets2d, "check", launched)
    monkeypatch.setattr(ops.nets2d, "stream_ptr", launched)
    yield ops.nets2d
    for c, s in zip(caches, saved):
        c.entries.clear()
        c.entries.update(s)


def test_tactile_unet_cache_rule(nets2d):
    from vtaco_amd import ops
    net = seeded_unet(depth=1, sf=8).to(DEV)
    assert ops.tactile_unet_supported(net, 1, H, W)
    cache = nets2d._tactile_unet_ws.entries
    first = ops.tactile_unet_workspace(net, 1, H, W)
    first_key = next(iter(cache))
    assert ops.tactile_unet_workspace(net, 1, H, W) is first                 # same shape, same stream: the identical tensor
    with torch.cuda.stream(torch.cuda.Stream()):
        other = ops.tactile_unet_workspace(net, 1, H, W)                     # same shape, another stream: its own buffer
        assert ops.tactile_unet_workspace(net, 1, H, W) is other
    assert other is not first and other.data_ptr() != first.data_ptr() and len(cache) == 2
    cache.clear()
    for n_img in range(1, 10):                                               # nine shapes: eight stay, the first has left
        ops.tactile_unet_workspace(net, n_img, H, W)
    assert len(cache) == 8 and first_key not in cache
    assert [k[-3] for k in cache] == list(range(2, 10))
    with ops.graph_keepalive() as keep:                                      # a miss and a hit: both are handed to the graph's owner
        miss = ops.tactile_unet_workspace(net, 11, H, W)
        assert ops.tactile_unet_workspace(net, 11, H, W) is miss
    assert len(keep) == 2 and keep[0] is miss and keep[1] is miss


def test_resnet_cache_rule(nets2d):
    from vtaco_amd import ops
    from vtaco_amd.encoder import encoder_dict
    net = encoder_dict["Resnet18"](num_classes=32).eval().to(DEV)
    assert ops.resnet_supported(net, 1, 8, 8)
    cache = nets2d._resnet_ws.entries
    with ops.graph_keepalive() as keep:
        first = ops.resnet_workspace(net, 1, 8, 8)
        assert ops.resnet_workspace(net, 1, 8, 8) is first
        with torch.cuda.stream(torch.cuda.Stream()):
            other = ops.resnet_workspace(net, 1, 8, 8)
    assert other is not first and other.data_ptr() != first.data_ptr() and len(cache) == 2
    assert [id(t) for t in keep] == [id(first), id(first), id(other)]
    first_key = next(iter(cache))
    for n_img in range(2, 9):                                                # with the two above: nine entries made, eight kept
        ops.resnet_workspace(net, n_img, 8, 8)
    assert len(cache) == 8 and first_key not in cache


def test_plane_unet_fresh_workspaces_are_not_stored(nets2d):
    from vtaco_amd import ops
    from vtaco_amd.encoder.unet import UNet
    net = UNet(32, in_channels=32, depth=2, start_filts=32).to(DEV)
    assert ops.plane_unet_supported(net, 8, 8)
    a = ops.plane_unet_workspace(net, 1, 8, 8, fresh=True)
    b = ops.plane_unet_workspace(net, 1, 8, 8, fresh=True)
    assert a is not b and a.data_ptr() != b.data_ptr() and not nets2d._plane_unet_ws.entries
    shared = ops.plane_unet_workspace(net, 1, 8, 8)
    assert ops.plane_unet_workspace(net, 1, 8, 8) is shared and shared is not a and shared is not b
    assert ops.plane_unet_workspace(net, 1, 8, 8, fresh=True) is not shared and list(nets2d._plane_unet_ws.entries.values()) == [shared]
    with ops.graph_keepalive() as keep:                                      # every return is handed on: a hit and a fresh one
        hit, new = ops.plane_unet_workspace(net, 1, 8, 8), ops.plane_unet_workspace(net, 1, 8, 8, fresh=True)
    assert hit is shared and len(keep) == 2 and keep[0] is shared and keep[1] is new


def test_train_workspace_comes_back_with_its_gen(nets2d):
    from vtaco_amd import ops
    net = seeded_unet(depth=1, sf=8).train().to(DEV)
    assert ops.tactile_unet_train_supported(net, 2, 2, H, W)
    ws = ops.tactile_unet_train_workspace(net, 2, 2, H, W)
    assert isinstance(ws, ops.TactileUnetTrainWorkspace) and ws.gen == 0
    ws.gen = 5
    again = ops.tactile_unet_train_workspace(net, 2, 2, H, W)
    assert again is ws and again.gen == 5
    with ops.graph_keepalive() as keep:
        assert ops.tactile_unet_train_workspace(net, 2, 1, H, W) is not ws  # the group is part of the key
        assert ops.tactile_unet_train_workspace(net, 2, 2, H, W) is ws
    assert keep == []                                                        # the train cache hands nothing to a graph
