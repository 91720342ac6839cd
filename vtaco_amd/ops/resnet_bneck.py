"""The tactile ResNet with Bottleneck blocks (Resnet50 / 101 / 152) in eval mode (resnet2d_bneck.hip): ``supported``, ``params``, ``pack``,
``workspace``, ``workspace_floats``, ``fwd``.  Callers write ``ops.resnet_bneck.fwd(...)``: nothing of this module is re-exported by the
package."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c, keep_for_graph
from .nets2d import _Pointers, _WorkspaceCache, _pack, resnet_workspace_floats


def workspace_floats(blocks_num, n_img, H, W):
    """The documented size of vt_resnet_bneck_fwd's workspace: four buffers of the largest stage's output [n_img][Hs][Ws][4 * (64 << s)],
    Hs = ceil(H / 2^(s + 2))."""
    return 4 * resnet_workspace_floats(blocks_num, n_img, H, W)


def _dims(net):
    prm = _lib.ResnetBneckParams()
    prm.blocks_num[:] = [len(stage) for stage in (net.layer1, net.layer2, net.layer3, net.layer4)]
    prm.num_classes = int(net.fc.out_features)
    return prm


def supported(net, n_img, H, W):
    prm = _dims(net)
    if max(prm.blocks_num) > _lib.VT_RESNET_MAX_BLOCKS or net.linear.in_features != 2048 or net.linear.out_features != 100:
        return False
    return bool(_lib.load().vt_resnet_bneck_supported(prm.blocks_num, prm.num_classes, int(n_img), int(H), int(W)))


def params(net):
    """(ResnetBneckParams, tensors it points to) of a ``layers.TactileResNet`` with Bottleneck blocks, in the state_dict's own layouts."""
    prm, p = _dims(net), _Pointers("resnet_bneck.pack")
    prm.conv1_w = p.ptr(net.conv1.weight, "conv1.weight")
    p.bn(prm.bn1, net.bn1, "bn1")
    for s, stage in enumerate((net.layer1, net.layer2, net.layer3, net.layer4)):
        for b, blk in enumerate(stage):
            k, name = prm.block[s][b], f"layer{s + 1}.{b}"
            for i in (1, 2, 3):
                setattr(k, f"conv{i}_w", p.ptr(getattr(blk, f"conv{i}").weight, f"{name}.conv{i}.weight"))
                p.bn(getattr(k, f"bn{i}"), getattr(blk, f"bn{i}"), f"{name}.bn{i}")
            if (blk.downsample is not None) != (b == 0):
                raise VtError(f"resnet_bneck.pack: {name}: a projection where the Bottleneck net has none (or none where it has one)")
            if blk.downsample is not None:
                k.down_w = p.ptr(blk.downsample[0].weight, name + ".downsample.0.weight")
                p.bn(k.down_bn, blk.downsample[1], name + ".downsample.1")
    prm.linear_w, prm.linear_b = p.ptr(net.linear.weight, "linear.weight"), p.ptr(net.linear.bias, "linear.bias")
    prm.fc_w, prm.fc_b = p.ptr(net.fc.weight, "fc.weight"), p.ptr(net.fc.bias, "fc.bias")
    return prm, p.keep


def pack(net):
    """The net's convs with their BatchNorms folded in, in fragment order, + linear and fc: the blob vt_resnet_bneck_fwd reads."""
    lib = _lib.load()
    prm = _dims(net)
    n = lib.vt_resnet_bneck_blob_bytes(prm.blocks_num, prm.num_classes) if max(prm.blocks_num) <= _lib.VT_RESNET_MAX_BLOCKS else 0
    if n == 0:
        raise VtError("Bottleneck tactile ResNet not built for this net (vt_resnet_bneck_supported)")
    return _pack("vt_resnet_bneck_pack", n, *params(net))


# (device, stream, blocks, classes, images, H, W) -> workspace
_ws = _WorkspaceCache("vt_resnet_bneck_workspace_bytes", "Bottleneck tactile ResNet shape not built (vt_resnet_bneck_supported)")


def workspace(net, n_img, H, W):
    """Workspace of vt_resnet_bneck_fwd, one per (device, STREAM, shape), like resnet_workspace."""
    prm, shape = _dims(net), (int(n_img), int(H), int(W))
    ws = _ws.get((torch.cuda.current_stream().cuda_stream, tuple(prm.blocks_num), prm.num_classes, *shape),
                              prm.blocks_num, prm.num_classes, *shape)
    keep_for_graph(ws)
    return ws


def fwd(x, net, blob, ws=None, stages=False):
    """TactileResNet.forward with Bottleneck blocks in eval mode on the HIP kernels: x [n_img, 3, H, W] -> [n_img, num_classes]
    (vt_resnet_bneck_fwd).  ``stages=True`` returns (out, [layer1..layer4 outputs, channels-last [n_img, Hs, Ws, 4 * (64 << s)]])."""
    x = _c(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise VtError(f"resnet_bneck.fwd: input must be [n_img, 3, H, W] (got {tuple(x.shape)})")
    n_img, _, H, W = x.shape
    if ws is None:
        ws = workspace(net, n_img, H, W)
    prm = _dims(net)
    out = torch.empty((n_img, prm.num_classes), dtype=torch.float32, device=x.device)
    taps, tap_ptrs = [], None
    if stages:
        up = lambda v: (v - 1) // 2 + 1
        h, w = up(up(H)), up(up(W))
        for s in range(4):
            taps.append(torch.empty((n_img, h, w, 4 * (64 << s)), dtype=torch.float32, device=x.device))
            h, w = up(h), up(w)
        tap_ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in taps])
    keep_for_graph(blob, x)
    check(_lib.load().vt_resnet_bneck_fwd(dev_ptr(x, "x"), n_img, H, W, ctypes.byref(prm), dev_ptr(blob, "blob"),
                                          ctypes.c_void_p(ws.data_ptr()), ws.numel(), dev_ptr(out, "out"), tap_ptrs, stream_ptr()),
          "vt_resnet_bneck_fwd")
    return (out, taps) if stages else out
