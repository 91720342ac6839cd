"""The tactile ResNet in train mode (resnet2d_train.hip): ``supported``, ``workspace``, ``fwd``, ``bwd``.  Callers write
``ops.resnet_train.fwd(...)``: nothing of this module is re-exported by the package."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c
from .nets2d import _WorkspaceCache, _grad_table, _resnet_dims, resnet_params


def supported(net, n_img, scenes, H, W):
    prm = _resnet_dims(net)
    if max(prm.blocks_num) > _lib.VT_RESNET_MAX_BLOCKS or net.linear.in_features != 512 or net.linear.out_features != 100:
        return False
    return bool(_lib.load().vt_resnet_train_supported(prm.blocks_num, prm.num_classes, int(n_img), int(scenes), int(H), int(W)))


class Workspace:
    """The workspace of one (device, stream, shape): the forward fills it and the backward reads it.  ``gen`` counts the forwards that
    wrote it, so a backward can tell whether its forward was the last one (layers._TactileResNetTrain runs the forward again if not)."""

    def __init__(self, buf):
        self.buf, self.gen = buf, 0


# (device, stream, blocks, classes, images, scenes, H, W) -> Workspace
_ws = _WorkspaceCache("vt_resnet_train_workspace_bytes", "tactile ResNet train shape not built (vt_resnet_train_supported)", wrap=Workspace)


def workspace(net, n_img, scenes, H, W):
    """Workspace of vt_resnet_train_fwd / vt_resnet_bwd, one per (device, STREAM, shape), like nets2d.resnet_workspace."""
    prm, shape = _resnet_dims(net), (int(n_img), int(scenes), int(H), int(W))
    return _ws.get((torch.cuda.current_stream().cuda_stream, tuple(prm.blocks_num), prm.num_classes, *shape),
                   prm.blocks_num, prm.num_classes, *shape)


def _shape(x, scenes, who):
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] % int(scenes):
        raise VtError(f"{who}: input must be [F * scenes, 3, H, W] (got {tuple(x.shape)}, scenes {scenes})")
    return x.shape[0], x.shape[2], x.shape[3]


def fwd(x, net, scenes=1, momentum=None, ws=None):
    """TactileResNet.forward in train mode on the HIP kernels (vt_resnet_train_fwd): x [F * scenes, 3, H, W], image-major (image f of
    scene b at row f * scenes + b), every BatchNorm with the statistics of each scene's F images alone -> [F * scenes, num_classes].
    ``momentum`` (a float): every running_mean / running_var is updated in place as ``scenes`` sequential calls would; None leaves
    them alone (num_batches_tracked is the caller's).  ``ws`` (``workspace``) keeps what ``bwd`` reads."""
    x = _c(x)
    n_img, H, W = _shape(x, scenes, "resnet_train.fwd")
    if ws is None:
        ws = workspace(net, n_img, scenes, H, W)
    prm, keep = resnet_params(net)
    out = torch.empty((n_img, prm.num_classes), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_resnet_train_fwd(dev_ptr(x, "x"), n_img, int(scenes), H, W, ctypes.byref(prm), -1.0 if momentum is None else float(momentum),
                                          ctypes.c_void_p(ws.buf.data_ptr()), ws.buf.numel(), dev_ptr(out, "out"), stream_ptr()),
          "vt_resnet_train_fwd")
    ws.gen += 1
    return out


def bwd(dout, x, net, scenes, ws):
    """Backward of ``fwd`` (vt_resnet_bwd): {parameter name: gradient} for every parameter of the net from dout, the input and the
    workspace the forward filled.  Gradients are written, not accumulated."""
    dout, x = _c(dout), _c(x)
    n_img, H, W = _shape(x, scenes, "resnet_train.bwd")
    prm, keep = resnet_params(net)
    g = _lib.ResnetGrads()
    grads, buf = _grad_table(x.device)
    g.conv1_w, g.bn1_w, g.bn1_b = buf("conv1.weight", net.conv1.weight), buf("bn1.weight", net.bn1.weight), buf("bn1.bias", net.bn1.bias)
    for s, stage in enumerate((net.layer1, net.layer2, net.layer3, net.layer4)):
        for b, blk in enumerate(stage):
            k, name = g.block[s][b], f"layer{s + 1}.{b}"
            k.conv1_w, k.conv2_w = buf(name + ".conv1.weight", blk.conv1.weight), buf(name + ".conv2.weight", blk.conv2.weight)
            k.bn1_w, k.bn1_b = buf(name + ".bn1.weight", blk.bn1.weight), buf(name + ".bn1.bias", blk.bn1.bias)
            k.bn2_w, k.bn2_b = buf(name + ".bn2.weight", blk.bn2.weight), buf(name + ".bn2.bias", blk.bn2.bias)
            if blk.downsample is not None:
                k.down_w = buf(name + ".downsample.0.weight", blk.downsample[0].weight)
                k.down_bn_w = buf(name + ".downsample.1.weight", blk.downsample[1].weight)
                k.down_bn_b = buf(name + ".downsample.1.bias", blk.downsample[1].bias)
    g.linear_w, g.linear_b = buf("linear.weight", net.linear.weight), buf("linear.bias", net.linear.bias)
    g.fc_w, g.fc_b = buf("fc.weight", net.fc.weight), buf("fc.bias", net.fc.bias)
    check(_lib.load().vt_resnet_bwd(dev_ptr(dout, "dout"), dev_ptr(x, "x"), n_img, int(scenes), H, W, ctypes.byref(prm),
                                    ctypes.c_void_p(ws.buf.data_ptr()), ws.buf.numel(), ctypes.byref(g), stream_ptr()), "vt_resnet_bwd")
    return grads
