"""The 2-D nets, each one packed blob + one workspace + one persistent launch: the hand encoder's plane U-Net (plane_unet.hip), the
tactile ResNet in eval mode (resnet2d.hip) and the tactile depth U-Net in eval mode (unet2d.hip) and train mode (unet2d_train.hip).

Every net has the same five entry points -- ``*_params``, ``*_supported``, ``*_pack``, ``*_workspace``, ``*_fwd`` / ``*_bwd`` -- built
from the shared pieces at the top of this file."""
import ctypes

import torch

from ._base import _lib, VtError, check, dev_ptr, stream_ptr, _c, keep_for_graph


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------

class _Pointers:
    """Fills a params struct with addresses and keeps what they point to alive (``keep``).  ``who`` names the caller in errors."""

    def __init__(self, who):
        self.who, self.keep = who, []

    def ptr(self, t, name):
        t = _c(t)
        self.keep.append(t)
        return dev_ptr(t, name).value

    def bn(self, dst, m, name):
        """The five fields of a BatchNormParams from an nn.BatchNorm2d."""
        if m.weight is None or m.running_mean is None:
            raise VtError(f"{self.who}: {name} has no affine parameters or no running statistics")
        dst.weight, dst.bias = self.ptr(m.weight, name + ".weight"), self.ptr(m.bias, name + ".bias")
        dst.running_mean, dst.running_var = self.ptr(m.running_mean, name + ".running_mean"), self.ptr(m.running_var, name + ".running_var")
        dst.eps = float(m.eps)


def _grad_table(device):
    """({parameter name: gradient}, buf): ``buf(name, like)`` makes the f32 gradient of parameter ``like``, files it under ``name`` and
    returns its address."""
    grads = {}

    def buf(name, like):
        t = torch.empty(like.shape, dtype=torch.float32, device=device)
        grads[name] = t
        return dev_ptr(t, name).value
    return grads, buf


_WS_CACHE_MAX = 8    # entries per workspace cache below


class _WorkspaceCache:
    """The workspaces of one net by key, at most _WS_CACHE_MAX of them: the oldest leaves first.  A captured graph keeps its workspace
    alive itself (keep_for_graph), so eviction is safe.  ``size_fn`` names the library's size query; 0 bytes raises ``not_built``."""

    def __init__(self, size_fn, not_built, wrap=lambda ws: ws):
        self.entries, self.size_fn, self.not_built, self.wrap = {}, size_fn, not_built, wrap

    def make(self, dev, *args):
        n = getattr(_lib.load(), self.size_fn)(*args)
        if n == 0:
            raise VtError(self.not_built)
        return self.wrap(torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", dev)))

    def get(self, key, *args):
        """The workspace under (current device, *key); a missing one is made for the size query's ``args``."""
        key = (torch.cuda.current_device(), *key)
        if key not in self.entries:
            ws = self.make(key[0], *args)
            while len(self.entries) >= _WS_CACHE_MAX:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = ws
        return self.entries[key]


def _dims(prm):
    """The four shape fields that lead both U-Net params structs, in the order every size query of their net takes them."""
    return tuple(getattr(prm, name) for name, _ in prm._fields_[:4])


def _pack(name, n, prm, keep):
    """The blob of ``n`` bytes that the library's ``name`` packs from the params struct."""
    blob = torch.empty(n // 4, dtype=torch.float32, device=keep[0].device)
    check(getattr(_lib.load(), name)(ctypes.byref(prm), dev_ptr(blob, "blob"), n, stream_ptr()), name)
    return blob


# ---- the hand encoder's 2-D U-Net as one persistent launch (plane_unet.hip) ------------------------------------------------------

def _plane_dims(net):
    prm = _lib.PlaneUnetParams()
    prm.depth, prm.in_channels, prm.start_filts, prm.num_classes = net.depth, net.in_channels, net.start_filts, net.num_classes
    return prm


def plane_unet_params(net):
    """(PlaneUnetParams, tensors it points to) of an ``encoder.unet.UNet`` (depth, channel counts, nn.Conv2d / nn.ConvTranspose2d
    weights in their own layout)."""
    prm, p = _plane_dims(net), _Pointers("plane_unet_pack")
    for l, d in enumerate(net.down_convs):
        for k, conv in enumerate((d.conv1, d.conv2)):
            prm.down_w[l][k], prm.down_b[l][k] = p.ptr(conv.weight, "down conv weight"), p.ptr(conv.bias, "down conv bias")
    for u, up in enumerate(net.up_convs):
        prm.up_tw[u], prm.up_tb[u] = p.ptr(up.upconv.weight, "upconv weight"), p.ptr(up.upconv.bias, "upconv bias")
        for k, conv in enumerate((up.conv1, up.conv2)):
            prm.up_w[u][k], prm.up_b[u][k] = p.ptr(conv.weight, "up conv weight"), p.ptr(conv.bias, "up conv bias")
    prm.final_w, prm.final_b = p.ptr(net.conv_final.weight, "conv_final.weight"), p.ptr(net.conv_final.bias, "conv_final.bias")
    return prm, p.keep


def plane_unet_supported(net, H, W):
    return bool(_lib.load().vt_plane_unet_supported(*_dims(_plane_dims(net)), int(H), int(W)))


def plane_unet_pack(net):
    """The net's weights in fragment order + its biases: the blob vt_plane_unet_fwd reads (vt_plane_unet_pack)."""
    lib = _lib.load()
    n = lib.vt_plane_unet_blob_bytes(*_dims(_plane_dims(net)))
    if n == 0:
        raise VtError("plane U-Net shape not built: depth 2..5, in_channels / start_filts / num_classes multiples of 32")
    return _pack("vt_plane_unet_pack", n, *plane_unet_params(net))


# (device, dims, images, H, W) -> every phase's activations; the key has no stream, unlike the tactile nets': deliberate-as-found
_plane_unet_ws = _WorkspaceCache("vt_plane_unet_workspace_bytes", "plane U-Net shape not built (vt_plane_unet_supported)")


def plane_unet_workspace(net, n_img, H, W, fresh=False):
    """Workspace of vt_plane_unet_fwd (every phase's channels-last activations).  Inference calls share one per shape (torch's current
    stream orders them); ``fresh`` makes a new one (the training forward keeps it for the backward)."""
    shape = (*_dims(_plane_dims(net)), int(n_img), int(H), int(W))
    ws = _plane_unet_ws.make(torch.cuda.current_device(), *shape) if fresh else _plane_unet_ws.get(shape, *shape)
    keep_for_graph(ws)
    return ws


def plane_unet_fwd(x, net, blob, ws=None):
    """UNet.forward on the HIP kernel: x [n_img, in_channels, H, W] -> [n_img, num_classes, H, W] (vt_plane_unet_fwd)."""
    x = _c(x)
    n_img, C, H, W = x.shape
    if C != net.in_channels:
        raise VtError(f"plane_unet_fwd: input has {C} channels, the net takes {net.in_channels}")
    if ws is None:
        ws = plane_unet_workspace(net, n_img, H, W)
    prm = _plane_dims(net)
    out = torch.empty((n_img, net.num_classes, H, W), dtype=torch.float32, device=x.device)
    keep_for_graph(blob)
    check(_lib.load().vt_plane_unet_fwd(dev_ptr(x, "x"), n_img, H, W, ctypes.byref(prm), dev_ptr(blob, "blob"),
                                        ctypes.c_void_p(ws.data_ptr()), ws.numel(), dev_ptr(out, "out"), stream_ptr()), "vt_plane_unet_fwd")
    return out


def plane_unet_bwd(x, net, blob, fwd_ws, dout):
    """Backward of plane_unet_fwd (vt_plane_unet_bwd): (dx, {parameter name: gradient}) from dout, the input, the packed weights and the
    workspace the forward filled.  Gradients are written, not accumulated."""
    lib = _lib.load()
    x, dout = _c(x), _c(dout)
    n_img, C, H, W = x.shape
    n = lib.vt_plane_unet_bwd_workspace_bytes(*_dims(_plane_dims(net)), n_img, H, W)
    if n == 0:
        raise VtError("plane U-Net shape not built (vt_plane_unet_supported)")
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    prm = _plane_dims(net)
    g = _lib.PlaneUnetGrads()
    grads, buf = _grad_table(x.device)
    for l, d in enumerate(net.down_convs):
        for k, cname in enumerate(("conv1", "conv2")):
            conv = getattr(d, cname)
            g.down_w[l][k], g.down_b[l][k] = buf(f"down_convs.{l}.{cname}.weight", conv.weight), buf(f"down_convs.{l}.{cname}.bias", conv.bias)
    for u, up in enumerate(net.up_convs):
        g.up_tw[u], g.up_tb[u] = buf(f"up_convs.{u}.upconv.weight", up.upconv.weight), buf(f"up_convs.{u}.upconv.bias", up.upconv.bias)
        for k, cname in enumerate(("conv1", "conv2")):
            conv = getattr(up, cname)
            g.up_w[u][k], g.up_b[u][k] = buf(f"up_convs.{u}.{cname}.weight", conv.weight), buf(f"up_convs.{u}.{cname}.bias", conv.bias)
    g.final_w, g.final_b = buf("conv_final.weight", net.conv_final.weight), buf("conv_final.bias", net.conv_final.bias)
    dx = torch.empty_like(x)
    check(lib.vt_plane_unet_bwd(dev_ptr(x, "x"), n_img, H, W, ctypes.byref(prm), dev_ptr(blob, "blob"), ctypes.c_void_p(fwd_ws.data_ptr()),
                                dev_ptr(dout, "dout"), ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.byref(g), dev_ptr(dx, "dx"),
                                stream_ptr()), "vt_plane_unet_bwd")
    return dx, grads


# ---- the tactile feature encoder in eval mode (resnet2d.hip) ---------------------------------------------------------------------

def resnet_fold_bn(weight, bn_weight, bn_bias, running_mean, running_var, eps):
    """Eval-mode ``bn(conv(x))`` as one conv: (folded weight, bias) in float64 -- ``w * gamma / sqrt(var + eps)`` per output channel and
    ``beta - mean * gamma / sqrt(var + eps)``.  vt_resnet_pack computes exactly this (f64) per fragment slot before it rounds to f32."""
    s = bn_weight.detach().double() / torch.sqrt(running_var.detach().double() + float(eps))
    w = weight.detach().double() * s.view(-1, *([1] * (weight.dim() - 1)))
    return w, bn_bias.detach().double() - running_mean.detach().double() * s


def resnet_workspace_floats(blocks_num, n_img, H, W):
    """The documented size of vt_resnet_fwd's workspace: four buffers of the largest stage's activations [n_img][Hs][Ws][64 << s],
    Hs = ceil(H / 2^(s + 2))."""
    up = lambda v: (v - 1) // 2 + 1
    h, w, most = up(up(H)), up(up(W)), 0
    for s in range(4):
        most = max(most, n_img * h * w * (64 << s))
        h, w = up(h), up(w)
    return 4 * most


def _resnet_dims(net):
    prm = _lib.ResnetParams()
    prm.blocks_num[:] = [len(stage) for stage in (net.layer1, net.layer2, net.layer3, net.layer4)]
    prm.num_classes = int(net.fc.out_features)
    return prm


def resnet_supported(net, n_img, H, W):
    prm = _resnet_dims(net)
    if max(prm.blocks_num) > _lib.VT_RESNET_MAX_BLOCKS or net.linear.in_features != 512 or net.linear.out_features != 100:
        return False
    return bool(_lib.load().vt_resnet_supported(prm.blocks_num, prm.num_classes, int(n_img), int(H), int(W)))


def resnet_params(net):
    """(ResnetParams, tensors it points to) of a ``layers.TactileResNet``: every conv weight, every BatchNorm's weight, bias, running
    statistics and eps, linear and fc, in the state_dict's own layouts."""
    prm, p = _resnet_dims(net), _Pointers("resnet_pack")
    prm.conv1_w = p.ptr(net.conv1.weight, "conv1.weight")
    p.bn(prm.bn1, net.bn1, "bn1")
    for s, stage in enumerate((net.layer1, net.layer2, net.layer3, net.layer4)):
        for b, blk in enumerate(stage):
            k, name = prm.block[s][b], f"layer{s + 1}.{b}"
            k.conv1_w, k.conv2_w = p.ptr(blk.conv1.weight, name + ".conv1.weight"), p.ptr(blk.conv2.weight, name + ".conv2.weight")
            p.bn(k.bn1, blk.bn1, name + ".bn1")
            p.bn(k.bn2, blk.bn2, name + ".bn2")
            if (blk.downsample is not None) != (b == 0 and s > 0):
                raise VtError(f"resnet_pack: {name}: a projection where the BasicBlock net has none (or none where it has one)")
            if blk.downsample is not None:
                k.down_w = p.ptr(blk.downsample[0].weight, name + ".downsample.0.weight")
                p.bn(k.down_bn, blk.downsample[1], name + ".downsample.1")
    prm.linear_w, prm.linear_b = p.ptr(net.linear.weight, "linear.weight"), p.ptr(net.linear.bias, "linear.bias")
    prm.fc_w, prm.fc_b = p.ptr(net.fc.weight, "fc.weight"), p.ptr(net.fc.bias, "fc.bias")
    return prm, p.keep


def resnet_pack(net):
    """The net's convs with their BatchNorms folded in, in fragment order, + linear and fc: the blob vt_resnet_fwd reads (vt_resnet_pack)."""
    lib = _lib.load()
    prm = _resnet_dims(net)
    n = lib.vt_resnet_blob_bytes(prm.blocks_num, prm.num_classes) if max(prm.blocks_num) <= _lib.VT_RESNET_MAX_BLOCKS else 0
    if n == 0:
        raise VtError("tactile ResNet not built for this net (vt_resnet_supported)")
    return _pack("vt_resnet_pack", n, *resnet_params(net))


# (device, stream, blocks, classes, images, H, W) -> workspace
_resnet_ws = _WorkspaceCache("vt_resnet_workspace_bytes", "tactile ResNet shape not built (vt_resnet_supported)")


def resnet_workspace(net, n_img, H, W):
    """Workspace of vt_resnet_fwd, one per (device, STREAM, shape): two encoders replayed side by side on two streams must not share
    their activations."""
    prm, shape = _resnet_dims(net), (int(n_img), int(H), int(W))
    ws = _resnet_ws.get((torch.cuda.current_stream().cuda_stream, tuple(prm.blocks_num), prm.num_classes, *shape),
                        prm.blocks_num, prm.num_classes, *shape)
    keep_for_graph(ws)
    return ws


def resnet_fwd(x, net, blob, ws=None):
    """TactileResNet.forward in eval mode on the HIP kernels: x [n_img, 3, H, W] -> [n_img, num_classes] (vt_resnet_fwd)."""
    x = _c(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise VtError(f"resnet_fwd: input must be [n_img, 3, H, W] (got {tuple(x.shape)})")
    n_img, _, H, W = x.shape
    if ws is None:
        ws = resnet_workspace(net, n_img, H, W)
    prm = _resnet_dims(net)
    out = torch.empty((n_img, prm.num_classes), dtype=torch.float32, device=x.device)
    keep_for_graph(blob, x)
    check(_lib.load().vt_resnet_fwd(dev_ptr(x, "x"), n_img, H, W, ctypes.byref(prm), dev_ptr(blob, "blob"),
                                    ctypes.c_void_p(ws.data_ptr()), ws.numel(), dev_ptr(out, "out"), stream_ptr()), "vt_resnet_fwd")
    return out


# ---- the tactile depth estimator in eval mode (unet2d.hip) -----------------------------------------------------------------------

def _tactile_dims(net):
    prm = _lib.TactileUnetParams()
    prm.depth, prm.start_filts, prm.in_channels, prm.num_classes = net.depth, net.start_filts, net.in_channels, net.num_classes
    return prm


def tactile_unet_supported(net, n_img, H, W):
    return bool(_lib.load().vt_tactile_unet_supported(*_dims(_tactile_dims(net)), int(n_img), int(H), int(W)))


def tactile_unet_params(net):
    """(TactileUnetParams, tensors it points to) of a ``layers.TactileUNet``: every conv's weight and bias, each block's ONE BatchNorm
    (weight, bias, running statistics, eps), the transposed convs and conv_final, in the state_dict's own layouts."""
    prm, p = _tactile_dims(net), _Pointers("tactile_unet_pack")

    def pair(w, b, bn, i, blk, name):
        p.bn(bn[i], blk.bn, name + ".bn")
        for k, conv in enumerate((blk.conv1, blk.conv2)):
            w[i][k], b[i][k] = p.ptr(conv.weight, f"{name}.conv{k + 1}.weight"), p.ptr(conv.bias, f"{name}.conv{k + 1}.bias")
    for i, blk in enumerate(net.down_convs):
        pair(prm.down_w, prm.down_b, prm.down_bn, i, blk, f"down_convs.{i}")
    for j, blk in enumerate(net.up_convs):
        i = prm.depth - 2 - j                                         # the level this block produces
        pair(prm.up_w, prm.up_b, prm.up_bn, i, blk, f"up_convs.{j}")
        prm.up_tw[i], prm.up_tb[i] = p.ptr(blk.upconv.weight, f"up_convs.{j}.upconv.weight"), p.ptr(blk.upconv.bias, f"up_convs.{j}.upconv.bias")
    prm.final_w, prm.final_b = p.ptr(net.conv_final.weight, "conv_final.weight"), p.ptr(net.conv_final.bias, "conv_final.bias")
    return prm, p.keep


def tactile_unet_pack(net):
    """The net's convs with their BatchNorms folded in, in fragment order: the blob vt_tactile_unet_fwd reads (vt_tactile_unet_pack)."""
    lib = _lib.load()
    n = lib.vt_tactile_unet_blob_bytes(*_dims(_tactile_dims(net)))
    if n == 0:
        raise VtError("tactile U-Net not built for this net (vt_tactile_unet_supported)")
    return _pack("vt_tactile_unet_pack", n, *tactile_unet_params(net))


# (device, stream, dims, images, H, W) -> workspace
_tactile_unet_ws = _WorkspaceCache("vt_tactile_unet_workspace_bytes", "tactile U-Net shape not built (vt_tactile_unet_supported)")


def tactile_unet_workspace(net, n_img, H, W):
    """Workspace of vt_tactile_unet_fwd, one per (device, STREAM, shape), like resnet_workspace."""
    shape = (*_dims(_tactile_dims(net)), int(n_img), int(H), int(W))
    ws = _tactile_unet_ws.get((torch.cuda.current_stream().cuda_stream, *shape), *shape)
    keep_for_graph(ws)
    return ws


def tactile_unet_fwd(x, net, blob, ws=None):
    """TactileUNet.forward in eval mode on the HIP kernels: x [n_img, in_channels, H, W] -> [n_img, num_classes, H, W] (vt_tactile_unet_fwd)."""
    x = _c(x)
    if x.dim() != 4 or x.shape[1] != net.in_channels:
        raise VtError(f"tactile_unet_fwd: input must be [n_img, {net.in_channels}, H, W] (got {tuple(x.shape)})")
    n_img, _, H, W = x.shape
    if ws is None:
        ws = tactile_unet_workspace(net, n_img, H, W)
    prm = _tactile_dims(net)
    out = torch.empty((n_img, prm.num_classes, H, W), dtype=torch.float32, device=x.device)
    keep_for_graph(blob, x)
    check(_lib.load().vt_tactile_unet_fwd(dev_ptr(x, "x"), n_img, H, W, ctypes.byref(prm), dev_ptr(blob, "blob"),
                                          ctypes.c_void_p(ws.data_ptr()), ws.numel(), dev_ptr(out, "out"), stream_ptr()), "vt_tactile_unet_fwd")
    return out


# ---- the tactile depth estimator in train mode (unet2d_train.hip) ----------------------------------------------------------------

def tactile_unet_train_supported(net, n_img, group, H, W):
    return bool(_lib.load().vt_tactile_unet_train_supported(*_dims(_tactile_dims(net)), int(n_img), int(group), int(H), int(W)))


class TactileUnetTrainWorkspace:
    """The workspace of one (device, stream, shape): the forward fills it and the backward reads it.  ``gen`` counts the forwards that
    wrote it, so a backward can tell whether its forward was the last one (layers._TactileUNetTrain runs the forward again if not)."""

    def __init__(self, buf):
        self.buf, self.gen = buf, 0


# (device, stream, dims, images, group, H, W) -> TactileUnetTrainWorkspace
_tactile_unet_train_ws = _WorkspaceCache("vt_tactile_unet_train_workspace_bytes", "tactile U-Net train shape not built (vt_tactile_unet_train_supported)",
                                         wrap=TactileUnetTrainWorkspace)


def tactile_unet_train_workspace(net, n_img, group, H, W):
    """Workspace of vt_tactile_unet_train_fwd / vt_tactile_unet_bwd, one per (device, STREAM, shape), like tactile_unet_workspace."""
    shape = (*_dims(_tactile_dims(net)), int(n_img), int(group), int(H), int(W))
    return _tactile_unet_train_ws.get((torch.cuda.current_stream().cuda_stream, *shape), *shape)


def tactile_unet_train_fwd(x, net, scenes=1, momentum=None, ws=None):
    """TactileUNet.forward in train mode on the HIP kernels (vt_tactile_unet_train_fwd): x [scenes * G, in_channels, H, W], scene-major,
    every BatchNorm with the statistics of each scene's G images alone -> [scenes * G, num_classes, H, W].  ``momentum`` (a float):
    the blocks' running_mean / running_var are updated in place as ``scenes`` sequential calls would; None leaves them alone
    (num_batches_tracked is the caller's).  ``ws`` (tactile_unet_train_workspace) keeps what tactile_unet_bwd reads."""
    x = _c(x)
    if x.dim() != 4 or x.shape[1] != net.in_channels or x.shape[0] % int(scenes):
        raise VtError(f"tactile_unet_train_fwd: input must be [scenes * G, {net.in_channels}, H, W] (got {tuple(x.shape)}, scenes {scenes})")
    n_img, _, H, W = x.shape
    group = n_img // int(scenes)
    if ws is None:
        ws = tactile_unet_train_workspace(net, n_img, group, H, W)
    prm, keep = tactile_unet_params(net)
    out = torch.empty((n_img, prm.num_classes, H, W), dtype=torch.float32, device=x.device)
    check(_lib.load().vt_tactile_unet_train_fwd(dev_ptr(x, "x"), n_img, group, H, W, ctypes.byref(prm), -1.0 if momentum is None else float(momentum),
                                                ctypes.c_void_p(ws.buf.data_ptr()), ws.buf.numel(), dev_ptr(out, "out"), stream_ptr()),
          "vt_tactile_unet_train_fwd")
    ws.gen += 1
    return out


def tactile_unet_bwd(dout, out, net, scenes, ws):
    """Backward of tactile_unet_train_fwd (vt_tactile_unet_bwd): {parameter name: gradient} for every parameter of the net from dout, the
    forward's output and the workspace it filled.  Gradients are written, not accumulated; a block's bn.weight / bn.bias gradient is
    the sum over its two uses."""
    dout, out = _c(dout), _c(out)
    n_img, _, H, W = out.shape
    prm, keep = tactile_unet_params(net)
    g = _lib.TactileUnetGrads()
    grads, buf = _grad_table(out.device)

    def pair(w, b, bw, bb, i, blk, name):
        for k, cname in enumerate(("conv1", "conv2")):
            conv = getattr(blk, cname)
            w[i][k], b[i][k] = buf(f"{name}.{cname}.weight", conv.weight), buf(f"{name}.{cname}.bias", conv.bias)
        bw[i], bb[i] = buf(name + ".bn.weight", blk.bn.weight), buf(name + ".bn.bias", blk.bn.bias)
    for i, blk in enumerate(net.down_convs):
        pair(g.down_w, g.down_b, g.down_bn_w, g.down_bn_b, i, blk, f"down_convs.{i}")
    for j, blk in enumerate(net.up_convs):
        i = prm.depth - 2 - j                                         # the level this block produces
        pair(g.up_w, g.up_b, g.up_bn_w, g.up_bn_b, i, blk, f"up_convs.{j}")
        g.up_tw[i], g.up_tb[i] = buf(f"up_convs.{j}.upconv.weight", blk.upconv.weight), buf(f"up_convs.{j}.upconv.bias", blk.upconv.bias)
    g.final_w, g.final_b = buf("conv_final.weight", net.conv_final.weight), buf("conv_final.bias", net.conv_final.bias)
    check(_lib.load().vt_tactile_unet_bwd(dev_ptr(dout, "dout"), dev_ptr(out, "out"), n_img, n_img // int(scenes), H, W, ctypes.byref(prm),
                                          ctypes.c_void_p(ws.buf.data_ptr()), ws.buf.numel(), ctypes.byref(g), stream_ptr()), "vt_tactile_unet_bwd")
    return grads
