"""Parameter containers and host-PyTorch layers of the hot path.

``ResnetBlockFC`` keeps the reference's parameter names (fc_0, fc_1, shortcut;
reference src/layers.py:8-50) so checkpoints load unchanged.  Inside the decoder
its arithmetic runs in the fused HIP kernel (vtaco_amd/csrc/decode.hip); the
``forward`` here is the plain PyTorch-ROCm path used by the PointNet encoder's
tiny per-point MLP (SURVEY.md K4, 0.16 GFLOP/scene, stays host PyTorch).
"""
from __future__ import annotations

import os

import torch
from torch import nn
from torch.nn import functional as F

from . import ops

# Which path a tactile net's forward takes: "hip" = the HIP kernels, "host" = the nn modules (MIOpen).  One environment variable per path,
# read at every call, so a tool can time both paths in one process:
#   VTACO_TACTILE_RESNET      the eval-mode forward of TactileResNet (vt_resnet_fwd, csrc/resnet2d.hip); default "hip"
#   VTACO_TACTILE_UNET        the eval-mode forward of TactileUNet (vt_tactile_unet_fwd, csrc/unet2d.hip)
#   VTACO_TACTILE_UNET_TRAIN  its train-mode forward and backward under autograd (vt_tactile_unet_train_fwd / vt_tactile_unet_bwd,
#                             csrc/unet2d_train.hip)
#   VTACO_TACTILE_RESNET_TRAIN  the train-mode forward and backward of TactileResNet under autograd (vt_resnet_train_fwd / vt_resnet_bwd,
#                             csrc/resnet2d_train.hip)
#   VTACO_TACTILE_BOTTLENECK  the eval-mode forward of a Bottleneck TactileResNet (Resnet50 / 101 / 152: vt_resnet_bneck_fwd,
#                             csrc/resnet2d_bneck.hip); VTACO_TACTILE_RESNET does not reach these nets.  Default "hip": the Resnet50
#                             stage at five 320x240 images replays in 1.56 ms against the modules' 2.14 (profiles/resnet_bneck_bench.json)
_TACTILE_UNET_DEFAULT = "hip"
_TACTILE_BOTTLENECK_DEFAULT = "hip"
_TACTILE_UNET_TRAIN_DEFAULT = "host"
_TACTILE_RESNET_TRAIN_DEFAULT = "host"


def _kernel_mode(variable, default):
    mode = os.environ.get(variable, default)
    if mode not in ("hip", "host"):
        raise ValueError(f"{variable} must be 'hip' or 'host' (got {mode!r})")
    return mode


def _tactile_resnet_mode():
    return _kernel_mode("VTACO_TACTILE_RESNET", "hip")


def _tactile_bottleneck_mode():
    return _kernel_mode("VTACO_TACTILE_BOTTLENECK", _TACTILE_BOTTLENECK_DEFAULT)


def _tactile_unet_mode():
    return _kernel_mode("VTACO_TACTILE_UNET", _TACTILE_UNET_DEFAULT)


def _tactile_unet_train_mode():
    return _kernel_mode("VTACO_TACTILE_UNET_TRAIN", _TACTILE_UNET_TRAIN_DEFAULT)


def _tactile_resnet_train_mode():
    return _kernel_mode("VTACO_TACTILE_RESNET_TRAIN", _TACTILE_RESNET_TRAIN_DEFAULT)


class _TactileResNetTrain(torch.autograd.Function):
    """TactileResNet.forward in train mode under autograd on the HIP kernels: ops.resnet_train.fwd / bwd.  ``params`` = the net's
    parameters in named_parameters() order (autograd inputs, so the optimiser's tensors receive the gradients); x gets none.  The
    workspace is shared per (device, stream, shape): if another forward of that shape ran before this call's backward, the backward
    first runs the forward again (running statistics untouched)."""

    @staticmethod
    def forward(ctx, x, net, scenes, *params):
        n_img, _, H, W = x.shape
        ws = ops.resnet_train.workspace(net, n_img, scenes, H, W)
        out = ops.resnet_train.fwd(x, net, scenes, momentum=float(net.bn1.momentum), ws=ws)
        with torch.no_grad():
            for bn in net._batchnorms():
                bn.num_batches_tracked += scenes                     # (also moves the eval path's blob stamp: the kernel wrote the statistics)
        ctx.net, ctx.scenes, ctx.ws, ctx.gen = net, scenes, ws, ws.gen
        ctx.save_for_backward(x, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        x = ctx.saved_tensors[0]                                     # (raises if a parameter changed since the forward)
        net = ctx.net
        if ctx.ws.gen != ctx.gen:
            ops.resnet_train.fwd(x, net, ctx.scenes, momentum=None, ws=ctx.ws)
            ctx.gen = ctx.ws.gen
        grads = ops.resnet_train.bwd(dout, x, net, ctx.scenes, ctx.ws)
        return (None, None, None) + tuple(grads[name] if need else None
                                          for (name, _), need in zip(net.named_parameters(), ctx.needs_input_grad[3:]))


class _TactileUNetTrain(torch.autograd.Function):
    """TactileUNet.forward in train mode under autograd on the HIP kernels: ops.tactile_unet_train_fwd, ops.tactile_unet_bwd.  ``params``
    = the net's parameters in named_parameters() order (autograd inputs, so the optimiser's tensors receive the gradients); x gets
    none.  The workspace is shared per (device, stream, shape): if another forward of that shape ran before this call's backward, the
    backward first runs the forward again (running statistics untouched)."""

    @staticmethod
    def forward(ctx, x, net, scenes, *params):
        n_img, _, H, W = x.shape
        ws = ops.tactile_unet_train_workspace(net, n_img, n_img // scenes, H, W)
        out = ops.tactile_unet_train_fwd(x, net, scenes, momentum=float(net.down_convs[0].bn.momentum), ws=ws)
        with torch.no_grad():
            for blk in list(net.down_convs) + list(net.up_convs):
                blk.bn.num_batches_tracked += 2 * scenes             # (also moves the eval path's blob stamp: the kernel wrote the statistics)
        ctx.net, ctx.scenes, ctx.ws, ctx.gen = net, scenes, ws, ws.gen
        ctx.save_for_backward(x, out, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, out = ctx.saved_tensors[:2]                               # (raises if a parameter changed since the forward)
        net = ctx.net
        if ctx.ws.gen != ctx.gen:
            ops.tactile_unet_train_fwd(x, net, ctx.scenes, momentum=None, ws=ctx.ws)
            ctx.gen = ctx.ws.gen
        grads = ops.tactile_unet_bwd(dout, out, net, ctx.scenes, ctx.ws)
        return (None, None, None) + tuple(grads[name] if need else None
                                          for (name, _), need in zip(net.named_parameters(), ctx.needs_input_grad[3:]))


class _TallLinear(torch.autograd.Function):
    """nn.Linear over a tall, skinny activation matrix ([tens of thousands of points] x [32..64 channels]) whose weight
    gradient dW = dy^T x is a 32 x 64 GEMM with K = 24 000: hipBLASLt runs that as one workgroup-starved kernel (0.5 ms,
    0.2 TFLOP/s -- the third largest item of the training step's profile).  The backward here splits K into batches
    (a batched GEMM of [S, out, N/S] x [S, N/S, in], then a sum over S): same arithmetic, all CUs busy."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
        if ctx.needs_input_grad[0]:
            dx = (dy2 @ weight).view_as(x)
        if ctx.needs_input_grad[1]:
            n = x2.shape[0]
            s = next((k for k in (128, 96, 64, 48, 32, 24, 16, 8, 4, 2) if n % k == 0), 1)
            dw = torch.bmm(dy2.view(s, n // s, -1).transpose(1, 2), x2.view(s, n // s, -1)).sum(0)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0)
        return dx, dw, db


def tall_linear(lin, x):
    """``lin(x)``; under autograd on tall inputs (>= 4096 rows) with the split-K weight gradient of _TallLinear."""
    if torch.is_grad_enabled() and x.is_cuda and x.numel() // x.shape[-1] >= 4096 and (lin.weight.requires_grad or x.requires_grad):
        return _TallLinear.apply(x, lin.weight, lin.bias)
    return lin(x)


class ResnetBlockFC(nn.Module):
    """x -> shortcut(x) + fc_1(relu(fc_0(relu(x)))); fc_1.weight starts at zero."""

    def __init__(self, size_in, size_out=None, size_h=None):
        super().__init__()
        size_out = size_in if size_out is None else size_out
        size_h = min(size_in, size_out) if size_h is None else size_h
        self.size_in, self.size_h, self.size_out = size_in, size_h, size_out
        self.fc_0 = nn.Linear(size_in, size_h)
        self.fc_1 = nn.Linear(size_h, size_out)
        self.shortcut = None if size_in == size_out else nn.Linear(size_in, size_out, bias=False)
        nn.init.zeros_(self.fc_1.weight)

    def forward(self, x):
        dx = tall_linear(self.fc_1, F.relu(tall_linear(self.fc_0, F.relu(x))))
        return (x if self.shortcut is None else tall_linear(self.shortcut, x)) + dx

    def packed(self):
        """(fc_0.weight, fc_0.bias, fc_1.weight, fc_1.bias) for vt_decoder_pack."""
        return self.fc_0.weight, self.fc_0.bias, self.fc_1.weight, self.fc_1.bias


class _ConvPair(nn.Module):
    """Two 3x3 convs sharing ONE BatchNorm module, ReLU after each (the reference's
    DownConv / UpConv bodies, src/layers.py:246-319, reuse `self.bn` twice)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.bn = nn.BatchNorm2d(cout)

    def _pair(self, x):
        x = F.relu(self.bn(self.conv1(x)))
        return F.relu(self.bn(self.conv2(x)))


class DownConv(_ConvPair):
    def __init__(self, in_channels, out_channels, pooling=True):
        super().__init__(in_channels, out_channels)
        self.pooling = pooling
        if pooling:
            self.pool = nn.MaxPool2d(2, 2)

    def forward(self, x):
        skip = self._pair(x)
        return (self.pool(skip) if self.pooling else skip), skip


class UpConv(_ConvPair):
    def __init__(self, in_channels, out_channels):
        super().__init__(2 * out_channels, out_channels)
        self.upconv = nn.ConvTranspose2d(in_channels, out_channels, 2, stride=2)

    def forward(self, from_down, from_up):
        return self._pair(torch.cat((self.upconv(from_up), from_down), dim=1))


class TactileUNet(nn.Module):
    """Tactile depth estimator (reference ``UNet``, src/layers.py:322-450): `depth`
    DownConvs (last without pooling), depth-1 UpConvs (transpose-conv up, concat),
    1x1 conv, sigmoid.  In eval mode without autograd on a HIP f32 input the forward is ``vt_tactile_unet_fwd`` (csrc/unet2d.hip:
    BatchNorm folded into the convs, pool / concat / conv_final / sigmoid fused into them, 12 launches at depth 3, bit-reproducible and
    batch-invariant).  In train mode under autograd with ``VTACO_TACTILE_UNET_TRAIN=hip`` the forward and the backward are
    ``vt_tactile_unet_train_fwd`` / ``vt_tactile_unet_bwd`` (csrc/unet2d_train.hip: batch statistics per scene, every parameter's
    gradient, bit-reproducible; ``train_hip_supported``).  Everything else runs the nn modules (``forward_modules``: host
    PyTorch-ROCm / MIOpen)."""

    def __init__(self, num_classes=1, in_channels=3, depth=4, start_filts=32, up_mode='transpose',
                 merge_mode='concat', **kwargs):
        super().__init__()
        if up_mode != 'transpose' or merge_mode != 'concat':
            raise ValueError("TactileUNet: only up_mode='transpose', merge_mode='concat' (the shipped config) are built")
        self.num_classes, self.in_channels, self.start_filts, self.depth = num_classes, in_channels, start_filts, depth
        widths = [start_filts * 2 ** i for i in range(depth)]
        self.down_convs = nn.ModuleList(
            DownConv(in_channels if i == 0 else widths[i - 1], w, pooling=i < depth - 1) for i, w in enumerate(widths))
        self.up_convs = nn.ModuleList(UpConv(widths[i], widths[i - 1]) for i in range(depth - 1, 0, -1))
        self.conv_final = nn.Conv2d(widths[0], num_classes, 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    def hip_supported(self, x):
        """Eval mode, no autograd through the call, a HIP f32 image batch, a shape vt_tactile_unet_supported covers."""
        if self.training or _tactile_unet_mode() != "hip" or not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return x.shape[1] == self.in_channels and x.shape[0] > 0 and ops.tactile_unet_supported(self, x.shape[0], x.shape[2], x.shape[3])

    def _blob_stamp(self):
        """(storage, version) of every parameter AND buffer: load_state_dict, an optimiser step and a train-mode forward (running
        statistics) all change it."""
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _blob(self):
        """The packed weights (BatchNorm folded in), repacked when the stamp moved.  Generator3D runs every stage eagerly before it
        captures it, so the packing launches never fall inside a stream capture."""
        stamp = self._blob_stamp()
        hit = self.__dict__.get("_blob_cache")
        if hit is None or hit[0] != stamp:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TactileUNet: weights changed since the last eager call; run one eval forward outside stream capture")
            hit = (stamp, ops.tactile_unet_pack(self))
            self.__dict__["_blob_cache"] = hit
        return hit[1]

    def train_hip_supported(self, x, scenes=1):
        """Train mode with autograd on, a parameter that requires grad, a HIP f32 image batch that does not, VTACO_TACTILE_UNET_TRAIN=hip,
        ordinary BatchNorms (affine, running statistics, one float momentum), a shape vt_tactile_unet_train_supported covers."""
        if _tactile_unet_train_mode() != "hip" or not self.training or not torch.is_grad_enabled():
            return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32) or x.requires_grad:
            return False
        if x.shape[1] != self.in_channels or x.shape[0] == 0 or scenes < 1 or x.shape[0] % scenes:
            return False
        if not any(p.requires_grad for p in self.parameters()):
            return False
        bns = [blk.bn for blk in list(self.down_convs) + list(self.up_convs)]
        m = bns[0].momentum
        if m is None or any(not (bn.affine and bn.track_running_stats) or bn.running_mean is None or bn.momentum != m or not bn.training
                            for bn in bns):
            return False
        if any(p.device != x.device or p.dtype != torch.float32 for p in self.parameters()):
            return False
        return ops.tactile_unet_train_supported(self, x.shape[0], x.shape[0] // scenes, x.shape[2], x.shape[3])

    def forward(self, x, scenes=1):
        """x [scenes * G, in_channels, H, W], scene-major; in train mode every BatchNorm sees each scene's G images alone."""
        if self.hip_supported(x):
            return ops.tactile_unet_fwd(x, self, self._blob())
        if self.train_hip_supported(x, scenes):
            return _TactileUNetTrain.apply(x, self, int(scenes), *[p for _, p in self.named_parameters()])
        if scenes > 1:
            G = x.shape[0] // scenes
            return torch.cat([self.forward_modules(x[s * G:(s + 1) * G]) for s in range(scenes)], dim=0)
        return self.forward_modules(x)

    def forward_scenes(self, imgs):
        """imgs [S, F, in_channels, H, W] -> [S, F, num_classes * H * W]: the reference's loop ``cat([self(imgs[s]) for s])``
        (models/__init__.py:115-136).  On the HIP train path it is ONE pass over the S * F images with per-scene statistics; otherwise
        the loop itself over ``forward_modules`` (or the eval kernels), so values, gradients and running statistics are the loop's."""
        S, Fn = imgs.shape[:2]
        return self.forward(imgs.reshape(S * Fn, *imgs.shape[2:]), scenes=S).view(S, Fn, -1)

    def forward_modules(self, x):
        """The nn modules one by one (host PyTorch-ROCm / MIOpen): train mode, autograd, shapes the HIP path does not cover."""
        skips = []
        for down in self.down_convs:
            x, skip = down(x)
            skips.append(skip)
        for i, up in enumerate(self.up_convs):
            x = up(skips[-(i + 2)], x)
        return torch.sigmoid(self.conv_final(x)) * 1


def _bn_scenes(bn, x, scenes):
    """``bn(x)`` for a batch of ``scenes`` groups of images ordered image-major (image f of scene b at row f * scenes + b), with the
    statistics of every scene's images alone -- what the reference's per-scene calls compute (models/__init__.py:115-136: train-mode
    BatchNorm sees the five images of ONE scene) -- from one pass: in that order [F * S, C, H, W] is [F, S * C, H, W], a batch of F
    images with S * C channels.  The running statistics move as the S calls in scene order would move them."""
    if scenes <= 1 or not bn.training:
        return bn(x)                                                  # (eval mode: the running statistics, whatever the order)
    N, C, H, W = x.shape
    xv = x.contiguous().view(N // scenes, scenes * C, H, W)
    w = bn.weight.repeat(scenes) if bn.weight is not None else None
    b = bn.bias.repeat(scenes) if bn.bias is not None else None
    if bn.track_running_stats and bn.running_mean is not None:
        mean, var = x.new_zeros(scenes * C), x.new_ones(scenes * C)
        y = F.batch_norm(xv, mean, var, w, b, True, 1.0, bn.eps)      # momentum 1: the buffers receive the batch statistics themselves
        with torch.no_grad():
            bn.num_batches_tracked += scenes
            if bn.momentum is None:
                raise NotImplementedError("_bn_scenes: cumulative-average BatchNorm (momentum=None) is not on this path")
            m = float(bn.momentum)
            # (kept on the module: a tensor made from host values would be a copy inside a stream capture)
            key = (scenes, m, x.dtype, x.device)
            cache = bn.__dict__.setdefault("_scene_coef", {})
            coef = cache.get(key)
            if coef is None:
                coef = cache[key] = torch.tensor([m * (1.0 - m) ** (scenes - 1 - k) for k in range(scenes)], dtype=x.dtype, device=x.device)
            bn.running_mean.mul_((1.0 - m) ** scenes).add_((coef[:, None] * mean.view(scenes, C)).sum(0))
            bn.running_var.mul_((1.0 - m) ** scenes).add_((coef[:, None] * var.view(scenes, C)).sum(0))
    else:
        y = F.batch_norm(xv, None, None, w, b, True, 0.0, bn.eps)
    return y.view(N, C, H, W)


class _ResidualPair(nn.Module):
    """Two 3x3 conv + BatchNorm stages with an identity (or 1x1-projected) skip: the basic ResNet block
    (reference ``BasicBlock``, src/layers.py:52-82; parameter names conv1/bn1/conv2/bn2/downsample)."""
    expansion = 1

    def __init__(self, in_channel, out_channel, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channel, out_channel, 3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_channel)
        self.conv2 = nn.Conv2d(out_channel, out_channel, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_channel)
        self.downsample = downsample

    def forward(self, x, scenes=1):
        if self.downsample is None:
            skip = x
        elif scenes > 1:
            skip = _bn_scenes(self.downsample[1], self.downsample[0](x), scenes)
        else:
            skip = self.downsample(x)
        y = _bn_scenes(self.bn2, self.conv2(F.relu(_bn_scenes(self.bn1, self.conv1(x), scenes))), scenes)
        return F.relu(y + skip)


class _Bottleneck(nn.Module):
    """1x1 reduce, 3x3 (carries the stride), 1x1 expand to 4 * channel, each with its BatchNorm, and an identity or 1x1-projected skip
    (reference ``Bottleneck``, src/layers.py:86-126; parameter names conv1/bn1/conv2/bn2/conv3/bn3/downsample)."""
    expansion = 4

    def __init__(self, in_channel, out_channel, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channel, out_channel, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(out_channel)
        self.conv2 = nn.Conv2d(out_channel, out_channel, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_channel)
        self.conv3 = nn.Conv2d(out_channel, out_channel * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(out_channel * self.expansion)
        self.downsample = downsample

    def forward(self, x, scenes=1):
        if self.downsample is None:
            skip = x
        elif scenes > 1:
            skip = _bn_scenes(self.downsample[1], self.downsample[0](x), scenes)
        else:
            skip = self.downsample(x)
        y = F.relu(_bn_scenes(self.bn1, self.conv1(x), scenes))
        y = F.relu(_bn_scenes(self.bn2, self.conv2(y), scenes))
        return F.relu(_bn_scenes(self.bn3, self.conv3(y), scenes) + skip)


class TactileResNet(nn.Module):
    """Tactile feature encoder of the shipped VTacO / VTacOH configs (``encoder_img: Resnet18``; reference ``ResNet`` with
    BasicBlocks, src/layers.py:127-195): 7x7/2 stem, 3x3/2 max-pool, four stages of residual pairs (64, 128, 256, 512; stride 2
    from the second), global average pool, Linear(512, 100), Linear(100, num_classes) -- no activation between the two.
    Five 320x240 images per scene.  In eval mode without autograd on a HIP f32 input the forward is ``vt_resnet_fwd``
    (csrc/resnet2d.hip: BatchNorm folded into the convs, 18 launches for Resnet18, bit-reproducible).  In train mode under autograd
    with ``VTACO_TACTILE_RESNET_TRAIN=hip`` the forward and the backward are ``vt_resnet_train_fwd`` / ``vt_resnet_bwd``
    (csrc/resnet2d_train.hip: batch statistics per scene, every parameter's gradient, bit-reproducible; ``train_hip_supported``).
    Everything else and ``VTACO_TACTILE_RESNET=host`` run the nn modules (``forward_modules``: host PyTorch-ROCm / MIOpen).
    With ``block=_Bottleneck`` (Resnet50 / 101 / 152 of the reference: stages 256..2048 wide, Linear(2048, 100)) the eval forward is
    ``vt_resnet_bneck_fwd`` (csrc/resnet2d_bneck.hip, 50 launches for Resnet50) under ``VTACO_TACTILE_BOTTLENECK=hip``; its train mode
    runs the nn modules."""

    def __init__(self, blocks_num=(2, 2, 2, 2), num_classes=32, block=_ResidualPair):
        super().__init__()
        self.block = block
        self.in_channel = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.layer1 = self._stage(64, blocks_num[0], 1)
        self.layer2 = self._stage(128, blocks_num[1], 2)
        self.layer3 = self._stage(256, blocks_num[2], 2)
        self.layer4 = self._stage(512, blocks_num[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.linear = nn.Linear(512 * block.expansion, 100)
        self.fc = nn.Linear(100, num_classes)
        for m in self.modules():                                       # src/layers.py:150-152
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    def _stage(self, channel, count, stride):
        block, wide, project = self.block, channel * self.block.expansion, None
        if stride != 1 or self.in_channel != wide:                     # src/layers.py:157-162 (a Bottleneck layer1.0 projects 64 -> 256)
            project = nn.Sequential(nn.Conv2d(self.in_channel, wide, 1, stride=stride, bias=False), nn.BatchNorm2d(wide))
        blocks = [block(self.in_channel, channel, stride=stride, downsample=project)]
        self.in_channel = wide
        blocks += [block(wide, channel) for _ in range(1, count)]
        return nn.Sequential(*blocks)

    def _bottleneck(self):
        return self.block is _Bottleneck

    def hip_supported(self, x):
        """Eval mode, no autograd through the call, a HIP f32 image batch, a shape vt_resnet_supported (vt_resnet_bneck_supported for a
        Bottleneck net) covers."""
        mode = _tactile_bottleneck_mode() if self._bottleneck() else _tactile_resnet_mode()
        if self.training or mode != "hip" or not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        supported = ops.resnet_bneck.supported if self._bottleneck() else ops.resnet_supported
        return x.shape[1] == 3 and x.shape[0] > 0 and supported(self, x.shape[0], x.shape[2], x.shape[3])

    def _blob_stamp(self):
        """(storage, version) of every parameter AND buffer: load_state_dict, an optimiser step and a train-mode forward (running
        statistics) all change it."""
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _blob(self):
        """The packed weights (BatchNorm folded in), repacked when the stamp moved.  Generator3D runs every stage eagerly before it
        captures it, so the packing launches never fall inside a stream capture."""
        stamp = self._blob_stamp()
        hit = self.__dict__.get("_blob_cache")
        if hit is None or hit[0] != stamp:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TactileResNet: weights changed since the last eager call; run one eval forward outside stream capture")
            hit = (stamp, (ops.resnet_bneck.pack if self._bottleneck() else ops.resnet_pack)(self))
            self.__dict__["_blob_cache"] = hit
        return hit[1]

    def _batchnorms(self):
        """Every BatchNorm of the net: the stem's, each block's bn1 / bn2 (/ bn3) and each projection's."""
        bns = [self.bn1]
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in stage:
                bns += [blk.bn1, blk.bn2] + ([blk.bn3] if hasattr(blk, "bn3") else []) + ([blk.downsample[1]] if blk.downsample is not None else [])
        return bns

    def train_hip_supported(self, x, scenes=1):
        """Train mode with autograd on, a parameter that requires grad, a HIP f32 image batch that does not, VTACO_TACTILE_RESNET_TRAIN=hip,
        ordinary BatchNorms (affine, running statistics, one float momentum), BasicBlock stages, a shape vt_resnet_train_supported
        covers (``scenes`` divides the batch; at least 2 values per scene and channel at layer4)."""
        if _tactile_resnet_train_mode() != "hip" or not self.training or not torch.is_grad_enabled():
            return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32) or x.requires_grad:
            return False
        if x.shape[1] != 3 or x.shape[0] == 0 or scenes < 1 or x.shape[0] % scenes:
            return False
        if not any(p.requires_grad for p in self.parameters()):
            return False
        if any(not isinstance(blk, _ResidualPair) for stage in (self.layer1, self.layer2, self.layer3, self.layer4) for blk in stage):
            return False
        bns = self._batchnorms()
        m = bns[0].momentum
        if m is None or any(type(bn) is not nn.BatchNorm2d or not (bn.affine and bn.track_running_stats) or bn.running_mean is None
                            or bn.momentum != m or not bn.training for bn in bns):
            return False
        if any(p.device != x.device or p.dtype != torch.float32 for p in self.parameters()):
            return False
        return ops.resnet_train.supported(self, x.shape[0], scenes, x.shape[2], x.shape[3])

    def forward(self, x, scenes=1):
        if self.hip_supported(x):
            return (ops.resnet_bneck.fwd if self._bottleneck() else ops.resnet_fwd)(x, self, self._blob())
        if self.train_hip_supported(x, scenes):
            return _TactileResNetTrain.apply(x, self, int(scenes), *[p for _, p in self.named_parameters()])
        return self.forward_modules(x, scenes)

    def forward_modules(self, x, scenes=1):
        """The nn modules one by one (host PyTorch-ROCm / MIOpen): train mode, autograd, shapes the HIP path does not cover."""
        x = self.maxpool(F.relu(_bn_scenes(self.bn1, self.conv1(x), scenes)))
        for stage in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in stage:
                x = block(x, scenes)
        return self.fc(self.linear(torch.flatten(self.avgpool(x), 1)))

    def forward_scenes(self, imgs):
        """imgs [S, F, 3, H, W] -> [S, F, num_classes]: the reference's loop ``cat([self(imgs[s]) for s])`` (models/__init__.py:115-136)
        as ONE pass over the S * F images -- the convolutions at batch S * F (MIOpen at batch five runs at a third of that rate), every
        BatchNorm with the statistics of each scene's images alone (_bn_scenes), so values, gradients and running statistics are the
        loop's."""
        S, Fn = imgs.shape[:2]
        x = imgs.transpose(0, 1).reshape(Fn * S, *imgs.shape[2:])       # image-major
        return self.forward(x, scenes=S).view(Fn, S, -1).transpose(0, 1)


def Resnet18(num_classes=32):
    return TactileResNet((2, 2, 2, 2), num_classes=num_classes)


def Resnet34(num_classes=32):
    return TactileResNet((3, 4, 6, 3), num_classes=num_classes)


def Resnet50(num_classes=32):
    return TactileResNet((3, 4, 6, 3), num_classes=num_classes, block=_Bottleneck)


def Resnet101(num_classes=32):
    return TactileResNet((3, 4, 23, 3), num_classes=num_classes, block=_Bottleneck)


def Resnet152(num_classes=32):
    return TactileResNet((3, 8, 36, 3), num_classes=num_classes, block=_Bottleneck)
