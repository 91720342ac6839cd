"""GPU: the hand encoder's 2-D U-Net as one persistent HIP launch (vt_plane_unet_fwd / vt_plane_unet_bwd, csrc/plane_unet.hip)
against the oracle's restatement of reference src/encoder/unet.py (oracle.unet2d_forward, pinned by g10 / g19)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- the kernel's own forward activations, and float64 references built on them ---------------------------------------------------

def _phases(depth, start, in_ch, classes):
    """pu_shape (plane_unet.hip) in launch order: (parameter prefix, Cin, Cout, kind, level of the output, ReLU) per phase."""
    w = lambda l: start << l
    ph = []
    for l in range(depth):
        ph += [(f"down_convs.{l}.conv1", in_ch if l == 0 else w(l - 1), w(l), "conv", l, True),
               (f"down_convs.{l}.conv2", w(l), w(l), "conv", l, True)]
    for u in range(depth - 1):
        lev = depth - 2 - u
        ph += [(f"up_convs.{u}.upconv", w(lev + 1), w(lev), "upT", lev, False),
               (f"up_convs.{u}.conv1", 2 * w(lev), w(lev), "conv", lev, True),
               (f"up_convs.{u}.conv2", w(lev), w(lev), "conv", lev, True)]
    return ph + [("conv_final", start, classes, "head", 0, False)]


def _kernel_acts(net, x):
    """vt_plane_unet_fwd's output and every phase's activation (float64 NCHW, CPU), decoded from its workspace: the phases' channels-last
    outputs one after the other (pu_ws_offset), the head's in ``out``."""
    from vtaco_amd import _lib, ops
    n_img, _, H, W = x.shape
    ph = _phases(net.depth, net.start_filts, net.in_channels, net.num_classes)
    ws = ops.plane_unet_workspace(net, n_img, H, W, fresh=True)
    out = ops.plane_unet_fwd(x, net, net._blob(), ws)
    flat = ws.view(torch.float32).cpu()
    acts, off = [], 0
    for _, _, cout, _, lev, _ in ph[:-1]:
        h, w = H >> lev, W >> lev
        acts.append(flat[off:off + n_img * h * w * cout].view(n_img, h, w, cout).permute(0, 3, 1, 2).double())
        off += n_img * h * w * cout
    nbytes = _lib.load().vt_plane_unet_workspace_bytes(net.depth, net.in_channels, net.start_filts, net.num_classes, n_img, H, W)
    assert off * 4 == nbytes == ws.numel(), (off * 4, nbytes)       # the mirror above is the kernel's layout
    return out, ws, acts + [out.detach().double().cpu()]


def _phase_inputs(depth, ph, x, acts):
    """The input view each phase's loader reads: x, the 2x2 max of the level above, or cat(transposed conv, skip)."""
    views = []
    for i, (name, _, _, kind, lev, _) in enumerate(ph):
        if i == 0:
            views.append(x)
        elif i < 2 * depth and i % 2 == 0:
            views.append(F.max_pool2d(acts[i - 1], 2))
        elif name.startswith("up_convs") and name.endswith("conv1"):
            views.append(torch.cat((acts[i - 1], acts[2 * lev + 1]), 1))
        else:
            views.append(acts[i - 1])
    return views


def _check_phases(net, x, acts, tol=1e-6):
    """Every phase's output against a float64 conv of the kernel's own input view: |kernel - ref| <= tol * (conv(|in|, |W|) + |b|)
    elementwise (ReLU is 1-Lipschitz: no branch to flip; the largest ratio measured on the MI355X over PHASE_SHAPES is 1.9e-7).
    Returns the largest ratio of the error to conv(|in|, |W|) + |b|."""
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    ph = _phases(net.depth, net.start_filts, net.in_channels, net.num_classes)
    worst = 0.0
    for i, (inp, (name, _, _, kind, _, relu)) in enumerate(zip(_phase_inputs(net.depth, ph, x.double().cpu(), acts), ph)):
        wt, b = sd[name + ".weight"], sd[name + ".bias"]
        op = (lambda v, k: F.conv_transpose2d(v, k, stride=2)) if kind == "upT" else \
             (lambda v, k: F.conv2d(v, k, padding=1 if kind == "conv" else 0))
        ref = op(inp, wt) + b[None, :, None, None]
        if relu:
            ref = ref.clamp_min(0.0)
        bound = op(inp.abs(), wt.abs()) + b.abs()[None, :, None, None]
        ratio = float(((acts[i] - ref).abs() / bound.clamp_min(1e-300)).max())
        assert ratio <= tol, (i, name, ratio)
        worst = max(worst, ratio)
    return worst


def _pinned_grads(net, x, wout, acts):
    """Float64 autograd through oracle.unet2d_forward restated with the KERNEL's branch decisions: every ReLU is z * (act > 0) and
    every max-pool a gather at the first maximum of the kernel's 2x2 window (row-major, as torch's max_pool2d).  The net is then
    linear, so these are the exact gradients of the function the kernel computed.  Returns (dx, {parameter name: gradient})."""
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in net.state_dict().items()}
    x = x.detach().double().cpu().requires_grad_(True)
    depth = net.depth

    def conv(t, pre, **kw):
        return F.conv2d(t, sd[pre + ".weight"], sd[pre + ".bias"], **kw)

    def pool(t, a):
        n, c, h, w = a.shape
        win = lambda v: v.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
        return win(t).gather(-1, win(a).argmax(-1, keepdim=True)).squeeze(-1)     # argmax: the first maximum
    y, skips = x, []
    for l in range(depth):
        y = conv(y, f"down_convs.{l}.conv1", padding=1) * (acts[2 * l] > 0)
        y = conv(y, f"down_convs.{l}.conv2", padding=1) * (acts[2 * l + 1] > 0)
        skips.append(y)
        if l < depth - 1:
            y = pool(y, acts[2 * l + 1])
    for u in range(depth - 1):
        i = 2 * depth + 3 * u
        pre = f"up_convs.{u}."
        y = torch.cat((F.conv_transpose2d(y, sd[pre + "upconv.weight"], sd[pre + "upconv.bias"], stride=2), skips[-(u + 2)]), 1)
        y = conv(y, pre + "conv1", padding=1) * (acts[i + 1] > 0)
        y = conv(y, pre + "conv2", padding=1) * (acts[i + 2] > 0)
    (conv(y, "conv_final") * wout.double().cpu()).sum().backward()
    return x.grad, {k: v.grad for k, v in sd.items()}


def _assert_grads_match(dx, grads, ref_dx, ref_grads, tag=""):
    """Elementwise at 3e-5 of the reference's largest entry: dx and every parameter gradient.  Returns the largest error / entry."""
    worst = 0.0
    for name, got in [("dx", dx)] + sorted(grads.items()):
        ref = ref_dx if name == "dx" else ref_grads[name]
        scale = max(1e-30, float(ref.abs().max()))
        err = float((got.detach().double().cpu() - ref).abs().max())
        assert err <= 3e-5 * scale, (tag, name, err, scale)
        worst = max(worst, err / scale)
    return worst


def _net(depth, in_ch, start, classes, seed):
    from vtaco_amd.encoder.unet import UNet
    torch.manual_seed(seed)
    net = UNet(classes, in_channels=in_ch, depth=depth, start_filts=start)
    with torch.no_grad():                                   # reset_params zeroes every bias: give them values
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape) * 0.05)
    return net


SHAPES = [  # depth, in_ch, start, classes, n_img, H, W
    (4, 32, 32, 32, 3, 32, 32),        # the shipped hand encoder: three planes of one scene
    (4, 32, 32, 32, 24, 32, 32),       # ... of a training batch of eight scenes
    (3, 64, 32, 96, 5, 16, 16),
    (2, 32, 32, 32, 9, 8, 8),          # bottom level 4 x 4: two images per pixel tile, a ragged last tile
    (4, 32, 32, 64, 2, 64, 64),        # 64 x 64 planes: two tiles per row
    (3, 32, 64, 32, 2, 64, 32),        # non-square, 64 filters
    (4, 512, 32, 512, 1, 64, 64),      # the t2d digit encoder's planes (c_dim 512, start_filts 32 through the config's typo)
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plane_unet_forward_against_the_oracle(shape):
    from oracle import vtaco_oracle as orc
    from vtaco_amd import ops
    depth, in_ch, start, classes, n_img, H, W = shape
    net = _net(depth, in_ch, start, classes, seed=depth * 7 + n_img)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n_img, in_ch, H, W, generator=g)
    x[x.abs() < 0.3] = 0.0                                   # planes are mostly empty cells
    with torch.no_grad():
        ref = orc.unet2d_forward({k: v.detach() for k, v in net.state_dict().items()}, x)
    net = net.to(DEV)
    assert net.hip_supported(x.to(DEV))
    with torch.no_grad():
        got = net(x.to(DEV))
        again = net(x.to(DEV))
    scale = max(1.0, float(ref.abs().max()))
    err = float((got.cpu() - ref).abs().max())
    assert err <= 2e-5 * scale, (err, scale)
    assert torch.equal(got, again)                           # fixed summation order: bit-reproducible
    # the nn.Conv2d modules (MIOpen) agree as well, and a changed weight is picked up (the blob is repacked)
    with torch.no_grad():
        mods = net.forward_modules(x.to(DEV))
        assert float((mods - got).abs().max()) <= 1e-4 * scale
        net.conv_final.bias.add_(1.0)
        assert float((net(x.to(DEV)) - got - 1.0).abs().max()) <= 1e-5 * scale


def test_plane_unet_refused_shapes_keep_the_modules():
    from vtaco_amd.encoder.unet import UNet
    torch.manual_seed(0)
    x = torch.randn(1, 32, 32, 32, device=DEV)
    for kw in (dict(start_filts=16), dict(merge_mode="add"), dict(up_mode="upsample"), dict(depth=5, start_filts=32)):
        net = UNet(32, in_channels=32, **dict(dict(depth=3), **kw)).to(DEV)
        assert not net.hip_supported(x)
        with torch.no_grad():
            assert net(x).shape == (1, 32, 32, 32)


BWD_SHAPES = [(4, 32, 32, 32, 3, 32, 32), (4, 32, 32, 32, 24, 32, 32), (3, 64, 32, 96, 5, 16, 16), (2, 32, 32, 32, 9, 8, 8),
              (3, 32, 64, 32, 2, 64, 32), (4, 512, 32, 512, 1, 64, 64)]


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plane_unet_backward_against_the_oracle_autograd(shape):
    """vt_plane_unet_bwd against torch-CPU autograd through the oracle's restatement: the input gradient and every parameter's
    gradient, with the framework's conv / pool operators made to raise on the device (nothing may fall back to MIOpen)."""
    from oracle import vtaco_oracle as orc
    depth, in_ch, start, classes, n_img, H, W = shape
    net = _net(depth, in_ch, start, classes, seed=depth * 5 + n_img)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n_img, in_ch, H, W, generator=g)
    x[x.abs() < 0.3] = 0.0
    wout = torch.randn(n_img, classes, H, W, generator=g)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    (orc.unet2d_forward(sd, xr) * wout).sum().backward()
    net = net.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    saved = F.conv2d, F.conv_transpose2d, F.max_pool2d

    def boom(*a, **k):
        raise AssertionError("a framework convolution / pool ran under the HIP U-Net")
    F.conv2d = F.conv_transpose2d = F.max_pool2d = boom
    try:
        out = net(xd)
        (out * wout.to(DEV)).sum().backward()
    finally:
        F.conv2d, F.conv_transpose2d, F.max_pool2d = saved

    # The net is piecewise linear: where the CPU's f32 forward and the kernel's differ in the last bit, a ReLU at ~0 or a max-pool
    # window with two near-equal entries can take the other branch (seen on the large cases: one window in 400 000), so the oracle's
    # own autograd is a strict reference on the small cases only.  Every case is held elementwise to the float64 gradients of the
    # function the kernel computed: its branch decisions read off its own activations (_pinned_grads).
    strict = n_img * H * W * max(in_ch, start) <= 6144 * 64         # (~ the number of ReLU / pool units)
    if strict:
        _assert_grads_match(xd.grad, {n: p.grad for n, p in net.named_parameters()}, xr.grad,
                            {n: v.grad.double() for n, v in sd.items()}, "oracle f32")
    out_k, _, acts = _kernel_acts(net, x.to(DEV))
    assert torch.equal(out_k, out.detach())                           # the same forward as the autograd path (bit-reproducible)
    ref_dx, ref_grads = _pinned_grads(net, x, wout, acts)
    worst = _assert_grads_match(xd.grad, {n: p.grad for n, p in net.named_parameters()}, ref_dx, ref_grads, "pinned f64")
    print(f"plane U-Net {shape}: largest gradient error / largest entry {worst:.3e}")
    # written, not accumulated into stale buffers; a second backward accumulates through autograd as usual
    g1 = {n: p.grad.clone() for n, p in net.named_parameters()}
    (net(xd) * wout.to(DEV)).sum().backward()
    for n, p in net.named_parameters():
        assert float((p.grad - 2 * g1[n]).abs().max()) <= 1e-6 * max(1.0, float(g1[n].abs().max())), n


# Accepted shapes the cases above do not reach.  Every phase of the nets above that splits K over 8 waves has a Cin that is a multiple
# of 64: widths of an odd multiple of 32 (96, 160, 288) exercise the split's remainder.
EDGE_SHAPES = [  # depth, in_ch, start, classes, n_img, H, W
    (3, 96, 32, 32, 2, 16, 16),        # phase 0 with Cin 96
    (3, 32, 96, 32, 3, 16, 16),        # Cin 96 / 192 / 288 along the encoder and decoder, forward and data gradient
    (2, 32, 32, 288, 2, 8, 8),         # the head's data gradient: Cin 288 over 8 waves
    (3, 160, 32, 32, 1, 16, 16),       # phase 0 with Cin 160
    (5, 32, 32, 32, 2, 64, 64),        # depth 5: a 4 x 4 bottom level
    (5, 32, 64, 32, 1, 64, 64),        # ... 1024 channels at the bottom
    (2, 32, 32, 32, 2, 64, 8),         # tall planes: 8 x 4 pixel tiles
    (2, 32, 32, 32, 1, 8, 128),        # wide planes: 4 tiles per row
    (3, 32, 32, 32, 1, 16, 256),       # ... 8 tiles per row
    (3, 32, 32, 32, 7, 16, 16),        # two images per tile at the bottom level, a ragged last group
]
PHASE_SHAPES = SHAPES + EDGE_SHAPES


@pytest.mark.parametrize("shape", PHASE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plane_unet_phases_and_pinned_backward_against_float64(shape):
    """Every phase of vt_plane_unet_fwd against a float64 conv of its own input view (a wrong phase is named, not hidden by the layers
    after it), and -- for the shapes BWD_SHAPES does not cover -- vt_plane_unet_bwd against the pinned float64 gradients."""
    from vtaco_amd import ops
    depth, in_ch, start, classes, n_img, H, W = shape
    net = _net(depth, in_ch, start, classes, seed=depth * 11 + n_img).to(DEV)
    assert ops.plane_unet_supported(net, H, W)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n_img, in_ch, H, W, generator=g)
    x[x.abs() < 0.3] = 0.0
    _, ws, acts = _kernel_acts(net, x.to(DEV))
    worst = _check_phases(net, x, acts)
    print(f"plane U-Net {shape}: largest phase error / (conv(|in|, |W|) + |b|) {worst:.3e}")
    if shape in BWD_SHAPES:
        return
    wout = torch.randn(n_img, classes, H, W, generator=g)
    dx, grads = ops.plane_unet_bwd(x.to(DEV), net, net._blob(), ws, wout.to(DEV))
    ref_dx, ref_grads = _pinned_grads(net, x, wout, acts)
    assert sorted(grads) == sorted(ref_grads)
    worst = _assert_grads_match(dx, grads, ref_dx, ref_grads, "pinned f64")
    print(f"plane U-Net {shape}: largest gradient error / largest entry {worst:.3e}")


def test_plane_unet_backward_routes_pool_ties_to_the_first_maximum():
    """Every 2x2 window an exact tie (conv weights zero, positive biases: constant activations): the max-pool's gradient must reach the
    window's FIRST entry, as torch's max_pool2d backward does -- compared with torch-CPU autograd exactly (the values tie on both sides)."""
    from oracle import vtaco_oracle as orc
    net = _net(3, 32, 32, 32, seed=2)
    with torch.no_grad():
        for l in (0, 1):
            for conv in (net.down_convs[l].conv1, net.down_convs[l].conv2):
                conv.weight.zero_()
                conv.bias.fill_(0.25 * (l + 1))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 32, 16, 16, generator=g)
    wout = torch.randn(2, 32, 16, 16, generator=g)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    (orc.unet2d_forward(sd, x) * wout).sum().backward()
    net = net.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    (net(xd) * wout.to(DEV)).sum().backward()
    for name, p in net.named_parameters():
        ref = sd[name].grad
        assert float((p.grad.cpu() - ref).abs().max()) <= 3e-5 * max(1e-6, float(ref.abs().max())), name
    assert float(net.down_convs[0].conv2.bias.grad.abs().max()) > 0      # the tied windows did carry gradient


def _g19_net():
    """vtaco_amd's UNet with the parameters the reference module drew for g19 (same seeds; every tensor's sums re-checked)."""
    from conftest import GOLDEN
    from vtaco_amd.encoder.unet import UNet
    z = np.load(os.path.join(GOLDEN, "g19_plane_unet.npz"))
    seed, bias_seed = int(z["seeds"][0]), int(z["seeds"][1])
    torch.manual_seed(seed)
    net = UNet(32, in_channels=32, depth=4, start_filts=32, merge_mode="concat")
    g = torch.Generator().manual_seed(bias_seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    # the fixture's sums were taken with 8 intra-op threads (make_plane_unet_goldens.py): torch's CPU reduction splits a tensor by the
    # thread count, so a float64 sum is bit-equal to the stored one only under the same count, whatever cores this host has
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        for name, p in net.named_parameters():
            ref = z[f"psum.{name}"]
            assert float(p.detach().double().sum()) == ref[0] and float(p.detach().double().abs().sum()) == ref[1], name
    finally:
        torch.set_num_threads(threads)
    return net, z


def test_plane_unet_against_the_reference_module_golden():
    """g19: the REAL reference src/encoder/unet.py at the shipped shape (depth 4, 32 filters, three 32 x 32 planes), forward and
    backward: output, dL/dx, and every parameter gradient's 64 sampled entries + sum against vt_plane_unet_fwd / _bwd."""
    net, z = _g19_net()
    net = net.to(DEV)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    out = net(x)
    (out * torch.from_numpy(z["w"]).to(DEV)).sum().backward()
    scale = float(np.abs(z["out"]).max())
    assert float((out.detach().cpu() - torch.from_numpy(z["out"])).abs().max()) <= 2e-5 * scale
    # (gradients against the fixture: flip-aware -- the reference ran on the CPU, a ReLU at ~0 or a near-tied pool window may take the
    # other branch here; a flipped unit moves dx on its receptive field and every parameter's sum a little)
    dscale = float(np.abs(z["dx"]).max())
    derr = (x.grad.cpu() - torch.from_numpy(z["dx"])).abs()
    assert float((derr > 3e-5 * dscale).float().mean()) < 0.10 and float(derr.norm()) <= 3e-2 * float(np.linalg.norm(z["dx"]))
    sample_seed = int(z["seeds"][3])
    for name, p in net.named_parameters():
        gr = p.grad.double().reshape(-1).cpu()
        idx = torch.randint(0, gr.numel(), (64,), generator=torch.Generator().manual_seed(sample_seed + sum(map(ord, name))))
        ref = torch.from_numpy(z[f"gsample.{name}"]).double()
        gs = z[f"gsum.{name}"]
        typical = max(1e-9, float(gs[1]) / gr.numel())                 # the gradient's mean |entry|
        assert float((gr[idx] - ref).abs().max()) <= 3e-2 * max(typical * 8, float(ref.abs().max())), name
        assert abs(float(gr.sum()) - gs[0]) <= 3e-2 * gs[1] + 1e-9, name
    # ... and, elementwise, the float64 gradients of the function the kernel computed at these inputs (its own branch decisions)
    out_k, _, acts = _kernel_acts(net, x.detach())
    assert torch.equal(out_k, out.detach())
    ref_dx, ref_grads = _pinned_grads(net, x, torch.from_numpy(z["w"]), acts)
    _assert_grads_match(x.grad, {n: p.grad for n, p in net.named_parameters()}, ref_dx, ref_grads, "g19 pinned f64")
