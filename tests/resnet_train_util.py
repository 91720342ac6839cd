"""Shared by tests/test_resnet_train_gpu.py and tests/test_resnet_train_cpu.py: the cases of the float64 gate, the host module's per-scene
training step on the CPU (float64 and float32), computed once per case, the error measure, the guard against framework operators and
a restatement of the train path's workspace.  Test infrastructure."""
import copy
import functools
import sys

import torch
from torch.nn import functional as F

from conftest import GOLDEN

CLASSES = 8
# (network, S scenes, G images per scene, (H, W), seed)
CASES = [("Resnet18", 1, 2, (64, 64), 101),      # layer4 is 2 x 2, every pixel on a border
         ("Resnet18", 2, 5, (37, 45), 102),      # odd extents at every stage: the stride-2 data gradient and the pool backward at ragged edges
         ("Resnet18", 3, 3, (40, 72), 103),      # non-square, groups of three
         ("Resnet18", 1, 5, (100, 76), 104),     # layer1 has 2 375 pixels: a ragged last 32-pixel tile, several slices per sum
         ("Resnet34", 2, 2, (48, 64), 100)]
# The seeds: a case is only a test of arithmetic while no ReLU, max-pool or L1-sign decision of the float64 reference sits within f32
# roundoff of a tie (one flipped ReLU in layer1 moves a gradient by ~4e-3, two hundred times e32).  Resnet34 at this size has 1.3 M
# such decisions; of the seeds 100..179 the one whose float64 forward keeps the smallest |pre-ReLU value| largest was taken (8.1e-6;
# smallest pool gap 2.7e-5, smallest |out - target| 3.0e-3) -- a choice by the reference alone, before any kernel ran on it.
IDS = [f"{n}-S{S}-G{G}-{hw[0]}x{hw[1]}" for n, S, G, hw, _ in CASES]
_PATCHED = ("conv2d", "batch_norm", "max_pool2d", "adaptive_avg_pool2d", "linear")


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


def seeded_resnet(name, seed, classes=CLASSES):
    sys.path.insert(0, GOLDEN)
    from make_resnet_goldens import deterministic_fill
    from vtaco_amd.encoder import encoder_dict
    net = encoder_dict[name](num_classes=classes)
    deterministic_fill(net, seed)
    return net.train()


def layer4_hw(H, W):
    up = lambda v: (v - 1) // 2 + 1
    for _ in range(5):
        H, W = up(H), up(W)
    return H, W


def case_inputs(case):
    name, S, G, (H, W), seed = case
    gen = torch.Generator().manual_seed(seed)
    imgs = torch.rand(S, G, 3, H, W, generator=gen)
    target = torch.randn(S, G, CLASSES, generator=gen)
    return seeded_resnet(name, seed), imgs, target


def host_step(net, imgs, target, dtype=torch.float32):
    """One L1 training step of a copy of the host module on the CPU, called once per scene in scene order: the output [S, G, classes],
    every parameter's gradient, every buffer afterwards."""
    net = copy.deepcopy(net).train().to(dtype)
    imgs, target = imgs.to(dtype), target.to(dtype)
    out = torch.stack([net.forward_modules(imgs[s]) for s in range(imgs.shape[0])], dim=0)
    F.l1_loss(out, target).backward()
    res = {"out": out.detach().contiguous()}
    res.update({"grad:" + n: p.grad.contiguous() for n, p in net.named_parameters()})
    res.update({"buf:" + n: b.detach().clone() for n, b in net.named_buffers()})
    return res


def rel_err(t, t64):
    """|| t - t64 ||_2 / || t64 ||_2 (the L2 form: a ReLU whose pre-activation changes sign between f32 and f64 moves single entries)."""
    return float((t.double().cpu() - t64).norm() / t64.norm())


@functools.lru_cache(maxsize=None)
def reference(i):
    """(net, imgs, target, the float64 step, e32 per tensor) of CASES[i]."""
    net, imgs, target = case_inputs(CASES[i])
    r64 = host_step(net, imgs, target, torch.float64)
    r32 = host_step(net, imgs, target, torch.float32)
    e32 = {k: rel_err(v, r64[k]) for k, v in r32.items() if not k.endswith("num_batches_tracked")}
    return net, imgs, target, r64, e32


def workspace_floats(blocks, n_img, scenes, H, W):
    """vt_resnet_train_workspace_bytes / 4, buffer by buffer (every buffer rounded up to 4 floats)."""
    up, up4 = (lambda v: (v - 1) // 2 + 1), (lambda n: (n + 3) // 4 * 4)
    N, S, G = n_img, scenes, n_img // scenes
    Hs, Ws = up(H), up(W)
    Hp, Wp = up(Hs), up(Ws)
    nsl = lambda hw: (G * hw + 1023) // 1024
    stat = lambda C: up4(2 * S * C) + up4(4 * S * C)                       # mean, rstd as floats; mean, variance as doubles
    total = up4(2 * 21 * 256)                                              # the stem's fragments
    total += up4(N * Hs * Ws * 64) + up4(N * Hp * Wp * 16) + up4(N * Hp * Wp * 64) + stat(64)     # the stem's z, the pool's positions, the pooled
    red = 3 * S * nsl(Hs * Ws) * 64
    wpart = S * ((Hs + 3) // 4) * 64 * 160
    most, cin, h, w = 0, 64, Hp, Wp
    for s, count in enumerate(blocks):
        cout = 64 << s
        for b in range(count):
            proj = b == 0 and s > 0
            if proj:
                h, w = up(h), up(w)
            n = N * h * w * cout
            total += up4(cout * cin * 9) + up4(cout * cout * 9) + (up4(cout * cin) if proj else 0)      # packed weights
            total += (5 if proj else 4) * up4(n) + (3 if proj else 2) * stat(cout)                        # z1, a1, z2, y (, zk); statistics
            most = max(most, n)
            red = max(red, 3 * S * nsl(h * w) * cout)
            rows = 4 * (cout // 64)
            wpart = max(wpart, S * ((h + rows - 1) // rows) * cout * cout * 9)
            cin = cout
    total += 2 * up4(N * 512) + 2 * up4(N * 100)                           # pooled features, linear's output, their gradients
    total += 4 * up4(most) + up4(N * Hs * Ws * 64)                         # four gradient buffers, the stem's gradient
    total += up4(4 * S * 512) + up4(8 * S * 512)                           # BatchNorm backward means and sums
    total += up4(2 * red) + up4(wpart)                                     # per-channel partials (doubles), weight-gradient partials
    total += up4(512 * 512 * 9) + up4(512 * 256)                           # transposed fragments for the data gradients
    return total
