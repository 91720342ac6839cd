"""Shared by tests/test_tactile_unet_train_gpu.py and tests/test_tactile_unet_train_cpu.py: the cases of the float64 gate, the host
module's per-scene training step on the CPU (float64, float32, and float32 with another summation order), computed once per case, and
the error measure.  Test infrastructure."""
import copy
import functools

import torch
from torch.nn import functional as F

from tactile_unet_util import seeded_unet

# (S, G, (C, H, W), depth, start_filts, seed)
CASES = [(1, 2, (3, 8, 8), 3, 32, 21),        # a 2 x 2 bottom level, every pixel on a border
         (2, 3, (3, 20, 28), 3, 32, 22),      # ragged patches, groups of three, non-square
         (2, 5, (3, 16, 12), 3, 8, 23),       # widths below a matrix tile
         (1, 2, (1, 16, 16), 1, 16, 24),      # no pool, no up path
         (2, 5, (3, 96, 80), 3, 32, 25)]      # weight-gradient and statistics sums spread over many workgroups
IDS = [f"S{S}-G{G}-{'x'.join(map(str, chw))}-d{d}-sf{sf}" for S, G, chw, d, sf, _ in CASES]


def case_inputs(case):
    S, G, chw, depth, sf, seed = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(S * G, *chw, generator=gen)
    target = torch.rand(S * G, 1, chw[1], chw[2], generator=gen)
    return seeded_unet(depth, sf, chw[0], 1, seed).train(), x, target


def host_step(net, x, target, S, dtype=torch.float32, channels_last=False):
    """One L1 training step of a copy of the host module on the CPU, called once per scene in scene order: the output, every
    parameter's gradient, every buffer afterwards."""
    net = copy.deepcopy(net).train().to(dtype)
    x, target = x.to(dtype), target.to(dtype)
    if channels_last:
        net, x = net.to(memory_format=torch.channels_last), x.contiguous(memory_format=torch.channels_last)
    G = x.shape[0] // S
    out = torch.cat([net.forward_modules(x[s * G:(s + 1) * G]) for s in range(S)], dim=0)
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
    """(net, x, target, the float64 step, e32 per tensor) of CASES[i]."""
    net, x, target = case_inputs(CASES[i])
    r64 = host_step(net, x, target, CASES[i][0], torch.float64)
    r32 = host_step(net, x, target, CASES[i][0], torch.float32)
    e32 = {k: rel_err(v, r64[k]) for k, v in r32.items() if not k.endswith("num_batches_tracked")}
    return net, x, target, r64, e32
