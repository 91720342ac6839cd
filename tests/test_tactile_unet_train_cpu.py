"""No GPU: the train-mode tactile U-Net's ABI (symbols, the covered set), ``TactileUNet.forward_scenes`` on the host, and the
conditioning of the float64 gate's cases (tests/test_tactile_unet_train_gpu.py)."""
import copy

import pytest
import torch
from tactile_unet_util import seeded_unet
from tactile_unet_train_util import CASES, IDS, case_inputs, host_step, reference, rel_err


def test_symbols_and_covered_set():
    from vtaco_amd import _lib
    lib = _lib.load()
    for name in ("vt_tactile_unet_train_supported", "vt_tactile_unet_train_workspace_bytes", "vt_tactile_unet_train_fwd", "vt_tactile_unet_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert [f[0] for f in _lib.TactileUnetGrads._fields_] == ["down_w", "down_b", "down_bn_w", "down_bn_b", "up_tw", "up_tb", "up_w", "up_b",
                                                             "up_bn_w", "up_bn_b", "final_w", "final_b"]
    sup, size = lib.vt_tactile_unet_train_supported, lib.vt_tactile_unet_train_workspace_bytes
    # (depth, start_filts, in_channels, num_classes, n_img, group, H, W)
    for S in (1, 12):
        assert sup(3, 32, 3, 1, 5 * S, 5, 320, 240) == 1 and size(3, 32, 3, 1, 5 * S, 5, 320, 240) > 0      # the shipped network
    assert sup(3, 8, 3, 1, 5, 5, 64, 48) == 1 and size(3, 8, 3, 1, 5, 5, 64, 48) > 0                          # g6_tactile.npz
    for bad in ((6, 8, 3, 1, 5, 5, 64, 64),          # depth 6
                (3, 8, 3, 1, 5, 5, 18, 12),          # H no multiple of 2^(depth-1)
                (3, 8, 3, 1, 6, 5, 16, 12)):         # n_img no multiple of the group
        assert sup(*bad) == 0 and size(*bad) == 0, bad


def test_forward_scenes_on_the_host_is_the_per_scene_loop():
    base = seeded_unet(3, 8, 3, 1, 51).train()
    gen = torch.Generator().manual_seed(52)
    imgs = torch.rand(3, 5, 3, 16, 12, generator=gen)
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    ya = a.forward_scenes(imgs)
    yb = torch.cat([b.forward_modules(imgs[s]).reshape(1, 5, -1) for s in range(3)], dim=0)
    assert ya.shape == (3, 5, 16 * 12) and torch.equal(ya, yb)
    w = torch.rand(ya.shape, generator=gen)
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), n
    assert int(a.down_convs[0].bn.num_batches_tracked) == 6


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_f64_gate_cases_are_well_conditioned(i):
    """A second f32 evaluation of the host module with another summation order (channels_last) stays within 8 e32 of the float64 step
    on every tensor: the gate of the GPU test does not fail on rounding alone.  Half of the outputs unsaturated."""
    S = CASES[i][0]
    net, x, target, r64, e32 = reference(i)
    torch.manual_seed(0)
    other = host_step(net, x, target, S, torch.float32, channels_last=True)
    bad = [(k, rel_err(other[k], r64[k]), e32[k]) for k in e32 if not rel_err(other[k], r64[k]) <= 8 * e32[k]]
    assert not bad, bad
    assert float(((r64["out"] > 0.05) & (r64["out"] < 0.95)).double().mean()) >= 0.5
