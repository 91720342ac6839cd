"""GPU: the decoder's field jet (vt_decode_jet, vt_decode_jet_composed: csrc/field_jet.hip) against the float64 autograd statement of
tests/refine_ref.py, at the seeded weights and point sets whose conditions tests/test_refine_ref_cpu.py asserts.

The gate is tests/test_decode_train_f64_gpu.py's: |got - ref64| <= 8 max(e32, 2^-24 bound) elementwise, e32 the largest error of the
same graph run in float32 on the CPU, bound the sum over magnitudes behind the number (refine_ref.jet_closed(magnitude=True)).  f is
gated at every point, the six derivatives at every point that is not near a kink; each of the 7 numbers has its own e32.  Every
comparison prints ``RATIO <tag>: ...``; the largest of a run on the MI355X are kept in profiles/refine_f64_ratios.txt.

f is ``ops.decode_fwd``'s exact-f32 logit to the bit: the same operations in the same order.  The fused kernel and the composed
form agree to the bit as well (asserted; stronger than the gate the two would otherwise share)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as rr
from decode_train_ref import gate_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
NAMES = ("f", "f_x", "f_y", "f_z", "f_xy", "f_xz", "f_yz")


@pytest.fixture(scope="module")
def decoder():
    from vtaco_amd import ops
    dec = rr.seeded_decoder()
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    dec = dec.to(DEV)
    blob, blob_t = ops.refine.refine_blobs(dec)
    return sd, blob, blob_t


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"


@pytest.mark.parametrize("B,N,R", rr.JET_CASES)
def test_jet_vs_float64_autograd(decoder, B, N, R):
    from vtaco_amd import ops
    sd, blob, blob_t = decoder
    grid, pts = rr.jet_grid(B, R), rr.jet_points(B, N, R)
    gd, pd = grid.to(DEV), pts.to(DEV)
    fused = ops.refine.decode_jet(gd, blob, blob_t, pd, form="fused")
    composed = ops.refine.decode_jet(gd, blob, blob_t, pd, form="composed")
    assert fused.shape == (B, N, 8) and (fused[..., 7] == 0).all()
    assert torch.equal(fused, composed), f"fused and composed differ: {float((fused - composed).abs().max())}"
    assert torch.equal(fused, ops.refine.decode_jet(gd, blob, blob_t, pd, form="fused"))                      # two runs, equal bits
    assert torch.equal(composed, ops.refine.decode_jet(gd, blob, blob_t, pd, form="composed"))
    logits = ops.decode_fwd(gd, blob, pts=pd, precision="f32")
    assert torch.equal(fused[..., 0], logits)                                                          # the forward's own bits
    got = fused.cpu()
    for b in range(B):
        g1 = grid[b:b + 1]
        j64, _ = rr.jet_autograd(sd, g1, pts[b])
        j32, _ = rr.jet_autograd(sd, g1, pts[b], dtype=torch.float32)
        _, mag = rr.jet_closed(sd, g1, pts[b], magnitude=True)
        ok = ~rr.near_kink(sd, g1, pts[b])
        assert float(ok.float().mean()) >= 0.95
        tag = f"jet B{B} N{N} R{R} b{b}"
        _gate(f"{tag} f", got[b, :, 0], j64[:, 0], j32[:, 0], mag[:, 0])
        for k in range(1, 7):
            _gate(f"{tag} {NAMES[k]}", got[b, ok, k], j64[ok, k], j32[ok, k], mag[ok, k])
        d = rr.divisor()
        out = (pts[b].double() / d + 0.5 >= 1) | (pts[b].double() / d + 0.5 < 0)
        for (a, c), col in (((0, 1), 4), ((0, 2), 5), ((1, 2), 6)):                                    # a clamped axis: exact zeros
            assert (got[b, :, col][out[:, a] | out[:, c]] == 0).all()


def test_fused_is_composed_beyond_one_pass(decoder):
    """2^17 + 37 points: every workgroup of the fused kernel walks several rounds of tiles and the composed form takes two passes
    through its workspace; equal bits, and the logits are the forward's."""
    from vtaco_amd import ops
    sd, blob, blob_t = decoder
    N = (1 << 17) + 37
    gd, pd = rr.jet_grid(1, 8).to(DEV), rr.jet_points(1, N, 8).to(DEV)
    fused = ops.refine.decode_jet(gd, blob, blob_t, pd, form="fused")
    assert torch.equal(fused, ops.refine.decode_jet(gd, blob, blob_t, pd, form="composed"))
    assert torch.equal(fused[..., 0], ops.decode_fwd(gd, blob, pts=pd, precision="f32"))


def test_jet_refuses_other_shapes(decoder):
    from vtaco_amd import ops
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.models import decoder_dict
    sd, blob, blob_t = decoder
    with pytest.raises(VtError, match="hidden 32, c_dim 32, 5 blocks"):
        ops.refine.decode_jet(torch.zeros(1, 64, 5, 5, 5, device=DEV), blob, blob_t, torch.zeros(1, 4, 3, device=DEV))
    with pytest.raises(VtError, match="hidden_size 32, c_dim 32, 5 ReLU blocks"):
        ops.refine.refine_blobs(decoder_dict["simple_local"](dim=3, c_dim=64, hidden_size=64))
    assert ops.refine.decode_jet(torch.zeros(1, 32, 5, 5, 5, device=DEV), blob, blob_t, torch.zeros(1, 0, 3, device=DEV)).shape == (1, 0, 8)
