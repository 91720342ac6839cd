"""GPU: one refinement iteration (vt_refine_sample, vt_refine_face_grad, vt_refine_step) and the loop (vt_refine) of csrc/refine.hip
against the float64 autograd statement of upstream's refine_mesh in tests/refine_ref.py, on the meshes of tests/refine_cases.py.

Tolerances: the gradient and the loss terms take tests/test_decode_train_f64_gpu.py's ratio and gate (|got - ref64| <= 8 max(e32,
2^-24 bound): e32 from the same graph in float32 on the CPU, bound the sum over magnitudes of the per-face terms that make the number),
on the faces whose point is not near a kink (refine_ref.near_kink); the step is within 2 float32 roundings of |v| + 10 lr of the float64
update from the same g and sq; a loop of k steps moves no vertex further than k lr / sqrt(1 - 0.99) plus one rounding (the normalised
step g / (sqrt(sq) + 1e-8) is below 1 / sqrt(0.01), since sq >= 0.01 g^2); the sampler's moments lie within 6 standard errors of
Dirichlet(1/2,1/2,1/2)'s (E x = 1/3, E x^2 = 1/5; x ~ Beta(1/2, 1): Var x = 4/45, Var x^2 = E x^4 - 1/25 = 1/9 - 1/25)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_cases as rc
import refine_ref as rr
from decode_train_ref import gate_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 8.0
U = 2.0 ** -24
THRESHOLD = 0.4
LR = 1e-4


@pytest.fixture(scope="module")
def scene():
    from vtaco_amd import ops
    dec = rr.seeded_decoder()
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    dec = dec.to(DEV)
    grid = rr.jet_grid(1, 8, seed=3)
    return {"sd": sd, "dec": dec, "blobs": ops.refine.refine_blobs(dec), "grid": grid, "gd": grid.to(DEV), "meshes": rc.meshes()}


def _gate(tag, got, r64, r32, bound):
    ratio, e32 = gate_ratio(got, r64, r32, bound)
    print(f"RATIO {tag}: {ratio:.3f} (e32 {e32:.3e})")
    assert ratio <= GATE, f"{tag}: |got - ref64| is {ratio:.3f} x max(e32, 2^-24 bound), above {GATE}"


def _device_gradient(s, verts, faces, eps, threshold=THRESHOLD):
    """(terms [F,2], gradient [V,3], points [F,3]) of one iteration's first three launches on the device, given eps."""
    from vtaco_amd import ops
    vd, fd = verts.to(DEV), faces.to(DEV)
    eps_d, pts = ops.refine.refine_sample(vd, fd, eps=eps.to(DEV))
    jet = ops.refine.decode_jet(s["gd"], *s["blobs"], pts.unsqueeze(0))
    terms, accum = ops.refine.refine_face_grad(vd, fd, eps_d, jet[0], threshold)
    moved, sq = vd.clone(), torch.zeros_like(vd)
    grad = ops.refine.refine_step(moved, accum, sq, lr=LR)
    assert (accum == 0).all()                                      # the step leaves the sums ready for the next iteration
    return terms.cpu(), grad.cpu(), pts.cpu()


@pytest.mark.parametrize("name", ["tetra", "fan", "mc", "degen"])
def test_face_grad_vs_float64_autograd(scene, name):
    s = scene
    verts, faces = s["meshes"][name]
    eps = rc.eps_for(faces.shape[0], seed=1)
    fp = rr.face_points(verts.double(), faces.long(), eps.double())
    keep = ~rr.near_kink(s["sd"], s["grid"], fp.float())
    assert int(keep.sum()) >= max(1, int(0.95 * faces.shape[0]) - 1)
    faces, eps = faces[keep].contiguous(), eps[keep].contiguous()
    terms, grad, pts = _device_gradient(s, verts, faces, eps)
    assert (pts.double() - fp[keep]).abs().max() <= 3 * U * float(verts.abs().max())     # three products of sum 1, two additions
    assert torch.isfinite(grad).all() and torch.isfinite(terms).all()
    t64, n64, gfv64, gv64 = rr.refine_loss(s["sd"], s["grid"], verts, faces, eps, THRESHOLD)
    t32, n32, _, gv32 = rr.refine_loss(s["sd"], s["grid"], verts, faces, eps, THRESHOLD, dtype=torch.float32)
    bound = torch.zeros_like(gv64).index_add_(0, faces.long().reshape(-1), gfv64.abs().reshape(-1, 3))
    _gate(f"refine/{name} target term", terms[:, 0], t64, t32, t64.abs())
    _gate(f"refine/{name} normal term", terms[:, 1], n64, n32, n64.abs())
    _gate(f"refine/{name} vertex gradient", grad, gv64, gv32, bound)


@pytest.mark.parametrize("name", ["fan", "mc", "degen"])
def test_vertex_gradient_bits_under_face_permutation(scene, name):
    verts, faces = scene["meshes"][name]
    eps = rc.eps_for(faces.shape[0], seed=2)
    perm = torch.randperm(faces.shape[0], generator=torch.Generator().manual_seed(9))
    _, g0, _ = _device_gradient(scene, verts, faces, eps)
    _, g1, _ = _device_gradient(scene, verts, faces[perm].contiguous(), eps[perm].contiguous())
    assert torch.equal(g0, g1) and g0.abs().max() > 0


def test_step_vs_float64_update(scene):
    from vtaco_amd import ops
    verts, faces = scene["meshes"]["mc"]
    eps = rc.eps_for(faces.shape[0], seed=4)
    vd, fd = verts.to(DEV), faces.to(DEV)
    eps_d, pts = ops.refine.refine_sample(vd, fd, eps=eps.to(DEV))
    jet = ops.refine.decode_jet(scene["gd"], *scene["blobs"], pts.unsqueeze(0))
    _, accum = ops.refine.refine_face_grad(vd, fd, eps_d, jet[0], THRESHOLD)
    sq0 = torch.rand(verts.shape, generator=torch.Generator().manual_seed(6)) * 1e-4
    sq0[::3] = 0.0                                                 # fresh accumulators next to used ones
    moved, sq = vd.clone(), sq0.to(DEV)
    g = ops.refine.refine_step(moved, accum, sq, lr=LR).cpu().double()
    v64, sq64 = rr.rmsprop_step(verts.double(), g, sq0.double(), lr=LR)
    assert ((moved.cpu().double() - v64).abs() <= 2 * U * (verts.double().abs() + LR * 10)).all()
    assert ((sq.cpu().double() - sq64).abs() <= U * sq64).all()                                # one rounding


@pytest.mark.parametrize("name", ["tetra", "fan", "mc", "degen"])
def test_loop_bound_determinism_and_untouched_parts(scene, name):
    from vtaco_amd import ops
    s = scene
    verts, faces = s["meshes"][name]
    vd, fd = verts.to(DEV), faces.to(DEV)
    k = 5
    run = lambda **kw: ops.refine.refine(vd, fd, s["gd"], s["dec"], k, THRESHOLD, 0.1, lr=LR, **kw)
    out, terms = run(seed=7, return_losses=True)
    assert out.shape == vd.shape and out.dtype == torch.float32 and terms.shape == (k, faces.shape[0], 2)
    assert torch.equal(vd.cpu(), verts) and torch.equal(fd.cpu(), faces)                      # inputs and faces unchanged
    assert torch.isfinite(out).all() and torch.isfinite(terms).all()
    moved = (out.cpu().double() - verts.double()).abs()
    assert (moved <= k * LR / np.sqrt(1 - 0.99) + U * verts.double().abs()).all(), float(moved.max())
    assert moved.max() > 0
    used = torch.zeros(verts.shape[0], dtype=torch.bool)
    used[faces.long().reshape(-1)] = True
    assert torch.equal(out.cpu()[~used], verts[~used])                                        # an unreferenced vertex stays, bit for bit
    assert torch.equal(out, run(seed=7)) and not torch.equal(out, run(seed=8))
    assert torch.equal(out, run(seed=7, form="composed"))                                     # both jet forms: one result


def test_device_sampler_is_dirichlet_half(scene):
    from vtaco_amd import ops
    F = 65536
    verts = scene["meshes"]["tetra"][0].to(DEV)
    faces = torch.randint(0, 4, (F, 3), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    eps, pts = ops.refine.refine_sample(verts, faces, seed=5, step=2)
    e = eps.cpu().double()
    assert (e >= 0).all() and ((e.sum(1) - 1).abs() <= 2 * U).all()
    se1, se2 = np.sqrt((4 / 45) / F), np.sqrt((1 / 9 - 1 / 25) / F)
    for i in range(3):
        assert abs(float(e[:, i].mean()) - 1 / 3) <= 6 * se1 and abs(float((e[:, i] ** 2).mean()) - 1 / 5) <= 6 * se2, i
    again, _ = ops.refine.refine_sample(verts, faces, seed=5, step=2)
    assert torch.equal(eps, again)
    for kw in (dict(seed=5, step=3), dict(seed=6, step=2)):
        other, _ = ops.refine.refine_sample(verts, faces, **kw)
        assert not torch.equal(eps, other)
    fp = (verts.cpu()[faces.cpu().long()].double() * e[:, :, None]).sum(1)
    assert (pts.cpu().double() - fp).abs().max() <= 3 * U * float(verts.abs().max())


def test_numpy_sampler_consumes_the_global_stream_as_upstream(scene):
    from vtaco_amd import ops
    s = scene
    verts, faces = s["meshes"]["fan"]
    F, k = faces.shape[0], 3
    np.random.seed(123)
    out = ops.refine.refine(verts.to(DEV), faces.to(DEV), s["gd"], s["dec"], k, THRESHOLD, 0.1, sampler="numpy")
    after = np.random.get_state()
    np.random.seed(123)
    draws = [np.random.dirichlet((0.5, 0.5, 0.5), size=F) for _ in range(k)]
    expect = np.random.get_state()
    assert after[0] == expect[0] and np.array_equal(after[1], expect[1]) and after[2:] == expect[2:]
    eps = torch.from_numpy(np.stack(draws).astype(np.float32))
    assert torch.equal(out, ops.refine.refine(verts.to(DEV), faces.to(DEV), s["gd"], s["dec"], k, THRESHOLD, 0.1, eps=eps))
