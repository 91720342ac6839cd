"""CPU: the float64 statement of the field jet and of mesh refinement (tests/refine_ref.py) checked against itself, the conditions the
GPU tests rest on, and the host side of ``refinement_step`` (constructor refusals, exports, header)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JET_CASES = rr.JET_CASES


@pytest.fixture(scope="module")
def sd():
    return {k: v.detach().clone() for k, v in rr.seeded_decoder().state_dict().items()}


def test_index_sampler_is_grid_sample(sd):
    """The twice-differentiable corner gather is F.grid_sample (border, align_corners) in value and gradient, clamped axes included."""
    for R in (5, 8):
        grid, pts = rr.jet_grid(1, R), rr.jet_points(1, 600, R)[0]
        out = []
        for sampler in ("index", "grid_sample"):
            p = pts.double().clone().requires_grad_()
            f = rr.field(sd, grid, p, sampler=sampler)
            g, = torch.autograd.grad(f.sum(), p)
            out.append((f.detach(), g))
        assert (out[0][0] - out[1][0]).abs().max() <= 1e-13 and (out[0][1] - out[1][1]).abs().max() <= 1e-12
        with pytest.raises(RuntimeError, match="grid_sampler_3d_backward"):        # why the index form is the reference
            p = pts.double().clone().requires_grad_()
            g, = torch.autograd.grad(rr.field(sd, grid, p, sampler="grid_sample").sum(), p, create_graph=True)
            torch.autograd.grad(g[:, 0].sum(), p)


@pytest.mark.parametrize("R", [5, 8])
def test_closed_form_jet_is_the_autograd_jet(sd, R):
    """Away from kinks the closed form equals float64 double backward to 1e-12 of the magnitude sum behind each number; the Hessian is
    symmetric with a zero diagonal; a clamped axis has zero first and second derivatives."""
    grid, pts = rr.jet_grid(1, R), rr.jet_points(1, 2053, R)[0]
    ok = ~rr.near_kink(sd, grid, pts)
    ja, H = rr.jet_autograd(sd, grid, pts)
    jc, mag = rr.jet_closed(sd, grid, pts, magnitude=True)
    assert ((ja - jc).abs()[ok] <= 1e-12 * mag[ok]).all(), float(((ja - jc).abs()[ok] / mag[ok].clamp(min=1e-300)).max())
    assert H.diagonal(dim1=1, dim2=2).abs().max() == 0.0
    assert (H - H.transpose(1, 2)).abs()[ok].max() <= 1e-12 * mag[ok][:, 4:].max()
    d = rr.divisor()
    out = (pts.double() / d + 0.5 >= 1) | (pts.double() / d + 0.5 < 0)
    assert out.any(0).all() and (out[:12].sum(1) >= 1)[:6].all()                     # each axis is clamped somewhere, both directions seeded
    g = ja[:, 1:4]
    assert (g[out] - jc[:, 1:4][out]).abs().max() <= 1e-12
    for (a, b), col in (((0, 1), 4), ((0, 2), 5), ((1, 2), 6)):
        assert ja[:, col][out[:, a] | out[:, b]].abs().max() == 0.0


def test_float32_graph_differs_only_near_kinks(sd):
    """What validates the bound: over 400 000 points the float32 CPU graph's ReLU masks, cells and clamp patterns differ from the
    float64 ones only at points near_kink flags -- and some do differ, so the check is not empty."""
    grid, pts = rr.jet_grid(1, 8), rr.jet_points(1, 400000, 8)[0]
    near = rr.near_kink(sd, grid, pts)
    m64, c64, k64 = rr.masks_and_cells(sd, grid, pts)
    m32, c32, k32 = rr.masks_and_cells(sd, grid, pts, dtype=torch.float32)
    diff = (m64 != m32).any(1) | (c64 != c32).any(1) | (k64 != k32).any(1)
    assert int(diff.sum()) >= 1
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    assert float(near.float().mean()) <= 0.05


@pytest.mark.parametrize("B,N,R", JET_CASES)
def test_near_kink_share_of_the_gpu_point_sets(sd, B, N, R):
    """A condition of the GPU tests, met by the reference alone: at most 5 % of each point set is near a kink (N = 1: the point is not)."""
    grid, pts = rr.jet_grid(B, R), rr.jet_points(B, N, R)
    for b in range(B):
        near = rr.near_kink(sd, grid[b:b + 1], pts[b])
        assert float(near.float().mean()) <= 0.05, (b, float(near.float().mean()))


def test_refine_meshes_near_kink_share_and_loss_gradient(sd):
    """The meshes of tests/test_refine_gpu.py: face points near a kink stay under 5 %, the per-face-corner gradients sum to the vertex
    gradient, a zero-area face and an unreferenced vertex give finite numbers, and the RMSprop step is torch's."""
    import refine_cases as rc
    grid = rr.jet_grid(1, 8, seed=3)
    for name, (verts, faces) in rc.meshes().items():
        eps = rc.eps_for(faces.shape[0], seed=1)
        fp = rr.face_points(verts.double(), faces.long(), eps.double()).float()
        near = rr.near_kink(sd, grid, fp)
        assert float(near.float().mean()) <= 0.05 or faces.shape[0] < 20, (name, float(near.float().mean()))
        t, n, gfv, gv = rr.refine_loss(sd, grid, verts, faces, eps, 0.4)
        assert torch.isfinite(gv).all() and torch.isfinite(t).all() and torch.isfinite(n).all(), name
        assert gfv.shape == (faces.shape[0], 3, 3) and gv.shape == verts.shape
        used = torch.zeros(verts.shape[0], dtype=torch.bool)
        used[faces.long().reshape(-1)] = True
        assert (gv[~used] == 0).all()
    v = torch.nn.Parameter(torch.randn(50, 3, dtype=torch.float64))
    opt = torch.optim.RMSprop([v], lr=1e-4)
    v0, sq = v.detach().clone(), torch.zeros(50, 3, dtype=torch.float64)
    for k in range(3):
        g = torch.randn(50, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(k))
        v.grad = g.clone()
        opt.step()
        v0, sq = rr.rmsprop_step(v0, g, sq)
        assert (v.detach() - v0).abs().max() <= 1e-15


class _Enc(torch.nn.Module):
    def __init__(self, planes):
        super().__init__()
        self.planes = planes


class _Model(torch.nn.Module):
    def __init__(self, decoder, encoder=None):
        super().__init__()
        self.decoder = decoder
        if encoder is not None:
            self.encoder = encoder


def test_constructor_refusals():
    from vtaco_amd._lib import VtError
    from vtaco_amd.conv_onet.generation import Generator3D
    from vtaco_amd.conv_onet.models import decoder_dict
    dec = decoder_dict["simple_local"](dim=3, c_dim=32, hidden_size=32)
    assert Generator3D(_Model(dec)).refinement_step == 0
    gen = Generator3D(_Model(dec), refinement_step=3)
    assert gen.refinement_step == 3 and gen.refine_sampler == "device"
    assert Generator3D(_Model(dec), refinement_step=np.int64(2), refine_sampler="numpy").refinement_step == 2
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(VtError, match="refinement_step"):
            Generator3D(_Model(dec), refinement_step=bad)
    with pytest.raises(VtError, match="refine_sampler"):
        Generator3D(_Model(dec), refinement_step=1, refine_sampler="torch")
    for kw in (dict(with_img=True), dict(with_img=True, encode_t2d=True)):
        with pytest.raises(VtError, match="tactile"):
            Generator3D(_Model(dec), refinement_step=1, **kw)
        Generator3D(_Model(dec), **kw)                                               # refinement_step 0 keeps every route
    with pytest.raises(VtError, match="attention"):
        Generator3D(_Model(decoder_dict["attention_local"](dim=3, c_dim=32, hidden_size=32)), refinement_step=1)
    with pytest.raises(VtError, match="plane features"):
        Generator3D(_Model(dec, _Enc(["xz", "xy", "yz"])), refinement_step=1)
    with pytest.raises(VtError, match="PointConv"):
        Generator3D(_Model(decoder_dict["simple_local_point"](dim=3, c_dim=32, hidden_size=32, gaussian_val=0.2)), refinement_step=1)
    for kw in (dict(c_dim=64, hidden_size=32), dict(c_dim=32, hidden_size=64), dict(c_dim=32, hidden_size=32, n_blocks=3),
               dict(c_dim=32, hidden_size=32, leaky=True)):
        with pytest.raises(VtError, match="hidden_size 32, c_dim 32, 5 ReLU blocks"):
            Generator3D(_Model(decoder_dict["simple_local"](dim=3, **kw)), refinement_step=1)
    # the routes that refuse when called, before they touch anything
    with pytest.raises(VtError, match="generate_mesh_graphed: refinement_step"):
        gen.generate_mesh_graphed(torch.zeros(1, 8, 3))
    with pytest.raises(VtError, match="generate_obj_mesh_sharded: refinement_step"):
        gen.generate_obj_mesh_sharded({"inputs": torch.zeros(1, 8, 3)})
    with pytest.raises(VtError, match="generate_obj_mesh_tactile: refinement_step"):
        gen.generate_obj_mesh_tactile({"inputs": torch.zeros(1, 8, 3)}, None, None, None)


def test_config_passes_refinement_step_and_sampler():
    src = open(os.path.join(ROOT, "vtaco_amd", "conv_onet", "config.py")).read()
    assert "refinement_step=g.get('refinement_step', 0)" in src and "refine_sampler=g.get('refine_sampler', 'device')" in src


def test_ops_exports_and_header_declarations():
    from vtaco_amd import ops
    from vtaco_amd._lib import SIGNATURES
    for name in ("decode_jet", "refine_sample", "refine_face_grad", "refine_step", "refine"):       # a submodule, as ops.mesh / ops.icp are:
        assert callable(getattr(ops.refine, name)), name                                           # tests/test_ops_surface_cpu.py pins ops' own names
    header = open(os.path.join(ROOT, "include", "vtaco_hip.h")).read()
    for sym in ("vt_decode_jet", "vt_decode_jet_composed", "vt_decode_jet_composed_workspace_bytes", "vt_refine_sample",
                "vt_refine_face_grad", "vt_refine_step", "vt_refine", "vt_refine_workspace_bytes", "vt_refine_accum_bytes"):
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in SIGNATURES, sym
    from vtaco_amd.conv_onet.generation import Generator3D, Mesh
    assert callable(Generator3D.refine_mesh) and callable(Mesh.refine)
